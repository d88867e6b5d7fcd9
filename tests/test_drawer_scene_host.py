"""The host side of a drawer scene whose environments differ: the slot, group and row tables, the wrappers' checks, the definition of
the grouped cameras pinned in numpy, and the C ABI's three new symbols.  No GPU."""
import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import drawer_scene_fixtures as DS
from tests.test_capi_symbols import header_functions

NEW_SYMBOLS = ("pm_mesh_depth_render_groups_f32", "pm_mesh_frame_render_groups_f32", "pm_body_pose_gather_f32")


@pytest.fixture(scope="module")
def groups(tmp_path_factory):
    return DS.load_groups(tmp_path_factory.mktemp("cabinets"))[1]


def camera(groups, **kw):
    from partmanip_amd.mesh2depth import DepthFromMesh
    intr = np.array([[60.0, 0, 20.0], [0, 60.0, 12.0], [0, 0, 1]])
    kw.setdefault("meshes", [D.finger_mesh()])
    return DepthFromMesh(5, "cpu", np.stack([D.look_at((0.3, 0.1, 0.2))]), intr, 24, 40, groups=groups, **kw)


# ------------------------------------------------------------------------------------------- DepthFromMesh(groups=)
def test_slots_groups_and_face_ranges(groups):
    cam = camera(groups, group_of=DS.GROUP_OF)
    want = DS.concat_groups([D.finger_mesh()], groups)
    assert cam.num_shared == 1 and cam.part_num == 1 + 7 == want["part_num"]
    assert cam.face_shared == 624 == want["F_shared"] and cam.group_off.tolist() == [0, 24, 108, 408] == want["group_off"].tolist()
    assert cam.max_group_faces == 300
    assert np.array_equal(cam.verts.numpy(), want["verts"]) and np.array_equal(cam.faces.numpy(), want["faces"])
    part = cam.vert_part.numpy()
    assert np.array_equal(part, want["vert_part"])
    faces = cam.faces.numpy()
    assert (part[faces[:624]] == 0).all()                                                 # the shared part
    assert sorted(set(part[faces[624:648]].ravel())) == [1, 2]                            # cabinet A: bodies 0, 1
    assert sorted(set(part[faces[648:732]].ravel())) == list(range(1, 8))                 # cabinet B: seven bodies
    assert sorted(set(part[faces[732:]].ravel())) == [2]                                  # cabinet S: body 0 has no mesh
    assert (part[faces].min(axis=1) == part[faces].max(axis=1)).all()                     # a face lies in one slot
    assert cam.group_of.tolist() == DS.GROUP_OF.tolist() and cam.group_of.dtype == np.int32
    assert tuple(cam.palette.shape) == (8, 3) and cam.labels is None
    assert camera(groups).group_of.tolist() == [0, 1, 2, 0, 1]                            # the default: env % num_objs
    assert camera(groups, meshes=[]).face_shared == 0


def test_bad_tables_are_refused_before_the_device(groups):
    with pytest.raises(ValueError, match="group_of"):
        camera(groups, group_of=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError, match="group_of"):
        camera(groups, group_of=[0, 1, -2, 0, 0])
    with pytest.raises(ValueError, match="group_of"):
        camera(groups, group_of=[0, 1, 2])
    with pytest.raises(ValueError, match="labels"):
        camera(groups, labels=[1] * 7)
    with pytest.raises(ValueError, match="groups"):
        camera(None, group_of=[0] * 5)
    with pytest.raises(ValueError, match=r"groups\[0\]\[1\]"):
        camera([[None, (np.zeros((3, 3)), np.array([[0, 1, 3]]))]])
    cam = camera(groups, group_of=DS.GROUP_OF)
    R, T = torch.zeros(2, 8, 3, 3), torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="group_of="):                                    # a slice needs its own group_of
        cam.render(R, T)
    with pytest.raises(ValueError, match="group_of"):
        cam.render(R, T, group_of=[0, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # ... and with one it reaches the device check
        cam.render(R, T, group_of=[0, -1])
    with pytest.raises(ValueError, match="pose_R"):
        cam.render(torch.zeros(5, 2, 3, 3), torch.zeros(5, 2, 3))
    from partmanip_amd.mesh2depth import DepthFromMesh
    plain = DepthFromMesh(5, "cpu", np.stack([D.look_at((0.3, 0.1, 0.2))]), np.eye(3), 24, 40, meshes=[D.finger_mesh()])
    with pytest.raises(ValueError, match="without groups"):
        plain.render(torch.zeros(5, 1, 3, 3), torch.zeros(5, 1, 3), group_of=[0] * 5)


def test_face_groups_validates_host_tables():
    from partmanip_amd.ops import face_groups
    off, eg, G, most = face_groups([0, 24, 108, 408], DS.GROUP_OF, 1032, 624, 5, "cpu")
    assert (G, most) == (3, 300) and off.dtype == eg.dtype == torch.int32 and off.tolist() == [0, 24, 108, 408]
    assert face_groups([0], [-1] * 5, 624, 624, 5, "cpu")[2:] == (0, 0)
    for bad_off, bad_eg, F, Fs in (([1, 24, 408], [0] * 5, 1032, 624), ([0, 30, 24, 408], [0] * 5, 1032, 624), ([0, 24, 407], [0] * 5, 1032, 624),
                                   ([0, 24, 408], [0, 1, 2, 0, 0], 1032, 624), ([0, 24, 408], [0, -2, 0, 0, 0], 1032, 624),
                                   ([0, 24, 408], [0] * 4, 1032, 624), ([0, 408], [0] * 5, 1032, 1033), ([0.0, 408.0], [0] * 5, 1032, 624)):
        with pytest.raises(ValueError):
            face_groups(bad_off, bad_eg, F, Fs, 5, "cpu")
    with pytest.raises(ValueError, match="max_group_faces"):
        face_groups([0, 24, 108, 408], DS.GROUP_OF, 1032, 624, 5, "cpu", max_group_faces=299)


# ------------------------------------------------------------------------------------------- the environment's row table
def test_scene_row_table():
    from partmanip_amd.envs import scene_row_table
    # N = 5 environments over 3 objects of 2, 7 and 2 bodies (env % 3), a robot of 17 bodies of which 3 are posed
    bodies = np.array([2, 7, 2, 2, 7])
    rb_row0 = np.concatenate([[0], np.cumsum(17 + bodies)[:-1]])
    rows = scene_row_table([0, 4, 16], rb_row0, rb_row0 + 17, bodies, max_bodies=7)
    assert rows.shape == (5, 10) and rows.dtype == np.int32
    assert rows[0].tolist() == [0, 4, 16, 17, 18, -1, -1, -1, -1, -1]
    assert rows[1].tolist() == [19, 23, 35] + list(range(36, 43))
    assert rows[3].tolist() == [62, 66, 78, 79, 80, -1, -1, -1, -1, -1]
    assert rows[4, 3:].tolist() == list(range(98, 105))
    used = rows[rows >= 0]
    assert np.unique(used).size == used.size and used.max() < (17 + bodies).sum()
    assert scene_row_table([0], [0, 10], [5, 15], [2, 1]).tolist() == [[0, 5, 6], [10, 15, -1]]
    with pytest.raises(ValueError, match="max_bodies"):
        scene_row_table([0], [0], [1], [3], max_bodies=2)


def test_env_builds_the_row_table_of_its_sim(groups):
    """make_open_drawer_env's own table is scene_row_table over the sim's rows; without a device only its host inputs are compared:
    the layout of kinematics.KinematicSim (robot rows, then the object's) is what tasks.open_drawer.build_masks lays out."""
    from partmanip_amd.envs import scene_row_table
    from partmanip_amd.tasks.open_drawer import build_masks
    bodies = np.array([2, 7, 2, 2, 7])
    rb, _, B, _ = build_masks(17, 12, bodies, [1, 3, 1, 1, 3], [1, 4, 1, 1, 4], [1, 5, 1, 1, 5], [0] * 5)
    rows = scene_row_table(np.arange(17), rb[:, 0], rb[:, 0] + 17, bodies)
    assert np.array_equal(rows[:, :17], rb[:, :17])
    for e in range(5):
        assert rows[e, 17 + int([1, 4, 1, 1, 4][e])] == rb[e, -2] and rows[e, 17 + int([1, 5, 1, 1, 5][e])] == rb[e, -1]
    assert rows.max() == B - 1


# ------------------------------------------------------------------------------------------- the definition, in numpy
def test_subset_image_equals_the_all_in_one_scene_with_nan_poses(groups):
    """What the grouped entries are defined to compute -- render_f32 of an environment's own rows -- is the image the ungrouped
    definition gives for the whole library in one scene when the absent objects carry NaN poses (a non-finite corner skips the
    triangle).  Pins the definition without a device."""
    sc = DS.raw_scene(groups)
    sc["group_bodies"] = [len(g) for g in groups]
    own = DS.subset_depth(sc)
    part, R, T = DS.all_in_one(sc)
    whole = D.render_f32(sc["verts"], part, sc["faces"], R, T, **{k: sc[k] for k in DS.CAMERA_KEYS})
    assert own.tobytes() == whole.tobytes()
    hit = own < sc["far"]
    assert hit.mean() > 0.05                                                              # the scene is in view
    only_shared = DS.subset_depth(sc, env_group=np.full(5, -1))
    assert np.array_equal(own[4], only_shared[4]) and all((own[b] != only_shared[b]).any() for b in range(4))
    assert (own[0] != own[3]).any()                                                       # same cabinet, other poses
    # the fixture's block structure: 624 shared rows end inside block 2, the 300-row group crosses 768 and ends at 924
    assert sc["F_shared"] % 256 != 0 and sc["F_shared"] // 256 == (sc["F_shared"] + 23) // 256
    lo, hi = sc["F_shared"], sc["F_shared"] + 300
    assert lo < 768 < hi and hi % 256 != 0


# ------------------------------------------------------------------------------------------- the C ABI
def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import ctypes
    from partmanip_amd import _lib
    fns = header_functions()
    for name, nargs in zip(NEW_SYMBOLS, (27, 41, 10)):
        assert fns[name] == ("int", nargs), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 163 == _lib.lib.pm_version()
    # the grouped entries are the ungrouped ones plus (F_shared, group_off, G, env_group, max_group_faces) after F
    for base in ("depth", "frame"):
        old, new = (_lib.SIGNATURES[f"pm_mesh_{base}_render{s}_f32"][1] for s in ("", "_groups"))
        assert new == old[:5] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + old[5:]


def test_new_entries_refuse_bad_arguments_before_any_launch():
    from partmanip_amd._lib import lib
    one = 1                                                   # any non-NULL pointer: nothing is launched or read
    depth = lambda F_shared, off, G, eg, most: lib.pm_mesh_depth_render_groups_f32(                     # noqa: E731
        one, one, 3, one, 10, F_shared, off, G, eg, most, one, one, 1, 1, one, 1, 1.0, 1.0, 0.0, 0.0, 4, 4, 0.01, 100.0, one, 16, None)
    assert depth(11, one, 1, one, 0) == -1 and depth(-1, one, 1, one, 0) == -1
    assert depth(5, one, -1, one, 0) == -1 and depth(5, one, 1, one, -1) == -1
    assert depth(5, None, 1, one, 5) == -1 and depth(5, one, 1, None, 5) == -1
    assert lib.pm_mesh_depth_render_groups_f32(None, one, 3, one, 10, 5, one, 1, one, 5, one, one, 1, 1, one, 1, 1.0, 1.0, 0.0, 0.0, 4, 4,
                                               0.01, 100.0, one, 16, None) == -1
    assert lib.pm_mesh_depth_render_groups_f32(one, one, 3, one, 10, 5, one, 1, one, 5, one, one, 2 ** 30, 1, one, 4, 1.0, 1.0, 0.0, 0.0, 4,
                                               4, 0.01, 100.0, one, 64, None) == -1           # a grid that does not fit
    frame = lambda F_shared, off, G, most: lib.pm_mesh_frame_render_groups_f32(                         # noqa: E731
        one, one, 3, one, 10, F_shared, off, G, one, most, one, one, 1, 1, one, 1, 1.0, 1.0, 0.0, 0.0, 4, 4, 0.01, 100.0, None, -1, one,
        0.25, 0.75, 255, 255, 255, one, 16, None, 0, None, 0, one, 128, None)
    assert frame(11, one, 1, 0) == -1 and frame(5, None, 1, 5) == -1 and frame(5, one, -1, 5) == -1 and frame(5, one, 1, -1) == -1
    gather = lib.pm_body_pose_gather_f32
    assert gather(None, 4, one, 1, 1, None, 0, one, one, None) == -1 and gather(one, 0, one, 1, 1, None, 0, one, one, None) == -1
    assert gather(one, 4, one, 1, 2, None, 1, one, one, None) == -1 and gather(one, 4, one, 1, 2, one, 3, one, one, None) == -1
    assert gather(one, 4, one, 0, 2, None, 0, one, one, None) == -1


def test_new_ops_refuse_cpu_tensors():
    from partmanip_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.body_pose_gather(torch.zeros(4, 13), torch.zeros(1, 2, dtype=torch.int32))
