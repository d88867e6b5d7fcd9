"""The host side of the grouped mesh observers (TSDFfromMesh(groups=), PCfromMesh(groups=), mesh2sdf.bake_groups,
ops.mesh_tsdf_query_groups, pm_mesh_tsdf_query_groups_f32's argument checks): tables, refusals, and what the test scenes of the GPU
files exercise according to the fp64 restatement.  No GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import drawer_scene_fixtures as DS
from tests import mesh_bake_ref as MB
from tests import mesh_groups_scene as S
from tests.test_capi_symbols import header_functions


# ------------------------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree_on_the_new_entry():
    from partmanip_amd import _lib
    name = "pm_mesh_tsdf_query_groups_f32"
    assert header_functions()[name] == ("int", 30)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 30 and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 163 == _lib.lib.pm_version()
    # the ungrouped entry plus (grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids) after the part tables
    old = _lib.SIGNATURES["pm_mesh_tsdf_query_f32"][1]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert args == old[:5] + [P, I, I, P, I, P, I] + old[5:]


def test_the_entry_refuses_bad_arguments_before_any_launch():
    from partmanip_amd._lib import lib
    one = 1                                                   # any non-NULL pointer: nothing is launched or read
    call = lambda slot=one, NG=6, NGs=2, off=one, G=3, eg=one, most=3, B=6, M=5, t0=0, t1=5, res=10, stride=1000, trunc=0.2, f=one: \
        lib.pm_mesh_tsdf_query_groups_f32(f, one, one, one, one, slot, NG, NGs, off, G, eg, most, one, one, B, M, t0, t1, res, 0.05, 0.0, 0.0,   # noqa: E731
                                          0.0, trunc, one, 0, one, stride, 1, None)
    for kw in (dict(f=None), dict(slot=None), dict(off=None), dict(eg=None), dict(NG=0), dict(NGs=-1), dict(NGs=7), dict(G=-1), dict(most=-1),
               dict(t0=-1), dict(t0=5), dict(t0=2, t1=2), dict(t1=6), dict(B=0), dict(B=65536), dict(M=0), dict(res=0), dict(stride=999),
               dict(trunc=0.0)):
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------- ops
def cpu_call(sc, **kw):
    from partmanip_amd import ops
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    o = TSDFfromMesh(1, S.SIZE, S.RES, "cpu", sdf_dicts=sc["parts"])
    a = dict(grid_slot=sc["grid_slot"], NG_shared=sc["NG_shared"], group_off=sc["group_off"], env_group=sc["env_group"])
    extra = {k: kw.pop(k) for k in list(kw) if k not in a}
    a.update(kw)
    return ops.mesh_tsdf_query_groups(o.sdf_field, o.sdf_field_off, o.sdf_field_res, o.sdf_bbox_min, o.sdf_voxel_size, a["grid_slot"],
                                      a["NG_shared"], a["group_off"], a["env_group"], torch.from_numpy(sc["R"]), torch.from_numpy(sc["T"]),
                                      S.RES, S.SIZE / S.RES, o._origin3, o.sdf_trunc, o._ground, **extra)


def test_wrapper_validates_host_tables_and_has_no_cpu_path():
    sc = S.small_scene()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # good tables reach the device check
        cpu_call(sc)
    for kw, what in ((dict(group_off=[0, 1, 3, 5]), "group_off"), (dict(group_off=[1, 1, 4, 4]), "group_off"),
                     (dict(group_off=[0, 2, 1, 4]), "group_off"), (dict(env_group=[0, 1, 3, -1, 1, 0]), "env_group"),
                     (dict(env_group=[0, 1, -2, -1, 1, 0]), "env_group"), (dict(env_group=[0, 1]), "env_group"),
                     (dict(grid_slot=[0, 1, 2, 2, 5, 4]), "grid_slot"), (dict(grid_slot=[0, 1, 2, 2, -1, 4]), "grid_slot"),
                     (dict(grid_slot=[0, 1, 2]), "grid_slot"), (dict(NG_shared=7), "NG_shared"), (dict(NG_shared=-1), "NG_shared"),
                     (dict(max_group_grids=2), "max_group_grids")):
        with pytest.raises(ValueError, match=what):
            cpu_call(sc, **kw)


def test_face_groups_names_the_callers_arguments():
    from partmanip_amd.ops import face_groups
    off, eg, G, most = face_groups([0, 1, 4, 4], [0, 1, 2, -1, 1, 0], 6, 2, 6, "cpu", names=("NG", "NG_shared", "max_group_grids"))
    assert (G, most) == (3, 3) and off.tolist() == [0, 1, 4, 4] and eg.dtype == torch.int32
    with pytest.raises(ValueError, match="NG - NG_shared = 4"):
        face_groups([0, 1, 3], [0] * 6, 6, 2, 6, "cpu", names=("NG", "NG_shared", "max_group_grids"))
    with pytest.raises(ValueError, match="F - F_shared = 4"):                             # the cameras' wording is unchanged
        face_groups([0, 1, 3], [0] * 6, 6, 2, 6, "cpu")


# ------------------------------------------------------------------------------------------- TSDFfromMesh(groups=)
def tsdf(sc, **kw):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    p = sc["parts"]
    kw.setdefault("groups", [[p[2]], [p[3], None, p[4], p[5]], []])
    return TSDFfromMesh(6, S.SIZE, S.RES, "cpu", sdf_dicts=kw.pop("sdf_dicts", p[:2]), **kw)


def test_tsdf_tables():
    sc = S.small_scene()
    o = tsdf(sc, group_of=sc["env_group"])
    assert o.groups and o.num_shared == 2 and o.part_num == 2 + 4 and o.max_group_grids == 3
    assert o.grid_slot.tolist() == [0, 1, 2, 2, 4, 5] and o.group_off.tolist() == [0, 1, 4, 4]      # a body without a mesh gets no row
    assert o.group_of.tolist() == sc["env_group"].tolist() and o.group_of.dtype == np.int32
    assert o.sdf_field_off.numel() == 6 and tuple(o.sdf_field_res.shape) == (6, 3)
    assert o.sdf_field.numel() == sum(p['sdf'].size for p in sc["parts"])
    assert tsdf(sc).group_of.tolist() == [0, 1, 2, 0, 1, 2]                               # the default: env % num_objs
    assert tsdf(sc, sdf_dicts=[]).num_shared == 0


def test_tsdf_refusals():
    sc = S.small_scene()
    for bad in ([0, 1, 3, 0, 0, 0], [0, 1, -2, 0, 0, 0], [0, 1, 2]):
        with pytest.raises(ValueError, match="group_of"):
            tsdf(sc, group_of=bad)
    with pytest.raises(ValueError, match="groups"):
        tsdf(sc, groups=None, group_of=[0] * 6)
    with pytest.raises(ValueError, match="groups"):
        tsdf(sc, groups=[])
    with pytest.raises(ValueError, match=r"groups\[0\]\[1\]"):
        tsdf(sc, groups=[[None, {'sdf': np.zeros((4, 4, 4))}]])
    o = tsdf(sc, group_of=sc["env_group"])
    R, T = torch.zeros(2, 6, 3, 3), torch.zeros(2, 6, 3)
    with pytest.raises(ValueError, match="group_of="):                                    # a slice needs its own group_of
        o.query_tsdf(R, T)
    with pytest.raises(ValueError, match="group_of"):
        o.query_tsdf(R, T, group_of=[0, 3])
    with pytest.raises(ValueError, match="pose_R"):
        o.query_tsdf(torch.zeros(6, 5, 3, 3), torch.zeros(6, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.query_tsdf(R, T, group_of=[0, -1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.query_tsdf_seperately(torch.zeros(6, 6, 3, 3), torch.zeros(6, 6, 3))
    with pytest.raises(ValueError, match="query_tsdf_seperately"):
        tsdf(sc, sdf_dicts=[]).query_tsdf_seperately(torch.zeros(6, 4, 3, 3), torch.zeros(6, 4, 3))


def test_tsdf_without_groups_is_as_before():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    sc = S.small_scene()
    o = TSDFfromMesh(2, S.SIZE, S.RES, "cpu", sdf_dicts=sc["parts"])
    assert not o.groups and o.part_num == 6 and o.sdf_field_off.numel() == 6
    with pytest.raises(ValueError, match="without groups"):
        o.query_tsdf(torch.zeros(2, 6, 3, 3), torch.zeros(2, 6, 3), group_of=[0, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.query_tsdf(torch.zeros(2, 6, 3, 3), torch.zeros(2, 6, 3))


# ------------------------------------------------------------------------------------------- PCfromMesh(groups=)
K = 40
GROUP_OF = np.array([0, 1, 2, -1, 1, 0, 2, 0, -1, 1, 1], dtype=np.int32)


def cloud(**kw):
    from partmanip_amd.mesh2pc import PCfromMesh
    shared = [MB.box_mesh((0.04, 0.03, 0.05), (0.0, 0.0, 0.01)), DS.ellipsoid_mesh((0.05, 0.03, 0.04))]
    groups = [[MB.box_mesh((0.02, 0.05, 0.03), (0.0, 0.0, 0.0)), None, DS.ellipsoid_mesh((0.03, 0.03, 0.06))],
              [MB.box_mesh((0.06, 0.02, 0.02), (0.01, 0.0, 0.0))], [None, None]]
    kw.setdefault("meshes", shared)
    kw.setdefault("groups", groups)
    kw.setdefault("num_points", K)
    return PCfromMesh(len(GROUP_OF), "cpu", group_of=kw.pop("group_of", GROUP_OF), seed=7, **kw), shared, groups


def test_cloud_library_and_the_stated_seeds():
    from partmanip_amd import meshio
    pc, shared, groups = cloud()
    assert pc.groups and pc.part_num == 5 and pc.num_shared == 2 and pc.pts_shared == 2 * K
    assert pc.group_off.tolist() == [0, 2 * K, 3 * K, 3 * K] and pc.max_group_points == 2 * K and tuple(pc.pts.shape) == (5 * K, 3)
    assert pc.part_of.numpy().reshape(-1, K)[:, 0].tolist() == [0, 1, 2, 4, 2] and pc.part_of.dtype == torch.int32
    pts = pc.pts.numpy().reshape(-1, K, 3)
    want = [meshio.sample_surface(*shared[i], K, torch.Generator().manual_seed(7 + i))[0] for i in range(2)]
    want += [meshio.sample_surface(*groups[k][j], K, torch.Generator().manual_seed(7 + 4096 * (k + 1) + j))[0] for k, j in ((0, 0), (0, 2), (1, 0))]
    assert np.array_equal(pts, np.stack(want))
    assert pc.own_rows(-1).tolist() == list(range(2 * K)) and pc.own_rows(1).tolist() == list(range(2 * K)) + list(range(4 * K, 5 * K))
    ready, _, _ = cloud(groups=[[pts[2], None, pts[3]], [pts[4]], [None, None]])          # ready (p, 3) points in place of meshes
    assert np.array_equal(ready.pts.numpy(), pc.pts.numpy()) and np.array_equal(ready.part_of.numpy(), pc.part_of.numpy())


def test_group_sel_rows_lie_in_the_shared_range_or_the_environments_own_group():
    pc, _, _ = cloud()
    sel = pc.group_sel(generator=torch.Generator().manual_seed(3)).numpy()
    assert sel.shape == (len(GROUP_OF), K) and sel.dtype == np.int32
    lo = pc.pts_shared + pc.group_off[np.maximum(GROUP_OF, 0)]
    hi = np.where(GROUP_OF >= 0, pc.pts_shared + pc.group_off[np.maximum(GROUP_OF, 0) + 1], lo)
    shared = (sel >= 0) & (sel < pc.pts_shared)
    own = (sel >= lo[:, None]) & (sel < hi[:, None])
    assert (shared | own).all() and own[GROUP_OF == 0].any() and own[GROUP_OF == 1].any() and not own[GROUP_OF == 2].any()
    assert all(len(set(row)) == K for row in sel.tolist())                                # a permutation's head: no repeats
    for g in (0, 1, 2, -1):
        rows = sel[GROUP_OF == g]
        assert (rows == rows[0]).all()                                                    # one draw per object
    # the stated draw: for every object in turn, then once for 'no object', the head of a permutation of its own cloud
    gen = torch.Generator().manual_seed(3)
    for g in (0, 1, 2, -1):
        rows = pc.own_rows(g)
        assert np.array_equal(sel[np.flatnonzero(GROUP_OF == g)[0]], rows[torch.randperm(len(rows), generator=gen)[:K].numpy()])
    # a slice with its own group_of; the global generator when none is given
    torch.manual_seed(9)
    a = pc.group_sel(group_of=[1, -1]).numpy()
    torch.manual_seed(9)
    b = pc.group_sel().numpy()
    assert np.array_equal(a[0], b[1]) and np.array_equal(a[1], b[3])


def test_cloud_refusals():
    few = np.random.RandomState(1).uniform(-0.1, 0.1, size=(K - 1, 3))                    # ready points, one fewer than K
    pc, _, _ = cloud(meshes=[], groups=[[MB.box_mesh()], [None, few]], group_of=np.arange(len(GROUP_OF)) % 2)
    with pytest.raises(ValueError, match=rf"num_points {K} exceeds the {K - 1} points of the cloud of object 1"):
        pc.group_sel()
    with pytest.raises(ValueError, match="exceeds the 0 points of the cloud of object 2"):         # no shared cloud, and object 2 has no mesh
        cloud(meshes=[])[0].group_sel()
    pc, _, _ = cloud(meshes=[], groups=[[MB.box_mesh()]], group_of=np.where(GROUP_OF < 0, -1, 0))   # ... or environments without an object
    with pytest.raises(ValueError, match="without an object"):
        pc.group_sel()
    assert (pc.group_sel(group_of=[0, 0]).numpy() >= 0).all()
    ok, _, _ = cloud(num_points=K, meshes=[], groups=[[MB.box_mesh()], [DS.ellipsoid_mesh((0.1, 0.1, 0.1)), None]],
                     group_of=np.arange(len(GROUP_OF)) % 2)
    assert (ok.group_sel().numpy() >= 0).all()                                            # nobody asks for the 'no object' row
    pc, _, _ = cloud()
    R, T = torch.zeros(len(GROUP_OF), 5, 3, 3), torch.zeros(len(GROUP_OF), 5, 3)
    with pytest.raises(ValueError, match="fps.*groups"):
        pc.query_pc(R, T, select='fps')
    with pytest.raises(ValueError, match="select"):
        pc.query_pc(R, T, select='nearest')
    with pytest.raises(ValueError, match="group_of="):
        pc.query_pc(R[:2], T[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T, select='all')
    for bad in ([0] * 3, [3] + [0] * 10):
        with pytest.raises(ValueError, match="group_of"):
            cloud(group_of=bad)
    with pytest.raises(ValueError, match=r"groups\[0\]\[0\]"):
        cloud(groups=[[np.zeros((4, 2))]])


def test_cloud_without_groups_is_as_before():
    from partmanip_amd.envs import pc_observer
    from partmanip_amd.mesh2pc import PCfromMesh
    shared = [MB.box_mesh(), DS.ellipsoid_mesh((0.05, 0.03, 0.04))]
    pc = PCfromMesh(3, "cpu", num_points=K, meshes=shared, seed=7)
    assert not pc.groups and pc.part_num == 2 and tuple(pc.pts.shape) == (2 * K, 3)
    assert pc.part_of.tolist() == [0] * K + [1] * K
    with pytest.raises(ValueError, match="without groups"):
        pc.query_pc(torch.zeros(3, 2, 3, 3), torch.zeros(3, 2, 3), group_of=[0] * 3)
    with pytest.raises(ValueError, match="without groups"):
        pc.group_sel()
    with pytest.raises(ValueError, match="meshes"):
        PCfromMesh(3, "cpu", num_points=K, meshes=[])
    torch.manual_seed(4)
    ob = pc_observer(pc)
    torch.manual_seed(4)
    assert ob.width == 3 * K and torch.equal(ob.sel, torch.randperm(2 * K)[:K].to(torch.int32))
    grouped, _, _ = cloud()
    torch.manual_seed(4)
    ob = pc_observer(grouped)
    torch.manual_seed(4)
    assert ob.width == 3 * K and torch.equal(ob.sel, grouped.group_sel())


# ------------------------------------------------------------------------------------------- the three observers agree
def test_the_three_observers_lay_one_object_structure_out_alike():
    """3 objects of 1, 4 and 0 bodies, the second body of the 4-body object without a mesh, behind 2 shared parts, 6 environments."""
    from tests import depth_render_ref as D
    from partmanip_amd.mesh2depth import DepthFromMesh
    from partmanip_amd.mesh2pc import PCfromMesh
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    sc = S.small_scene()
    p = sc["parts"]
    box = [MB.box_mesh((0.02 + 0.01 * i, 0.03, 0.04), (0.0, 0.0, 0.01 * i)) for i in range(6)]       # 8 vertices, 12 faces each
    structure = lambda b: [[b[2]], [b[3], None, b[4], b[5]], []]                              # noqa: E731
    intr = np.array([[60.0, 0, 20.0], [0, 60.0, 12.0], [0, 0, 1]])

    def build(group_of):
        return (DepthFromMesh(6, "cpu", np.stack([D.look_at((0.3, 0.1, 0.2))]), intr, 24, 40, meshes=box[:2], groups=structure(box), group_of=group_of),
                TSDFfromMesh(6, S.SIZE, S.RES, "cpu", sdf_dicts=p[:2], groups=structure(p), group_of=group_of),
                PCfromMesh(6, "cpu", num_points=K, meshes=box[:2], groups=structure(box), group_of=group_of, seed=7))

    cam, grids, pc = build(sc["env_group"])
    for o in (cam, grids, pc):
        assert o.groups and o.num_shared == 2 and o.part_num == 2 + 4
        assert o.group_of.tolist() == sc["env_group"].tolist() and o.group_of.dtype == np.int32
        assert len(o.group_off) - 1 == 3
    # the rows of one body, per observer: 12 faces over 8 vertices, 1 grid, K points
    assert cam.group_off.tolist() == [0, 12, 48, 48] and grids.group_off.tolist() == [0, 1, 4, 4] and pc.group_off.tolist() == [0, K, 4 * K, 4 * K]
    assert (cam.max_group_faces, grids.max_group_grids, pc.max_group_points) == (36, 3, 3 * K)
    assert (cam.face_shared, pc.pts_shared) == (24, 2 * K)
    # every library row of body j names slot num_shared + j; the mesh-less body (slot 3) has no row anywhere: 6 bodies' rows in all
    slots = [0, 1, 2 + 0, 2 + 0, 2 + 2, 2 + 3]
    vert_slot, point_slot = cam.vert_part.numpy().reshape(-1, 8), pc.part_of.numpy().reshape(-1, K)
    assert tuple(cam.faces.shape) == (6 * 12, 3) and grids.sdf_field_off.numel() == 6 and tuple(pc.pts.shape) == (6 * K, 3)
    assert (vert_slot == np.asarray(slots)[:, None]).all() and vert_slot.shape[0] == 6
    assert grids.grid_slot.tolist() == slots
    assert (point_slot == np.asarray(slots)[:, None]).all() and point_slot.shape[0] == 6
    face_slot = cam.vert_part.numpy()[cam.faces.numpy()]
    assert (face_slot == np.repeat(slots, 12)[:, None]).all()
    # the default: env % num_objs, for all three
    for o in build(None):
        assert o.group_of.tolist() == [0, 1, 2, 0, 1, 2] and o.group_of.dtype == np.int32


# ------------------------------------------------------------------------------------------- bake_groups
def test_bake_groups_refuses_a_grid_of_2_to_the_31_cells_before_baking():
    from partmanip_amd.mesh2sdf import bake_grid_layout, bake_groups
    big = MB.box_mesh((2.0, 1.5, 1.0), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError) as e:
        bake_groups("cpu", [[None], [MB.box_mesh(), None, big]], 0.04, 0.002)
    msg = str(e.value)
    assert "groups[1][2]" in msg and "body 2 of object 1" in msg and "2^31" in msg
    fit = float(re.search(r"a voxel_size of ([0-9.e+-]+) or more fits", msg).group(1))
    assert 0.002 < fit < 0.004
    cells = lambda vs: int(np.prod(np.asarray(bake_grid_layout(big[0], 0.04, vs)[0], dtype=np.float64)))     # noqa: E731
    assert cells(0.002) >= 2 ** 31 > cells(fit * 1.001)
    assert bake_groups("cpu", [[None, None], []], 0.04, 0.002) == [[None, None], []]      # nothing to bake: no device is touched


# ------------------------------------------------------------------------------------------- what the GPU scenes exercise (fp64)
def test_small_scene_own_rows_change_a_fifth_of_the_voxels_or_more():
    sc = S.small_scene()
    assert S.RES % 4 != 0 and sc["M"] == 5 and sc["grid_slot"].tolist() == [0, 1, 2, 2, 3, 4]
    for b, g in enumerate(sc["env_group"]):
        own, shared = S.restate_own(sc, b), S.restate_own(sc, b, rows=[0, 1])
        changed = (np.abs(own - shared) > 1e-6).mean()
        assert (0.17 <= changed <= 0.45) if g in (0, 1) else changed == 0, (b, changed)


def test_boundary_scene_every_row_past_ordinal_63_changes_its_environment():
    sc = S.boundary_scene()
    assert sc["NG_shared"] == 63 and sc["M"] == 66 and [len(S.own_rows(sc, b)) for b in range(4)] == [66, 65, 64, 63]
    assert all(p['sdf'].shape == (8, 8, 8) for p in sc["parts"])
    for b in range(3):
        rows, full = S.own_rows(sc, b), S.restate_own(sc, b)
        for tt in range(63, len(rows)):
            without = S.restate_own(sc, b, rows=[r for r in rows if r != rows[tt]])
            assert (np.abs(without - full) > 1e-3).sum() >= 10, (b, tt)
