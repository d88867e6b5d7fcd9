"""The grouped cameras on the GPU: every environment draws the shared parts and its own cabinet (pm_mesh_depth_render_groups_f32,
pm_mesh_frame_render_groups_f32), the poses of a whole scene from one launch (pm_body_pose_gather_f32), and the closed loop of
make_open_drawer_env(scene_meshes=).  Every image check is an equality: the definition is order-free (tests/depth_render_ref,
tests/frame_render_ref evaluate it in numpy float32 over an environment's own face subset).  The one tolerance is body_pose_gather's
bare slots against a float64 quaternion-to-matrix: 4 x the error of a numpy float32 evaluation of the same association; the observed
ratio goes to the margins file (profiles/drawer_scene_margins.json keeps the first run's)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import drawer_scene_fixtures as DS
from tests import frame_render_ref as FR
from tests import kinematic_episode as E
from tests import mesh_bake_ref as MB
from tests.helpers import GOLDEN, npy, record_margin, same_bits, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
MOBILE_URDF = os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf")


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    return DS.load_groups(tmp_path_factory.mktemp("cabinets"))             # (assets, groups)


@pytest.fixture(scope="module")
def scene(loaded):
    sc = DS.raw_scene(loaded[1])
    sc["want"] = DS.subset_depth(sc)
    sc["want"].setflags(write=False)
    return sc


def dev(sc):
    return {k: t(sc[k], device=DEV) for k in ("verts", "vert_part", "faces", "R", "T", "cam_pose")}


def depth_groups(sc, d=None, group_off=None, env_group=None, **kw):
    from partmanip_amd import ops
    d = d or dev(sc)
    out = ops.mesh_depth_render_groups(d["verts"], d["vert_part"], d["faces"], sc["F_shared"], sc["group_off"] if group_off is None else
                                       group_off, sc["env_group"] if env_group is None else env_group, d["R"], d["T"], d["cam_pose"],
                                       sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["H"], sc["W"], sc["near"], sc["far"], **kw)
    return npy(out).reshape(len(sc["R"]), -1, sc["H"], sc["W"])


# ------------------------------------------------------------------------------------------- 1. the depth camera
def test_depth_equals_the_definition_on_every_environments_own_subset(scene):
    got = depth_groups(scene)
    assert same_bits(got, scene["want"])
    assert (got < scene["far"]).mean() > 0.05
    assert same_bits(depth_groups(scene), got)                                            # the bits repeat
    # the same tables already on the device, with the bound the host would have computed, and with a larger one
    i32 = lambda a: t(np.asarray(a, dtype=np.int32), device=DEV)                         # noqa: E731
    for most in (300, 1000):
        assert same_bits(depth_groups(scene, group_off=i32(scene["group_off"]), env_group=i32(scene["env_group"]), max_group_faces=most), got)
    # written into the head of a wider row: the tail is left alone
    from partmanip_amd import ops
    d = dev(scene)
    n = got[0].size
    rows = torch.full((5, n + 3), -7.0, device=DEV)
    ops.mesh_depth_render_groups(d["verts"], d["vert_part"], d["faces"], scene["F_shared"], scene["group_off"], scene["env_group"], d["R"],
                                 d["T"], d["cam_pose"], scene["fx"], scene["fy"], scene["cx"], scene["cy"], scene["H"], scene["W"],
                                 scene["near"], scene["far"], out=rows)
    assert same_bits(npy(rows[:, :n]).reshape(got.shape), got) and bool((rows[:, n:] == -7.0).all())


def test_depth_without_a_shared_range(loaded):
    sc = DS.raw_scene(loaded[1], shared=[])
    assert sc["F_shared"] == 0 and sc["part_num"] == 7
    got = depth_groups(sc)
    assert same_bits(got, DS.subset_depth(sc))
    assert (got[4] == F32(sc["far"])).all() and (got[:4] < sc["far"]).any(axis=(1, 2, 3)).all()


def test_depth_with_an_empty_group(loaded):
    groups = loaded[1] + [[None, None, None]]
    sc = DS.raw_scene(groups, group_of=[3, 1, 2, 0, 3])
    assert sc["group_off"].tolist() == [0, 24, 108, 408, 408]
    got = depth_groups(sc)
    assert same_bits(got, DS.subset_depth(sc))
    shared_only = DS.subset_depth(sc, env_group=np.full(5, -1))
    assert same_bits(got[[0, 4]], shared_only[[0, 4]]) and not same_bits(got[1], shared_only[1])


def test_depth_with_no_group_anywhere_is_the_existing_entry_on_the_shared_faces(scene):
    from partmanip_amd import ops
    none = np.full(5, -1, dtype=np.int32)
    got = depth_groups(scene, env_group=none)
    assert same_bits(got, DS.subset_depth(scene, env_group=none))
    d = dev(scene)
    old = ops.mesh_depth_render(d["verts"], d["vert_part"], d["faces"][:scene["F_shared"]].contiguous(), d["R"], d["T"], d["cam_pose"],
                                scene["fx"], scene["fy"], scene["cx"], scene["cy"], scene["H"], scene["W"], scene["near"], scene["far"])
    assert same_bits(npy(old).reshape(got.shape), got)
    # G = 0 (a one-entry table on the device, which nothing reads): every id is out of range
    i32 = lambda a: t(np.asarray(a, dtype=np.int32), device=DEV)                         # noqa: E731
    assert same_bits(depth_groups(scene, group_off=i32([0]), env_group=i32(scene["env_group"]), max_group_faces=0), got)


def test_depth_a_bad_table_on_the_device_reads_nothing_out_of_range(scene):
    """Host tables are validated by the wrapper; tables that are already on the device are not read there, so the kernel clamps:
    a group id outside [-1, G) draws the shared faces only, a group's rows are cut to [F_shared, F) and to max_group_faces."""
    i32 = lambda a: t(np.asarray(a, dtype=np.int32), device=DEV)                         # noqa: E731
    ids = np.array([3, 1, -5, 2 ** 31 - 1, 0], dtype=np.int32)
    got = depth_groups(scene, group_off=i32(scene["group_off"]), env_group=i32(ids), max_group_faces=300)
    as_none = np.where((ids >= 0) & (ids < 3), ids, -1)
    assert same_bits(got, DS.subset_depth(scene, env_group=as_none))
    assert same_bits(got[[0, 2, 3]], DS.subset_depth(scene, env_group=np.full(5, -1))[[0, 2, 3]])
    # offsets below 0 and past F - F_shared: group 0 becomes rows [0, 24), group 1 rows [24, 408) of the group range
    clamped = dict(scene, group_off=np.array([0, 24, 408], dtype=np.int32))
    got = depth_groups(scene, group_off=i32([-7, 24, 10 ** 6]), env_group=i32([0, 1, 1, 0, -1]), max_group_faces=1000)
    assert same_bits(got, DS.subset_depth(clamped, env_group=np.array([0, 1, 1, 0, -1])))
    # a bound below the largest group: the first rows of the group, nothing else
    got = depth_groups(scene, group_off=i32(scene["group_off"]), env_group=i32(scene["env_group"]), max_group_faces=50)
    cam = {k: scene[k] for k in DS.CAMERA_KEYS}
    want = np.concatenate([D.render_f32(scene["verts"], scene["vert_part"], scene["faces"][DS.env_rows(scene, b, max_group_faces=50)],
                                        scene["R"][b:b + 1], scene["T"][b:b + 1], **cam) for b in range(5)])
    assert same_bits(got, want)


def test_wrappers_refuse_bad_host_tables(scene):
    with pytest.raises(ValueError, match="group_off"):
        depth_groups(scene, group_off=[0, 24, 108, 407])
    with pytest.raises(ValueError, match="env_group"):
        depth_groups(scene, env_group=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError, match="max_group_faces"):
        depth_groups(scene, group_off=t(scene["group_off"], device=DEV), env_group=t(scene["env_group"], device=DEV))


# ------------------------------------------------------------------------------------------- 2. the frame camera
def test_frame_equals_the_definition_on_every_environments_own_subset(scene, loaded):
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc = scene
    intr = np.array([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]])
    labels = [5, 1, 2, 3, 1, 2, 3, 9]
    small = [[None if m is None else (np.asarray(m[0], dtype=F32) * F32(0.15), m[1]) for m in bodies] for bodies in loaded[1]]
    cam = DepthFromMesh(5, DEV, sc["cam_pose"], intr, sc["H"], sc["W"], meshes=[D.finger_mesh()], groups=small, group_of=sc["env_group"],
                        labels=labels, miss_label=-3)
    assert same_bits(npy(cam.verts), sc["verts"]) and np.array_equal(npy(cam.faces), sc["faces"])
    R, T = t(sc["R"], device=DEV), t(sc["T"], device=DEV)
    frame = cam.render_frame(R, T)
    kw = {k: sc[k] for k in DS.CAMERA_KEYS}
    for b in range(5):
        rows = DS.env_rows(sc, b)
        depth, face, seg, rgb = FR.frame_f32(sc["verts"], sc["vert_part"], sc["faces"][rows], sc["R"][b:b + 1], sc["T"][b:b + 1],
                                             part_label=labels, miss_label=-3, **kw)
        assert same_bits(npy(frame.depth[b]), depth[0]), b
        assert np.array_equal(npy(frame.seg[b]), seg[0]) and np.array_equal(npy(frame.rgb[b]), rgb[0]), b
    assert same_bits(npy(frame.depth), sc["want"]) and same_bits(npy(cam.render(R, T)), sc["want"])
    seen = set(np.unique(npy(frame.seg)))
    assert {-3, 5} <= seen and seen & {1, 2, 3}
    # a one-environment slice with its own group_of: the recorder's call
    one_host = cam.render_frame(R[1:2], T[1:2], depth=False, seg=False, group_of=[1])
    assert torch.equal(one_host.rgb[0], frame.rgb[1])
    one = cam.render(R[2:3], T[2:3], group_of=cam._group_of[2:3])
    assert torch.equal(one[0], frame.depth[2])
    dev = cam.render_frame(R[1:2], T[1:2], depth=False, seg=False, group_of=cam._group_of[1:2])    # ... and as an int32 device tensor
    assert dev.rgb.dtype == torch.uint8 and torch.equal(dev.rgb[0], frame.rgb[1]) and torch.equal(dev.rgb, one_host.rgb)


# ------------------------------------------------------------------------------------------- 3. body poses, 4. the closed loop
def quat_to_mat(q, dtype):
    """torch_jit_utils.py:375-403 in numpy of the given dtype, in the kernels' association."""
    q = np.asarray(q, dtype=dtype)
    i, j, k, r = (q[..., c] for c in range(4))
    two_s = dtype(2) / (((i * i + j * j) + k * k) + r * r)
    m = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r), two_s * (i * j + k * r),
                  1 - two_s * (i * i + k * k), two_s * (j * k - i * r), two_s * (i * k - j * r), two_s * (j * k + i * r),
                  1 - two_s * (i * i + j * j)], axis=-1)
    assert m.dtype == dtype
    return m.reshape(q.shape[:-1] + (3, 3))


N = 5
CAM_INTR = np.array([[36.0, 0, 20.0], [0, 36.0, 12.0], [0, 0, 1]])
IM_H, IM_W = 24, 40


@pytest.fixture(scope="module")
def loop(loaded, tmp_path_factory):
    """make_open_drawer_env(scene_meshes=) over the three cabinets with depth_img and depth_tsdf observers and a recorder of
    environment 1; reset, then three steps of an opening action.  Everything the tests compare, read back once."""
    from partmanip_amd.depth2tsdf import TSDFVolume
    from partmanip_amd.envs import depth_img_observer, depth_tsdf_observer, frame_recorder, make_open_drawer_env
    from partmanip_amd.mesh2depth import DepthFromMesh
    from partmanip_amd.urdf import load_urdf
    assets, groups = loaded
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)["mobile"]}, "explore_step": 40, "maxEpisodeLength": 200, "random_reset": False}
    nr = len(load_urdf(MOBILE_URDF).robot_kwargs()["mesh_bodies"])
    robot = [D.finger_mesh()] + [MB.box_mesh((0.04, 0.03, 0.05), (0.0, 0.0, 0.0))] * (nr - 1)
    obj_id = np.arange(N) % 3
    cam_pose = np.stack([D.look_at((0.7, 1.0, 1.3), (-0.5, 0.0, 0.7)), D.look_at((0.9, -0.5, 1.0), (-0.5, 0.0, 0.7))])
    cam = DepthFromMesh(N, DEV, cam_pose, CAM_INTR, IM_H, IM_W, meshes=robot, groups=groups, group_of=obj_id)
    vol = TSDFVolume(DEV, 2.0, 20, (-1.5, -1.0, 0.0))
    vol.register_camera(cam_pose, CAM_INTR, IM_H, IM_W, N)
    env = make_open_drawer_env(cfg, N, DEV, MOBILE_URDF, assets, E.DT, hold="always", scene_meshes=groups, recorder=frame_recorder(cam, env=1),
                               observers={"depth_img": depth_img_observer(cam), "depth_tsdf": depth_tsdf_observer(cam, vol)})
    snap = lambda obs: dict(img=npy(obs["depth_img"]).copy(), tsdf=obs["depth_tsdf"].clone(),                      # noqa: E731
                            R=npy(env.compute_scene_pose()[0]).copy(), T=npy(env.compute_scene_pose()[1]).copy(),
                            task_R=npy(env.task.pose_R).copy(), task_T=npy(env.task.pose_T).copy(), rb=npy(env.sim.rigid_body).copy(),
                            q=npy(env.task.part_dof_state)[:, 0].copy(),
                            integ=vol.integrate(obs["depth_img"].reshape(N, 2, IM_H, IM_W)).reshape(N, -1).clone(),
                            frame=cam.render_frame(*env.compute_scene_pose()))
    first = snap(env.reset())
    bb = npy(env.task.part_bbox).astype(np.float64)
    pull = bb[:, 0] - bb[:, 4]
    a = np.zeros((N, 10), dtype=np.float32)
    a[:, 3:6] = pull / np.linalg.norm(pull, axis=1, keepdims=True)
    png = os.path.join(tmp_path_factory.mktemp("frames"), "frame.png")
    for i in range(3):
        obs, _, reset, _ = env.step(t(a, device=DEV), save_image_path=png if i == 2 else None)
        assert not bool(reset.any())
    return dict(env=env, cam=cam, nr=nr, first=first, last=snap(obs), png=png, obj_id=obj_id, assets=assets, groups=groups, robot=robot)


def test_body_pose_gather_against_the_task_and_float64(loop):
    env, nr, s = loop["env"], loop["nr"], loop["last"]
    rows = npy(env.scene_rows)
    assert rows.shape == (N, nr + 7) and tuple(s["R"].shape) == (N, nr + 7, 3, 3)
    # the 13 slots the task poses as well: its robot parts, the target link and the handle -- the same bits
    link = nr + loop["assets"].target_link[loop["obj_id"]]
    handle = nr + loop["assets"].target_handle[loop["obj_id"]]
    e = np.arange(N)
    mine_R = np.concatenate([s["R"][:, :nr], s["R"][e, link][:, None], s["R"][e, handle][:, None]], axis=1)
    mine_T = np.concatenate([s["T"][:, :nr], s["T"][e, link][:, None], s["T"][e, handle][:, None]], axis=1)
    assert mine_R.shape[1] == nr + 2 == s["task_R"].shape[1] == 13
    assert torch.equal(torch.from_numpy(mine_R), torch.from_numpy(s["task_R"])) and torch.equal(torch.from_numpy(mine_T), torch.from_numpy(s["task_T"]))
    # NaN poses exactly where the table says -1
    empty = rows < 0
    assert empty.any() and empty[:, :nr].sum() == 0
    assert np.isnan(s["R"][empty]).all() and np.isnan(s["T"][empty]).all()
    assert np.isfinite(s["R"][~empty]).all() and np.isfinite(s["T"][~empty]).all()
    # every cabinet body: the position is the row's, the matrix quat_to_mat of its quaternion
    cab = ~empty
    cab[:, :nr] = False
    src = s["rb"].reshape(-1, 13)[rows[cab]]
    assert same_bits(s["T"][cab], src[:, :3])
    want = quat_to_mat(src[:, 3:7], np.float64)
    e_ref = np.abs(quat_to_mat(src[:, 3:7], np.float32).astype(np.float64) - want).max()
    err = np.abs(s["R"][cab].astype(np.float64) - want).max()
    print(f"body_pose_gather: {cab.sum()} cabinet bodies, err {err:.3e}, e_ref {e_ref:.3e}, ratio {err / max(e_ref, 1e-300):.3f}")
    record_margin("drawer scene body_pose_gather: cabinet rotation matrices / e_ref", err / max(e_ref, 1e-300), 4.0, worst_abs=float(err))
    assert e_ref > 0 and err <= 4 * e_ref


def own_image(loop, s, b):
    """render_f32 of environment b's own meshes (robot parts, then its cabinet's bodies) under the poses read back from the gather."""
    sc = DS.concat_groups(loop["robot"], [loop["groups"][loop["obj_id"][b]]])
    cam = loop["cam"]
    return D.render_f32(sc["verts"], sc["vert_part"], sc["faces"], s["R"][b:b + 1], s["T"][b:b + 1], npy(cam.cam_pose), cam.fx, cam.fy, cam.cx,
                        cam.cy, IM_H, IM_W, cam.near, cam.far)[0]


@pytest.mark.parametrize("when", ["first", "last"])
def test_closed_loop_every_environment_sees_its_own_cabinet(loop, when):
    s = loop[when]
    img = s["img"].reshape(N, 2, IM_H, IM_W)
    for b in range(N):
        want = own_image(loop, s, b)
        print(f"{when}: environment {b} (object {loop['obj_id'][b]}): {(want < 100).sum()} pixels hit")
        assert same_bits(img[b], want), b
    assert same_bits(img[0], img[3])                                                      # the same cabinet in the same state
    assert not same_bits(img[0], img[1]) and not same_bits(img[1], img[2])                # different cabinets
    assert torch.equal(s["tsdf"], s["integ"])                                             # depth_tsdf = integrate(that image)
    assert same_bits(npy(s["frame"].depth), img)


def test_closed_loop_the_held_drawer_moves_in_the_image(loop):
    first, last, nr = loop["first"], loop["last"], loop["nr"]
    assert (last["q"] > first["q"]).all()                                                 # the drawer opened
    link = nr + loop["assets"].target_link[loop["obj_id"]]
    seg = npy(first["frame"].seg)
    a, b = (s["img"].reshape(N, 2, IM_H, IM_W) for s in (first, last))
    masks = [seg[e] == link[e] for e in range(N)]
    for e, mask in enumerate(masks):
        print(f"environment {e}: {mask.sum()} pixels of the target link, {(a[e][mask] != b[e][mask]).sum()} changed")
    for e, mask in enumerate(masks):
        assert mask.sum() >= 4 and (a[e][mask] != b[e][mask]).any(), e


def test_closed_loop_the_recorder_writes_the_grouped_frame_of_its_environment(loop):
    got = FR.read_png(loop["png"])
    assert got.shape == (IM_H, IM_W, 3)
    assert np.array_equal(got, npy(loop["last"]["frame"].rgb[1, 0]))
    assert (got != 255).any()
