"""Frame camera on the GPU: DepthFromMesh.render_frame (pm_mesh_frame_render_f32, csrc/mesh_frame.hip) against the definition of the
three images evaluated in numpy float32 (tests/frame_render_ref.frame_f32), against the depth kernel in the same process, and through
KinematicEnv's recorder and depth_img observer.

The contract fixes every operation's rounding and the winner of a pixel (nearest, then the smaller row of `faces`), so every
comparison here is an equality of bytes: a difference is a bug in the kernel or in the reference, not something with a tolerance."""
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import frame_render_ref as FR
from tests import kinematic_episode as E
from tests import mesh_bake_ref as MB
from tests.helpers import bits, npy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25
EYE = np.eye(3, dtype=np.float32)


def t(x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype).to(DEV)                   # a copy: the shared scene arrays are read-only


def intrinsic(sc):
    return np.array([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]])


def scene_meshes():
    finger = D.finger_mesh()
    return [finger, finger, MB.box_mesh(D.BOX_HALF, (0.0, 0.0, 0.0))]


def frame_gpu(sc, part_label=None, miss_label=-1, palette=None, ambient=0.25, background=(255, 255, 255), **outs):
    """ops.mesh_frame_render on a scene dict of tests/depth_render_ref -> (depth, seg, rgb) numpy, shaped (B, V, H, W[, 3])."""
    from partmanip_amd import ops
    B, M, V, H, W = len(sc["R"]), sc["R"].shape[1], len(sc["cam_pose"]), sc["H"], sc["W"]
    ws = torch.empty(8 * B * V * H * W, dtype=torch.uint8, device=DEV)
    pal = FR.default_palette(M) if palette is None else np.asarray(palette, dtype=np.float32)
    d, s, c = ops.mesh_frame_render(t(sc["verts"]), t(sc["vert_part"]), t(sc["faces"]), t(sc["R"]), t(sc["T"]), t(sc["cam_pose"]),
                                    sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, sc["near"], sc["far"], ws,
                                    part_label=None if part_label is None else t(part_label, torch.int32), miss_label=miss_label,
                                    palette=t(pal), ambient=ambient, background=background, **outs)
    torch.cuda.synchronize()
    return (None if d is None else npy(d).reshape(B, V, H, W), None if s is None else npy(s).reshape(B, V, H, W),
            None if c is None else npy(c).reshape(B, V, H, W, 3))


def assert_frame(got, want, what=""):
    """got (depth, seg, rgb) against frame_f32's (depth, face, seg, rgb): the differing pixels are printed, then all must be zero."""
    depth, _, seg, rgb = want
    bad = [int((bits(got[0]) != bits(depth)).sum()), int((got[1] != seg).sum()), int((got[2] != rgb).any(axis=-1).sum())]
    print(f"{what} pixels that differ from frame_f32 (depth, seg, rgb): {bad} of {seg.size}")
    assert got[1].dtype == np.int32 and got[2].dtype == np.uint8
    assert bad == [0, 0, 0], what


# ------------------------------------------------------------------------------------------- 1. the seeded scene
def test_seeded_scene_equals_frame_f32_and_the_depth_kernel_and_repeats():
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc, depth, face, seg, rgb = FR.seeded_frame()
    cam = DepthFromMesh(3, DEV, sc["cam_pose"], intrinsic(sc), sc["H"], sc["W"], meshes=scene_meshes())
    R, T = t(sc["R"]), t(sc["T"])
    fr = cam.render_frame(R, T)
    first = [npy(x).copy() for x in fr]
    assert tuple(fr.depth.shape) == (3, 2, 24, 40) and fr.depth.dtype == torch.float32
    assert tuple(fr.seg.shape) == (3, 2, 24, 40) and fr.seg.dtype == torch.int32
    assert tuple(fr.rgb.shape) == (3, 2, 24, 40, 3) and fr.rgb.dtype == torch.uint8
    assert np.array_equal(bits(first[0]), bits(cam.render(R, T)))                          # the existing kernel, same process
    assert_frame(first, (depth, face, seg, rgb), "seeded scene:")
    ws = cam._keys.buf.data_ptr()
    second = cam.render_frame(R, T)
    assert cam._keys.buf.data_ptr() == ws and cam._keys.buf.numel() >= 8 * 3 * 2 * 24 * 40  # the workspace is reused
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), npy(b).view(np.uint8))                      # every byte repeats
    assert_frame(frame_gpu(sc), (depth, face, seg, rgb), "the op itself:")
    small = cam.render_frame(R[:1], T[:1])                                                  # b = 1 fits the workspace of b = 3
    assert cam._keys.buf.data_ptr() == ws and np.array_equal(npy(small.rgb), rgb[:1])


# ------------------------------------------------------------------------------------------- 2. the tie-break
def test_coincident_triangles_go_to_the_smaller_face_index():
    tri, want = D.dyadic_triangle()
    covered = want[0, 0] == 2.0
    assert covered.sum() == 21
    verts = np.concatenate([tri["verts"], tri["verts"]])
    base = dict(tri, verts=verts, vert_part=np.array([0, 0, 0, 1, 1, 1], dtype=np.int32), R=EYE[None, None].repeat(2, axis=1),
                T=np.zeros((1, 2, 3), dtype=np.float32))
    for faces, winner in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
        sc = dict(base, faces=np.array(faces, dtype=np.int32))
        got = frame_gpu(sc)
        assert (got[1][0, 0][covered] == winner).all() and (got[1][0, 0][~covered] == -1).all(), faces
        assert np.array_equal(bits(got[0]), bits(want))
        assert_frame(got, FR.frame_f32(**sc), f"coincident, faces {faces}:")


def test_pixels_exactly_on_a_shared_edge_go_to_the_smaller_face_index():
    """The dyadic triangle A (pixel centres (1, 1), (6, 1), (1, 6)) and its complement B in the square ((6, 1), (6, 6), (1, 6)),
    as two parts: the six pixel centres with r + c = 7 lie exactly on the shared edge and both triangles hit them at z = 2."""
    tri, _ = D.dyadic_triangle()
    verts = np.array([(-1.5, -1.5, 2.0), (1.0, -1.5, 2.0), (-1.5, 1.0, 2.0), (1.0, -1.5, 2.0), (1.0, 1.0, 2.0), (-1.5, 1.0, 2.0)], dtype=np.float32)
    base = dict(tri, verts=verts, vert_part=np.array([0, 0, 0, 1, 1, 1], dtype=np.int32), R=EYE[None, None].repeat(2, axis=1),
                T=np.zeros((1, 2, 3), dtype=np.float32))
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    square = (rr >= 1) & (rr <= 6) & (cc >= 1) & (cc <= 6)
    edge, a_side, b_side = square & (rr + cc == 7), square & (rr + cc < 7), square & (rr + cc > 7)
    assert edge.sum() == 6
    for part, faces in ((0, [[0, 1, 2]]), (1, [[3, 4, 5]])):                                # the premise: each alone hits the edge pixels
        alone = D.render_f32(**dict(base, faces=np.array(faces, dtype=np.int32)))[0, 0]
        assert (alone[edge] == 2.0).all() and np.array_equal(alone == 2.0, edge | (a_side if part == 0 else b_side))
    for faces, first_part in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
        sc = dict(base, faces=np.array(faces, dtype=np.int32))
        got = frame_gpu(sc)
        seg = got[1][0, 0]
        assert (seg[edge] == first_part).all(), faces
        assert (seg[a_side] == 0).all() and (seg[b_side] == 1).all() and (seg[~square] == -1).all()
        assert (got[0][0, 0][square] == 2.0).all()
        assert_frame(got, FR.frame_f32(**sc), f"shared edge, faces {faces}:")


# ------------------------------------------------------------------------------------------- 3. occlusion, labels, background
def test_a_small_part_in_front_of_a_large_one():
    from partmanip_amd.mesh2depth import DepthFromMesh
    finger, box = D.finger_mesh(), MB.box_mesh((0.004, 0.012, 0.004), (0.0, 0.0, 0.0))
    verts, vert_part, faces = D.concat_meshes([finger, box])
    centre = finger[0].mean(axis=0)
    T = np.array([[-centre + [0.0, 0.0, 0.30], [0.004, 0.003, 0.20]]], dtype=np.float32)
    sc = dict(verts=verts, vert_part=vert_part, faces=faces, R=EYE[None, None].repeat(2, axis=1), T=T, cam_pose=np.eye(4, dtype=np.float32)[None],
              fx=150.0, fy=150.0, cx=20.0, cy=12.0, H=24, W=40, near=0.01, far=100.0)
    nf = len(finger[1])
    far_hit = D.render_f32(**dict(sc, faces=faces[:nf]))[0, 0] < 100
    near_z = D.render_f32(**dict(sc, faces=faces[nf:]))[0, 0]
    near_hit = near_z < 100
    assert near_hit.sum() >= 20 and (far_hit & ~near_hit).sum() >= 20 and (near_hit & far_hit).sum() >= 20
    labels, miss, background = [5, 9], -3, (10, 20, 30)
    cam = DepthFromMesh(1, DEV, sc["cam_pose"], intrinsic(sc), 24, 40, meshes=[finger, box], labels=labels, miss_label=miss,
                        background=background, ambient=0.5)
    fr = cam.render_frame(t(sc["R"]), t(sc["T"]))
    got = [npy(x) for x in fr]
    seg, rgb = got[1][0, 0], got[2][0, 0]
    assert (seg[near_hit] == 9).all() and (seg[far_hit & ~near_hit] == 5).all() and (seg[~far_hit & ~near_hit] == miss).all()
    assert np.array_equal(bits(got[0][0, 0][near_hit]), bits(near_z[near_hit]))
    assert (rgb[seg == miss] == np.array(background, dtype=np.uint8)).all()
    assert (rgb[seg != miss] != np.array(background, dtype=np.uint8)).any(axis=-1).all()    # the palette has no such colour
    assert_frame(got, FR.frame_f32(**sc, part_label=labels, miss_label=miss, background=background, ambient=0.5), "occlusion:")


# ------------------------------------------------------------------------------------------- 4. shapes and views
def test_odd_sizes_three_views_out_view_and_outputs_switched_off():
    from partmanip_amd.mesh2depth import DepthFromMesh
    rng = np.random.RandomState(11)
    meshes = [D.finger_mesh(), MB.box_mesh((0.03, 0.05, 0.02), (0.0, 0.0, 0.0))]
    verts, vert_part, faces = D.concat_meshes(meshes)
    H, W, V, B = 7, 13, 3, 2
    cams = np.stack([D.look_at((0.2, -0.15, 0.2)), D.look_at((-0.1, 0.25, 0.15)), D.look_at((0.05, 0.05, 0.3), up=(0.0, 1.0, 0.0))])
    sc = dict(verts=verts, vert_part=vert_part, faces=faces, R=D.rotations(rng, (B, 2)),
              T=rng.uniform(-0.05, 0.05, size=(B, 2, 3)).astype(np.float32), cam_pose=cams, fx=21.0, fy=20.0, cx=6.5, cy=3.25, H=H, W=W,
              near=0.01, far=100.0)
    want = FR.frame_f32(**sc)
    assert 0.05 < (want[1] >= 0).mean() < 0.95 and all((want[1][:, v] >= 0).any() for v in range(V))
    cam = DepthFromMesh(B, DEV, cams, intrinsic(sc), H, W, meshes=meshes)
    R, T = t(sc["R"]), t(sc["T"])
    n, tail = V * H * W, 11
    buf = torch.full((B, n + tail), SENTINEL, device=DEV)
    fr = cam.render_frame(R, T, out_depth=buf[:, :n + 4])
    assert fr.depth.data_ptr() == buf.data_ptr() and tuple(fr.depth.shape) == (B, V, H, W)
    assert_frame([npy(x) for x in fr], want, "7 x 13, three views:")
    assert (buf[:, n:] == SENTINEL).all()
    for off in ("depth", "seg", "rgb"):
        part = cam.render_frame(R, T, **{off: False})
        for name, a, b in zip(("depth", "seg", "rgb"), part, fr):
            if name == off:
                assert a is None
            else:
                assert a.shape == b.shape and np.array_equal(npy(a).view(np.uint8), npy(b).view(np.uint8)), (off, name)
    only = cam.render_frame(R, T, depth=False, seg=False)
    assert only.depth is None and only.seg is None and np.array_equal(npy(only.rgb), want[3])


# ------------------------------------------------------------------------------------------- 5. skipped triangles
def test_bad_indices_and_a_nan_pose_never_reach_seg_or_rgb():
    sc, _, _, _, _ = FR.seeded_frame()
    NV, M = len(sc["verts"]), 3
    faces, vert_part, T = sc["faces"].copy(), sc["vert_part"].copy(), sc["T"].copy()
    faces[5, 1] = NV + 7                                     # one face index out of range
    faces[900, 2] = -1
    bad_vertex = int(sc["faces"][700, 0])
    vert_part[bad_vertex] = M + 2                            # one vert_part out of range
    T[1, 0, 2] = np.nan                                      # one NaN in one environment's pose_T
    bad = dict(sc, faces=faces, vert_part=vert_part, T=T)
    got = frame_gpu(bad)
    assert np.isfinite(got[0]).all() and set(np.unique(got[1])) <= {-1, 0, 1, 2}
    assert not (got[1][1] == 0).any()                        # environment 1: part 0 has the NaN pose
    drop = np.zeros(len(faces), dtype=bool)
    drop[[5, 900]] = True
    drop |= (sc["faces"] == bad_vertex).any(axis=1)
    part_of_face = sc["vert_part"][sc["faces"][:, 0]]
    for b in range(3):                                       # the scene without them: the same triangles dropped by hand
        d = drop | (part_of_face == 0) if b == 1 else drop
        clean = dict(sc, faces=sc["faces"][~d], R=sc["R"][b:b + 1], T=sc["T"][b:b + 1].copy())
        if b == 1:
            clean["T"][0, 0] = 0.0                           # part 0 has no triangle left; any finite pose will do
        assert_frame([g[b:b + 1] for g in got], FR.frame_f32(**clean), f"environment {b} against the clean scene:")
    want = FR.frame_f32(**bad)
    assert not np.isin(want[1], np.nonzero(drop)[0]).any()
    assert_frame(got, want, "the bad scene itself:")


# ------------------------------------------------------------------------------------------- 6. the near plane
def test_a_triangle_through_the_near_plane_is_tested_against_the_whole_image():
    verts = np.array([[-0.2, -0.1, 0.5], [0.3, -0.1, 0.5], [0.0, 0.2, -0.3],            # crosses z = near
                      [-0.2, -0.1, -0.5], [0.3, -0.1, -0.5], [0.0, 0.2, -0.4],          # wholly behind the camera
                      [-0.05, 0.0, 0.7], [0.1, 0.02, 0.8], [0.0, 0.1, 0.75]], dtype=np.float32)      # wholly in front
    faces = np.arange(9, dtype=np.int32).reshape(3, 3)
    base = dict(verts=verts, vert_part=np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], dtype=np.int32), R=EYE[None, None].repeat(3, axis=1),
                T=np.zeros((1, 3, 3), dtype=np.float32), cam_pose=np.eye(4, dtype=np.float32)[None], fx=30.0, fy=30.0, cx=16.0, cy=10.0,
                H=20, W=32, near=0.01, far=100.0)
    for pick, must_hit in (([0], True), ([1], False), ([0, 1, 2], True)):
        sc = dict(base, faces=faces[pick])
        want = FR.frame_f32(**sc)
        assert (want[1] >= 0).any() == must_hit
        assert_frame(frame_gpu(sc), want, f"near plane, faces {pick}:")


# ------------------------------------------------------------------------------------------- 7. the C ABI's refusals
def test_refusals_leave_the_outputs_untouched():
    from partmanip_amd import ops
    from partmanip_amd._lib import lib
    sc, _ = D.dyadic_triangle()
    n = 64
    depth = torch.full((1, n), SENTINEL, device=DEV)
    seg = torch.full((1, n), 12345, dtype=torch.int32, device=DEV)
    rgb = torch.full((1, 3 * n), 77, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(8 * n + 8, dtype=torch.uint8, device=DEV)
    arrays = [t(sc[k]) for k in ("verts", "vert_part", "faces", "R", "T", "cam_pose")]
    pal = t(FR.default_palette(1))

    def through_ops(workspace):
        ops.mesh_frame_render(*arrays, 4.0, 4.0, 4.0, 4.0, 8, 8, 0.01, 100.0, workspace, palette=pal, depth=depth, seg=seg, rgb=rgb)

    def through_lib(d, s, c, palette):
        v, vp, f, R, T, cam = (a.data_ptr() for a in arrays)
        return lib.pm_mesh_frame_render_f32(v, vp, 3, f, 1, R, T, 1, 1, cam, 1, 4.0, 4.0, 4.0, 4.0, 8, 8, 0.01, 100.0, None, -1, palette,
                                            0.25, 0.75, 255, 255, 255, d, n, s, n, c, 3 * n, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="PM_EWORKSPACE"):
        through_ops(ws[:8 * n - 8])
    with pytest.raises(RuntimeError, match="PM_EALIGN"):
        through_ops(ws[4:])
    assert through_lib(None, None, None, pal.data_ptr()) == -1
    assert through_lib(depth.data_ptr(), seg.data_ptr(), rgb.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (depth == SENTINEL).all() and (seg == 12345).all() and (rgb == 77).all()
    through_ops(ws)                                                                        # and the same call goes through when nothing is wrong
    torch.cuda.synchronize()
    assert (depth.reshape(8, 8)[1, 1] == 2.0) and (seg != 12345).all() and (rgb != 77).any()


# ------------------------------------------------------------------------------------------- 8. the environment
def test_recorder_writes_the_frame_and_depth_img_observer_fills_its_row(tmp_path):
    from partmanip_amd.envs import depth_img_observer, frame_recorder, make_grasp_cube_env
    from partmanip_amd.mesh2depth import DepthFromMesh
    N, H, W = 4, 16, 24
    tree, bp, dof = E.scene()

    def grasp_env(**kw):
        return make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, free_body_pose=E.CUBE_POSE, **kw)
    plain = grasp_env()                                                                   # no recorder: also tells where the hand is
    plain.reset()
    _, T0 = plain.task.compute_scene_pose()
    hand = npy(T0)[1, 9].astype(np.float64)
    intr = np.array([[40.0, 0, W / 2.0], [0, 40.0, H / 2.0], [0, 0, 1]])
    cam = DepthFromMesh(N, DEV, D.look_at(hand + (0.2, -0.15, 0.15), target=hand)[None], intr, H, W, meshes=[D.finger_mesh()] * 12)
    a = torch.zeros(N, 7, device=DEV)
    a[:, 2] = -1.0
    plain.step(a, save_image_path=str(tmp_path / "plain" / "0.png"))
    assert not (tmp_path / "plain").exists()                                              # without a recorder the path is ignored

    for observers in (None, {"depth_img": depth_img_observer(cam)}):
        env = grasp_env(recorder=frame_recorder(cam, env=1), observers=observers, add_proprio_obs=observers is not None)
        env.reset()
        folder = tmp_path / ("with" if observers else "without") / "Iter0"
        obs, _, _, _ = env.step(a, save_image_path=str(folder / "0.png"))
        R, T = env.task.compute_scene_pose()
        want = npy(cam.render_frame(R[1:2], T[1:2]).rgb[0, 0])
        got = FR.read_png(str(folder / "0.png"))
        assert got.shape == (H, W, 3) and np.array_equal(got, want)
        shown = (want != 255).any(axis=-1)
        print(f"pixels of the frame that show a part: {int(shown.sum())} of {H * W}, colours {len(np.unique(want[shown], axis=0))}")
        assert 10 <= shown.sum() < H * W and len(np.unique(want[shown], axis=0)) >= 2          # the hand is in the picture
        obs, _, _, _ = env.step(a, save_image_path=None)
        assert os.listdir(folder) == ["0.png"]                                            # nothing is written for None
        if observers:
            width = H * W
            assert env.num_obs["depth_img"] == width + env.num_obs["proprio_state"]
            R, T = env.task.compute_scene_pose()
            assert tuple(obs["depth_img"].shape) == (N, width + env.num_obs["proprio_state"])
            assert torch.equal(obs["depth_img"][:, :width], cam.render(R, T).reshape(N, width))
            assert torch.equal(obs["depth_img"][:, width:], obs["proprio_state"])
            assert (obs["depth_img"][:, :width] < 100).any()
    bare = grasp_env(observers={"depth_img": depth_img_observer(cam)})
    assert bare.num_obs["depth_img"] == H * W
