"""Depth camera over the posed part meshes (partmanip_amd.mesh2depth.DepthFromMesh, pm_mesh_depth_render_f32, partmanip_amd.camera),
everything that needs no GPU: the camera rig against the fixture made from the reference's own gen_camera_pose
(tests/golden/make_camera_golden.py), the definition of the image (tests/depth_render_ref.render_f32) against an independent fp64
ray caster and against the posed surface itself, the C ABI's argument checks and the host logic on the 'cpu' device.

Bounds.  Camera poses: both sides are fp64 with errors of ~1e-15, the bound is 1e-9 absolute.  Image against the fp64 caster, on the
pixels outside every triangle's boundary band (where a depth image is continuous; at most 2 % of the pixels may be left out): hit
or miss agrees everywhere, and the depth differs by at most 4 x the worst value observed on the CPU for the committed seed
(5.673e-07 m, so 2.27e-06 m).  Back-projected hit pixels lie on the posed surface within 4 x the observed worst distance
(8.526e-08 m, so 3.41e-07 m).  4 x is the project's margin convention; the observed values are kept in
profiles/mesh_depth_margins.json."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import mesh_bake_ref as MB
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def margins():
    with open(os.path.join(ROOT, "profiles", "mesh_depth_margins.json")) as f:
        return {m["name"]: m for m in json.load(f)["margins"]}


# ------------------------------------------------------------------------------------------- 1. the camera rig
@pytest.mark.parametrize("task", ("grasp_cube", "open_drawer"))
def test_gen_camera_pose_equals_the_reference_fixture(task):
    from partmanip_amd import camera
    with np.load(os.path.join(GOLDEN, "camera_poses_ref.npz")) as z:
        fx = {k: z[k] for k in z.files}
    look_at, radius, want = fx[task + "_look_at"], float(fx[task + "_radius"]), fx[task + "_pose_mat"]
    got = camera.gen_camera_pose(look_at, [tuple(r) for r in fx["alpha_range_list"]], fx["num_point_ver_list"].tolist(),
                                 int(fx["num_point_hor"]), tuple(fx["beta_range"]), radius)
    err = float(np.abs(got - want).max())
    print(f"{task}: max |gen_camera_pose - reference| = {err:.2e}")
    assert got.shape == want.shape == (3, 4, 4) and got.dtype == np.float64
    assert err <= 1e-9
    for pose in got:
        Rm, t = pose[:3, :3], pose[:3, 3]
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1) < 1e-12
        to_target = (look_at - t) / np.linalg.norm(look_at - t)
        assert np.abs(Rm[:, 2] - to_target).max() < 1e-12                       # the camera looks along +z at look_at
        assert abs(np.linalg.norm(look_at - t) - radius) < 1e-12
        assert np.array_equal(pose[3], [0, 0, 0, 1])
    # the shipped rig: hand_base.py:162-191
    poses, intr, h, w = camera.shipped_rig(dict(look_at=look_at.tolist(), radius=radius))
    assert np.array_equal(poses, got) and (h, w) == (288, 512)
    f = 512 / 2.0 / np.tan(np.deg2rad(69.75) / 2.0)
    assert np.allclose(intr, [[f, 0, 256], [0, f, 144], [0, 0, 1]], rtol=1e-15, atol=0)
    poses, intr, h, w = camera.shipped_rig(dict(look_at=look_at.tolist(), radius=radius), image_mode=True)
    assert np.array_equal(poses, got[:1]) and (h, w) == (72, 128)
    assert np.allclose(intr, [[f / 4, 0, 64], [0, f / 4, 36], [0, 0, 1]], rtol=1e-15, atol=0)
    assert not hasattr(camera, "scipy")


# ------------------------------------------------------------------------------------------- 2. the definition of the image
def test_render_f32_agrees_with_the_fp64_ray_caster_off_the_boundary_band():
    sc, z32, z64, band = D.seeded_scene_images()
    assert len(sc["faces"]) == 624 + 624 + 12 and z32.shape == (3, 2, 24, 40) and z32.dtype == np.float32
    far = sc["far"]
    hit32, hit64 = z32 < far, z64 < far
    keep = ~band
    both = hit32 & hit64 & keep
    worst = float(np.abs(z32.astype(np.float64) - z64)[both].max())
    observed = margins()["seeded scene: max |render_f32 - cast_f64| on non-band hits (m)"]["observed"]
    print(f"hits {hit64.mean():.3%}, band pixels {band.mean():.3%} ({band.sum()} of {band.size}), "
          f"hit/miss disagreements off the band {int(((hit32 != hit64) & keep).sum())}, worst |z32 - z64| = {worst:.3e} m "
          f"(recorded {observed:.3e}, tolerance {4 * observed:.3e})")
    assert 0.25 <= hit64.mean() <= 0.75 and 0.25 <= hit32.mean() <= 0.75
    assert band.mean() <= 0.01                                                  # the seed: the fp64 caster alone
    assert band.mean() <= 0.02
    assert np.array_equal(hit32[keep], hit64[keep])
    assert worst <= 4 * observed
    assert (z32[hit32] > sc["near"]).all() and (z32[~hit32] == np.float32(far)).all()


def test_hit_pixels_back_project_onto_the_posed_surface():
    """Independent of any ray formula: x = (u - cx) z / fx, y = (v - cy) z / fy, world = R_cam (x, y, z) + t (the reference's
    depth2tsdf.py:147-152) must lie on a posed triangle."""
    sc, z32, _, _ = D.seeded_scene_images()
    tri = D.posed_triangles64(sc["verts"], sc["vert_part"], sc["faces"], sc["R"], sc["T"])
    C = sc["cam_pose"].astype(np.float64)
    uu, vv = np.meshgrid(np.arange(sc["W"], dtype=np.float64), np.arange(sc["H"], dtype=np.float64))
    worst = 0.0
    for b in range(z32.shape[0]):
        for v in range(z32.shape[1]):
            z = z32[b, v].astype(np.float64)
            hit = z < sc["far"]
            local = np.stack([(uu - sc["cx"]) * z / sc["fx"], (vv - sc["cy"]) * z / sc["fy"], z], axis=-1)[hit]
            world = local @ C[v, :3, :3].T + C[v, :3, 3]
            d = np.sqrt(MB._tri_d2(world, tri[b]).min(axis=1))
            worst = max(worst, float(d.max()))
    observed = margins()["seeded scene: max distance of a back-projected hit pixel to the posed surface (m)"]["observed"]
    print(f"worst distance of a back-projected hit to the posed surface {worst:.3e} m (recorded {observed:.3e}, "
          f"tolerance {4 * observed:.3e})")
    assert worst <= 4 * observed


def test_known_answer_of_the_fp32_definition():
    """The GPU test's dyadic triangle, here against the helper: both restatements of the definition agree with exact fractions."""
    sc, want = D.dyadic_triangle()
    got = D.render_f32(**sc)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want == 2.0).sum() > 8 and (want == sc["far"]).sum() > 8


# ------------------------------------------------------------------------------------------- 3. the entry point
def test_entry_point_rejects_bad_arguments_before_any_launch():
    from partmanip_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION >= 159
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first

    def call(verts=p, vert_part=p, NV=8, faces=p, F=4, R=p, T=p, B=2, M=3, cam=p, V=2, fx=60.0, fy=60.0, cx=20.0, cy=12.0, H=24,
             W=40, near=0.01, far=100.0, out=p, out_stride=2 * 24 * 40):
        return lib.pm_mesh_depth_render_f32(verts, vert_part, NV, faces, F, R, T, B, M, cam, V, fx, fy, cx, cy, H, W, near, far, out,
                                            out_stride, None)
    for name in ("verts", "vert_part", "faces", "R", "T", "cam", "out"):
        assert call(**{name: None}) == -1, name
    for name in ("NV", "F", "B", "M", "V", "H", "W"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(near=0.0) == -1 and call(near=-1.0) == -1 and call(near=float("nan")) == -1
    assert call(far=0.01) == -1 and call(far=0.005) == -1 and call(far=float("nan")) == -1
    assert call(out_stride=2 * 24 * 40 - 1) == -1 and call(out_stride=0) == -1


# ------------------------------------------------------------------------------------------- 4. host logic on 'cpu'
def test_render_refuses_cpu_tensors_and_wrong_shapes():
    from partmanip_amd import ops
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc = D.seeded_scene()
    intr = np.array([[60.0, 0, 20], [0, 60.0, 12], [0, 0, 1]])
    finger = D.finger_mesh()
    cam = DepthFromMesh(3, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[finger, finger, MB.box_mesh(D.BOX_HALF, (0.0, 0.0, 0.0))])
    assert cam.part_num == 3 and cam.num_view == 2 and (cam.near, cam.far) == (0.01, 100.0)
    assert cam.faces.dtype == torch.int32 and tuple(cam.faces.shape) == (1260, 3) and cam.vert_part.dtype == torch.int32
    assert np.array_equal(cam.faces.numpy(), sc["faces"]) and np.array_equal(cam.vert_part.numpy(), sc["vert_part"])
    assert np.array_equal(cam.verts.numpy(), sc["verts"]) and (cam.fx, cam.fy, cam.cx, cam.cy) == (60.0, 60.0, 20.0, 12.0)
    R, T = torch.from_numpy(sc["R"]), torch.from_numpy(sc["T"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.render(R, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_depth_render(cam.verts, cam.vert_part, cam.faces, R, T, cam.cam_pose, 60.0, 60.0, 20.0, 12.0, 24, 40)
    for bad_R, bad_T in ((R[:, :2], T), (R, T[:, :2]), (R.reshape(3, 3, 9), T), (R, T[:2]), (R.double(), T.double())):
        with pytest.raises(ValueError):
            cam.render(bad_R, bad_T)
    for bad_out in (torch.empty(3 * 1920), torch.empty(2, 1920), torch.empty(3, 1919)):  # 1-D, wrong row count, too few columns
        with pytest.raises(ValueError, match="out"):
            cam.render(R, T, out=bad_out)                    # the out view is checked before the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.render(R, T, out=torch.empty(3, 1920))
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"][0], intr, 24, 40, meshes=[finger])               # (4, 4), not (V, 4, 4)
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"], intr[:2], 24, 40, meshes=[finger])
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[finger], near=0.0)
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[finger], far=0.005)
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[])
    with pytest.raises(ValueError):
        DepthFromMesh(1, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[(finger[0], np.array([[0, 1, len(finger[0])]]))])
