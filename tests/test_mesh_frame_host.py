"""Frame camera (partmanip_amd.mesh2depth.DepthFromMesh.render_frame, pm_mesh_frame_render_f32, partmanip_amd.png), everything that
needs no GPU: the numpy definition of the three images (tests/frame_render_ref.frame_f32) tied to the depth camera's yardstick and
checked by a property that shares nothing with its argmin, the PNG writer's round trip, the host argument checks and the C ABI's
workspace size and refusals.  Every comparison is an equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import frame_render_ref as FR
from tests import mesh_bake_ref as MB


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------- 1. the reference
def test_frame_f32_depth_equals_the_depth_yardstick_bit_for_bit():
    sc, z32, _, _ = D.seeded_scene_images()
    _, depth, face, seg, rgb = FR.seeded_frame()
    assert depth.dtype == np.float32 and depth.shape == z32.shape == (3, 2, 24, 40)
    assert np.array_equal(bits(depth), bits(z32))
    assert np.array_equal(face >= 0, z32 < sc["far"]) and face.max() < 1260
    assert seg.dtype == np.int32 and rgb.dtype == np.uint8 and rgb.shape == (3, 2, 24, 40, 3)
    assert set(np.unique(seg)) == {-1, 0, 1, 2}
    assert (rgb[face < 0] == 255).all()
    tri, want = D.dyadic_triangle()
    depth, face, seg, rgb = FR.frame_f32(**tri)
    assert np.array_equal(bits(depth), bits(want))
    assert np.array_equal(face == 0, want == 2.0) and np.array_equal(face == -1, want == 100.0)
    # the triangle faces the camera: g = (0, 0, 6.25), l = 1, k = 0.25 + 0.75 = 1, the colour is the palette's own
    assert (rgb[face == 0] == FR.default_palette(1)[0].astype(np.uint8)).all()


def test_every_part_alone_renders_its_own_pixels_and_nothing_nearer_elsewhere():
    """Shares nothing with frame_f32's argmin: part p's faces alone through render_f32 give the full depth exactly where seg == p
    and a depth no smaller everywhere else.  No pixel is excluded."""
    sc, depth, face, seg, _ = FR.seeded_frame()
    part_of_face = sc["vert_part"][sc["faces"][:, 0]]
    seen = 0
    for p in range(3):
        alone = D.render_f32(**dict(sc, faces=sc["faces"][part_of_face == p]))
        mine = seg == p
        assert mine.sum() >= 50, p                           # the scene shows every part (a statement about the scene)
        assert np.array_equal(bits(alone[mine]), bits(depth[mine])), p
        assert (alone[~mine] >= depth[~mine]).all(), p
        seen += int(mine.sum())
    assert seen == int((seg >= 0).sum()) and ((seg == -1) == (depth == np.float32(sc["far"]))).all()
    assert np.array_equal(part_of_face[face[face >= 0]], seg[face >= 0])


# ------------------------------------------------------------------------------------------- 2. the PNG writer
@pytest.mark.parametrize("shape", [(7, 13, 3), (7, 13), (1, 1, 3), (13, 7)])
def test_write_png_round_trip(shape, tmp_path):
    from partmanip_amd.png import write_png
    rng = np.random.RandomState(sum(shape))
    img = rng.randint(0, 256, size=shape).astype(np.uint8)
    path = tmp_path / "video" / "g" / "Iter0" / "3.png"                                  # a directory that does not exist yet
    write_png(str(path), img)
    assert path.exists()
    back = FR.read_png(str(path))
    assert back.dtype == np.uint8 and back.shape == shape and np.array_equal(back, img)


@pytest.mark.parametrize("shape", [(7, 13, 3), (13, 7)])
def test_write_png_opens_in_an_imaging_library(shape, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from partmanip_amd.png import write_png
    img = np.random.RandomState(1).randint(0, 256, size=shape).astype(np.uint8)
    path = tmp_path / "a.png"
    write_png(str(path), img)
    with Image.open(str(path)) as im:
        assert im.mode == ("RGB" if len(shape) == 3 else "L")
        assert np.array_equal(np.asarray(im), img)


def test_write_png_refuses_other_arrays(tmp_path):
    from partmanip_amd.png import write_png
    for bad in (np.zeros((4, 4, 4), dtype=np.uint8), np.zeros((4, 4), dtype=np.float32), np.zeros((4,), dtype=np.uint8),
                np.zeros((0, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            write_png(str(tmp_path / "x.png"), bad)
    assert not (tmp_path / "x.png").exists()


# ------------------------------------------------------------------------------------------- 3. host logic on 'cpu'
def test_render_frame_and_the_constructor_refuse_bad_arguments_before_the_device():
    from partmanip_amd.mesh2depth import PALETTE, DepthFromMesh, Frame
    sc = D.seeded_scene()
    intr = np.array([[60.0, 0, 20], [0, 60.0, 12], [0, 0, 1]])
    finger = D.finger_mesh()
    meshes = [finger, finger, MB.box_mesh(D.BOX_HALF, (0.0, 0.0, 0.0))]
    mk = lambda **kw: DepthFromMesh(3, "cpu", sc["cam_pose"], intr, 24, 40, meshes=meshes, **kw)      # noqa: E731
    cam = mk()
    assert len(PALETTE) == 12 and Frame._fields == ("depth", "seg", "rgb")
    assert cam.labels is None and cam.miss_label == -1 and cam.background == (255, 255, 255)
    assert (cam.ambient, cam.one_minus_ambient) == (0.25, 0.75)
    assert np.array_equal(cam.palette.numpy(), np.asarray(PALETTE[:3], dtype=np.float32))
    assert np.array_equal(DepthFromMesh(1, "cpu", sc["cam_pose"], intr, 24, 40, meshes=[finger] * 14).palette.numpy()[12:],
                          np.asarray(PALETTE[:2], dtype=np.float32))                     # cycled
    lab = mk(labels=[1, 1, 0], miss_label=7, palette=[[0, 0, 0], [255, 255, 255], [1.5, 2, 3]], ambient=1.0, background=(0, 10, 255))
    assert lab.labels.dtype == torch.int32 and lab.labels.tolist() == [1, 1, 0] and lab.miss_label == 7
    assert (lab.ambient, lab.one_minus_ambient) == (1.0, 0.0)
    for bad in (dict(labels=[1, 1]), dict(labels=[1, 1, 0, 0]), dict(labels=[0.5, 1, 1]), dict(palette=[[0, 0, 0]] * 2),
                dict(palette=[[0, 0, 256.0]] * 3), dict(palette=[[0, -1, 0]] * 3), dict(palette=[[0, float("nan"), 0]] * 3),
                dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=float("nan")), dict(background=(0, 0)),
                dict(background=(0, 0, 256)), dict(background=(-1, 0, 0))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            mk(**bad)
    R, T = torch.from_numpy(sc["R"]), torch.from_numpy(sc["T"])
    with pytest.raises(ValueError, match="all switched off"):
        cam.render_frame(R, T, depth=False, seg=False, rgb=False)
    with pytest.raises(ValueError, match="out_depth"):
        cam.render_frame(R, T, depth=False, out_depth=torch.empty(3, 1920))
    for bad_R, bad_T in ((R[:, :2], T), (R, T[:, :2]), (R, T[:2]), (R.double(), T.double())):
        with pytest.raises(ValueError):
            cam.render_frame(bad_R, bad_T)
    for bad_out in (torch.empty(3 * 1920), torch.empty(2, 1920), torch.empty(3, 1919)):
        with pytest.raises(ValueError, match="out"):
            cam.render_frame(R, T, out_depth=bad_out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.render_frame(R, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.render_frame(R, T, seg=False, rgb=False, out_depth=torch.empty(3, 1920))
    assert cam._keys.buf is None                                                           # nothing was allocated on the way


# ------------------------------------------------------------------------------------------- 4. the entry point
def test_workspace_bytes_is_eight_bytes_per_pixel():
    from partmanip_amd._lib import lib
    for B, V, H, W in ((1, 1, 1, 1), (3, 2, 24, 40), (2, 3, 7, 13), (64, 3, 288, 512), (1024, 3, 288, 512)):
        assert lib.pm_mesh_frame_workspace_bytes(B, V, H, W) == 8 * B * V * H * W
    assert lib.pm_mesh_frame_workspace_bytes(64, 3, 288, 512) == 226492416                 # the 226 MB of the shipped rig at 64 environments


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from partmanip_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first
    n = 2 * 24 * 40
    need = 8 * 2 * n

    def call(verts=p, vert_part=p, NV=8, faces=p, F=4, R=p, T=p, B=2, M=3, cam=p, V=2, fx=60.0, fy=60.0, cx=20.0, cy=12.0, H=24,
             W=40, near=0.01, far=100.0, label=p, miss=-1, palette=p, ambient=0.25, oma=0.75, bg=(255, 255, 255), depth=p,
             depth_stride=n, seg=p, seg_stride=n, rgb=p, rgb_stride=3 * n, ws=p, ws_bytes=need):
        return lib.pm_mesh_frame_render_f32(verts, vert_part, NV, faces, F, R, T, B, M, cam, V, fx, fy, cx, cy, H, W, near, far, label,
                                            miss, palette, ambient, oma, bg[0], bg[1], bg[2], depth, depth_stride, seg, seg_stride,
                                            rgb, rgb_stride, ws, ws_bytes, None)
    EINVAL, EWORKSPACE, EALIGN = -1, -2, -3
    for name in ("verts", "vert_part", "faces", "R", "T", "cam"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("NV", "F", "B", "M", "V", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(near=0.0) == EINVAL and call(near=float("nan")) == EINVAL and call(far=0.005) == EINVAL and call(far=float("nan")) == EINVAL
    assert call(depth=None, seg=None, rgb=None) == EINVAL
    assert call(palette=None) == EINVAL
    for name, least in (("depth_stride", n), ("seg_stride", n), ("rgb_stride", 3 * n)):
        assert call(**{name: least - 1}) == EINVAL, name
    assert call(ambient=-0.5) == EINVAL and call(oma=-0.5) == EINVAL and call(ambient=0.5, oma=0.75) == EINVAL
    assert call(ambient=float("nan")) == EINVAL and call(oma=float("nan")) == EINVAL
    assert call(bg=(256, 0, 0)) == EINVAL and call(bg=(0, -1, 0)) == EINVAL and call(bg=(0, 0, 300)) == EINVAL
    # the workspace is judged once the arguments are in order: size first, then alignment
    assert call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE and call(ws=None) == EWORKSPACE
    assert call(ws=ctypes.c_void_p(68)) == EALIGN and call(ws=ctypes.c_void_p(65), ws_bytes=need + 64) == EALIGN
    assert call(ws=ctypes.c_void_p(68), ws_bytes=need - 1) == EWORKSPACE
    assert call(W=40, H=12288) == EINVAL                                                   # the per-block table of dx and dy
