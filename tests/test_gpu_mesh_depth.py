"""Depth camera on the GPU: partmanip_amd.mesh2depth.DepthFromMesh (pm_mesh_depth_render_f32, csrc/mesh_depth.hip) against the
definition of the image evaluated in numpy float32 over all pixel x triangle pairs (tests/depth_render_ref.render_f32).

The contract fixes the association and the rounding of every operation and the minimum over triangles is order-free, so every
comparison with render_f32 is an equality of the uint32 views.  The one check against the independent fp64 ray caster (occlusion)
is restricted to pixels off every triangle's boundary band and uses the depth tolerance of the host test
(profiles/mesh_depth_margins.json: 4 x the worst |render_f32 - cast_f64| observed on the CPU, 2.27e-06 m)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import mesh_bake_ref as MB
from tests.helpers import ROOT, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25


def t(x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype).to(DEV)                   # a copy: the shared scene arrays are read-only


def render_gpu(sc, out=None):
    """ops.mesh_depth_render on a scene dict of tests/depth_render_ref -> (B, V, H, W) tensor."""
    from partmanip_amd import ops
    B, V, H, W = len(sc["R"]), len(sc["cam_pose"]), sc["H"], sc["W"]
    res = ops.mesh_depth_render(t(sc["verts"]), t(sc["vert_part"]), t(sc["faces"]), t(sc["R"]), t(sc["T"]), t(sc["cam_pose"]), sc["fx"],
                                sc["fy"], sc["cx"], sc["cy"], H, W, sc["near"], sc["far"], out)
    torch.cuda.synchronize()
    return res[:, :V * H * W].reshape(B, V, H, W)


def intrinsic(sc):
    return np.array([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]])


def scene_meshes():
    finger = D.finger_mesh()
    return [finger, finger, MB.box_mesh(D.BOX_HALF, (0.0, 0.0, 0.0))]


def axis_angle(rng, shape, max_angle):
    axis = rng.standard_normal(shape + (3,))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    ang = rng.uniform(-max_angle, max_angle, size=shape)
    K = np.zeros(shape + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return (np.eye(3) + s * K + (1 - c) * (K @ K)).astype(np.float32)


def test_known_answer_dyadic_triangle():
    """One triangle facing an identity camera at z = 2; every number is a small dyadic, so every fp32 operation is exact and the
    expected image comes from Python fractions (tests/depth_render_ref.dyadic_triangle), not from render_f32."""
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc, want = D.dyadic_triangle()
    cam = DepthFromMesh(1, DEV, sc["cam_pose"], intrinsic(sc), 8, 8, meshes=[(sc["verts"], sc["faces"])])
    got = cam.render(t(sc["R"]), t(sc["T"]))
    assert tuple(got.shape) == (1, 1, 8, 8) and got.dtype == torch.float32
    assert np.array_equal(bits(got), bits(want))
    img = got[0, 0].cpu().numpy()
    inside = np.array([[1 <= c and 1 <= r and r + c <= 7 for c in range(8)] for r in range(8)])     # edges and corners included
    assert inside.sum() == 21 and (img[inside] == 2.0).all() and (img[~inside] == 100.0).all()


def test_seeded_scene_equals_render_f32_and_repeats():
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc, z32, _, _ = D.seeded_scene_images()
    cam = DepthFromMesh(3, DEV, sc["cam_pose"], intrinsic(sc), sc["H"], sc["W"], meshes=scene_meshes())
    R, T = t(sc["R"]), t(sc["T"])
    first = cam.render(R, T).clone()
    second = cam.render(R, T)
    assert tuple(first.shape) == (3, 2, 24, 40)
    diff = bits(first) != bits(z32)
    print(f"pixels that differ from render_f32: {int(diff.sum())} of {diff.size}")
    assert not diff.any()
    assert np.array_equal(bits(second), bits(first))
    assert np.array_equal(bits(render_gpu(sc)), bits(z32))                              # the op itself, without the class


def test_odd_sizes_and_out_view_with_sentinel_tail():
    """70 x 130 (the width is no multiple of the wave), one view, five environments, out = a view of a wider buffer."""
    rng = np.random.RandomState(11)
    verts, vert_part, faces = D.concat_meshes([D.finger_mesh(), MB.box_mesh((0.03, 0.05, 0.02), (0.0, 0.0, 0.0))])
    H, W, B = 70, 130, 5
    sc = dict(verts=verts, vert_part=vert_part, faces=faces, R=D.rotations(rng, (B, 2)),
              T=rng.uniform(-0.05, 0.05, size=(B, 2, 3)).astype(np.float32), cam_pose=D.look_at((0.2, -0.15, 0.2))[None], fx=210.0,
              fy=200.0, cx=64.5, cy=35.25, H=H, W=W, near=0.01, far=100.0)
    n, tail = H * W, 13
    buf = torch.full((B, n + tail), SENTINEL, device=DEV)
    got = render_gpu(sc, out=buf[:, :n + 5])
    want = D.render_f32(**sc)
    hits = (want < 100).mean()
    print(f"hit share {hits:.3f}")
    assert 0.05 < hits < 0.9
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(bits(got), bits(want))
    assert (buf[:, n:] == SENTINEL).all()
    # one environment: the row stride of a one-row view is arbitrary (n + 5, n + 5 and 1 here) and must reach the kernel as n
    one = dict(sc, R=sc["R"][:1], T=sc["T"][:1])
    want1 = render_gpu(one)
    wide, flat, col = (torch.full(s, SENTINEL, device=DEV) for s in ((1, n + 5), (n + 5,), (n + 5, 1)))
    for base, out in ((wide, wide[:, :n]), (flat, flat[None]), (col, col.t())):
        got = render_gpu(one, out=out)
        assert got.data_ptr() == base.data_ptr() and np.array_equal(bits(got), bits(want1))
        assert (base.reshape(-1)[n:] == SENTINEL).all()


def test_big_triangles_cover_the_frustum_without_a_crack():
    """A quad of two triangles that covers the whole frustum under 4 seeded poses: no pixel may be `far`, in particular none on the
    shared edge, and the wave-cooperative path (boxes of the whole image) gives the bits of render_f32."""
    rng = np.random.RandomState(5)
    verts = np.array([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    B = 4
    T = np.concatenate([rng.uniform(-0.2, 0.2, size=(B, 1, 2)), rng.uniform(1.0, 2.0, size=(B, 1, 1))], axis=-1).astype(np.float32)
    sc = dict(verts=verts, vert_part=np.zeros(4, dtype=np.int32), faces=faces, R=axis_angle(rng, (B, 1), 0.3), T=T,
              cam_pose=np.eye(4, dtype=np.float32)[None], fx=60.0, fy=60.0, cx=20.0, cy=12.0, H=24, W=40, near=0.01, far=100.0)
    got = render_gpu(sc)
    want = D.render_f32(**sc)
    assert (want < 100).all()
    assert (got < 100).all() and (got > 0.5).all()
    assert np.array_equal(bits(got), bits(want))


def test_near_plane_triangles_are_tested_against_the_whole_image():
    verts = np.array([[-0.2, -0.1, 0.5], [0.3, -0.1, 0.5], [0.0, 0.2, -0.3],            # crosses z = near
                      [-0.2, -0.1, -0.5], [0.3, -0.1, -0.5], [0.0, 0.2, -0.4],          # wholly behind the camera
                      [-0.05, 0.0, 0.7], [0.1, 0.02, 0.8], [0.0, 0.1, 0.75]], dtype=np.float32)      # wholly in front
    faces = np.arange(9, dtype=np.int32).reshape(3, 3)
    base = dict(verts=verts, vert_part=np.zeros(9, dtype=np.int32), R=np.eye(3, dtype=np.float32)[None, None],
                T=np.zeros((1, 1, 3), dtype=np.float32), cam_pose=np.eye(4, dtype=np.float32)[None], fx=30.0, fy=30.0, cx=16.0, cy=10.0,
                H=20, W=32, near=0.01, far=100.0)
    for pick, must_hit in (([0], True), ([1], False), ([0, 1, 2], True)):
        sc = dict(base, faces=faces[pick])
        got, want = render_gpu(sc), D.render_f32(**sc)
        assert ((want < 100).any()) == must_hit
        assert np.array_equal(bits(got), bits(want)), pick


def test_bad_indices_and_a_nan_pose_skip_their_triangles_only():
    sc, _, _, _ = D.seeded_scene_images()
    NV, M = len(sc["verts"]), 3
    faces, vert_part, T = sc["faces"].copy(), sc["vert_part"].copy(), sc["T"].copy()
    faces[5, 1] = NV + 7                                     # one face index out of range
    faces[900, 2] = -1
    bad_vertex = int(sc["faces"][700, 0])
    vert_part[bad_vertex] = M + 2                            # one vert_part out of range
    T[1, 0, 2] = np.nan                                      # one NaN in one environment's pose_T
    bad = dict(sc, faces=faces, vert_part=vert_part, T=T)
    got = render_gpu(bad)
    assert torch.isfinite(got).all()
    # the scene without them: the same triangles dropped by hand, per environment
    drop = np.zeros(len(faces), dtype=bool)
    drop[[5, 900]] = True
    drop |= (sc["faces"] == bad_vertex).any(axis=1)
    assert 3 <= drop.sum() < 40
    part_of_face = sc["vert_part"][sc["faces"][:, 0]]
    for b in range(3):
        d = drop | (part_of_face == 0) if b == 1 else drop
        clean = dict(sc, faces=sc["faces"][~d], R=sc["R"][b:b + 1], T=sc["T"][b:b + 1].copy())
        if b == 1:
            clean["T"][0, 0] = 0.0                           # part 0 has no triangle left; any finite pose will do
        want = D.render_f32(**clean)
        assert np.array_equal(bits(got[b:b + 1]), bits(want)), b
    assert np.array_equal(bits(got), bits(D.render_f32(**bad)))


def test_occlusion_keeps_the_nearer_surface():
    """The box in front of a finger: where both are hit the image carries the nearer depth (fp64 caster, off the band)."""
    with open(os.path.join(ROOT, "profiles", "mesh_depth_margins.json")) as f:
        tol = 4 * json.load(f)["margins"][0]["observed"]
    finger, box = D.finger_mesh(), MB.box_mesh((0.004, 0.012, 0.004), (0.0, 0.0, 0.0))
    verts, vert_part, faces = D.concat_meshes([finger, box])
    centre = finger[0].mean(axis=0)
    R = np.eye(3, dtype=np.float32)[None, None].repeat(2, axis=1)
    T = np.array([[-centre + [0.0, 0.0, 0.30], [0.004, 0.003, 0.20]]], dtype=np.float32)
    sc = dict(verts=verts, vert_part=vert_part, faces=faces, R=R, T=T, cam_pose=np.eye(4, dtype=np.float32)[None], fx=150.0, fy=150.0,
              cx=20.0, cy=12.0, H=24, W=40, near=0.01, far=100.0)
    got = render_gpu(sc)[0, 0].cpu().numpy().astype(np.float64)
    nf = len(finger[1])
    z_f, band_f = D.cast_f64(**dict(sc, faces=faces[:nf]))
    z_b, band_b = D.cast_f64(**dict(sc, faces=faces[nf:]))
    keep = ~(band_f | band_b)[0, 0]
    both = (z_f[0, 0] < 100) & (z_b[0, 0] < 100) & keep
    nearer, farther = np.minimum(z_f, z_b)[0, 0], np.maximum(z_f, z_b)[0, 0]
    print(f"pixels where both are hit: {int(both.sum())}; finger only {int(((z_f[0, 0] < 100) & (z_b[0, 0] >= 100)).sum())}; "
          f"worst |z - nearer| = {np.abs(got - nearer)[both].max():.3e} (tolerance {tol:.3e})")
    assert both.sum() >= 20 and ((z_f[0, 0] < 100) & (z_b[0, 0] >= 100) & keep).sum() >= 20
    assert (farther[both] - nearer[both]).min() > 0.01
    assert np.abs(got - nearer)[both].max() <= tol
    assert np.abs(got - nearer)[keep].max() <= tol          # everywhere off the band, misses included
    assert np.array_equal(bits(render_gpu(sc)), bits(D.render_f32(**sc)))


def test_render_feeds_depth2pc_unchanged():
    from partmanip_amd.depth2tsdf import TSDFVolume
    from partmanip_amd.mesh2depth import DepthFromMesh
    sc, z32, _, _ = D.seeded_scene_images()
    cam = DepthFromMesh(2, DEV, sc["cam_pose"], intrinsic(sc), sc["H"], sc["W"], meshes=scene_meshes())
    depth = cam.render(t(sc["R"][:2]), t(sc["T"][:2]))
    vol = TSDFVolume(DEV, size=0.5, resolution=50, _vol_origin=(-0.25, -0.25, -0.25))
    vol.register_camera(sc["cam_pose"], intrinsic(sc), sc["H"], sc["W"], 2)
    got = vol.depth2pc(depth, K=64)
    want = vol.depth2pc(t(z32[:2]), K=64)
    assert tuple(got.shape) == (2, 64, 3) and torch.isfinite(got).all()
    assert np.array_equal(bits(got), bits(want))
    assert got.abs().max() < 0.25 and got.abs().max() > 0.02                             # points of the scene, inside the crop
