"""Yardsticks of the depth camera (partmanip_amd/mesh2depth.py: DepthFromMesh.render, csrc/mesh_depth.hip).  Not product code.

(a) render_f32: the definition of the image (include/partmanip_hip.h, pm_mesh_depth_render_f32) evaluated in numpy float32 over
    ALL pixel x triangle pairs -- no boxes, no schedule.  numpy rounds every float32 product, sum and difference on its own and its
    float32 division is IEEE, which is the stated arithmetic, so the GPU image must equal it bit for bit.
(b) cast_f64: an independent fp64 ray caster that shares no code or formula with (a): the triangles are posed in world space, the
    ray leaves the camera position along R_cam (dx, dy, 1), and each triangle is intersected by Moller-Trumbore (edge vectors, a
    determinant, barycentrics u, v and the ray parameter; the direction's camera-z component is 1, so the parameter IS the
    z-depth).  It also flags, per pixel, whether the ray lies in the boundary band of any triangle: normalised barycentrics
    beta = (1 - u - v, u, v) with -1e-3 < min beta < 1e-3 and the plane hit between near and far.  Off the band an fp32 and an
    fp64 evaluation must agree on hit or miss; on it a depth image is discontinuous and they need not.

Plus the seeded scene both test files use."""
import functools
import os

import numpy as np

from tests import mesh_bake_ref as MB
from tests.helpers import GOLDEN

F32 = np.float32
BAND = 1e-3


# ------------------------------------------------------------------------------------------------------------ (a)
def render_f32(verts, vert_part, faces, R, T, cam_pose, fx, fy, cx, cy, H, W, near, far, faces_per_chunk=256):
    """(B, V, H, W) float32.  verts (NV, 3), vert_part (NV), faces (F, 3), R (B, M, 3, 3), T (B, M, 3), cam_pose (V, 4, 4)."""
    verts, R, T, C = (np.asarray(a, dtype=F32) for a in (verts, R, T, cam_pose))
    vert_part, faces = np.asarray(vert_part).astype(np.int64), np.asarray(faces).astype(np.int64)
    NV, (B, M), V = len(verts), R.shape[:2], len(C)
    fx, fy, cx, cy, near, far = (F32(a) for a in (fx, fy, cx, cy, near, far))
    face_ok = ((faces >= 0) & (faces < NV)).all(axis=1)
    safe_faces = np.where(face_ok[:, None], faces, 0)
    part = vert_part[safe_faces]                                                        # (F, 3)
    face_ok &= ((part >= 0) & (part < M)).all(axis=1)
    safe_part = np.where((vert_part >= 0) & (vert_part < M), vert_part, 0)
    dx = ((np.arange(W).astype(F32) - cx) / fx)[None, :, None]                          # (1, W, 1)
    dy = ((np.arange(H).astype(F32) - cy) / fy)[:, None, None]                          # (H, 1, 1)
    assert dx.dtype == F32 and dy.dtype == F32
    out = np.full((B, V, H, W), far, dtype=F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            Rv, Tv = R[b][safe_part], T[b][safe_part]                                   # (NV, 3, 3), (NV, 3)
            x = verts
            xw = np.stack([((x[:, 0] * Rv[:, j, 0] + x[:, 1] * Rv[:, j, 1]) + x[:, 2] * Rv[:, j, 2]) + Tv[:, j] for j in range(3)], axis=1)
            for v in range(V):
                d = xw - C[v, :3, 3][None]
                p = np.stack([(d[:, 0] * C[v, 0, k] + d[:, 1] * C[v, 1, k]) + d[:, 2] * C[v, 2, k] for k in range(3)], axis=1)
                assert p.dtype == F32
                tri = p[safe_faces]                                                     # (F, 3, 3)
                ok = face_ok & np.isfinite(tri).all(axis=(1, 2))
                tri = tri[ok]
                img = out[b, v]
                for lo in range(0, len(tri), faces_per_chunk):
                    p0, p1, p2 = (tri[lo:lo + faces_per_chunk, i] for i in range(3))

                    def cross(a, c):
                        return (a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0])
                    w = [(dx * n[0] + dy * n[1]) + n[2] for n in (cross(p1, p2), cross(p2, p0), cross(p0, p1))]   # (H, W, f) each
                    s = (w[0] + w[1]) + w[2]
                    z = ((w[0] * p0[:, 2] + w[1] * p1[:, 2]) + w[2] * p2[:, 2]) / s
                    assert z.dtype == F32
                    same = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
                    hit = same & (s != 0) & (z > near) & (z < far)
                    np.minimum(img, np.where(hit, z, far).min(axis=2), out=img)
    return out


# ------------------------------------------------------------------------------------------------------------ (b)
def posed_triangles64(verts, vert_part, faces, R, T):
    """(B, F, 3, 3) float64 world-space corners: R x + T with the fp32 inputs taken as exact."""
    x = np.asarray(verts, dtype=np.float64)
    part = np.asarray(vert_part).astype(np.int64)
    R, T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
    world = np.einsum("bnji,ni->bnj", R[:, part], x) + T[:, part]                       # (B, NV, 3)
    return world[:, np.asarray(faces).astype(np.int64)]


def cast_f64(verts, vert_part, faces, R, T, cam_pose, fx, fy, cx, cy, H, W, near, far, rays_per_chunk=64):
    """(depth (B, V, H, W) float64 with `far` at misses, band (B, V, H, W) bool).  Valid indices and finite poses only."""
    tri = posed_triangles64(verts, vert_part, faces, R, T)
    C = np.asarray(cam_pose, dtype=np.float64)
    B, V = len(tri), len(C)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    local = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], axis=-1).reshape(-1, 3)    # (HW, 3)
    depth = np.full((B, V, H * W), float(far))
    band = np.zeros((B, V, H * W), dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            a = tri[b, :, 0][None]
            e1, e2 = tri[b, :, 1][None] - a, tri[b, :, 2][None] - a
            for v in range(V):
                dirs = local @ C[v, :3, :3].T                                           # world direction of every pixel's ray
                s = C[v, :3, 3][None, None] - a                                         # (1, F, 3)
                qv = np.cross(s, e1)
                for lo in range(0, H * W, rays_per_chunk):
                    dd = dirs[lo:lo + rays_per_chunk, None]                             # (r, 1, 3)
                    h = np.cross(dd, e2)
                    det = (e1 * h).sum(-1)
                    bu = (s * h).sum(-1) / det
                    bv = (dd * qv).sum(-1) / det
                    t = (e2 * qv).sum(-1) / det
                    inside_clip = (det != 0) & (t > near) & (t < far)
                    beta = np.minimum(np.minimum(bu, bv), 1.0 - bu - bv)
                    hit = inside_clip & (beta >= 0)
                    depth[b, v, lo:lo + rays_per_chunk] = np.where(hit, t, float(far)).min(axis=1)
                    band[b, v, lo:lo + rays_per_chunk] = (inside_clip & (beta > -BAND) & (beta < BAND)).any(axis=1)
    return depth.reshape(B, V, H, W), band.reshape(B, V, H, W)


# ------------------------------------------------------------------------------------------------------------ scenes
def concat_meshes(meshes):
    """[(vertices, faces)] -> verts (NV, 3) float32, vert_part (NV) int32, faces (F, 3) int32."""
    verts, part, faces, base = [], [], [], 0
    for i, (v, f) in enumerate(meshes):
        verts.append(np.asarray(v, dtype=F32))
        part.append(np.full(len(v), i, dtype=np.int32))
        faces.append(np.asarray(f, dtype=np.int64) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(part), np.concatenate(faces).astype(np.int32)


def rotations(rng, shape):
    q = rng.standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(shape + (3, 3)).astype(F32)


def look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera->world, the camera looking along +z with x right and y down."""
    position, target, up = (np.asarray(a, dtype=np.float64) for a in (position, target, up))
    z = (target - position) / np.linalg.norm(target - position)
    x = np.cross(z, up) / np.linalg.norm(np.cross(z, up))
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, position
    return pose.astype(F32)


def finger_mesh():
    from partmanip_amd import meshio
    return meshio.load_mesh(os.path.join(GOLDEN, "finger.stl"))


SCENE_SEED = 3
BOX_HALF = (0.06, 0.05, 0.04)                                # the 0.12 x 0.10 x 0.08 box


def seeded_scene(seed=SCENE_SEED, envs=3, views=2, H=24, W=40):
    """The finger fixture twice plus a box (624 + 624 + 12 triangles) under seeded poses (translations within +-0.06), seen by
    `views` cameras about 0.3 m from the origin; fx = fy = 60, principal point at the image centre."""
    rng = np.random.RandomState(seed)
    finger = finger_mesh()
    verts, vert_part, faces = concat_meshes([finger, finger, MB.box_mesh(BOX_HALF, (0.0, 0.0, 0.0))])
    R = rotations(rng, (envs, 3))
    T = rng.uniform(-0.06, 0.06, size=(envs, 3, 3)).astype(F32)
    cams = []
    for _ in range(views):
        d = rng.standard_normal(3)
        d[2] = abs(d[2]) + 0.3                              # above the horizon, away from `up`
        cams.append(look_at(0.3 * d / np.linalg.norm(d)))
    return dict(verts=verts, vert_part=vert_part, faces=faces, R=R, T=T, cam_pose=np.stack(cams), fx=60.0, fy=60.0, cx=W / 2.0,
                cy=H / 2.0, H=H, W=W, near=0.01, far=100.0)


@functools.lru_cache(maxsize=None)
def seeded_scene_images():
    """(scene, render_f32 image, cast_f64 depth, band) of the seeded scene, computed once per process; callers do not modify them."""
    sc = seeded_scene()
    z32 = render_f32(**sc)
    z64, band = cast_f64(**sc)
    for a in (z32, z64, band):
        a.setflags(write=False)
    return sc, z32, z64, band


# ------------------------------------------------------------------------------------------------------------ known answer
def dyadic_triangle():
    """(scene, expected (1, 1, 8, 8) float32): one triangle facing an identity camera at z = 2, identity pose, 8 x 8 image, fx = fy =
    cx = cy = 4.  Its corners project onto the pixel centres (1, 1), (6, 1) and (1, 6), so pixels lie exactly on its edges and
    corners.  The expected image is the definition evaluated in exact rational arithmetic (Python fractions, nothing of render_f32);
    every intermediate is checked to be a float32 value, so every fp32 operation of the definition is exact on this scene."""
    from fractions import Fraction as Fr
    H = W = 8
    fx = fy = cx = cy = 4.0
    near, far = 0.01, 100.0
    corners = [(-1.5, -1.5, 2.0), (1.0, -1.5, 2.0), (-1.5, 1.0, 2.0)]

    def exact(x):
        assert Fr(float(F32(float(x)))) == x, f"{x} is not a float32 value"
        return x

    def cross(a, c):
        return tuple(exact(exact(a[i] * c[j]) - exact(a[j] * c[i])) for i, j in ((1, 2), (2, 0), (0, 1)))
    p = [tuple(Fr(v) for v in c) for c in corners]
    n = [cross(p[1], p[2]), cross(p[2], p[0]), cross(p[0], p[1])]
    want = np.full((1, 1, H, W), far, dtype=F32)
    for r in range(H):
        for c in range(W):
            dx, dy = exact((Fr(c) - Fr(cx)) / Fr(fx)), exact((Fr(r) - Fr(cy)) / Fr(fy))
            w = [exact(exact(exact(dx * ni[0]) + exact(dy * ni[1])) + ni[2]) for ni in n]
            s = exact(exact(w[0] + w[1]) + w[2])
            if not (all(x >= 0 for x in w) or all(x <= 0 for x in w)) or s == 0:
                continue
            z = exact(exact(exact(exact(w[0] * p[0][2]) + exact(w[1] * p[1][2])) + exact(w[2] * p[2][2])) / s)
            if Fr(near) < z < Fr(far):
                want[0, 0, r, c] = F32(float(z))
    verts = np.asarray(corners, dtype=F32)
    scene = dict(verts=verts, vert_part=np.zeros(3, dtype=np.int32), faces=np.array([[0, 1, 2]], dtype=np.int32),
                 R=np.eye(3, dtype=F32)[None, None], T=np.zeros((1, 1, 3), dtype=F32), cam_pose=np.eye(4, dtype=F32)[None], fx=fx, fy=fy,
                 cx=cx, cy=cy, H=H, W=W, near=near, far=far)
    return scene, want
