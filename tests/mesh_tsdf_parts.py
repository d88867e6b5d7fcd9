"""Test infrastructure of the mesh-TSDF observation (partmanip_amd/mesh2sdf.py): seeded synthetic parts, seeded poses and a
small fp64 restatement of the contract, written from its description (a loop over parts on un-padded grids) -- it shares no
text with the reference and none with the kernel.  Used by tests/golden/make_mesh_tsdf_golden.py (dev machine) and by
tests/test_mesh_tsdf_host.py / tests/test_gpu_mesh_tsdf.py."""
import hashlib

import numpy as np

SIZE, RES = 0.5, 50                       # the reference's workspace: 0.5 m cube, 50^3 voxels
ORIGIN = (-0.25, -0.25, -0.0503)
N_PARTS = 12                              # link0..7, hand, finger, finger, cube
CONT_SEED, CUT_SEED = 2101, 2102          # seeds of the two fixture families' parts


def _box_sdf(p, h):
    q = np.abs(p) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def _ellipsoid_sdf(p, r):
    """First-order distance to an ellipsoid (exact on a sphere): k0 (k0 - 1) / k1 with k0 = |p / r|, k1 = |p / r^2|."""
    k0 = np.linalg.norm(p / r, axis=-1)
    k1 = np.linalg.norm(p / (r * r), axis=-1)
    return k0 * (k0 - 1.0) / np.maximum(k1, 1e-12)


def make_parts(seed, family, n_parts=N_PARTS, size=SIZE, res=RES):
    """n_parts dicts {'sdf': (X,Y,Z) float32, 'bbox_min': (3,) float32, 'voxel_size': float}: boxes and ellipsoids with
    half-extents of 2-7 cm (different per part and axis, so the grid shapes differ), centred a little off the part frame's origin,
    on a 4 mm grid (5 mm for every fifth part), signed distance clamped to +-sdf_trunc.
    family 'cut': the grid covers extent + 2 * sdf_trunc, centred on cells, as the reference's own bake lays it out
    (mesh2sdf.py:213-223) -- it ends inside the truncation band.  family 'cont': five more cells on every side, so every value
    on the border of the valid box is +sdf_trunc and the volume is a continuous function of the pose."""
    assert family in ("cont", "cut")
    rng = np.random.RandomState(seed)
    trunc = 4 * size / res
    parts = []
    for i in range(n_parts):
        half = rng.uniform(0.02, 0.07, size=3)
        centre = rng.uniform(-0.01, 0.01, size=3)
        vs = float(np.float32(0.005 if i % 5 == 3 else 0.004))
        shape = np.ceil((2 * half + 2 * trunc) / vs).astype(np.int64)
        pad = 5 if family == "cont" else 0
        idx = np.stack(np.meshgrid(*[np.arange(s + 2 * pad) for s in shape], indexing="ij"), axis=-1)
        pts = (idx - (shape // 2 + pad)) * vs + centre
        d = _box_sdf(pts - centre, half) if i % 2 == 0 else _ellipsoid_sdf(pts - centre, half)
        sdf = np.clip(d, -trunc, trunc).astype(np.float32)
        parts.append({'sdf': sdf, 'bbox_min': pts.reshape(-1, 3).min(axis=0).astype(np.float32), 'voxel_size': vs})
    return parts


def fixture_parts(family):
    """The 12 parts of a fixture family in the reference's loading order; the two fingers are ONE file loaded twice
    (mesh2sdf.py:145), so part 10 is part 9."""
    parts = make_parts(CONT_SEED if family == "cont" else CUT_SEED, family)
    parts[10] = parts[9]
    return parts


def parts_digest(parts):
    """SHA-256 over every part's shape, grid bytes, bbox_min and voxel_size: pins regenerated parts to the ones a fixture was made with."""
    h = hashlib.sha256()
    for d in parts:
        h.update(np.asarray(d['sdf'].shape, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(d['sdf'], dtype=np.float32).tobytes())
        h.update(np.asarray(d['bbox_min'], dtype=np.float32).tobytes())
        h.update(np.float64(d['voxel_size']).tobytes())
    return h.hexdigest()


def random_poses(seed, B, M=N_PARTS):
    """fp32 poses: unit-quaternion rotations (B, M, 3, 3), translations uniform in [-0.2, 0.2]^2 x [0, 0.35] (B, M, 3)."""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=(B, M, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1).reshape(B, M, 3, 3)
    T = np.stack([rng.uniform(-0.2, 0.2, size=(B, M)), rng.uniform(-0.2, 0.2, size=(B, M)), rng.uniform(0.0, 0.35, size=(B, M))], axis=-1)
    return R.astype(np.float32), T.astype(np.float32)


def seeded_pred(seed, B=1, res=RES, size=SIZE, origin=ORIGIN):
    """A predicted TSDF (B, res^3) float32 in [-1, 1] for initialize_sdf: the truncated distance to six seeded spheres."""
    rng = np.random.RandomState(seed)
    vox = size / res
    ii = np.stack(np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij"), axis=-1).reshape(-1, 3)
    c = ii * vox + np.asarray(origin)
    out = []
    for _ in range(B):
        cen = rng.uniform(0.0, size, size=(6, 3)) + np.asarray(origin)
        rad = rng.uniform(0.03, 0.08, size=6)
        d = (np.linalg.norm(c[:, None, :] - cen[None], axis=-1) - rad[None]).min(axis=1)
        out.append(np.clip(d / (4 * vox), -1.0, 1.0))
    return np.stack(out).astype(np.float32)


def load_family(name, golden_dir):
    """A fixture family is stored one environment per file (<name>_env<b>.npz; 125 000 fp64 values with few repeats do not
    compress below ~0.35 MB per environment): arrays whose first dimension is the environment are concatenated, the rest
    is taken from the first file."""
    import glob
    import os
    files = sorted(glob.glob(os.path.join(golden_dir, name + "_env*.npz")))
    assert files, name
    per = []
    for f in files:
        with np.load(f) as z:
            per.append({k: z[k] for k in z.files})
    out = {}
    for k, v0 in per[0].items():
        out[k] = v0 if k in ("part_sha", "seed") else np.concatenate([d[k] for d in per], axis=0)
    return out


def save_family(name, golden_dir, shared, per_env):
    """Inverse of load_family: `per_env` arrays are split along their first dimension."""
    import os
    B = next(iter(per_env.values())).shape[0]
    sizes = []
    for b in range(B):
        path = os.path.join(golden_dir, f"{name}_env{b}.npz")
        np.savez_compressed(path, **shared, **{k: v[b:b + 1] for k, v in per_env.items()})
        sizes.append(os.path.getsize(path))
    return sizes


def restate(parts, pose_R, pose_T, res=RES, size=SIZE, origin=ORIGIN, base=None, p0=0, p1=None):
    """fp64 restatement: returns (volume (B, res, res, res), border margin (B, res^3)).
    Per part p in [p0, p1): q = (c_v - T) R; u = (q - bbox_min) / voxel_size; valid iff 1 <= u_a and u_a - shape_a <= -2 on
    all axes; valid -> trilinear value of the part's own grid at u, else 1; volume = clamp(min(min_p, base) / (4 vox_size), -1, 1)
    with base = the voxel's world z unless given as (B, res^3) (already in metres).  The border margin of a voxel is the
    smallest |u_a - 1| or |u_a - (shape_a - 2)| over the parts and axes: a sample closer to a border than fp32 round-off may
    legitimately fall on either side in an fp32 evaluation."""
    pose_R = np.asarray(pose_R, dtype=np.float64)
    pose_T = np.asarray(pose_T, dtype=np.float64)
    B, M = pose_R.shape[:2]
    p1 = M if p1 is None else p1
    vox = size / res
    ii = np.stack(np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij"), axis=-1).reshape(-1, 3)
    c = ii * vox + np.asarray([np.float32(o) for o in origin], dtype=np.float64)
    n = c.shape[0]
    best = np.broadcast_to(c[:, 2], (B, n)).copy() if base is None else np.asarray(base, dtype=np.float64).reshape(B, n).copy()
    margin = np.full((B, n), np.inf)
    for b in range(B):
        for p in range(p0, p1):
            g = np.asarray(parts[p]['sdf'], dtype=np.float64)
            shp = np.asarray(g.shape, dtype=np.float64)
            u = ((c - pose_T[b, p]) @ pose_R[b, p] - np.asarray(parts[p]['bbox_min'], dtype=np.float64)) / float(parts[p]['voxel_size'])
            margin[b] = np.minimum(margin[b], np.minimum(np.abs(u - 1.0), np.abs(u - (shp - 2.0))).min(axis=1))
            ok = np.all((u >= 1.0) & (u - shp <= -2.0), axis=1)
            val = np.ones(n)
            uo = u[ok]
            l = np.floor(uo).astype(np.int64)
            x, y, z = (uo - l).T
            i, j, k = l.T
            val[ok] = (((g[i, j, k] * (1 - z) + g[i, j, k + 1] * z) * (1 - y) + (g[i, j + 1, k] * (1 - z) + g[i, j + 1, k + 1] * z) * y) * (1 - x)
                       + ((g[i + 1, j, k] * (1 - z) + g[i + 1, j, k + 1] * z) * (1 - y)
                          + (g[i + 1, j + 1, k] * (1 - z) + g[i + 1, j + 1, k + 1] * z) * y) * x)
            best[b] = np.minimum(best[b], val)
    return np.clip(best / (4 * vox), -1.0, 1.0).reshape(B, res, res, res), margin
