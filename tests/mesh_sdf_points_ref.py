"""A numpy restatement of the posed-point distance query (include/partmanip_hip.h, pm_mesh_sdf_points_f32 and its grouped entry),
written from the contract's text and not from the kernel: `restate(..., dtype=np.float32)` rounds once per operation, as the
contract demands of the kernel (numpy's float32 arithmetic is IEEE single, its division a true division), so the kernel is compared
with it bit for bit; `dtype=np.float64` is the yardstick both are measured against.  Plus the seeded scenes the host and GPU tests
share.  Used by tests/test_mesh_sdf_points_host.py, tests/test_gpu_mesh_sdf_points.py and tests/test_gpu_contact_env.py."""
import numpy as np

from tests import mesh_tsdf_parts as P

SEGMENTS = (1, 64, 66)
NP_ = sum(SEGMENTS)


def sample(part, R, T, w, f):
    """One part's grid at the world points w (n, 3) under the pose (R, T), in dtype f: (values (n,), 1 where invalid; u (n, 3))."""
    g = np.asarray(part['sdf'], dtype=f)
    mn = np.asarray(part['bbox_min'], dtype=np.float32).astype(f)
    vs = f(np.float32(part['voxel_size']))
    shp = np.asarray(g.shape, dtype=f)
    d = w - T[None]
    q = np.stack([(d[:, 0] * R[0, j] + d[:, 1] * R[1, j]) + d[:, 2] * R[2, j] for j in range(3)], axis=1)
    u = (q - mn[None]) / vs
    ok = np.all((u >= 1) & (u - shp[None] <= -2), axis=1)
    val = np.ones(len(w), dtype=f)
    uo = u[ok]
    l = uo.astype(np.int64)                                  # u >= 1: truncation is the floor
    x, y, z = (uo - l.astype(f)).T
    i, j, k = l.T
    lo = (g[i, j, k] * (1 - z) + g[i, j, k + 1] * z) * (1 - y) + (g[i, j + 1, k] * (1 - z) + g[i, j + 1, k + 1] * z) * y
    hi = (g[i + 1, j, k] * (1 - z) + g[i + 1, j, k + 1] * z) * (1 - y) + (g[i + 1, j + 1, k] * (1 - z) + g[i + 1, j + 1, k + 1] * z) * y
    val[ok] = (lo * (1 - x) + hi * x) + f(0)
    return val, u


def pose_points(R, T, pts, carrier, f):
    """World points (n, 3) of one environment: ((R[a,0] x0 + R[a,1] x1) + R[a,2] x2) + T[a] with the carrier's pose, x for carrier
    -1; `ok` is False for a carrier outside [-1, M)."""
    M = R.shape[0]
    w = np.array(pts, dtype=f)
    ok = (carrier >= -1) & (carrier < M)
    for c in np.unique(carrier):
        if not 0 <= c < M:
            continue
        s = carrier == c
        x = np.asarray(pts, dtype=f)[s]
        w[s] = np.stack([((R[c, a, 0] * x[:, 0] + R[c, a, 1] * x[:, 1]) + R[c, a, 2] * x[:, 2]) + T[c, a] for a in range(3)], axis=1)
    return w, ok


def restate(parts, pose_R, pose_T, pts, carrier=None, own=None, p0=0, p1=None, segments=None, dtype=np.float32):
    """parts: the grid dicts (the rows of the library); pts (NP, 3) shared or (B, NP, 3); carrier (NP,) or None; own: None (ordinal p
    is part p under slot p) or per environment the list of (row, slot) of its own ordinals in order; [p0, p1) the ordinals sampled;
    segments: point counts or None.  Returns dict(dist (B, NP), arg (B, NP) int32, seg_min (B, NS), seg_arg (B, NS) int32, margin
    (B, NP): the smallest distance, in cells, of a sampled u to a border of its validity test)."""
    f = dtype
    with np.errstate(all="ignore"):
        R, T = np.asarray(pose_R, dtype=f), np.asarray(pose_T, dtype=f)
        B, M = R.shape[:2]
        pts = np.asarray(pts)                                # float32 as the kernel gets them; float64 only for the fp64 lattice check
        NP = pts.shape[-2]
        car = np.full(NP, -1, dtype=np.int64) if carrier is None else np.asarray(carrier, dtype=np.int64)
        dist, arg = np.ones((B, NP), dtype=f), np.full((B, NP), -1, dtype=np.int32)
        margin = np.full((B, NP), np.inf)
        bad = set()
        for b in range(B):
            rows = [(p, p) for p in range(M)] if own is None else own[b]
            named = set(range(M)) if own is None else ({s for _, s in rows if 0 <= s < M} | {int(c) for c in car if 0 <= c < M})
            if any(not (np.isfinite(R[b, s]).all() and np.isfinite(T[b, s]).all()) for s in named):
                dist[b] = np.nan
                bad.add(b)
                continue
            w, ok = pose_points(R[b], T[b], pts if pts.ndim == 2 else pts[b], car, f)
            m, am = np.ones(NP, dtype=f), np.full(NP, -1, dtype=np.int32)
            top = len(rows) if p1 is None else p1
            for t, (row, slot) in enumerate(rows):
                if not p0 <= t < top or not 0 <= slot < M:
                    continue
                val, u = sample(parts[row], R[b, slot], T[b, slot], w, f)
                val[~ok] = 1
                shp = np.asarray(parts[row]['sdf'].shape, dtype=np.float64)
                margin[b] = np.minimum(margin[b], np.minimum(np.abs(u - 1.0), np.abs(u - (shp - 2.0))).min(axis=1))
                first = (val < m) | (np.isnan(val) & ~np.isnan(m))
                am[first] = t
                m = np.where((val < m) | np.isnan(val), val, m)
            dist[b], arg[b] = m, am
        out = dict(dist=dist, arg=arg, margin=margin)
        if segments is not None:
            NS = len(segments)
            out["seg_min"], out["seg_arg"] = np.ones((B, NS), dtype=f), np.full((B, NS), -1, dtype=np.int32)
            for b in range(B):
                o = 0
                for s, cnt in enumerate(segments):
                    d = dist[b, o:o + cnt]
                    if b in bad:                                 # the NaN environment: NaN / -1 whatever the segment holds
                        out["seg_min"][b, s] = np.nan
                    elif cnt:
                        nan = np.flatnonzero(np.isnan(d))
                        i = int(nan[0]) if len(nan) else int(np.argmin(d))
                        out["seg_min"][b, s], out["seg_arg"][b, s] = d[i], o + i
                    o += cnt
        return out


# ---------------------------------------------------------------------------------------------- scenes
def lattice(res=10, size=P.SIZE, origin=P.ORIGIN, dtype=np.float32):
    """The workspace lattice's voxel centres (res^3, 3): float32(i) * float32(vox) + float32(origin) in float32 (what the TSDF kernel
    computes), or in float64 i * vox + float32(origin) (what mesh_tsdf_parts.restate computes)."""
    ii = np.stack(np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij"), axis=-1).reshape(-1, 3)
    o = np.asarray([np.float32(v) for v in origin])
    if dtype == np.float32:
        return ii.astype(np.float32) * np.float32(size / res) + o.astype(np.float32)
    return ii * (size / res) + o.astype(np.float64)


def scene(seed, B, n_parts=4, M=None):
    """n_parts synthetic 'cont' parts (differing shapes and voxel sizes), fp32 poses of M >= n_parts slots for B environments, and
    NP_ = 131 points in segments (1, 64, 66): body-frame points within 8 cm of their carrier's origin with carriers drawn from the
    slots [n_parts, M) and -1, so the points ride on bodies of their own and sense the parts under other poses; their placement puts
    a good share of them inside the parts' valid boxes (the tests assert it)."""
    M = n_parts + 3 if M is None else M
    rng = np.random.RandomState(seed)
    parts = P.make_parts(seed, "cont", n_parts=n_parts)
    R, T = P.random_poses(seed + 1, B, M)
    T[:, n_parts:] = T[:, :1] + rng.uniform(-0.02, 0.02, size=(B, M - n_parts, 3)).astype(np.float32)   # the carriers sit near part 0
    T[:, 1:n_parts] = T[:, :1] + rng.uniform(-0.06, 0.06, size=(B, n_parts - 1, 3)).astype(np.float32)  # and the parts overlap
    pts = rng.uniform(-0.08, 0.08, size=(NP_, 3)).astype(np.float32)
    carrier = rng.randint(n_parts, M, size=NP_)
    carrier[rng.rand(NP_) < 0.2] = -1
    world = (T[:, :1] + rng.uniform(-0.14, 0.14, size=(B, NP_, 3))).astype(np.float32)     # per-environment world points round part 0
    return dict(parts=parts, R=R, T=T, pts=pts, carrier=carrier, world=world, M=M, n_parts=n_parts)
