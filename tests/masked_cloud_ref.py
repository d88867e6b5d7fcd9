"""numpy statement of the masked depth cloud (TSDFVolume.depth2pc_masked), from plain indexing over a cropped world cloud -- the
reference's own (tests/golden/depth2pc_small.npz) or oracle.ref_cpu.depth2pc's: keep the non-zero rows plus the first zero row, in
order, remember their indices, sample them with oracle.ref_cpu.fps, read seg at the remembered indices.  Nothing here calls the code
under test."""
import numpy as np

from oracle import ref_cpu


def plus_zero_rows(cloud):
    """The cloud (..., 3) with every row that equals (0, 0, 0) by value written as +0.0.  The reference zeroes a cropped point by
    multiplying it with its mask, which keeps the signs (-0.0 where the coordinate was negative); pm_depth_backproject_f32 has always
    stored +0.0 there.  Equal by value, so no selection changes; this makes the reference's data comparable bit for bit."""
    out = np.array(cloud, dtype=np.float32, copy=True)
    out[(out == 0).all(axis=-1)] = 0.0
    return out


def compact(world):
    """world (P, 3) -> (xyz (n, 3), src (n,) int64): the rows that differ from (0, 0, 0) by value plus the first row that does not,
    in ascending order."""
    zero = (world == 0).all(axis=1)
    keep = ~zero
    if zero.any():
        keep[int(np.argmax(zero))] = True
    src = np.flatnonzero(keep)
    return world[src], src


def sample(xyz, K):
    """Indices (K,) of farthest point sampling that keeps sampling once the cloud is exhausted: every distance is then zero and the
    lowest index wins, where oracle.ref_cpu.fps pads with -1."""
    idx = ref_cpu.fps(xyz[None], K)[0]
    return np.where(idx < 0, 0, idx)


def masked_cloud(world, seg, K, zero_label=0.0, cap=None):
    """world (B, P, 3) float32, seg (B, P) ints -> (rows (B, K, 4) float32, xyz list, src list, lengths (B,)): per environment the
    compact cloud (its first `cap` rows where cap is given), K sampled rows of it and, as the fourth column, seg at the row's source
    pixel -- zero_label for the row (0, 0, 0)."""
    B = world.shape[0]
    rows = np.empty((B, K, 4), dtype=np.float32)
    clouds, srcs, lengths = [], [], np.empty(B, dtype=np.int64)
    for b in range(B):
        xyz, src = compact(world[b])
        if cap is not None:
            xyz, src = xyz[:cap], src[:cap]
        idx = sample(xyz, K)
        rows[b, :, :3] = xyz[idx]
        label = seg[b].reshape(-1)[src[idx]].astype(np.float32)
        rows[b, :, 3] = np.where((xyz[idx] == 0).all(axis=1), np.float32(zero_label), label)
        clouds.append(xyz), srcs.append(src)
        lengths[b] = len(src)
    return rows, clouds, srcs, lengths
