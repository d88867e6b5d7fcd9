"""Time the mesh bake (TSDFfromMesh.mesh2sdf -> pm_mesh_sdf_bake_f32, csrc/mesh_bake.hip) on one GPU: the finger (624 triangles,
51 x 67 x 54 voxels) and a 100 x 100 torus (20 000 triangles, 151 x 151 x 70 voxels: the size of the Franka's link0 at the 2 mm
grid).  Device events around warmed repetitions of the launch pair (record kernel + bake kernel), with the per-brick triangle cull
on and off.  Beside it:

 (a) a chunked tensor-library evaluation of the same contract (edge projections, face distance, solid angles through atan2) on
     the same GPU in the same process, timed on the first `--torch-voxels` voxels of the grid and reported as pairs per second
     (its time for the whole grid is that rate applied to all pairs: it has no cull and no data-dependent work);
 (b) the VALU-issue floor: VALU instructions of the inner loop per (voxel, triangle) pair, counted in the gfx950 disassembly of
     mesh_bake_kernel (134 when the pair takes the distance path, 71 when the cull skips it) x pairs / 64 lanes, over the chip's
     wave-instruction issue rate (compute units x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction).

Prints one JSON line (redirect it to profiles/mesh_bake_timing.json).

    python tools/time_mesh_bake.py [--tiny] [--reps 10]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from partmanip_amd import meshio, ops  # noqa: E402
from partmanip_amd.mesh2sdf import bake_grid_layout  # noqa: E402
from tools.timing import timed  # noqa: E402

DEV = "cuda:0"
TRUNC, VOXEL = 4 * 0.5 / 50, 0.002
VALU_PER_PAIR_FULL, VALU_PER_PAIR_CULLED = 134, 71          # counted in the disassembly of mesh_bake_kernel<true>
CLOCK_HZ, CYCLES_PER_WAVE_INSTR = 2.4e9, 2


def torus(R, r, nu, nv):
    u, v = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    pts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return pts.astype(np.float32), faces.astype(np.int64)


def dot(a, b):
    return (a * b).sum(-1)


def torch_bake(tri, pts, trunc, pairs_per_chunk=1 << 22):
    """The contract with tensor-library calls: tri (F, 3, 3), pts (n, 3) -> (n,) clamped signed distance."""
    A, B, C = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n_ = torch.cross(B - A, C - A, dim=-1)
    nn = n_.norm(dim=-1, keepdim=True)
    nhat = n_ / nn
    out = torch.empty(len(pts), device=pts.device)
    step = max(1, pairs_per_chunk // tri.shape[0])
    for lo in range(0, len(pts), step):
        p = pts[lo:lo + step, None]
        a, b, c = A - p, B - p, C - p
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = dot(a, torch.cross(b, c, dim=-1))
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        turn = torch.atan2(num, den).sum(dim=1)
        best = None
        inside = None
        for q, s, e in ((a, A, B), (b, B, C), (c, C, A)):
            d = e - s
            t = torch.clamp(-dot(q, d) / dot(d, d), 0, 1)
            x = q + d * t[..., None]
            d2 = dot(x, x)
            best = d2 if best is None else torch.minimum(best, d2)
            ok = dot(torch.cross(nhat, d, dim=-1), q) <= 0
            inside = ok if inside is None else inside & ok
        h = dot(a, nhat)
        d2 = torch.where(inside, h * h, best).min(dim=1)[0]
        dist = torch.sqrt(d2)
        out[lo:lo + step] = torch.clamp(torch.where(turn.abs() >= math.pi, -dist, dist), -trunc, trunc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="one coarse torus, 3 repetitions (the test suite's smoke run)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-voxels", type=int, default=32768)
    a = ap.parse_args()
    if a.tiny:
        cases = [("torus16x16", torus(0.0151, 0.0063, 16, 16))]
        reps, torch_voxels = 3, 4096
    else:
        cases = [("finger.stl", meshio.load_mesh(os.path.join(ROOT, "tests", "golden", "finger.stl"))),
                 ("torus100x100", torus(0.0811, 0.0294, 100, 100))]
        reps, torch_voxels = max(a.reps, 10), a.torch_voxels
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue_rate = cus * 4 * CLOCK_HZ / CYCLES_PER_WAVE_INSTR
    rows = []
    for name, (v, f) in cases:
        f = meshio.drop_double_corner_faces(v, f)
        shape, centre, bbox_min = bake_grid_layout(v, TRUNC, VOXEL)
        tri = torch.from_numpy(v[f]).to(DEV)
        cells, F = shape[0] * shape[1] * shape[2], len(f)
        pairs = cells * F
        on = lambda: ops.mesh_sdf_bake(tri, shape, VOXEL, centre.tolist(), TRUNC, True)        # noqa: E731
        off = lambda: ops.mesh_sdf_bake(tri, shape, VOXEL, centre.tolist(), TRUNC, False)      # noqa: E731
        g_on, g_off = on(), off()                                                              # warm both
        torch.cuda.synchronize()
        same_bits = bool(torch.equal(g_on.view(torch.int32), g_off.view(torch.int32)))
        ms_on, ms_off = [], []
        for _ in range(2):                                                                     # alternate in one process
            ms_on.append(timed(on, (reps + 1) // 2))
            ms_off.append(timed(off, (reps + 1) // 2))
        h_on, h_off = float(np.mean(ms_on)), float(np.mean(ms_off))
        # (a) the tensor-library evaluation on the first torch_voxels voxels
        nv_ = min(torch_voxels, cells)
        idx = torch.arange(nv_)
        ax = [(torch.arange(s) - s // 2).float() * VOXEL + centre[k] for k, s in enumerate(shape)]
        pts = torch.stack([ax[0][idx // (shape[1] * shape[2])], ax[1][(idx // shape[2]) % shape[1]], ax[2][idx % shape[2]]], dim=1).to(DEV)
        ref = lambda: torch_bake(tri, pts, TRUNC)                                              # noqa: E731
        t_out = ref()
        torch.cuda.synchronize()
        t_ms = timed(ref, 2)
        diff = float((t_out - g_on.reshape(-1)[:nv_]).abs().max())
        torch_pairs_per_s = nv_ * F / (t_ms * 1e-3)
        torch_full_ms = pairs / torch_pairs_per_s * 1e3
        floor_ms = VALU_PER_PAIR_FULL * pairs / 64 / issue_rate * 1e3
        rows.append(dict(mesh=name, triangles=F, shape=list(shape), voxels=cells, pairs=pairs,
                         hip_ms=round(h_on, 4), hip_ms_cull_off=round(h_off, 4), hip_ms_rounds=[round(x, 4) for x in ms_on],
                         hip_calls=2 * ((reps + 1) // 2), pairs_per_s=round(pairs / (h_on * 1e-3)),
                         pairs_per_s_cull_off=round(pairs / (h_off * 1e-3)), cull_on_equals_cull_off_bits=same_bits,
                         torch_voxels=nv_, torch_ms_on_those=round(t_ms, 3), torch_pairs_per_s=round(torch_pairs_per_s),
                         torch_ms=round(torch_full_ms, 2), speedup_over_torch=round(torch_full_ms / h_on, 1),
                         max_abs_diff_hip_vs_torch=diff, valu_floor_ms_cull_off=round(floor_ms, 4),
                         share_of_valu_floor=round(floor_ms / h_off, 4)))
    print(json.dumps(dict(tool="time_mesh_bake", device=torch.cuda.get_device_name(0), compute_units=cus, bound="VALU issue",
                          valu_per_pair_full=VALU_PER_PAIR_FULL, valu_per_pair_culled=VALU_PER_PAIR_CULLED,
                          wave_instr_per_s=issue_rate, trunc=TRUNC, voxel_size=VOXEL, cases=rows)))


if __name__ == "__main__":
    main()
