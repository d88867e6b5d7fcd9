"""Time TSDFfromMesh.query_tsdf (pm_mesh_tsdf_query_f32) beside a plain tensor-library evaluation of the same contract, in one
process, alternating: 12 synthetic parts, res = 50, B in {64 (the size of the reference's own __main__, mesh2sdf.py:355-373), 1024,
4096}.  Device events around >= 20 warmed HIP calls (the tensor-library side gets as many calls as fit ~2 s, at least 2).
Prints one JSON line: ms per call for both, environments/s, and the HIP call's share of its bandwidth floor = (4 B res^3 output
bytes + one read of the part grids) / 6.29 TB/s (the measured HBM copy rate of the MI355X).

    python tools/time_mesh_tsdf.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.mesh2sdf import TSDFfromMesh  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, timed  # noqa: E402

DEV = "cuda:0"
RES, SIZE, M = 50, 0.5, 12


def synthetic_parts(seed=11):
    """Boxes and ellipsoids, half-extents 2-7 cm, on a 4 mm grid that covers the truncation band plus five cells."""
    rng = np.random.RandomState(seed)
    trunc = 4 * SIZE / RES
    parts = []
    for i in range(M):
        half = rng.uniform(0.02, 0.07, size=3)
        vs = 0.004
        shape = np.ceil((2 * half + 2 * trunc) / vs).astype(np.int64) + 10
        idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
        pts = (idx - shape // 2) * vs
        if i % 2 == 0:
            q = np.abs(pts) - half
            d = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
        else:
            k0, k1 = np.linalg.norm(pts / half, axis=-1), np.linalg.norm(pts / (half * half), axis=-1)
            d = k0 * (k0 - 1.0) / np.maximum(k1, 1e-12)
        parts.append({'sdf': np.clip(d, -trunc, trunc).astype(np.float32), 'bbox_min': pts.reshape(-1, 3).min(axis=0).astype(np.float32),
                      'voxel_size': vs})
    return parts


def poses(B, seed=12):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(B, M, 4, generator=g), dim=-1)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(B, M, 3, 3)
    u = torch.rand(B, M, 3, generator=g)
    T = torch.stack([u[..., 0] * 0.4 - 0.2, u[..., 1] * 0.4 - 0.2, u[..., 2] * 0.35], dim=-1)
    return R.to(DEV).contiguous(), T.to(DEV).contiguous()


def torch_query(obj, shapes, offs, R, T, out, chunk=64):
    """Steps 1-4 of the contract with tensor-library calls, a loop over the parts on the un-padded grids, `chunk` environments
    at a time so that the (chunk, n, 3) intermediates fit."""
    c = obj.vox_coords
    for b0 in range(0, R.shape[0], chunk):
        Rc, Tc = R[b0:b0 + chunk], T[b0:b0 + chunk]
        best = obj.vox_coords[:, 2].unsqueeze(0).repeat(Rc.shape[0], 1)
        for p in range(obj.part_num):
            shp = obj.sdf_field_res[p]
            u = (torch.bmm(c[None] - Tc[:, p, None, :], Rc[:, p]) - obj.sdf_bbox_min[p]) / obj.sdf_voxel_size[p]
            ok = ((u >= 1) & (u - shp <= -2)).all(dim=-1)
            u = u * ok[..., None]
            l = u.long()
            x, y, z = (u - l).unbind(-1)
            ry, rz = shapes[p][1], shapes[p][2]                        # host copies: no device read in the loop
            sy, sx = rz, rz * ry
            i0 = offs[p] + (l[..., 0] * ry + l[..., 1]) * rz + l[..., 2]
            f = obj.sdf_field
            val = ((f[i0] * (1 - z) + f[i0 + 1] * z) * (1 - y) + (f[i0 + sy] * (1 - z) + f[i0 + sy + 1] * z) * y) * (1 - x) \
                + ((f[i0 + sx] * (1 - z) + f[i0 + sx + 1] * z) * (1 - y) + (f[i0 + sx + sy] * (1 - z) + f[i0 + sx + sy + 1] * z) * y) * x
            best = torch.minimum(best, torch.where(ok, val, torch.ones_like(val)))
        out[b0:b0 + chunk] = torch.clamp(best / obj.sdf_trunc, -1, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="B = 4, 3 calls (the test suite's smoke run)")
    ap.add_argument("--sizes", default="64,1024,4096")
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    hip_calls = 3 if a.tiny else 20
    parts = synthetic_parts()
    rows = []
    for B in sizes:
        obj = TSDFfromMesh(B, SIZE, RES, DEV, sdf_dicts=parts)
        shapes, offs = obj.sdf_field_res.cpu().tolist(), obj.sdf_field_off.cpu().tolist()
        R, T = poses(B)
        n = RES ** 3
        out_h = torch.empty(B, n, device=DEV)
        out_t = torch.empty(B, n, device=DEV)
        hip = lambda: obj.query_tsdf(R, T, out=out_h)                      # noqa: E731
        ref = lambda: torch_query(obj, shapes, offs, R, T, out_t)                        # noqa: E731
        hip(); hip(); ref()                                                # warm both
        torch.cuda.synchronize()
        t_one = timed(ref, 1)
        torch_calls = 3 if a.tiny else int(max(2, min(20, 2000.0 / max(t_one, 1e-3))))
        hip_ms, torch_ms = [], []
        for _ in range(2):                                                 # alternate in one process
            hip_ms.append(timed(hip, hip_calls))
            torch_ms.append(timed(ref, torch_calls))
        h, tt = float(np.mean(hip_ms)), float(np.mean(torch_ms))
        diff = float((out_h - out_t).abs().max())
        floor_ms = (4.0 * B * n + 4.0 * obj.sdf_field.numel()) / HBM_BYTES_PER_S * 1e3
        rows.append(dict(B=B, hip_ms=round(h, 5), torch_ms=round(tt, 4), hip_env_per_s=round(B / (h * 1e-3)),
                         torch_env_per_s=round(B / (tt * 1e-3)), speedup=round(tt / h, 1), floor_ms=round(floor_ms, 5),
                         hip_share_of_floor=round(floor_ms / h, 4), hip_calls=2 * hip_calls, torch_calls=2 * torch_calls,
                         hip_ms_rounds=[round(v, 5) for v in hip_ms], max_abs_diff_hip_vs_torch=diff,
                         valid_lt1_fraction=round(float((out_h < 1).float().mean()), 3)))
        del obj, out_h, out_t
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="time_mesh_tsdf", device=torch.cuda.get_device_name(0), res=RES, parts=M, bound="bandwidth",
                          hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=rows)))


if __name__ == "__main__":
    main()
