"""Time PCfromMesh.query_pc (pm_mesh_pc_query_f32) beside a tensor-library evaluation of the same contract (the reference's
bmm over every point of every part + index through a host permutation, mesh2pc.py:61-64), in one process, alternating: 12 parts x
1024 points, B in {64 (the size of the reference's own __main__), 1024, 4096}.  Device events around warmed calls.
Prints one JSON line and writes it to profiles/mesh_pc_timing.json (--out; nothing is written with --tiny).  hip_ms: 'random'
(the default: host randperm + its copy + one launch, what a caller of the reference's interface pays), 'sel' (a selection already on the device: the launch alone), 'all' (every point, 12 x the output) and 'fps'
(the 'all' launch into a scratch cloud + ops.fps + a second launch).  share_of_output_bandwidth_floor = (12 B K output bytes /
6.29 TB/s, the measured HBM copy rate of the MI355X) / hip_ms, for 'sel' and 'all'.

    python tools/time_mesh_pc.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.mesh2pc import PCfromMesh, random_poses  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, timed  # noqa: E402

DEV = "cuda:0"
M, P = 12, 1024


def synthetic_parts(m, p, seed=21):
    """Points on the surfaces of seeded boxes with half-extents of 2-7 cm."""
    rng = np.random.RandomState(seed)
    parts = []
    for _ in range(m):
        half = rng.uniform(0.02, 0.07, size=3)
        x = rng.uniform(-1, 1, size=(p, 3))
        axis, side = rng.randint(0, 3, size=p), rng.choice([-1.0, 1.0], size=p)
        x[np.arange(p), axis] = side
        parts.append(x * half)
    return np.stack(parts).astype(np.float32)


def torch_query(all_pc, R, T, num_envs, num_points):
    """mesh2pc.py:61-64 with tensor-library calls."""
    posed = torch.bmm(all_pc, R.reshape(-1, 3, 3).transpose(-1, -2)) + T.reshape(-1, 1, 3)
    posed = posed.reshape(num_envs, -1, 3)
    randperm = torch.randperm(posed.shape[1])
    return posed[:, randperm[:num_points], :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="B = 4, 3 parts x 64 points, 3 calls (the test suite's smoke run)")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/mesh_pc_timing.json; "
                                                "none with --tiny)")
    ap.add_argument("--modes", default="random,sel,all,fps", help="which hip_ms columns to measure")
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    m, p = (3, 64) if a.tiny else (M, P)
    calls = 3 if a.tiny else 20
    parts = synthetic_parts(m, p)
    rows = []
    for B in sizes:
        pc = PCfromMesh(B, DEV, num_points=p, part_pcs=parts)
        R, T = random_poses(B, m, torch.Generator(device=DEV).manual_seed(22), DEV)
        all_pc = pc.all_pc                                                   # the reference's per-environment repeat
        sel = torch.randperm(m * p, device=DEV)[:p].to(torch.int32)
        out_k = torch.empty(B, 3 * p, device=DEV)
        out_all = torch.empty(B, 3 * m * p, device=DEV)
        fns = dict(random=lambda: pc.query_pc(R, T, out=out_k), sel=lambda: pc.query_pc(R, T, out=out_k, sel=sel),
                   all=lambda: pc.query_pc(R, T, out=out_all, select='all'), fps=lambda: pc.query_pc(R, T, out=out_k, select='fps'))
        fns = {k: fn for k, fn in fns.items() if k in a.modes.split(",")}
        ref = lambda: torch_query(all_pc, R, T, B, p)                        # noqa: E731
        for fn in list(fns.values()) + [ref]:                                # warm everything
            fn()
        torch.cuda.synchronize()
        # same contract: under one seed both sides pick the same subset
        torch.manual_seed(5)
        got = pc.query_pc(R, T).clone()
        torch.manual_seed(5)
        diff = float((got - ref()).abs().max())
        fps_calls = 2 if not a.tiny and B >= 1024 else calls                 # fps walks 12288 points per pick
        ms = {k: [] for k in fns}
        torch_ms = []
        for _ in range(2):                                                   # alternate in one process
            for k, fn in fns.items():
                ms[k].append(timed(fn, fps_calls if k == 'fps' else calls))
            torch_ms.append(timed(ref, calls))
        hip = {k: float(np.mean(v)) for k, v in ms.items()}
        tt = float(np.mean(torch_ms))
        floor = {'sel': 12.0 * B * p / HBM_BYTES_PER_S * 1e3, 'all': 12.0 * B * m * p / HBM_BYTES_PER_S * 1e3}
        rows.append(dict(B=B, hip_ms={k: round(v, 5) for k, v in hip.items()}, torch_ms=round(tt, 5),
                         speedup={k: round(tt / v, 2) for k, v in hip.items() if k in ('random', 'sel')},
                         floor_ms={k: round(v, 6) for k, v in floor.items()},
                         share_of_output_bandwidth_floor={k: round(floor[k] / hip[k], 4) for k in floor if k in hip},
                         hip_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms.items()},
                         torch_ms_rounds=[round(x, 5) for x in torch_ms], calls=2 * calls, fps_calls=2 * fps_calls,
                         max_abs_diff_hip_vs_torch=diff))
        del pc, all_pc, out_k, out_all
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_mesh_pc", device=torch.cuda.get_device_name(0), parts=m, points_per_part=p, bound="bandwidth",
                           hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mesh_pc_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
