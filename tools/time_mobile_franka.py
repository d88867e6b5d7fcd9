"""Time OpenDrawerTensors.begin_step / end_step with the mobile Franka (pm_franka_control_mobile_f32 + pm_open_drawer_reset_f32,
pm_open_drawer_post_f32 at 12 DOFs / 17 bodies) beside the fixed-base Franka (pm_franka_control_f32, 9 DOFs / 13 bodies) in one
process, alternating: 13 posed parts, three cabinet types with (bodies, DOFs) = (3, 1), (5, 3), (4, 2), N in {64, 1024, 4096}, the 'ik'
drive with random_reset.  Device events around warmed calls.  Prints one JSON line and writes it to
profiles/mobile_franka_timing.json (--out; nothing is written with --tiny).

No threshold is set on the times: both paths are launch-bound, and the number to read a mobile time against is the fixed-base time of
the same run.  device_ops: the number of ATen operations the wrapper dispatches to the device per call (views and metadata operations
excluded) plus one per kernel (two in begin_step, one in end_step); it must be the same for both robots, and the tool fails if it is
not.

    python tools/time_mobile_franka.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.tasks import Franka, MobileFranka, OpenDrawerTensors  # noqa: E402
from partmanip_amd.tasks.open_drawer import build_masks  # noqa: E402
from tools.timing import count_ops, timed  # noqa: E402

DEV = "cuda:0"
TYPES = ((3, 1, 1, 2, 0), (5, 3, 2, 4, 2), (4, 2, 3, 1, 1))
ROOT = [0.3, -0.1, 0.05, 0.2, -0.3, 0.6, 0.7]
KERNELS = dict(begin_step=2, end_step=1)


def make_side(N, robot, nl, seed=41):
    """A task around `robot` with its state tensors: (task, {name: call})."""
    nrb, nd = robot.num_rigid_body, robot.num_dofs
    types = [TYPES[i % 3] for i in range(N)]
    rbm, dfm, B, D = build_masks(nrb, nd, *[[ty[c] for ty in types] for c in range(5)])
    g = torch.Generator(device=DEV).manual_seed(seed)
    rb = torch.rand(B, 13, device=DEV, generator=g) - 0.5
    rb[:, 3:7] = torch.nn.functional.normalize(torch.randn(B, 4, device=DEV, generator=g), dim=-1)
    root = torch.randn(N, 2, 13, device=DEV, generator=g) * 0.1
    root[:, :, 3:7] = torch.nn.functional.normalize(torch.randn(N, 2, 4, device=DEV, generator=g), dim=-1)
    dof = torch.stack([torch.rand(D, device=DEV, generator=g) * 0.03, torch.randn(D, device=DEV, generator=g)], dim=-1).contiguous()
    half = torch.tensor([0.02, 0.08, 0.015], device=DEV)
    signs = torch.tensor([[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, -1], [-1, 1, -1], [-1, 1, 1], [-1, -1, 1]],
                         device=DEV, dtype=torch.float32)
    task = OpenDrawerTensors(N, DEV, {"explore_step": 40, "random_reset": True}, 1 / 60, rbm, dfm, np.arange(N) % 3,
                             (signs * half).expand(N, 8, 3).contiguous(), torch.tensor([1.0, 0, 0], device=DEV).expand(N, 3).contiguous(),
                             torch.zeros(N, device=DEV), torch.full((N,), 0.2, device=DEV), 3, num_rigid_bodies=B, num_dof_states=D,
                             robot=robot)
    jac = torch.randn(N, nl, 6, nd, device=DEV, generator=g)
    act = torch.rand(N, robot.num_actions, device=DEV, generator=g) * 2 - 1
    u = torch.rand(N, 4, device=DEV, generator=g)
    pa = torch.zeros(D, device=DEV)
    return task, dict(begin_step=lambda: task.begin_step(act, jac, dof, root, pa, u=u), end_step=lambda: task.end_step(rb, dof, root))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 5, 3 calls")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/mobile_franka_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [5] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 200
    rows = []
    for N in sizes:
        cfg = {"driveMode": "ik", "root": ROOT}
        sides = dict(mobile=make_side(N, MobileFranka(cfg, 1 / 60, N, DEV), 16), fixed=make_side(N, Franka(cfg, 1 / 60, N, DEV), 12))
        fns = {side: d for side, (_, d) in sides.items()}
        for d in fns.values():                                 # warm everything; end_step first, as a run does
            for k in ("end_step", "begin_step", "end_step", "begin_step"):
                d[k]()
        torch.cuda.synchronize()
        finite = {side: bool(torch.isfinite(task.pos_act).all()) and bool(torch.isfinite(task.rew_buf).all()) for side, (task, _) in sides.items()}
        ops = {side: {k: count_ops(fn) + KERNELS[k] for k, fn in d.items()} for side, d in fns.items()}
        if ops["mobile"] != ops["fixed"]:
            raise SystemExit(f"device operations per step differ: {ops}")
        ms = {side: {k: [] for k in d} for side, d in fns.items()}
        for _ in range(3):                                     # alternate in one process
            for side, d in fns.items():
                for k, fn in d.items():
                    ms[side][k].append(timed(fn, calls))
        mean = {side: {k: float(np.mean(v)) for k, v in d.items()} for side, d in ms.items()}
        rows.append(dict(N=N, mobile_ms={k: round(v, 5) for k, v in mean["mobile"].items()},
                         fixed_ms={k: round(v, 5) for k, v in mean["fixed"].items()},
                         mobile_over_fixed={k: round(mean["mobile"][k] / mean["fixed"][k], 3) for k in mean["mobile"]},
                         device_ops=ops["mobile"], device_ops_fixed=ops["fixed"], outputs_finite=finite,
                         mobile_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["mobile"].items()},
                         fixed_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["fixed"].items()}, calls=3 * calls))
        del sides, fns
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_mobile_franka", device=torch.cuda.get_device_name(0),
                           mobile=dict(dofs=12, robot_bodies=17, jacobian_links=16, actions=10),
                           fixed=dict(dofs=9, robot_bodies=13, jacobian_links=12, actions=7), parts=13, sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mobile_franka_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
