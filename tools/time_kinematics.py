"""Time KinematicSim.step (pm_articulation_step_f32: drive, forward kinematics, velocities and the Jacobian in one launch) beside a
tensor-library evaluation of the same contract (this tool's own batched quaternion / cross-product restatement of
include/partmanip_hip.h's description), in one process, alternating: the fixed-base Franka (13 bodies, 9 DOFs) and the mobile one
(16 bodies, 12 DOFs) from the URDFs under tests/golden, N in {64, 1024, 4096}, exact tracking of targets near the current pose.
Device events around warmed calls.  Prints one JSON line and writes it to profiles/kinematics_timing.json (--out; nothing is written
with --tiny).

device_ops: ATen operations dispatched to the device per step (views and metadata operations excluded), plus one for the kernel on
the HIP side.  share_of_bytes_floor = (output bytes of a step, (nb 13 + (nb - 1) 6 nd + 2 nd) floats per environment, / 6.29 TB/s, the
measured HBM copy rate of the MI355X) / hip_ms.  envs_per_block is what the launch rule of csrc/task_common.h chose.  No threshold is
set anywhere: at these sizes the step is expected to be launch-bound, like the task kernels.

    python tools/time_kinematics.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from partmanip_amd.kinematics import KinematicSim  # noqa: E402
from partmanip_amd.urdf import PRISMATIC, REVOLUTE, load_urdf  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, count_ops, timed  # noqa: E402

DEV = "cuda:0"
DT = 1.0 / 60.0
URDFS = dict(fixed="franka_panda_sdf.urdf", mobile="franka_panda_sdf_mobile.urdf")
BASE = (0.3, -0.1, 0.05, 0.0, 0.0, 0.6, 0.8)


def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack((aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz), -1)


def qrot(q, v):
    u, w = q[..., :3], q[..., 3:]
    c = torch.cross(u, v.expand_as(u), dim=-1)
    return v + 2 * (w * c + torch.cross(u, c, dim=-1))


class TorchSim:
    """The contract with tensor-library calls batched over the environments (a Python loop over the bodies, as the chain demands)."""

    def __init__(self, tree, N, base_pose):
        f = dict(dtype=torch.float32, device=DEV)
        self.tree, self.N = tree, N
        self.lo, self.hi = torch.tensor(tree.lower, **f), torch.tensor(tree.upper, **f)
        self.oq, self.ot, self.ax = (torch.tensor(a, **f) for a in (tree.origin_q, tree.origin_t, tree.axis))
        bp = torch.tensor(base_pose, **f)
        self.bp, self.bq = bp[:3].expand(N, 3), (bp[3:] / bp[3:].norm()).expand(N, 4)
        self.anc = [[b2 for b2 in self._path(b) if tree.jtype[b2]] for b in range(tree.num_bodies)]

    def _path(self, b):
        while b >= 0:
            yield b
            b = int(self.tree.parent[b])

    def step(self, dof_state, targets):
        tr, N = self.tree, self.N
        q = dof_state[..., 0]
        qn = torch.clamp(targets, self.lo, self.hi)
        qd = (qn - q) / DT
        dof_state.copy_(torch.stack((qn, qd), -1))
        pos, quat, jp, ja = [], [], {}, {}
        for b in range(tr.num_bodies):
            p = int(tr.parent[b])
            pp, pq = (self.bp, self.bq) if p < 0 else (pos[p], quat[p])
            x = pp + qrot(pq, self.ot[b])
            fq = qmul(pq, self.oq[b].expand(N, 4))
            d = int(tr.dof[b])
            if tr.jtype[b] == REVOLUTE:
                ja[b], jp[b] = qrot(fq, self.ax[b]), x
                h = qn[:, d:d + 1] / 2
                fq = qmul(fq, torch.cat((self.ax[b] * torch.sin(h), torch.cos(h)), -1))
            elif tr.jtype[b] == PRISMATIC:
                ja[b] = qrot(fq, self.ax[b])
                x = x + ja[b] * qn[:, d:d + 1]
            pos.append(x), quat.append(fq / fq.norm(dim=-1, keepdim=True))
        jac = torch.zeros(N, tr.num_bodies, 6, tr.num_dofs, dtype=torch.float32, device=DEV)
        for b in range(tr.num_bodies):
            for jb in self.anc[b]:
                d = int(tr.dof[jb])
                if tr.jtype[jb] == REVOLUTE:
                    jac[:, b, :3, d] = torch.cross(ja[jb], pos[b] - jp[jb], dim=-1)
                    jac[:, b, 3:, d] = ja[jb]
                else:
                    jac[:, b, :3, d] = ja[jb]
        vel = torch.einsum("nbrd,nd->nbr", jac, qd)
        return torch.cat((torch.stack(pos, 1), torch.stack(quat, 1), vel), -1), dof_state, jac[:, 1:].contiguous()


def envs_per_block(N, nb, nd, eb=64, grid_min=512, lds_max=49152):
    """ts_envs_per_block of csrc/task_common.h at this kernel's bytes per environment."""
    env_bytes = 8 * ((7 * nb) | 1) + 4 * ((13 * nb + 5 * nd) | 1)
    while eb > 1 and (eb * env_bytes > lds_max or (eb > 4 and -(-N // eb) < grid_min)):
        eb >>= 1
    return eb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 5, 3 calls")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/kinematics_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [5] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 200
    rows = []
    for name, file in URDFS.items():
        tree = load_urdf(os.path.join(ROOT, "tests", "golden", file))
        nb, nd = tree.num_bodies, tree.num_dofs
        for N in sizes:
            g = torch.Generator(device=DEV).manual_seed(17)
            lo, hi = torch.tensor(tree.lower, dtype=torch.float32, device=DEV), torch.tensor(tree.upper, dtype=torch.float32, device=DEV)
            q0 = lo + (0.2 + 0.6 * torch.rand(N, nd, device=DEV, generator=g)) * (hi - lo)
            targets = (q0 + 0.01 * (hi - lo) * (torch.rand(N, nd, device=DEV, generator=g) - 0.5)).contiguous()
            sim = KinematicSim(tree, N, DEV, DT, base_pose=BASE)
            ref = TorchSim(tree, N, BASE)
            sim.set_dof_state(q0)
            ref_state = sim.dof_state.clone()
            rb, dof, jac = sim.step(targets)
            rb_t, dof_t, jac_t = ref.step(ref_state, targets)
            diff = dict(rigid_body=float((rb - rb_t).abs().max()), dof_state=float((dof - dof_t).abs().max()),
                        jacobian=float((jac - jac_t).abs().max()))
            fns = dict(hip=lambda: sim.step(targets), torch=lambda: ref.step(ref_state, targets))
            for fn in fns.values():
                fn(), fn()
            torch.cuda.synchronize()
            ops = dict(hip=count_ops(fns["hip"]) + 1, torch=count_ops(fns["torch"]))
            ms = {side: [] for side in fns}
            for _ in range(3):                                 # alternate in one process
                for side, fn in fns.items():
                    ms[side].append(timed(fn, calls))
            mean = {side: float(np.mean(v)) for side, v in ms.items()}
            out_bytes = 4 * (nb * 13 + (nb - 1) * 6 * nd + 2 * nd) * N
            floor = out_bytes / HBM_BYTES_PER_S * 1e3
            rows.append(dict(robot=name, bodies=nb, dofs=nd, N=N, envs_per_block=envs_per_block(N, nb, nd), hip_ms=round(mean["hip"], 5),
                             torch_ms=round(mean["torch"], 5), speedup=round(mean["torch"] / mean["hip"], 2), device_ops=ops,
                             output_bytes=out_bytes, floor_ms=round(floor, 7), share_of_bytes_floor=round(floor / mean["hip"], 5),
                             hip_ms_rounds=[round(x, 5) for x in ms["hip"]], torch_ms_rounds=[round(x, 5) for x in ms["torch"]],
                             calls=3 * calls, max_abs_diff_hip_vs_torch=diff))
            del sim, ref
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_kinematics", device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(ROOT, "profiles", "kinematics_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
