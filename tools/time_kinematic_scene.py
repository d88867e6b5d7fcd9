"""Time the object launch of KinematicSim.step (pm_articulation_objects_step_f32: one cabinet tree per environment posed into the flat
tensors, with the hold rule on) beside a tensor-library evaluation of the same contract (this tool's own batched restatement of
include/partmanip_hip.h's description: a Python loop over the bodies, velocities propagated down the tree), in one process,
alternating.  Three object sizes, each as a library of its own: the synthetic cabinets of tests/cabinet_fixtures.py, A (2 bodies,
1 DOF), B (7 bodies, 3 DOFs), C (64 bodies, 64 DOFs); N in {64, 1024, 4096}; and, HIP side only, the three interleaved as e % 3 (the
launch is then sized for the largest tree).  Device events around warmed calls.  Prints one JSON line and writes it to
profiles/kinematic_scene_timing.json (--out; nothing is written with --tiny).

bytes_written = (13 nb + 2) floats per environment (the body rows and the target DOF row); share_of_bytes_floor = (bytes_written /
6.29 TB/s, the measured HBM copy rate of the MI355X) / hip_ms.  device_ops: ATen operations dispatched to the device per step on the
tensor-library side, one launch on the HIP side.  No threshold is set anywhere: the launch is expected to be launch-bound, like its
sibling (tools/time_kinematics.py).

    python tools/time_kinematic_scene.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from partmanip_amd.kinematics import ObjectLibrary  # noqa: E402
from partmanip_amd.urdf import PRISMATIC, REVOLUTE  # noqa: E402
from tests import cabinet_fixtures as CF  # noqa: E402
from tools.time_kinematics import qmul, qrot  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, count_ops, timed  # noqa: E402

DEV = "cuda:0"
DT = 1.0 / 60.0
POSE = (-0.6, 0.0, 0.5, 0.0, 0.0, 1.0, 0.0)


class TorchObjects:
    """The contract for ONE tree with tensor-library calls batched over the environments."""

    def __init__(self, tree, N, tgt):
        f = dict(dtype=torch.float32, device=DEV)
        self.tree, self.N, self.tgt = tree, N, tgt
        self.lo, self.hi = float(np.float32(tree.lower[tgt])), float(np.float32(tree.upper[tgt]))
        self.oq, self.ot, self.ax = (torch.tensor(a, **f) for a in (tree.origin_q, tree.origin_t, tree.axis))

    def step(self, dof_state, pose, tips, hold):
        tr, N = self.tree, self.N
        q, qd = dof_state[..., 0].clone(), dof_state[..., 1].clone()
        bp, bq = pose[:, :3], pose[:, 3:] / pose[:, 3:].norm(dim=-1, keepdim=True)
        zero = torch.zeros(N, 3, dtype=torch.float32, device=DEV)
        pos, quat, lin, ang = [], [], [], []
        for b in range(tr.num_bodies):
            p = int(tr.parent[b])
            pp, pq, pv, pw = (bp, bq, zero, zero) if p < 0 else (pos[p], quat[p], lin[p], ang[p])
            x = pp + qrot(pq, self.ot[b])
            fq = qmul(pq, self.oq[b].expand(N, 4))
            v, w = pv + torch.cross(pw, x - pp, dim=-1), pw
            d, jt = int(tr.dof[b]), int(tr.jtype[b])
            if jt in (REVOLUTE, PRISMATIC):
                a = qrot(fq, self.ax[b])
                if d == self.tgt:                              # the hold rule, where the walk reaches the target joint
                    pm, vm = tips[:, :, :3].mean(1), tips[:, :, 7:10].mean(1)
                    c = a if jt == PRISMATIC else torch.cross(a, pm - x, dim=-1)
                    cc = (c * c).sum(-1)
                    dq = torch.where(cc == 0, torch.zeros_like(cc), DT * (c * vm).sum(-1) / cc)
                    qn = torch.where(hold, torch.clamp(q[:, d] + dq, self.lo, self.hi), q[:, d])
                    qd[:, d] = (qn - q[:, d]) / DT
                    q[:, d] = qn
                    dof_state[:, d, 0], dof_state[:, d, 1] = qn, qd[:, d]
                if jt == REVOLUTE:
                    h = q[:, d:d + 1] / 2
                    fq = qmul(fq, torch.cat((self.ax[b] * torch.sin(h), torch.cos(h)), -1))
                    w = w + a * qd[:, d:d + 1]
                else:
                    x = x + a * q[:, d:d + 1]
                    v = v + a * qd[:, d:d + 1]
            pos.append(x), quat.append(fq / fq.norm(dim=-1, keepdim=True)), lin.append(v), ang.append(w)
        return torch.cat((torch.stack(pos, 1), torch.stack(quat, 1), torch.stack(lin, 1), torch.stack(ang, 1)), -1), dof_state


def envs_per_block(N, max_nb, max_nd, eb=64, grid_min=512, lds_max=49152):
    """ts_envs_per_block of csrc/task_common.h at this kernel's bytes per environment."""
    env_bytes = 8 * ((7 * max_nb) | 1) + 4 * ((13 * max_nb + 6 * max_nd) | 1)
    while eb > 1 and (eb * env_bytes > lds_max or (eb > 4 and -(-N // eb) < grid_min)):
        eb >>= 1
    return eb


class HipScene:
    """N environments of the given trees interleaved e % K, two tip rows in front of each object, the hold rule on everywhere."""

    def __init__(self, trees, N, tgts):
        self.lib = ObjectLibrary(trees, DEV)
        g = torch.Generator(device=DEV).manual_seed(17)
        k = np.arange(N) % len(trees)
        nb, nd = np.array(self.lib.num_bodies)[k], np.array(self.lib.num_dofs)[k]
        rb_row0 = np.concatenate([[0], np.cumsum(2 + nb)[:-1]]) + 2
        dof_row0 = np.concatenate([[0], np.cumsum(nd)[:-1]])
        i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=DEV)      # noqa: E731
        self.k, self.nb, self.nd = k, nb, nd
        self.obj_type, self.rb_row0, self.dof_row0, self.order = i32(k), i32(rb_row0), i32(dof_row0), self.lib.order_of(k)
        self.tips = i32(np.stack([rb_row0 - 2, rb_row0 - 1], 1))
        self.target = i32(np.asarray(tgts)[k])
        self.rigid_body = torch.zeros(int(rb_row0[-1] + nb[-1]), 13, device=DEV)
        self.tip_values = 0.02 * torch.randn(N, 2, 13, device=DEV, generator=g)            # a few cm/s: the joints stay inside their limits
        self.rigid_body[self.tips.long().reshape(-1)] = self.tip_values.reshape(-1, 13)
        lo = torch.clamp(self.lib.dof_lower, min=-3.0)
        hi = torch.clamp(self.lib.dof_upper, max=3.0)
        off = self.lib.dof_off.tolist()
        cols = torch.as_tensor(np.concatenate([np.arange(off[i], off[i + 1]) for i in k]), device=DEV)
        self.dof_state = torch.zeros(int(dof_row0[-1] + nd[-1]), 2, device=DEV)
        self.dof_state[:, 0] = (lo + 0.5 * (hi - lo))[cols]
        self.pose = torch.tensor(POSE, device=DEV).expand(N, 7).contiguous()
        self.hold, self.reset = torch.ones(N, dtype=torch.bool, device=DEV), torch.zeros(N, dtype=torch.bool, device=DEV)

    def step(self):
        self.lib.step(self.obj_type, self.pose, self.rb_row0, self.dof_row0, self.dof_state, self.rigid_body, order=self.order,
                      hold=self.hold, reset=self.reset, target_dof=self.target, tip_rows=self.tips, dt=DT)
        return self.rigid_body, self.dof_state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 5, 3 calls")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/kinematic_scene_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [5] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 200
    trees = dict(A=CF.tree_of("A", 0.5), B=CF.tree_of("B", 0.5), C=CF.tree_of("C"))
    tgt = dict(A=0, B=1, C=40)
    rows = []
    for name in ("A", "B", "C", "A+B+C"):
        names = name.split("+")
        for N in sizes:
            sc = HipScene([trees[n] for n in names], N, [tgt[n] for n in names])
            fns = dict(hip=sc.step)
            diff = None
            if len(names) == 1:
                tree = trees[name]
                ref = TorchObjects(tree, N, tgt[name])
                ref_state = sc.dof_state.view(N, tree.num_dofs, 2).clone()
                rb_t, dof_t = ref.step(ref_state, sc.pose, sc.tip_values, sc.hold)
                rb, dof = sc.step()
                got = rb.view(N, 2 + tree.num_bodies, 13)[:, 2:]
                diff = dict(rigid_body=float((got - rb_t).abs().max()), dof_state=float((dof.view(N, -1, 2) - dof_t).abs().max()))
                fns["torch"] = lambda ref=ref, st=ref_state, sc=sc: ref.step(st, sc.pose, sc.tip_values, sc.hold)
            for fn in fns.values():
                fn(), fn()
            torch.cuda.synchronize()
            ops = dict(hip=1)
            if "torch" in fns:
                ops["torch"] = count_ops(fns["torch"])
            ms = {side: [] for side in fns}
            for _ in range(3):                                 # alternate in one process
                for side, fn in fns.items():
                    ms[side].append(timed(fn, calls if side == "hip" else max(3, calls // 4)))
            mean = {side: float(np.mean(v)) for side, v in ms.items()}
            out_bytes = int(4 * (13 * sc.nb.sum() + 2 * N))
            floor = out_bytes / HBM_BYTES_PER_S * 1e3
            row = dict(objects=name, bodies=[trees[n].num_bodies for n in names], dofs=[trees[n].num_dofs for n in names], N=N,
                       envs_per_block=envs_per_block(N, sc.lib.max_bodies, sc.lib.max_dofs), hip_ms=round(mean["hip"], 5),
                       bytes_written=out_bytes, floor_ms=round(floor, 7), share_of_bytes_floor=round(floor / mean["hip"], 5),
                       hip_ms_rounds=[round(x, 5) for x in ms["hip"]], device_ops=ops, calls=3 * calls)
            if "torch" in fns:
                row.update(torch_ms=round(mean["torch"], 5), speedup=round(mean["torch"] / mean["hip"], 2),
                           torch_ms_rounds=[round(x, 5) for x in ms["torch"]], max_abs_diff_hip_vs_torch=diff)
            rows.append(row)
            del sc
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_kinematic_scene", device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, dt=DT,
                           hold_rule="on in every environment", sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(ROOT, "profiles", "kinematic_scene_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
