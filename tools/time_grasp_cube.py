"""Time GraspCubeTensors.begin_step / end_step (pm_franka_control_f32, pm_grasp_cube_post_f32) beside a tensor-library evaluation
of the same contract (this tool's own restatement of include/partmanip_hip.h's description: gathers, cats, a batched 6 x 6
inverse), in one process, alternating: 14 bodies, 9 DOFs, 12 posed parts, N in {64, 1024, 4096}.  Device events around warmed calls.
Prints one JSON line and writes it to profiles/grasp_cube_timing.json (--out; nothing is written with --tiny).

launches: for the tensor-library side the number of ATen operations dispatched per step that run on the device (views and
metadata operations excluded: a lower bound on its kernel launches); for the HIP side the same count of what the wrapper does
around its kernel (the progress increment, the three operations that form succ_rate) plus one for the kernel itself.
share_of_bytes_floor = (bytes a step has to read and write / 6.29 TB/s, the measured HBM copy rate of the MI355X) / hip_ms: at these
sizes (7.0 + 2.1 MB per step at 4096 environments) the floor is about a microsecond and the launch itself is what is timed.

    python tools/time_grasp_cube.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.tasks import GraspCubeTensors  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, count_ops, timed  # noqa: E402

DEV = "cuda:0"
NB, ND, NL, M = 14, 9, 12, 12
IND = [[0, 1], [0, 2], [1, 2], [1, 0], [2, 0], [2, 1]] * 4


def quat_to_mat(q):
    i, j, k, r = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r), two_s * (i * j + k * r),
                     1 - two_s * (i * i + k * k), two_s * (j * k - i * r), two_s * (i * k - j * r), two_s * (j * k + i * r),
                     1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


class TorchTask:
    """The contract with tensor-library calls, state kept as the task keeps it."""

    def __init__(self, task):
        self.t = task
        N, dev = task.num_envs, task.device
        self.ind = torch.tensor(IND, device=dev)
        self.rew = torch.zeros(N, device=dev)
        self.success = torch.zeros(N, dtype=torch.bool, device=dev)
        self.progress = torch.zeros(N, dtype=torch.long, device=dev)
        self.emr = torch.full((N,), -100.0, device=dev)
        self.ems = torch.zeros(N, dtype=torch.long, device=dev)
        self.eye = torch.eye(6, device=dev) * 0.05 ** 2
        self.one = torch.ones(1, dtype=torch.long, device=dev)

    def deamb(self, q):
        R = quat_to_mat(q)
        two = R[:, :, self.ind].transpose(-2, -3).clone()
        two[:, :12, 0] = -two[:, :12, 0]
        two[:, 6:18, 1] = -two[:, 6:18, 1]
        third = torch.linalg.cross(two[..., 0], two[..., 1], dim=-1).unsqueeze(-1)
        cand = torch.cat([two, third], dim=-1)
        tr = cand[..., 0, 0] + cand[..., 1, 1] + cand[..., 2, 2]
        return cand[torch.arange(cand.shape[0], device=q.device), tr.argmax(dim=1)]

    def end_step(self, rb, dof, root):
        t, r = self.t, self.t.robot
        self.progress += 1
        L, Rt = rb[:, r.ltip_rb_index], rb[:, r.rtip_rb_index]
        tip = (L + Rt) / 2
        gl = (L[:, :3] - Rt[:, :3]).norm(dim=-1)
        lo, hi = t.pose_lower_limit, t.pose_upper_limit
        obj = root[:, t.obj_actor]
        tip_s = 2 * (tip[:, :7] - lo) / (hi - lo) - 1
        obj_s = 2 * (obj[:, :3] - lo[:3]) / (hi[:3] - lo[:3]) - 1
        o = self.deamb(obj[:, 3:7])
        qn = 2 * (dof[:, :, 0] - r.dof_lower_limits_tensor) / (r.dof_upper_limits_tensor - r.dof_lower_limits_tensor) - 1
        qv = dof[:, :, 1]
        normal = torch.cat([tip_s, obj_s, o.reshape(len(o), -1), qn, qv], dim=-1)
        proprio = torch.cat([tip_s, qn, qv], dim=-1)
        dist = (tip[:, :3] - obj[:, :3]).norm(dim=-1)
        reached = dist < 0.02
        close = (0.1 - gl) * reached + 0.1 * (gl - 0.1) * (~reached)
        h = quat_to_mat(tip[:, 3:7])
        p1 = ((h[:, :, 0] * o[:, :, 0]).abs() + (h[:, :, 1] * o[:, :, 1]).abs()).sum(dim=-1)
        p2 = ((h[:, :, 0] * o[:, :, 1]).abs() + (h[:, :, 1] * o[:, :, 0]).abs()).sum(dim=-1)
        rot = -h[:, 2, 2] + torch.max(p1, p2) - 3
        dgoal = (obj[:, :3] - t.success_pos).norm(dim=-1)
        rgoal = torch.clamp(0.2 - dgoal, min=0) * reached
        self.success = (dgoal <= t.goal_thresh) & reached
        self.rew = -dist + 0.5 * rot + 5 * close + 20 * rgoal + 3 * self.success
        extras = torch.stack([-dist, close, rot, rgoal, (obj[:, :3] - t.obj_default_pos).norm(dim=-1), self.rew, obj[:, 2],
                              (obj[:, 2] > 0.1).float()], dim=1)
        parts = rb[:, t.part_body.long(), :7]
        pose_R = torch.matmul(quat_to_mat(parts[..., 3:]), t.part_C.unsqueeze(0))
        return normal, proprio, self.rew, extras, pose_R, parts[..., :3].contiguous()

    def begin_step(self, actions, dof, jac):
        t, r = self.t, self.t.robot
        na = r.num_dofs - 2
        q = dof[:, :, 0]
        J = (jac[:, r.ltip_rb_index - 1, :, :na] + jac[:, r.rtip_rb_index - 1, :, :na]) / 2
        JT = J.transpose(1, 2)
        u = (JT @ torch.inverse(J @ JT + self.eye) @ (actions[:, :6] * 0.005).unsqueeze(-1)).squeeze(-1)
        g = actions[:, 6:7] * t.dt / 5
        tgt = torch.cat([q[:, :na] + u, q[:, na:] + g], dim=-1)
        tgt = torch.max(torch.min(tgt, r.dof_upper_limits_tensor), r.dof_lower_limits_tensor)
        self.ems = torch.where(self.rew < self.emr, self.ems, self.progress)
        self.emr = torch.maximum(self.rew, self.emr)
        reset = (self.progress >= self.ems + t.explore_step) | self.success
        reset_succ = self.success.clone()
        succ_rate = self.success.int().sum(dim=-1, keepdim=True) / torch.clamp(reset.int().sum(), min=1)
        tgt = torch.where(reset.unsqueeze(-1), r.default_dof_pos, tgt)
        self.progress = torch.where(reset, 0, self.progress)
        self.success = self.success & ~reset
        self.emr = torch.where(reset, -100.0, self.emr)
        self.ems = torch.where(reset, 0, self.ems)
        return tgt, reset, reset_succ, succ_rate


def make_state(N, seed=31):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rb = torch.rand(N, NB, 13, device=DEV, generator=g) - 0.5
    rb[..., 3:7] = torch.nn.functional.normalize(torch.randn(N, NB, 4, device=DEV, generator=g), dim=-1)
    root = torch.randn(N, 2, 13, device=DEV, generator=g) * 0.1
    root[:, 1, 3:7] = torch.nn.functional.normalize(torch.randn(N, 4, device=DEV, generator=g), dim=-1)
    near = torch.arange(N, device=DEV) % 2 == 0                # half the environments within reach
    tip = root[:, 1, :3] + torch.where(near.unsqueeze(-1), 0.005, 0.1) * torch.nn.functional.normalize(torch.randn(N, 3, device=DEV, generator=g), dim=-1)
    rb[:, 10, :3], rb[:, 12, :3] = tip + 0.01, tip - 0.01
    rb[:, 12, 3:7] = rb[:, 10, 3:7]
    dof = torch.stack([torch.rand(N, ND, device=DEV, generator=g) * 0.03, torch.randn(N, ND, device=DEV, generator=g)], dim=-1)
    jac = torch.randn(N, NL, 6, ND, device=DEV, generator=g)
    act = torch.rand(N, 7, device=DEV, generator=g) * 2 - 1
    return rb.contiguous(), dof.contiguous(), root.contiguous(), jac.contiguous(), act.contiguous()


def step_bytes():
    """Bytes one environment's step has to move (reads + writes), from the shapes."""
    end = (NB * 13 + ND * 2 + 7) * 4 + (19 + 2 * ND + 7 + 2 * ND + 1 + 8 + M * 12) * 4 + 2 + 16
    begin = (7 + ND * 2 + 2 * 6 * (ND - 2) + 1 + 1) * 4 + 1 + 8 + 8 + (ND + 1) * 4 + 8 + 8 + 3
    return dict(begin_step=begin, end_step=end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 4, 3 calls (the test suite's smoke run)")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/grasp_cube_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 200
    rows = []
    per_env = step_bytes()
    for N in sizes:
        task = GraspCubeTensors(N, DEV, {"robot": {"driveMode": "ik"}, "explore_step": 40}, 1 / 60)
        ref = TorchTask(task)
        rb, dof, root, jac, act = make_state(N)
        fns = dict(hip=dict(begin_step=lambda: task.begin_step(act, dof, jac), end_step=lambda: task.end_step(rb, dof, root)),
                   torch=dict(begin_step=lambda: ref.begin_step(act, dof, jac), end_step=lambda: ref.end_step(rb, dof, root)))
        # same contract: one round of both, compared
        obs, rew, _, _ = task.end_step(rb, dof, root)
        normal, proprio, rew_t, extras_t, pose_R, pose_T = ref.end_step(rb, dof, root)
        diff = max(float((obs["normal_state"] - normal).abs().max()), float((rew - rew_t).abs().max()),
                   float((task.pose_R - pose_R).abs().max()), float((task._extras - extras_t).abs().max()))
        flags_equal = bool(torch.equal(task.success, ref.success))
        pos_act, reset = task.begin_step(act, dof, jac)
        tgt, reset_t, _, succ_rate = ref.begin_step(act, dof, jac)
        diff_ctl = float((pos_act - tgt).abs().max())
        flags_equal = flags_equal and bool(torch.equal(reset, reset_t)) and bool(torch.equal(task.progress_buf, ref.progress))
        for side in fns.values():                              # warm everything
            for fn in side.values():
                fn()
        torch.cuda.synchronize()
        launches = {side: {k: count_ops(fn) + (1 if side == "hip" else 0) for k, fn in d.items()} for side, d in fns.items()}
        ms = {side: {k: [] for k in d} for side, d in fns.items()}
        for _ in range(3):                                     # alternate in one process
            for side, d in fns.items():
                for k, fn in d.items():
                    ms[side][k].append(timed(fn, calls))
        mean = {side: {k: float(np.mean(v)) for k, v in d.items()} for side, d in ms.items()}
        floor = {k: per_env[k] * N / HBM_BYTES_PER_S * 1e3 for k in per_env}
        rows.append(dict(N=N, hip_ms={k: round(v, 5) for k, v in mean["hip"].items()},
                         torch_ms={k: round(v, 5) for k, v in mean["torch"].items()},
                         speedup={k: round(mean["torch"][k] / mean["hip"][k], 2) for k in mean["hip"]}, launches=launches,
                         bytes_per_step={k: per_env[k] * N for k in per_env}, floor_ms={k: round(v, 7) for k, v in floor.items()},
                         # (three significant digits: at --tiny's N = 4 the share is ~5e-6, which five decimals round to 0 or 1e-5)
                         share_of_bytes_floor={k: float(f"{floor[k] / mean['hip'][k]:.3g}") for k in floor},
                         hip_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["hip"].items()},
                         torch_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["torch"].items()}, calls=3 * calls,
                         max_abs_diff_hip_vs_torch=dict(end_step=diff, begin_step=diff_ctl), flags_equal=flags_equal))
        del task, ref
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_grasp_cube", device=torch.cuda.get_device_name(0), bodies=NB, dofs=ND, parts=M, bound="launch",
                           hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grasp_cube_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
