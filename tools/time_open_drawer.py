"""Time OpenDrawerTensors.begin_step / end_step (pm_franka_control_f32 + pm_open_drawer_reset_f32, pm_open_drawer_post_f32) beside a
tensor-library evaluation of the same contract (this tool's own restatement of include/partmanip_hip.h's description: two fancy-index
gathers, cats, a batched 6 x 6 inverse, masked scatters without a host read), in one process, alternating: 13 robot bodies, 9 DOFs, 13
posed parts, three cabinet types with (bodies, DOFs) = (3, 1), (5, 3), (4, 2), N in {64, 1024, 4096}.  Device events around warmed
calls.  Prints one JSON line and writes it to profiles/open_drawer_timing.json (--out; nothing is written with --tiny).

launches: for the tensor-library side the number of ATen operations dispatched per step that run on the device (views and metadata
operations excluded: a lower bound on its kernel launches); for the HIP side the same count of what the wrapper does around its
kernels (the progress increment, the three operations that form succ_rate) plus one per kernel (two in begin_step).
share_of_bytes_floor = (bytes a step has to read and write / 6.29 TB/s, the measured HBM copy rate of the MI355X) / hip_ms.

    python tools/time_open_drawer.py [--tiny] [--sizes 64,1024,4096]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.tasks import OpenDrawerTensors  # noqa: E402
from partmanip_amd.tasks.open_drawer import build_masks  # noqa: E402
from tools.time_grasp_cube import quat_to_mat  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, count_ops, timed  # noqa: E402

DEV = "cuda:0"
NRB, ND, NL, M = 13, 9, 12, 13
TYPES = ((3, 1, 1, 2, 0), (5, 3, 2, 4, 2), (4, 2, 3, 1, 1))


def quat_rotate(q, v):
    w, qv = q[:, 3:4], q[:, :3]
    return v * (2.0 * w ** 2 - 1.0) + torch.linalg.cross(qv, v, dim=-1) * w * 2.0 + qv * (qv * v).sum(-1, keepdim=True) * 2.0


def quat_mul(a, b):
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    ww, yy, zz = (z1 + x1) * (x2 + y2), (w1 - y1) * (w2 + z2), (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2), qq - zz + (z1 + y1) * (w2 - x2),
                        qq - ww + (z1 - y1) * (y2 - z2)], dim=-1)


class TorchTask:
    """The contract with tensor-library calls, state kept as the task keeps it."""

    def __init__(self, task):
        self.t = task
        N, dev = task.num_envs, task.device
        self.rbm, self.dfm = task.rigid_body_mask.long(), task.dof_state_mask.long()
        self.obj_id = task.obj_id.long()
        self.rew = torch.zeros(N, device=dev)
        self.success = torch.zeros(N, dtype=torch.bool, device=dev)
        self.progress = torch.zeros(N, dtype=torch.long, device=dev)
        self.emr = torch.full((N,), -100.0, device=dev)
        self.ems = torch.zeros(N, dtype=torch.long, device=dev)
        self.eye = torch.eye(6, device=dev) * 0.05 ** 2
        self.basis = torch.eye(3, device=dev)
        self.flags = torch.zeros(task.num_objs, dtype=torch.bool, device=dev)
        self.dof = torch.zeros(N, ND + 1, 2, device=dev)

    def end_step(self, rb_all, dof_all, root):
        t, r = self.t, self.t.robot
        nd = r.num_dofs
        self.progress += 1
        g, d = rb_all[self.rbm], dof_all[self.dfm]
        self.dof = d
        obj = root[:, t.obj_actor]
        L, Rt = g[:, r.ltip_rb_index], g[:, r.rtip_rb_index]
        tip = (L + Rt) / 2
        gl = (L[:, :3] - Rt[:, :3]).norm(dim=-1)
        q = d[:, nd, 0]
        bbox = torch.matmul(t.part_bbox_init + q[:, None, None] * t.part_axis_dir_init[:, None, :],
                            quat_to_mat(obj[:, 3:7]).transpose(-1, -2)) + obj[:, None, :3]
        h_out, h_long, h_short = bbox[:, 0] - bbox[:, 4], bbox[:, 1] - bbox[:, 0], bbox[:, 3] - bbox[:, 0]
        mid = (bbox[:, 0] + bbox[:, 6]) / 2
        l_out, l_long, l_short = h_out.norm(dim=-1), h_long.norm(dim=-1), h_short.norm(dim=-1)
        h_out, h_long, h_short = h_out / l_out[:, None], h_long / l_long[:, None], h_short / l_short[:, None]
        qn = 2 * (d[:, :nd, 0] - r.dof_lower_limits_tensor) / (r.dof_upper_limits_tensor - r.dof_lower_limits_tensor) - 1
        normal = torch.cat([tip, mid, h_out, h_short, h_long, l_out[:, None], l_long[:, None], l_short[:, None], qn, d[:, :nd, 1],
                            q[:, None]], dim=-1)
        delta = tip[:, :3] - mid
        r_out = (delta * h_out).sum(-1).abs() < l_out / 2
        r_short = ((L[:, :3] - mid) * h_short).sum(-1) * ((Rt[:, :3] - mid) * h_short).sum(-1) < 0
        r_long = (delta * h_long).sum(-1).abs() < l_long / 2
        reached = r_out & r_short & r_long
        reaching = -delta.norm(dim=-1) + 0.1 * (r_out | r_short | r_long)
        rot4 = tip[:, 3:7]
        grip = quat_rotate(rot4, self.basis[2].expand(len(q), 3))
        sep = quat_rotate(rot4, self.basis[1].expand(len(q), 3))
        down = quat_rotate(rot4, self.basis[0].expand(len(q), 3))
        rot = (-grip * h_out).sum(-1) + torch.max((sep * h_short).sum(-1), (-sep * h_short).sum(-1)) \
            + torch.max((down * h_long).sum(-1), (-down * h_long).sum(-1)) - 3
        close = (0.1 - gl) * reached + 0.1 * (gl - 0.1) * (~reached)
        grasp = reached & (gl < l_short + 0.01) & (rot > -0.2)
        lo, hi = t.part_joint_lower_limits, t.part_joint_upper_limits
        frac = (q - lo) / hi
        jsr = grasp * (0.1 + torch.clamp(frac, max=t.suc_prop))
        open_ng = frac > 0.1
        base = reaching + 0.5 * rot + 5 * close + 5 * jsr
        self.success = grasp & (q - lo >= t.suc_prop * hi)
        self.rew = base + base.abs() * rot + 2 * self.success
        self.flags |= torch.zeros_like(self.flags, dtype=torch.int32).index_add_(0, self.obj_id, self.success.int()) > 0
        extras = torch.stack([(grasp & open_ng).float(), open_ng.float(), reaching, close, rot, jsr, self.rew, grasp.float()], dim=1)
        parts = g[:, t.part_slot.long(), :7]
        pose_R = torch.matmul(quat_to_mat(parts[..., 3:]), t.part_C.unsqueeze(0))
        return normal, self.rew, extras, bbox, pose_R, parts[..., :3].contiguous()

    def begin_step(self, actions, jac, dof_all, root, pos_act_all, u):
        t, r = self.t, self.t.robot
        nd = r.num_dofs
        na = nd - 2
        q = self.dof[:, :nd, 0]
        J = (jac[:, r.ltip_rb_index - 1, :, :na] + jac[:, r.rtip_rb_index - 1, :, :na]) / 2
        JT = J.transpose(1, 2)
        du = (JT @ torch.inverse(J @ JT + self.eye) @ (actions[:, :6] * 0.005).unsqueeze(-1)).squeeze(-1)
        tgt = torch.cat([q[:, :na] + du, q[:, na:] + actions[:, 6:7] * t.dt / 5], dim=-1)
        tgt = torch.max(torch.min(tgt, r.dof_upper_limits_tensor), r.dof_lower_limits_tensor)
        self.ems = torch.where(self.rew < self.emr, self.ems, self.progress)
        self.emr = torch.maximum(self.rew, self.emr)
        reset = (self.progress >= self.ems + t.explore_step) | self.success
        succ_rate = self.success.int().sum(dim=-1, keepdim=True) / torch.clamp(reset.int().sum(), min=1)
        tgt = torch.where(reset.unsqueeze(-1), r.default_dof_pos, tgt)
        self.progress = torch.where(reset, 0, self.progress)
        self.success = self.success & ~reset
        self.emr = torch.where(reset, -100.0, self.emr)
        self.ems = torch.where(reset, 0, self.ems)
        # the state half, without a host read: masked values written through the tables
        pos_act_all[self.dfm[:, :nd]] = tgt
        new = torch.cat([torch.stack([r.default_dof_pos.expand(len(q), nd), torch.zeros_like(q)], dim=-1),
                         torch.stack([t.part_joint_lower_limits, torch.zeros_like(t.part_joint_lower_limits)], dim=-1)[:, None]], dim=1)
        self.dof = torch.where(reset[:, None, None], new, self.dof)
        dof_all[self.dfm] = self.dof
        obj = t.obj_default_root.expand(len(q), 7).clone()
        if u is not None:
            obj[:, :3] += u[:, :3] * t.reset_t_range * 2 - t.reset_t_range
            ang = u[:, 3] * t.reset_r_range * 2 - t.reset_r_range
            zero = torch.zeros_like(ang)
            obj[:, 3:7] = quat_mul(obj[:, 3:7], torch.stack([zero, zero, torch.sin(ang), torch.cos(ang)], dim=-1))
        fresh = torch.zeros_like(root)
        fresh[:, t.robot_actor, :7] = t.robot_default_root
        fresh[:, t.obj_actor, :7] = obj
        root.copy_(torch.where(reset[:, None, None], fresh, root))
        return tgt, reset, succ_rate


def make_state(N, seed=37):
    types = [TYPES[i % 3] for i in range(N)]
    rbm, dfm, B, D = build_masks(NRB, ND, *[[ty[c] for ty in types] for c in range(5)])
    g = torch.Generator(device=DEV).manual_seed(seed)
    rb = torch.rand(B, 13, device=DEV, generator=g) - 0.5
    rb[:, 3:7] = torch.nn.functional.normalize(torch.randn(B, 4, device=DEV, generator=g), dim=-1)
    root = torch.randn(N, 2, 13, device=DEV, generator=g) * 0.1
    root[:, :, 3:7] = torch.nn.functional.normalize(torch.randn(N, 2, 4, device=DEV, generator=g), dim=-1)
    dof = torch.stack([torch.rand(D, device=DEV, generator=g) * 0.03, torch.randn(D, device=DEV, generator=g)], dim=-1)
    # an axis-aligned handle box near the object's origin, the tool centre inside it for half the environments
    half = torch.tensor([0.02, 0.08, 0.015], device=DEV)
    signs = torch.tensor([[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, -1], [-1, 1, -1], [-1, 1, 1], [-1, -1, 1]],
                         device=DEV, dtype=torch.float32)
    bbox = (signs * half).expand(N, 8, 3).contiguous()
    axis = torch.tensor([1.0, 0, 0], device=DEV).expand(N, 3).contiguous()
    mt = torch.from_numpy(rbm.astype(np.int64)).to(DEV)
    near = (torch.arange(N, device=DEV) % 2 == 0).unsqueeze(-1)
    centre = root[:, 1, :3] + torch.where(near, 0.0, 0.3)
    rb[mt[:, 10], :3], rb[mt[:, 12], :3] = centre + 0.012, centre - 0.012
    rb[mt[:, 12], 3:7] = rb[mt[:, 10], 3:7]
    const = dict(rigid_body_mask=rbm, dof_state_mask=dfm, obj_id=np.arange(N) % 3, part_bbox_init=bbox, part_axis_dir_init=axis,
                 part_joint_lower_limits=torch.zeros(N, device=DEV), part_joint_upper_limits=torch.full((N,), 0.2, device=DEV),
                 num_objs=3, num_rigid_bodies=B, num_dof_states=D)
    jac = torch.randn(N, NL, 6, ND, device=DEV, generator=g)
    act = torch.rand(N, 7, device=DEV, generator=g) * 2 - 1
    u = torch.rand(N, 4, device=DEV, generator=g)
    return const, rb.contiguous(), dof.contiguous(), root.contiguous(), jac.contiguous(), act.contiguous(), u, B, D


def step_bytes(B_per_env, D_per_env):
    """Bytes one environment's step has to move (reads + writes), from the shapes (cabinet rows that are not gathered excluded)."""
    end = ((NRB + 2) * 13 + (ND + 1) * 2 + 7 + 24 + 3 + 2) * 4 + (NRB + 2 + ND + 1 + 1) * 4 \
        + (29 + 2 * ND + 1 + 8 + 24 + ND * 2 + 2 + M * 12) * 4 + 2
    begin = (7 + ND * 2 + 2 * 6 * (ND - 2) + 1 + 1) * 4 + 1 + 8 + 8 + (ND + 1) * 4 + 8 + 8 + 3 + (ND + 1) * 4 + ND * 4 + 1 + ND * 4
    return dict(begin_step=begin, end_step=end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 5, 3 calls")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/open_drawer_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [5] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 200
    rows = []
    for N in sizes:
        const, rb, dof, root, jac, act, u, B, D = make_state(N)
        cfg = {"robot": {"driveMode": "ik", "root": [0.3, -0.1, 0.05, 0, 0, 0.6, 0.8]}, "explore_step": 40, "random_reset": True}
        task = OpenDrawerTensors(N, DEV, cfg, 1 / 60, **const)
        ref = TorchTask(task)
        per_env = step_bytes(B / N, D / N)
        state = [(dof.clone(), root.clone(), torch.zeros(D, device=DEV)) for _ in range(2)]
        (dof_h, root_h, pa_h), (dof_t, root_t, pa_t) = state
        fns = dict(hip=dict(begin_step=lambda: task.begin_step(act, jac, dof_h, root_h, pa_h, u=u),
                            end_step=lambda: task.end_step(rb, dof_h, root_h)),
                   torch=dict(begin_step=lambda: ref.begin_step(act, jac, dof_t, root_t, pa_t, u),
                              end_step=lambda: ref.end_step(rb, dof_t, root_t)))
        # same contract: one round of both, compared
        obs, rew, _, _ = task.end_step(rb, dof_h, root_h)
        normal, rew_t, extras_t, bbox_t, pose_R, pose_T = ref.end_step(rb, dof_t, root_t)
        diff = max(float((obs["normal_state"] - normal).abs().max()), float((rew - rew_t).abs().max()),
                   float((task.pose_R - pose_R).abs().max()), float((task._extras - extras_t).abs().max()),
                   float((task.part_bbox - bbox_t).abs().max()))
        flags_equal = bool(torch.equal(task.success, ref.success)) and bool(torch.equal(task.succ_objid_lst, ref.flags))
        n_success = int(task.success.sum())
        task.begin_step(act, jac, dof_h, root_h, pa_h, u=u)
        tgt, reset_t, _ = ref.begin_step(act, jac, dof_t, root_t, pa_t, u)
        diff_ctl = max(float((task.pos_act - tgt).abs().max()), float((pa_h - pa_t).abs().max()), float((dof_h - dof_t).abs().max()),
                       float((root_h - root_t).abs().max()))
        flags_equal = flags_equal and bool(torch.equal(task.reset_buf, reset_t)) and bool(torch.equal(task.progress_buf, ref.progress))
        for side in fns.values():                              # warm everything
            for fn in side.values():
                fn()
        torch.cuda.synchronize()
        kernels = dict(begin_step=2, end_step=1)
        launches = {side: {k: count_ops(fn) + (kernels[k] if side == "hip" else 0) for k, fn in d.items()} for side, d in fns.items()}
        ms = {side: {k: [] for k in d} for side, d in fns.items()}
        for _ in range(3):                                     # alternate in one process
            for side, d in fns.items():
                for k, fn in d.items():
                    ms[side][k].append(timed(fn, calls))
        mean = {side: {k: float(np.mean(v)) for k, v in d.items()} for side, d in ms.items()}
        floor = {k: per_env[k] * N / HBM_BYTES_PER_S * 1e3 for k in per_env}
        rows.append(dict(N=N, rigid_bodies=B, dof_states=D, hip_ms={k: round(v, 5) for k, v in mean["hip"].items()},
                         torch_ms={k: round(v, 5) for k, v in mean["torch"].items()},
                         speedup={k: round(mean["torch"][k] / mean["hip"][k], 2) for k in mean["hip"]}, launches=launches,
                         bytes_per_step={k: per_env[k] * N for k in per_env}, floor_ms={k: round(v, 7) for k, v in floor.items()},
                         share_of_bytes_floor={k: round(floor[k] / mean["hip"][k], 5) for k in floor},
                         hip_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["hip"].items()},
                         torch_ms_rounds={k: [round(x, 5) for x in v] for k, v in ms["torch"].items()}, calls=3 * calls,
                         max_abs_diff_hip_vs_torch=dict(end_step=diff, begin_step=diff_ctl), flags_equal=flags_equal,
                         successes_in_compared_round=n_success))
        del task, ref
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_open_drawer", device=torch.cuda.get_device_name(0), robot_bodies=NRB, dofs=ND, parts=M,
                           reset_r_range=math.pi / 12, hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=rows))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "open_drawer_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
