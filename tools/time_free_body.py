"""Time the free body's launch (pm_free_body_step_f32: the cube of the kinematic grasp_cube loop, one thread per environment) and one
whole KinematicEnv.step in `normal_state` mode, each beside a tensor-library evaluation of the same contract in one process,
alternating.  N in {64, 1024, 4096}.  Device events around warmed calls (tools/timing.py).  Prints one JSON line and writes it to
profiles/free_body_timing.json (--out; nothing is written with --tiny).

The launch: the four rules mixed e % 4 (reset, latch, carry, released) over random tips, the grip and the body's row restored
before every call on both sides alike (two copy_, inside the timed window of both).  Tensor-library side: this tool's own batched
restatement of include/partmanip_hip.h's description in float32 (every rule evaluated for every environment, then selected).
The step: KinematicEnv.step over the shipped fixed-base URDF with zero actions, as env-steps / s; the tensor-library side is the same
step with the free body's launch alone replaced by the restatement above (the rest of the step are the launches earlier tools time:
time_grasp_cube.py, time_kinematics.py).  device_ops: ATen operations dispatched per call, counting one per HIP launch.  No threshold
is set anywhere: the launch is launch-bound like its siblings, and the numbers are a record.

    python tools/time_free_body.py [--tiny] [--sizes 64,1024,4096]
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
from partmanip_amd import ops  # noqa: E402
from partmanip_amd.envs import make_grasp_cube_env  # noqa: E402
from tools.time_kinematics import qmul, qrot  # noqa: E402
from tools.timing import count_ops, timed  # noqa: E402

DEV = "cuda:0"
DT = 1.0 / 60.0
URDF = os.path.join(ROOT, "tests", "golden", "franka_panda_sdf.urdf")
DEFAULT_POSE = (0.0, 0.0, 0.025, 0.0, 0.0, 0.0, 1.0)
PARAMS = dict(reset_range=0.15, rest_z=0.025, fall_speed=0.3)


def torch_free_body(tip_l, tip_r, body, grip, hold, reset, default_pose, u, reset_range, rest_z, fall_speed):
    """(row (N, 13), grip (N, 8)) by the contract, in float32."""
    N = body.shape[0]
    p = (tip_l[:, :3] + tip_r[:, :3]) / 2
    qh = tip_l[:, 3:7] / tip_l[:, 3:7].norm(dim=-1, keepdim=True)
    conj = qh * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=body.device)
    latched = grip[:, 7] != 0
    zero3 = torch.zeros(N, 3, device=body.device)
    # 1. reset
    xy = default_pose[:2] + (2 * u[:, :2] - 1) * reset_range
    th = 2 * math.pi * u[:, 2] - math.pi
    yaw = torch.stack((torch.zeros_like(th), torch.zeros_like(th), torch.sin(th), torch.cos(th)), -1)
    r_row = torch.cat((xy, default_pose[2:3].expand(N, 1), qmul(default_pose[3:].expand(N, 4), yaw), zero3, zero3), -1)
    # 2. latch
    rel = torch.cat((qrot(conj, body[:, :3] - p), qmul(conj, body[:, 3:7]), torch.ones(N, 1, device=body.device)), -1)
    l_row = torch.cat((body[:, :7], zero3, zero3), -1)
    # 3. carry
    cn = p + qrot(qh, grip[:, :3])
    qn = qmul(qh, grip[:, 3:7])
    c_row = torch.cat((cn, qn / qn.norm(dim=-1, keepdim=True), (cn - body[:, :3]) / DT, tip_l[:, 10:]), -1)
    # 4. released
    z = body[:, 2]
    zn = torch.where(z > rest_z, torch.clamp(z - fall_speed * DT, min=rest_z), z)
    f_row = torch.cat((body[:, :2], zn[:, None], body[:, 3:7], zero3[:, :2], ((zn - z) / DT)[:, None], zero3), -1)
    latch = hold & ~latched & ~reset
    carry = hold & latched & ~reset
    row = torch.where(reset[:, None], r_row, torch.where(latch[:, None], l_row, torch.where(carry[:, None], c_row, f_row)))
    g = torch.where(latch[:, None], rel, grip)
    g[:, 7] = torch.where(reset | ~hold, torch.zeros_like(z), g[:, 7])
    return row, g


class Launch:
    """N environments, dense (N, 3, 13): the two tips and the body."""

    def __init__(self, N):
        g = torch.Generator(device=DEV).manual_seed(23)
        f = dict(device=DEV, generator=g)
        self.N = N
        self.rb = 0.3 * torch.randn(N, 3, 13, **f)
        self.root = torch.zeros(N, 2, 13, device=DEV)
        self.root[:, 1] = 0.3 * torch.randn(N, 13, **f)
        e = torch.arange(N, device=DEV)
        self.hold, self.reset = (e % 4 == 1) | (e % 4 == 2), e % 4 == 0
        self.grip0 = torch.randn(N, 8, **f)
        self.grip0[:, 7] = (e % 4 == 2).float()
        self.grip = self.grip0.clone()
        self.u = torch.rand(N, 3, **f)
        self.tip_rows = torch.stack((3 * e, 3 * e + 1), 1).to(torch.int32).contiguous()
        self.body_row = (3 * e + 2).to(torch.int32)
        self.default_pose = torch.tensor(DEFAULT_POSE, device=DEV)
        self.body0 = self.root[:, 1].clone()

    def hip(self):
        self.grip.copy_(self.grip0)
        self.root[:, 1].copy_(self.body0)
        ops.free_body_step(self.rb, self.tip_rows, self.body_row, self.root, 1, self.hold, self.reset, self.grip, self.default_pose, DT,
                           u=self.u, **PARAMS)
        return self.root[:, 1], self.grip

    def torch(self):
        self.grip.copy_(self.grip0)
        self.root[:, 1].copy_(self.body0)
        return torch_free_body(self.rb[:, 0], self.rb[:, 1], self.root[:, 1], self.grip, self.hold, self.reset, self.default_pose, self.u,
                               **PARAMS)


def torch_sim_step(sim):
    """KinematicSim.step with the free body's launch replaced by the tensor-library restatement."""
    lt, rt = (int(v) % sim.rigid_body.shape[1] for v in sim.tip_rows[0])
    half = torch.full((sim.num_envs, 3), 0.5, device=DEV)      # u = 1 / 2 is the default pose itself

    def step(pos_act, reset=None, hold=None, u=None):
        sim.art.step(sim.dof_state, sim.base_pose, targets=pos_act, reset=reset, vmax=sim.max_velocity, dt=sim.dt, rigid_body=sim.rigid_body,
                     jacobian=sim.jacobian)
        uu = half if u is None else u
        row, g = torch_free_body(sim.rigid_body[:, lt], sim.rigid_body[:, rt], sim.root[:, 1], sim.grip, sim._no_flags if hold is None else hold,
                                 sim._no_flags if reset is None else reset, sim.free_body_pose, uu, sim.reset_range, sim.rest_z, sim.fall_speed)
        sim.root[:, 1].copy_(row), sim.rigid_body[:, -1].copy_(row), sim.grip.copy_(g)
        return sim.rigid_body, sim.dof_state, sim.jacobian
    return step


def measure(fns, calls):
    for fn in fns.values():
        fn(), fn()
    torch.cuda.synchronize()
    ops_n = {side: count_ops(fn) for side, fn in fns.items()}
    ms = {side: [] for side in fns}
    for _ in range(3):                                         # alternate in one process
        for side, fn in fns.items():
            ms[side].append(timed(fn, calls))
    return {side: float(np.mean(v)) for side, v in ms.items()}, {side: [round(x, 5) for x in v] for side, v in ms.items()}, ops_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 5, 3 calls")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/free_body_timing.json; none "
                                                "with --tiny)")
    a = ap.parse_args()
    sizes = [5] if a.tiny else [int(v) for v in a.sizes.split(",")]
    calls = 3 if a.tiny else 2000
    launches, steps = [], []
    for N in sizes:
        L = Launch(N)
        row_t, g_t = L.torch()
        row_t, g_t = row_t.clone(), g_t.clone()
        row_h, g_h = L.hip()
        diff = dict(row=float((row_h - row_t).abs().max()), grip=float((g_h - g_t).abs().max()))
        mean, rounds, ops_n = measure(dict(hip=L.hip, torch=L.torch), calls)
        # both sides restore grip and the body's row first (2 copies); the HIP side then issues one launch the counter cannot see
        launches.append(dict(N=N, hip_ms=round(mean["hip"], 5), torch_ms=round(mean["torch"], 5), speedup=round(mean["torch"] / mean["hip"], 2),
                             hip_ms_rounds=rounds["hip"], torch_ms_rounds=rounds["torch"],
                             device_ops=dict(hip=ops_n["hip"] + 1, torch=ops_n["torch"], of_which_restore=2), max_abs_diff_hip_vs_torch=diff,
                             bytes_written=int(4 * N * (13 + 13 + 8)), calls=3 * calls))
        env = make_grasp_cube_env({"robot": {"driveMode": "ik", "mobile": False}}, N, DEV, URDF, DT, base_pose=(0, -0.5, 0, 0, 0, 0.707, 0.707))
        env.reset()
        actions = torch.zeros(N, 7, device=DEV)
        hip_step = env.sim.step
        torch_step = torch_sim_step(env.sim)

        def run(step):
            env.sim.step = step
            env.step(actions)
        mean, rounds, ops_n = measure(dict(hip=lambda: run(hip_step), torch=lambda: run(torch_step)), max(3, calls // 2))
        env.sim.step = hip_step
        # HIP launches per step the counter cannot see: franka_control, articulation_step, free_body_step, grasp_cube_post
        steps.append(dict(N=N, obs_mode="normal_state", hip_ms=round(mean["hip"], 5), torch_free_body_ms=round(mean["torch"], 5),
                          env_steps_per_s=round(N / mean["hip"] * 1e3), env_steps_per_s_torch_free_body=round(N / mean["torch"] * 1e3),
                          hip_ms_rounds=rounds["hip"], torch_ms_rounds=rounds["torch"],
                          device_ops=dict(hip=ops_n["hip"] + 4, torch_free_body=ops_n["torch"] + 3), calls=3 * max(3, calls // 2)))
        del env, L
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_free_body", device=torch.cuda.get_device_name(0), dt=DT, rules="reset / latch / carry / released as e % 4",
                           launch=launches, env_step=steps))
    print(line)
    out = a.out or (None if a.tiny else os.path.join(ROOT, "profiles", "free_body_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
