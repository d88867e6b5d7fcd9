"""Time the swept contact test (pm_articulation_sweep_f32 / pm_articulation_sweep_groups_f32) beside the same contract built from the
existing launches, in one process, alternating, and the whole KinematicEnv.step of grasp_cube with resolve=None and resolve='block'
(the whole-step rows are grasp_cube only: the sweep rows cover both scenes, an open_drawer step is not timed here).

Workload: the golden Franka, 3 sensing bodies x 512 points on the hand's and the fingers' slots, N in {64, 1024, 4096} environments,
S in {4, 8, 16} parts per step, against the two scenes of tools/time_contact.py:
  cube      one target grid (a 5 cm box on 2.5 mm cells) at slot 11 of 12, the ungrouped entry;
  cabinets  a grouped library of 8 synthetic cabinets of 2-7 bodies behind 11 shared grids, the grouped entry.
The targets sit within a few centimetres of the hand, so most points fall inside a valid box and the gathers are paid for.
`composed_ms` is the same result from existing launches: the (S + 1) N candidate joint states through Articulation.forward (which
writes the Jacobian), ops.body_pose_gather, ContactSensor.sense and a tensor-library selection; the tool asserts that both give the
same bits before it reports a time.  No threshold: the lines say what was measured.

    python tools/time_guarded_step.py [--tiny] [--sizes 64,1024,4096] [--out profiles/guarded_step_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from partmanip_amd import ops  # noqa: E402
from partmanip_amd.contact import ContactSensor, StepGuard  # noqa: E402
from partmanip_amd.kinematics import Articulation  # noqa: E402
from partmanip_amd.mesh2sdf import TSDFfromMesh  # noqa: E402
from partmanip_amd.tasks.franka import coordinate_transform_matrix  # noqa: E402
from partmanip_amd.tasks.grasp_cube import default_part_body  # noqa: E402
from partmanip_amd.urdf import load_urdf  # noqa: E402
from tools.time_contact import BODIES, PER_BODY, SCENE, SLOTS, URDF, box_grid, rotations  # noqa: E402
from tools.time_mesh_tsdf import synthetic_parts  # noqa: E402
from tools.timing import timed  # noqa: E402

DEV = "cuda:0"
DT = 1.0 / 60.0
SUBSTEPS = (4, 8, 16)


def build(scene, N, tree, dof0, base, per_body=PER_BODY, seed=21):
    """(sensor, slot_body, slot_C, pose_R, pose_T, dof_state, targets) of a scene: the robot places slots 0 .. 10, the targets sit
    round the hand at the default joint state, the targets of the step are up to 0.05 rad away."""
    g = torch.Generator().manual_seed(seed)
    nb, nd = tree.num_bodies, tree.num_dofs
    robot = synthetic_parts()[:11]
    if scene == "cube":
        tsdf = TSDFfromMesh(N, 0.5, 50, DEV, sdf_dicts=robot + [box_grid()])
        targets = (11, 12)
    else:
        tsdf = TSDFfromMesh(N, 0.5, 50, DEV, sdf_dicts=robot, groups=[synthetic_parts(seed=31 + k)[:n] for k, n in enumerate(BODIES)])
        targets = (11, 11 + max(BODIES))
    M = tsdf.part_num
    pts = (torch.rand(len(SLOTS) * per_body, 3, generator=g) - 0.5) * torch.tensor([0.04, 0.02, 0.06])
    sensor = ContactSensor(tsdf, pts.numpy(), np.repeat(SLOTS, per_body), [per_body] * len(SLOTS), targets, names=("hand", "lfinger", "rfinger"))
    part_body = np.asarray(default_part_body(nb + 1)[:11])
    slot_body = np.concatenate([part_body, np.full(M - 11, -1)]).astype(np.int32)
    slot_C = coordinate_transform_matrix().to(DEV).contiguous()
    art = Articulation(tree, N, DEV)
    q = torch.as_tensor(dof0, dtype=torch.float32) + (torch.rand(N, nd, generator=g) - 0.5) * 0.1
    ds = torch.zeros(N, nd, 2)
    ds[..., 0] = q
    ds = ds.to(DEV)
    rb, _ = art.forward(ds, base)
    hand = rb[:, part_body[8], :3].cpu()
    R = rotations(N, M, g)
    T = hand[:, None] + (torch.rand(N, M, 3, generator=g) - 0.5) * (0.06 if scene == "cube" else 0.16)
    tg = (q + (torch.rand(N, nd, generator=g) - 0.5) * 0.1).to(DEV).contiguous()
    return art, sensor, slot_body, slot_C, R.to(DEV).contiguous(), T.to(DEV).contiguous(), ds, tg


def composed(art, sensor, slot_body, slot_C, R, T, ds, tg, base, S, margin, bufs):
    """The contract from existing launches, on (S + 1) N environments: returns (sweep_dist, steps, targets_out)."""
    N, nd, nb = ds.shape[0], ds.shape[1], art.num_bodies
    lo, hi = art.dof_lower, art.dof_upper
    q = ds[..., 0]
    qn = torch.clamp(tg, lo, hi)
    a = (torch.arange(S + 1, device=DEV, dtype=torch.float32) / torch.full((S + 1,), float(S), device=DEV))[:, None, None]   # a true division
    cand = torch.clamp(q[None] + a * (qn - q)[None], lo, hi)
    cand[0], cand[S] = torch.clamp(q, lo, hi), qn
    big = bufs["ds"]
    big[..., 0] = cand.reshape(-1, nd)
    art.forward(big, base, rigid_body=bufs["rb"], jacobian=bufs["jac"])
    Rg, Tg = ops.body_pose_gather(bufs["rb"], bufs["rows"], slot_C, bufs["R"], bufs["T"])
    placed = bufs["placed"]
    Rk = torch.where(placed[None, :, None, None], Rg, R.repeat(S + 1, 1, 1, 1))
    Tk = torch.where(placed[None, :, None], Tg, T.repeat(S + 1, 1, 1))
    per = max(1, 65535 // N) * N                              # the point query takes at most 65535 environments per launch
    go = bufs["group_of"]
    D = torch.cat([sensor.sense(Rk[i:i + per], Tk[i:i + per], group_of=None if go is None else go[i:i + per], per_point=False)
                   .body_dist.min(dim=1)[0] for i in range(0, (S + 1) * N, per)]).view(S + 1, N).t()
    adm = (D[:, 1:] > margin) | (D[:, 1:] >= D[:, :-1])
    steps = torch.cumprod(adm.to(torch.int32), dim=1).sum(dim=1).to(torch.int32)
    out = cand.permute(1, 0, 2)[torch.arange(N, device=DEV), steps.long()]
    return D, steps, out


def sweep_rows(sizes, tiny=False):
    tree = load_urdf(URDF)
    with open(SCENE) as f:
        s = json.load(f)
    base = torch.tensor(s["root"], dtype=torch.float32)
    base[3:] /= base[3:].norm()
    base = base.to(DEV)
    calls = 3 if tiny else 50
    rows = []
    for N in sizes:
        for scene in ("cube", "cabinets"):
            art, sensor, slot_body, slot_C, R, T, ds, tg = build(scene, N, tree, s["dof"], base, per_body=64 if tiny else PER_BODY)
            nb, nd, M = art.num_bodies, art.num_dofs, sensor.tsdf.part_num
            for S in SUBSTEPS:
                guard = StepGuard(sensor, slot_body, slot_C, substeps=S, margin=0.0)
                guard.set_scene(R, T)
                sim = argparse.Namespace(art=art, num_envs=N, dof_state=ds, base_pose=base, dt=DT, max_velocity=None, dof_row0=None)
                big = (S + 1) * N
                sb = torch.as_tensor(slot_body, device=DEV)
                f32 = dict(dtype=torch.float32, device=DEV)
                rows_t = torch.where(sb[None] >= 0, torch.arange(big, device=DEV)[:, None] * nb + sb[None], -1).to(torch.int32).contiguous()
                group_of = None
                if sensor.tsdf.groups:                        # the big batch is candidate-major: environment b sits at k N + b
                    group_of = torch.as_tensor(np.tile(sensor.tsdf.group_of, S + 1), dtype=torch.int32, device=DEV)
                bufs = dict(ds=torch.zeros(big, nd, 2, **f32), rb=torch.zeros(big, nb, 13, **f32), jac=torch.zeros(big, nb - 1, 6, nd, **f32),
                            rows=rows_t, R=torch.empty(big, M, 3, 3, **f32), T=torch.empty(big, M, 3, **f32), placed=sb >= 0, group_of=group_of)
                hip = lambda: guard.sweep(sim, tg)                                        # noqa: E731
                ref = lambda: composed(art, sensor, slot_body, slot_C, R, T, ds, tg, base, S, 0.0, bufs)   # noqa: E731
                hip(), ref()
                torch.cuda.synchronize()
                D, st, out = ref()
                same = bool(torch.equal(D.contiguous().view(torch.int32), guard.sweep_dist.view(torch.int32)) and torch.equal(st, guard.steps)
                            and torch.equal(out.contiguous().view(torch.int32), guard.targets.view(torch.int32)))
                assert same, (scene, N, S)
                hip_ms, ref_ms = [], []
                for _ in range(2):                                                       # alternate in one process
                    hip_ms.append(timed(hip, calls))
                    ref_ms.append(timed(ref, max(2, calls // 5)))
                rows.append(dict(scene=scene, N=N, S=S, points=sensor.num_points, sweep_ms=round(float(np.mean(hip_ms)), 5),
                                 composed_ms=round(float(np.mean(ref_ms)), 4), ratio=round(float(np.mean(ref_ms) / np.mean(hip_ms)), 1),
                                 sweep_ms_rounds=[round(v, 5) for v in hip_ms], same_bits=same,
                                 in_range=round(float((guard.sweep_dist < 1).float().mean()), 3),
                                 cut=round(float((guard.steps < S).float().mean()), 3)))
                del bufs
            del art, sensor, R, T, ds, tg
            torch.cuda.empty_cache()
    return rows


def step_rows(sizes, steps=50):
    """ms per KinematicEnv.step of grasp_cube (no observers): without contact=, with the sensor, and with resolve='block' at S = 8."""
    from partmanip_amd.envs import make_grasp_cube_env
    with open(SCENE) as f:
        s = json.load(f)
    cfg = {"robot": {"driveMode": "ik", "mobile": False}, "explore_step": 40, "maxEpisodeLength": 200}
    tree = load_urdf(URDF)
    rows = []
    for N in sizes:
        g = torch.Generator().manual_seed(3)
        pts = (torch.rand(len(SLOTS) * PER_BODY, 3, generator=g) - 0.5) * torch.tensor([0.04, 0.02, 0.06])
        tsdf = TSDFfromMesh(N, 0.5, 50, DEV, sdf_dicts=synthetic_parts()[:11] + [box_grid()])
        sensor = ContactSensor(tsdf, pts.numpy(), np.repeat(SLOTS, PER_BODY), [PER_BODY] * 3, (11, 12), names=("hand", "lfinger", "rfinger"))
        a = torch.rand(N, 7, generator=g).to(DEV) * 2 - 1
        envs = {"plain": {}, "contact": dict(contact=sensor), "block": dict(contact=sensor, resolve="block", block_substeps=8)}
        built = {k: make_grasp_cube_env(cfg, N, DEV, tree, DT, base_pose=s["root"], dof=s["dof"], **kw) for k, kw in envs.items()}
        for env in built.values():
            env.reset()
            for _ in range(5):
                env.step(a)
        torch.cuda.synchronize()
        ms = {}
        for rnd in range(2):                                                             # alternate
            for k, env in built.items():
                ms.setdefault(k, []).append(timed(lambda: env.step(a), steps))
        rows.append(dict(N=N, steps=2 * steps, **{f"{k}_step_ms": round(float(np.mean(v)), 4) for k, v in ms.items()},
                         plain_step_ms_rounds=[round(v, 4) for v in ms["plain"]],
                         block_adds_ms=round(float(np.mean(ms["block"]) - np.mean(ms["contact"])), 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 4, 64 points per body, 3 calls (a smoke run)")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="also write the JSON there (profiles/guarded_step_timing.json)")
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    res = dict(tool="time_guarded_step", device=torch.cuda.get_device_name(0), bodies=len(SLOTS), points_per_body=64 if a.tiny else PER_BODY,
               cabinets=list(BODIES), substeps=list(SUBSTEPS), sweep=sweep_rows(sizes, a.tiny), step=step_rows(sizes, 3 if a.tiny else 50))
    print(json.dumps(res))
    if a.out and not a.tiny:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
