"""SHA-256 of everything the task step writes, for comparing two builds of the library bit for bit (PARTMANIP_HIP_LIB selects one;
run the tool once per library, each in its own process, and diff the listings).

Cases: GraspCubeTensors with the fixed and the mobile Franka under the 'ik' and 'pos' drives; OpenDrawerTensors with both robots over
three cabinet types, without random_reset and with it and a given u; each at N = 1, 5, 257 and 8260 with the default part list and at
N = 4130 with that list repeated to M = 60 parts (8 environments per block, set by the LDS cap).  States are seeded numpy draws, so
they do not depend on the device.  Each case runs end_step, begin_step, a trivial simulator (DOF position <- its target) and
end_step again, and prints one line per case and step, `case step tensor=sha256 ...`, with one SHA-256 per tensor written, the
rewritten root / dof_state_all rows and pos_act_all among them.

    python tools/task_step_digest.py [--sizes 1,5,257,8260] [--out listing.txt]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.tasks import Franka, GraspCubeTensors, MobileFranka, OpenDrawerTensors  # noqa: E402
from partmanip_amd.tasks.open_drawer import build_masks  # noqa: E402

DEV = "cuda:0"
TYPES = ((3, 1, 1, 2, 0), (5, 3, 2, 4, 2), (4, 2, 3, 1, 1))     # a cabinet's bodies, DOFs, target link, handle, target DOF
ROOT = [0.3, -0.1, 0.05, 0.2, -0.3, 0.6, 0.7]
M_CAP, N_CAP = 60, 4130
POST = ("rew_buf", "_extras", "success", "is_reached", "pose_R", "pose_T")
PRE = ("pos_act", "reset_buf", "reset_succ", "progress_buf", "success", "epis_max_rew", "epis_max_step")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unit(rng, *shape):
    q = rng.normal(size=shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_robot(mobile, drive, N):
    cfg = {"driveMode": drive, "root": ROOT}
    return MobileFranka(cfg, 1 / 60, N, DEV) if mobile else Franka(cfg, 1 / 60, N, DEV)


def rows(rng, n, centre, robot, index):
    """n x 13 body rows, the two tips of each environment (rows index[:, tip]) around `centre`, inside reach for every other one."""
    rb = rng.uniform(-0.5, 0.5, size=(n, 13))
    rb[:, 3:7] = unit(rng, n)
    near = np.where(np.arange(len(centre)) % 2 == 0, 0.0, 0.3)[:, None]
    lt, rt = index[:, robot.ltip_rb_index], index[:, robot.rtip_rb_index]
    rb[lt, :3], rb[rt, :3] = centre + near + 0.01, centre + near - 0.01
    rb[rt, 3:7] = rb[lt, 3:7]
    return rb.astype(np.float32)


def episode(rng, task, N):
    task.progress_buf.copy_(t(rng.randint(0, 100, size=N).astype(np.int64)))
    task.epis_max_rew.copy_(t(rng.uniform(-3, 8, size=N).astype(np.float32)))
    task.epis_max_step.copy_(t(rng.randint(0, 60, size=N).astype(np.int64)))


def repeated(part, part_C, M):
    reps = -(-M // part.numel())
    return part.repeat(reps)[:M].contiguous(), part_C.repeat(reps, 1, 1)[:M].contiguous()


def grasp_cube(N, mobile, drive, M, seed):
    rng = np.random.RandomState(seed)
    robot = make_robot(mobile, drive, N)
    nb, nd = robot.num_rigid_body + 1, robot.num_dofs
    kw = dict(num_bodies=nb, robot=robot)
    if M:
        d = GraspCubeTensors(1, DEV, {}, 1 / 60, **kw)
        kw["part_body"], kw["part_C"] = repeated(d.part_body, d.part_C, M)
    task = GraspCubeTensors(N, DEV, {"explore_step": 40}, 1 / 60, **kw)
    root = (rng.normal(size=(N, 2, 13)) * 0.1).astype(np.float32)
    root[:, :, 3:7] = unit(rng, N, 2)
    rb = rows(rng, N * nb, root[:, 1, :3], robot, np.arange(N * nb).reshape(N, nb)).reshape(N, nb, 13)
    dof = np.stack([rng.uniform(0, 0.03, size=(N, nd)), rng.normal(size=(N, nd))], axis=-1).astype(np.float32)
    jac = rng.normal(size=(N, nb - 2, 6, nd)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(N, robot.num_actions)).astype(np.float32)
    rb, dof, root, jac, act = t(rb), t(dof), t(root), t(jac), t(act)
    episode(rng, task, N)
    post = lambda: dict(normal_state=task.obs_buf["normal_state"], proprio=task.obs_buf["proprio_state"],   # noqa: E731
                        **{k: getattr(task, k) for k in POST})
    task.end_step(rb, dof, root)
    yield "end0", post()
    task.begin_step(act, dof, jac)
    yield "begin", dict(succ_rate=task.extras["succ_rate"], **{k: getattr(task, k) for k in PRE})
    dof[:, :, 0] = task.pos_act
    task.end_step(rb, dof, root)
    yield "end1", post()


def open_drawer(N, mobile, random_reset, M, seed):
    rng = np.random.RandomState(seed)
    robot = make_robot(mobile, "ik", N)
    nrb, nd = robot.num_rigid_body, robot.num_dofs
    types = [TYPES[i % 3] for i in range(N)]
    rbm, dfm, B, D = build_masks(nrb, nd, *[[ty[c] for ty in types] for c in range(5)])
    half = np.array([0.02, 0.08, 0.015])
    signs = np.array([[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, -1], [-1, 1, -1], [-1, 1, 1], [-1, -1, 1]])
    const = (rbm, dfm, np.arange(N) % 3, np.broadcast_to((signs * half).astype(np.float32), (N, 8, 3)).copy(),
             np.broadcast_to(np.array([1, 0, 0], dtype=np.float32), (N, 3)).copy(), np.zeros(N, dtype=np.float32),
             np.full(N, 0.2, dtype=np.float32), 3)
    kw = dict(num_rigid_bodies=B, num_dof_states=D, robot=robot)
    if M:
        d = OpenDrawerTensors(N, DEV, {}, 1 / 60, *const, **kw)
        kw["part_slot"], kw["part_C"] = repeated(d.part_slot, d.part_C, M)
    task = OpenDrawerTensors(N, DEV, {"explore_step": 40, "random_reset": random_reset}, 1 / 60, *const, **kw)
    root = (rng.normal(size=(N, 2, 13)) * 0.1).astype(np.float32)
    root[:, :, 3:7] = unit(rng, N, 2)
    rb = rows(rng, B, root[:, 1, :3], robot, rbm)
    dof = np.stack([rng.uniform(0, 0.03, size=D), rng.normal(size=D)], axis=-1).astype(np.float32)
    jac = rng.normal(size=(N, nrb - 1, 6, nd)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(N, robot.num_actions)).astype(np.float32)
    u = t(rng.uniform(0, 1, size=(N, 4)).astype(np.float32)) if random_reset else None
    rb, dof, root, jac, act, pa = t(rb), t(dof), t(root), t(jac), t(act), torch.zeros(D, device=DEV)
    episode(rng, task, N)
    post = lambda: dict(normal_state=task.obs_buf["normal_state"], part_bbox=task.part_bbox, succ_objid=task.succ_objid_lst,   # noqa: E731
                        robot_dof_state=task.robot_dof_state, part_dof_state=task.part_dof_state, **{k: getattr(task, k) for k in POST})
    task.end_step(rb, dof, root)
    yield "end0", post()
    task.begin_step(act, jac, dof, root, pa, u=u)
    yield "begin", dict(succ_rate=task.extras["succ_rate"], root=root, dof_state_all=dof, pos_act_all=pa,
                        robot_dof_state=task.robot_dof_state, part_dof_state=task.part_dof_state, **{k: getattr(task, k) for k in PRE})
    m = t(dfm[:, :nd].astype(np.int64))
    dof[m, 0] = pa[m]
    task.end_step(rb, dof, root)
    yield "end1", post()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,5,257,8260", help=f"N of the cases with the default part list; N = {N_CAP} with M = {M_CAP} always runs")
    ap.add_argument("--out", default=None, help="file the listing is also written to")
    a = ap.parse_args()
    shapes = [(int(v), 0) for v in a.sizes.split(",")] + [(N_CAP, M_CAP)]
    lines = []
    for i, (N, M) in enumerate(shapes):
        size = f"N={N}" + (f",M={M}" if M else "")
        cases = [(f"grasp_cube/{'mobile' if mob else 'fixed'}/{drive}/{size}", grasp_cube(N, mob, drive, M, 100 + i))
                 for mob in (False, True) for drive in ("ik", "pos")]
        cases += [(f"open_drawer/{'mobile' if mob else 'fixed'}/{'random_reset' if rnd else 'plain'}/{size}", open_drawer(N, mob, rnd, M, 200 + i))
                  for mob in (False, True) for rnd in (False, True)]
        for name, steps in cases:
            for step, tensors in steps:
                sha = {k: hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in tensors.items()}
                lines.append(f"{name} {step} " + " ".join(f"{k}={v}" for k, v in sha.items()))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
