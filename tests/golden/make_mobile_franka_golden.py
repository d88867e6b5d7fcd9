"""Dev-machine generator of the mobile Franka fixtures (tests/test_mobile_franka_host.py, tests/test_gpu_mobile_franka.py): runs the
REFERENCE's own open_drawer.compute_observations, compute_reward, hand_base.pre_physics_step (franka.control with `mobile`) and
open_drawer.reset_idx on the CPU, once in float32 and once in float64, for the robot of the reference's shipped open_drawer task: three
virtual base joints in front of the arm, 12 DOFs, 17 bodies, tips 14 / 16, a 16-link Jacobian.

    python tests/golden/make_mobile_franka_golden.py /path/to/reference

Everything that does not know the robot comes from make_open_drawer_golden.py, loaded here as a private copy whose robot constants
are set to the mobile asset's (its functions read them when they are called) and whose build_task sets `robot.mobile`: the stand-in
isaacgym modules, the scene construction, the cabinet types, the four pre-physics RUNS and its check_conditions.  Added here: the
action rows (N, 10) for 'ik' and (N, 11) for 'pos', base positions within 0.004 of a limit with the action pushing outward in some
environments, and the rows of rigid_body_all that nothing reads (velocities of every body but the tips, poses of bodies that are
neither posed parts nor tips) set to zero and the Jacobian's entries cut to 16 significant bits, both to keep the files small.

Writes mobile_franka_ref_small.npz (N = 5; robot root and default DOFs of the reference's cfg/tasks/open_drawer.yaml) and
mobile_franka_ref_70.npz (N = 70; a tilted root quaternion, so that base_R is far from symmetric).  check_conditions (asserted here
and again on the committed files by tests/test_mobile_franka_host.py) carries the open_drawer generator's conditions over and adds the
mobile ones."""
import os
os.environ["PYTORCH_JIT"] = "0"                               # before torch is imported
import importlib.util  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import mobile_franka_ref as MF  # noqa: E402

NRB, ND, NBASE, NL, LTIP, RTIP = 17, 12, 3, 16, 14, 16
MESH_BODIES = (3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15)            # link0-7, hand, left finger, right finger
DOF_LO = np.array([-0.2, -0.2, -0.1, -2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0], dtype=np.float32)
DOF_HI = np.array([0.2, 0.2, 0.1, 2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04], dtype=np.float32)
# (file, N, seed, robot root, default DOFs); the first pair of constants is the shipped yaml's
CASES = (("mobile_franka_ref_small", 5, 7101, (0.4, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0),
          (0, 0, 0, -0.2724, -0.1511, 0.2898, -2.3792, -2.8973, 2.4690, 2.3973, 0.04, 0.04)),
         ("mobile_franka_ref_70", 70, 7102, (0.3, -0.1, 0.05, 0.2, -0.3, 0.6, 0.7),
          (0.05, -0.03, 0.02, 0.3, -0.4, -0.3, -2.2, -0.1, 2.0, -0.5, 0.04, 0.04)))
PUSH_INSIDE, PUSH_ACTION = 0.002, 0.9                         # distance from the limit; the action's size along the pushed axis


def part_defaults():
    C = np.zeros((13, 3, 3), dtype=np.float32)
    C[:, 0, 0] = 1
    C[:11, 1, 2] = -1
    C[:11, 2, 1] = 1
    C[10, 1, 2] = 1
    C[11] = C[12] = np.eye(3)
    return np.array(list(MESH_BODIES) + [NRB, NRB + 1], dtype=np.int32), C


def base_generator():
    """make_open_drawer_golden.py as a private module with the mobile robot's constants."""
    spec = importlib.util.spec_from_file_location("_mobile_franka_open_drawer_golden", os.path.join(HERE, "make_open_drawer_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    g.NRB, g.ND, g.NL, g.LTIP, g.RTIP, g.DOF_LO, g.DOF_HI, g.part_defaults = NRB, ND, NL, LTIP, RTIP, DOF_LO, DOF_HI, part_defaults
    fixed = g.build_task

    def build_task(*a, **k):
        task = fixed(*a, **k)
        task.robot.mobile = True
        return task

    g.build_task = build_task
    return g


def pushed(N):
    """(environment, base axis, side) of the base positions that sit next to a limit."""
    envs = [i for i in range(N) if N < 10 or i % 5 == 2]       # a few environments: every one, whichever of them a run resets
    return [(i, i % 3, 1.0 if (i // 2) % 2 else -1.0) for i in envs]


def make_inputs(g, N, seed, robot_root, default_dof):
    g.ROBOT_ROOT, g.DEFAULT_DOF = np.array(robot_root, dtype=np.float32), np.array(default_dof, dtype=np.float32)
    inp = g.make_inputs(N, seed)
    rng = np.random.RandomState(seed + 1000)
    act, act_pos = rng.uniform(-1, 1, size=(N, 7 + NBASE)), rng.uniform(-1, 1, size=(N, ND - 1))
    R = MF.base_matrix(g.ROBOT_ROOT)
    dfm, dof = inp["dof_state_mask"], inp["dof_state_all"].copy()
    for i, axis, side in pushed(N):
        lim = (DOF_HI if side > 0 else DOF_LO)[axis]
        dof[dfm[i, axis], 0] = lim - side * PUSH_INSIDE
        d = rng.uniform(-0.3, 0.3, size=3)                    # R^T (0.005 a[:3]) = 0.005 d: 0.0045 outward along `axis`
        d[axis] = side * PUSH_ACTION
        act[i, :3] = act_pos[i, :3] = R @ d
    assert np.abs(act).max() <= 1 and np.abs(act_pos).max() <= 1
    rb, rbm = inp["rigid_body_all"].copy(), inp["rigid_body_mask"]
    tips = np.zeros(len(rb), dtype=bool)
    tips[rbm[:, [LTIP, RTIP]].reshape(-1)] = True
    read = tips.copy()
    read[rbm[:, inp["part_slot"]].reshape(-1)] = True
    rb[~tips, 7:] = 0
    rb[~read] = 0
    jac = (inp["jac"].view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)       # 16 significant bits: products still round
    inp.update(jac=jac, actions=act.astype(np.float32), actions_pos=act_pos.astype(np.float32), dof_state_all=dof, rigid_body_all=rb)
    return inp


def base_targets(fx, run, drive):
    """(unclamped float64 base targets (N, 3) of the restated drive, the reference's float64 ones, the run's reset flags)."""
    dfm = fx["dof_state_mask"]
    q = fx["dof_state_all"][dfm[:, :ND]]
    free = MF.unclamped(fx["actions" if drive == "ik" else "actions_pos"], q, fx["jac"], LTIP - 1, RTIP - 1, float(fx["dt"]), drive,
                        MF.base_matrix(fx["robot_default_root"]))[:, :NBASE]
    return free, fx[f"out64_{run}_pos_act_all"][dfm[:, :NBASE]], fx[f"out64_{run}_reset"]


def check_conditions(fx, g=None):
    """The conditions of the fixtures; fx: the dict that is (or was) written to the .npz."""
    g = g or base_generator()
    g.check_conditions(fx)                                    # every condition of the open_drawer fixtures, at nd = 12 / nrb = 17
    N = fx["root"].shape[0]
    dfm = fx["dof_state_mask"]
    assert fx["actions"].shape == (N, 10) and fx["actions_pos"].shape == (N, 11) and fx["jac"].shape == (N, NL, 6, ND)
    assert np.array_equal(fx["part_slot"], list(MESH_BODIES) + [NRB, NRB + 1]) and int(fx["ltip"]) == LTIP and int(fx["rtip"]) == RTIP
    others = [l for l in range(NL) if l not in (LTIP - 1, RTIP - 1)]
    assert not fx["jac"][:, others].any() and (fx["jac"][:, [LTIP - 1, RTIP - 1]] != 0).all()
    R = MF.base_matrix(fx["robot_default_root"])
    if N == 70:
        assert np.abs(R - R.T).max() >= 0.3
    lo, hi = fx["dof_lo"][:NBASE].astype(np.float64), fx["dof_hi"][:NBASE].astype(np.float64)
    # base targets: clamped at a limit in at least 2 environments that go on, on both sides somewhere; at least half of the base
    # targets of the environments that go on are not clamped (and, where there are enough environments, at least half of those
    # environments have no clamped base target at all); nothing sits closer than the threshold margin to a limit before the clamp
    sides = set()
    for run, drive, mode, rnd in g.RUNS:
        free, got, rs = base_targets(fx, run, drive)
        over = (free > hi) | (free < lo)
        assert np.abs(np.stack([free - lo, free - hi])).min() >= g.MARGIN, run
        live = ~rs
        assert np.array_equal(got[live][over[live]], np.where(free > hi, hi, lo)[live][over[live]]), run
        need = 2 if mode == "train" else min(2, int(live.sum()))      # the small fixture's test runs leave one environment going
        assert over[live].any(axis=1).sum() >= need and over[live].sum() * 2 <= over[live].size, run
        if N >= 10:
            assert (~over[live].any(axis=1)).sum() * 2 >= live.sum(), run
            sides |= {-1} if (free[live] < lo).any() else set()
            sides |= {1} if (free[live] > hi).any() else set()
    assert N < 10 or sides == {-1, 1}
    q = fx["dof_state_all"][dfm[:, :NBASE], 0].astype(np.float64)
    assert (np.minimum(q - lo, hi - q).min(axis=1) <= 0.004).sum() >= 2
    # the restated contract reproduces the reference's float64 run ...
    after = MF.post(fx)
    for run, drive, mode, rnd in g.RUNS:
        s, _, root, dof, pa = MF.begin_step(fx, after, drive, mode == "train", rnd)
        for k, v in (("pos_act_all", pa), ("root", root), ("dof_state_all", dof)):
            assert np.abs(v - fx[f"out64_{run}_{k}"]).max() <= 1e-12, (run, k)
        assert np.array_equal(s["reset"], fx[f"out64_{run}_reset"]), run
    # ... and each mobile-specific term is visible: a drive without it misses the reference's 'ik' targets by at least 100 e_ref in
    # at least a quarter of the environments that go on (the un-transposed base_R where base_R is not symmetric: the 70 fixture)
    ref = fx["out64_ik_train_pos_act_all"]
    e_ref = float(np.abs(fx["out32_ik_train_pos_act_all"].astype(np.float64) - ref).max())
    live = ~fx["out64_ik_train_reset"]
    assert e_ref > 0
    for wrong in MF.WRONG:
        if wrong == "no_transpose" and np.abs(R - R.T).max() < 0.3:
            continue
        tgt = MF.begin_step(fx, after, "ik", True, False, wrong=wrong)[1]
        miss = np.abs(tgt - ref[dfm[:, :ND]]).max(axis=1)
        assert (miss[live] >= 100 * e_ref).sum() * 4 >= live.sum(), (wrong, miss[live], e_ref)


def main(reference_root):
    g = base_generator()
    mods, gym = g.load_reference(reference_root)
    for name, N, seed, robot_root, default_dof in CASES:
        inp = make_inputs(g, N, seed, robot_root, default_dof)
        torch.set_default_dtype(torch.float64)
        rew64 = g.run_reference(mods, gym, inp, torch.float64)["rew"]
        emr, ems = g.bookkeeping_before(inp, rew64)
        o64 = g.run_reference(mods, gym, inp, torch.float64, (emr, ems))
        torch.set_default_dtype(torch.float32)
        o32 = g.run_reference(mods, gym, inp, torch.float32, (emr, ems))
        fx = {k: v for k, v in inp.items() if not k.startswith("u_")}
        fx.update(before_epis_max_rew=emr, before_epis_max_step=ems)
        fx.update({"out32_" + k: v for k, v in o32.items()})
        fx.update({"out64_" + k: v for k, v in o64.items()})
        check_conditions(fx, g)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **fx)
        e = {k: float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in ("normal_state", "rew", "pose_R", "ik_train_pos_act_all",
                                                                                  "pos_test_pos_act_all")}
        print(f"{name}: {os.path.getsize(path)} bytes; reached {int(o64['is_reached'].sum())}, success {int(o64['success'].sum())}, "
              f"reset {int(o64['ik_train_reset'].sum())} / {N}; e_ref {e}")


if __name__ == "__main__":
    main(sys.argv[1])
