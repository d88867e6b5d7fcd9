"""The mobile Franka on the GPU: partmanip_amd.tasks.MobileFranka behind OpenDrawerTensors and GraspCubeTensors
(pm_franka_control_mobile_f32 in csrc/task_grasp_cube.hip, and the first runs of pm_open_drawer_post_f32 / pm_open_drawer_reset_f32 at
nd = 12, nrb = 17) against the REFERENCE's own task code with `mobile` set (fixtures of tests/golden/make_mobile_franka_golden.py)
and against the numpy restatement of the contract (tests/mobile_franka_ref.py).

Tolerance of the parity tests (the rule of tests/test_gpu_open_drawer.py): e_ref = max |out32 - out64| of a fixture's output group is
what the reference's own float32 run loses against its float64 run; the kernel must stay within 4 e_ref of out64.  Flags and integers
must be equal; a group with e_ref = 0 (rows that are copies of constants) must be equal.  Where a test compares states the fixtures do
not cover against the float64 restatement, the bound is stated at the comparison.  Every margin goes through record_margin (folded into
profiles/mobile_franka_margins.json)."""
import functools

import numpy as np
import pytest
import torch

from tests import grasp_cube_ref as G
from tests import mobile_franka_ref as MF
from tests import open_drawer_ref as OD
from tests import helpers
from tests.helpers import load, npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
within = functools.partial(helpers.within, prefix="mobile_franka ")
SENTINEL = -777.25
EPS = float(np.finfo(np.float32).eps)
ND, NRB, NBASE = 12, 17, 3
MESH = [3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15]
GROUPS = ("normal_state", "part_bbox", "rew", "pose_R", "pose_T")
RUNS = (("ik_train", "ik", "train", False), ("ik_test_rand", "ik", "test", True), ("pos_train_rand", "pos", "train", True),
        ("pos_test", "pos", "test", False))
FIXTURES = ["mobile_franka_ref_small", "mobile_franka_ref_70"]


def make_robot(fx, n, drive="ik"):
    from partmanip_amd.tasks import MobileFranka
    return MobileFranka({"driveMode": drive, "mobile": True, "dof": fx["default_dof_pos"].tolist(), "root": fx["robot_default_root"].tolist()},
                        float(fx["dt"]), n, DEV)


def make_task(fx, idx=None, drive="ik", random_reset=False):
    """A task over the environments idx (any order; default all) of a fixture; the flat state tensors are shared."""
    from partmanip_amd.tasks import OpenDrawerTensors
    idx = np.arange(fx["root"].shape[0]) if idx is None else np.asarray(idx)
    cfg = {"explore_step": int(fx["explore_step"]), "maxEpisodeLength": 200, "random_reset": random_reset}
    task = OpenDrawerTensors(len(idx), DEV, cfg, float(fx["dt"]), fx["rigid_body_mask"][idx], fx["dof_state_mask"][idx], fx["obj_id"][idx],
                             fx["part_bbox_init"][idx], fx["part_axis_dir_init"][idx], fx["joint_lo"][idx], fx["joint_hi"][idx],
                             int(fx["num_objs"]), num_rigid_bodies=fx["rigid_body_all"].shape[0], num_dof_states=fx["dof_state_all"].shape[0],
                             obj_default_root=fx["obj_default_root"], robot=make_robot(fx, len(idx), drive))
    task.succ_objid_lst.copy_(t(fx["before_succ_objid"]))
    assert task.num_obs["normal_state"] == 53 and task.part_slot.tolist() == MESH + [NRB, NRB + 1] == fx["part_slot"].tolist()
    return task


def post_outputs(task):
    return dict(normal_state=npy(task.obs_buf["normal_state"]), part_bbox=npy(task.part_bbox), rew=npy(task.rew_buf), extras=npy(task._extras),
                success=npy(task.success), is_reached=npy(task.is_reached), pose_R=npy(task.pose_R), pose_T=npy(task.pose_T),
                robot_dof_state=npy(task.robot_dof_state), part_dof_state=npy(task.part_dof_state))


def run_post(fx, idx=None):
    idx = np.arange(fx["root"].shape[0]) if idx is None else np.asarray(idx)
    task = make_task(fx, idx)
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"][idx]))
    return post_outputs(task), task


def run_pre(fx, idx=None, drive="ik", mode="train", rnd=False, actions=None, jac=None):
    """end_step then begin_step over the environments idx, from the fixture's state before the step; everything begin_step writes."""
    idx = np.arange(fx["root"].shape[0]) if idx is None else np.asarray(idx)
    task = make_task(fx, idx, drive=drive, random_reset=rnd)
    task.train_test_flag = mode
    if mode == "test":
        task.max_episode_length = int(fx["max_episode_length_test"])
    task.progress_buf.copy_(t(fx["before_progress"][idx] - 1))
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"][idx]))
    task.epis_max_rew.copy_(t(fx["before_epis_max_rew"][idx]))
    task.epis_max_step.copy_(t(fx["before_epis_max_step"][idx]))
    rew = npy(task.rew_buf)
    dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"][idx]), t(fx["pos_act_all_before"])
    act = t((fx["actions" if drive == "ik" else "actions_pos"] if actions is None else actions)[idx])
    out_pa, reset = task.begin_step(act, t((fx["jac"] if jac is None else jac)[idx]), dof_all, root, pa_all, u=t(fx["u"][idx]))
    assert out_pa is pa_all and reset is task.reset_buf
    out = dict(pos_act_all=npy(pa_all), root=npy(root), dof_state_all=npy(dof_all), pos_act=npy(task.pos_act), reset=npy(reset),
               reset_succ=npy(task.reset_succ), progress=npy(task.progress_buf), success=npy(task.success),
               epis_max_rew=npy(task.epis_max_rew), epis_max_step=npy(task.epis_max_step), robot_dof_state=npy(task.robot_dof_state),
               part_dof_state=npy(task.part_dof_state), rew=rew)
    return out, task


PER_ENV = ("root", "pos_act", "reset", "reset_succ", "progress", "success", "epis_max_rew", "epis_max_step", "robot_dof_state", "part_dof_state")


# ------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity_after_physics(name):
    fx = load(name)
    task = make_task(fx)
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    obs, rew, _, extras = task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))
    rot, pos = task.compute_scene_pose()
    got = dict(normal_state=npy(obs["normal_state"]), part_bbox=npy(task.part_bbox), rew=npy(rew), pose_R=npy(rot), pose_T=npy(pos))
    assert got["normal_state"].shape[1] == 53 and got["pose_R"].shape[1:] == (13, 3, 3)
    for k in GROUPS:
        assert got[k].dtype == np.float32 and got[k].shape == fx["out64_" + k].shape, k
        within(name, k, got[k], fx["out32_" + k], fx["out64_" + k])
    for i, col in enumerate(OD.EXTRAS):
        e = npy(extras[col])
        if col in ("is_open", "is_open_notgrasp", "is_grasped"):
            assert np.array_equal(e, fx["out64_extras"][:, i].astype(np.float32)), col
        else:
            within(name, "extras." + col, e, fx["out32_extras"][:, i], fx["out64_extras"][:, i])
    assert np.array_equal(npy(task.success), fx["out64_success"]) and np.array_equal(npy(task.is_reached), fx["out64_is_reached"])
    assert np.array_equal(npy(extras["is_reached"]), fx["out64_is_reached"])
    assert np.array_equal(npy(extras["success_objnum"]), fx["out64_succ_objid"])       # with the flag that was set beforehand
    assert fx["before_succ_objid"].any() and not np.array_equal(fx["before_succ_objid"], fx["out64_succ_objid"])
    assert np.array_equal(npy(extras["raw_reward"]), got["rew"])
    assert same_bits(npy(task.robot_dof_state), fx["dof_state_all"][fx["dof_state_mask"][:, :ND]])
    assert same_bits(npy(task.part_dof_state), fx["dof_state_all"][fx["dof_state_mask"][:, ND]])
    assert np.array_equal(npy(task.progress_buf), fx["before_progress"])
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))       # sticky: a second step clears nothing
    assert np.array_equal(npy(task.succ_objid_lst), fx["out64_succ_objid"])


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity_before_physics(name):
    fx = load(name)
    N, D = fx["root"].shape[0], fx["dof_state_all"].shape[0]
    dfm = fx["dof_state_mask"]
    for run, drive, mode, rnd in RUNS:
        got, task = run_pre(fx, drive=drive, mode=mode, rnd=rnd)
        assert task.num_actions == (10 if drive == "ik" else 11)
        o = lambda k, p=64: fx[f"out{p}_{run}_{k}"]             # noqa: E731
        for k in ("pos_act_all", "root", "dof_state_all"):
            within(f"{name} {run}", k, got[k], o(k, 32), o(k))
        rs = o("reset")
        # the base targets on their own: the group's e_ref is set by the arm's solve
        base = got["pos_act_all"][dfm[:, :NBASE]]
        e_base = float(np.abs(o("pos_act_all", 32)[dfm[:, :NBASE]].astype(np.float64) - o("pos_act_all")[dfm[:, :NBASE]]).max())
        err = float(np.abs(base.astype(np.float64) - o("pos_act_all")[dfm[:, :NBASE]]).max())
        if e_base > 0:
            record_margin(f"mobile_franka {name} {run}: base targets max |hip - out64| / e_ref", err / e_base, 4.0, e_ref=e_base)
        assert err <= 4 * e_base, (run, err, e_base)
        lo, hi = fx["dof_lo"][:NBASE], fx["dof_hi"][:NBASE]
        assert ((base[~rs] == lo) | (base[~rs] == hi)).any(axis=1).sum() >= min(2, int((~rs).sum())), run      # clamped at the limit itself
        assert np.array_equal(got["reset"], rs) and np.array_equal(got["progress"], o("after_progress")), run
        assert np.array_equal(got["success"], o("after_success")) and np.array_equal(got["epis_max_step"], o("after_epis_max_step"))
        emr = np.where(rs, np.float32(-100.0), np.maximum(got["rew"], fx["before_epis_max_rew"]) if mode == "train" else fx["before_epis_max_rew"])
        assert same_bits(got["epis_max_rew"], emr.astype(np.float32))
        # what the reference leaves alone holds its value bit for bit: rows of environments that go on, a cabinet's other joints,
        # the target entries of everything that is not a robot DOF
        keep_dof = np.ones(D, dtype=bool)
        keep_dof[dfm[rs].reshape(-1)] = False
        assert keep_dof.sum() > 0 and same_bits(got["dof_state_all"][keep_dof], fx["dof_state_all"][keep_dof]), run
        assert same_bits(got["root"][~rs], fx["root"][~rs]), run
        keep_pa = np.ones(D, dtype=bool)
        keep_pa[dfm[:, :ND].reshape(-1)] = False
        assert keep_pa.sum() >= N and same_bits(got["pos_act_all"][keep_pa], fx["pos_act_all_before"][keep_pa]), run
        # the compact tensors carry the rewritten rows; resetting environments get the default pose over all 12 DOFs
        assert same_bits(got["robot_dof_state"], got["dof_state_all"][dfm[:, :ND]]) and same_bits(got["part_dof_state"], got["dof_state_all"][dfm[:, ND]])
        assert same_bits(got["pos_act_all"][dfm[:, :ND]], got["pos_act"])
        assert same_bits(got["pos_act"][rs], np.broadcast_to(fx["default_dof_pos"], (int(rs.sum()), ND)))
        slot = task._counters[2 * task._slot:2 * task._slot + 2].cpu().numpy()
        assert int(slot[0]) == int(fx["out64_success"].sum()) and int(slot[1]) == int(rs.sum())
        if mode == "train":
            assert np.array_equal(got["reset_succ"], o("reset_succ"))
            assert np.array_equal(npy(task.extras["succ_rate"]), o("succ_rate").reshape(1))


# ------------------------------------------------------------------------------------------- 2. independence
def test_every_environment_alone_in_the_batch_and_in_a_permuted_batch_gives_the_same_bits():
    fx = load("mobile_franka_ref_70")
    N = 70
    dfm = fx["dof_state_mask"]
    full, _ = run_post(fx)
    perm = np.random.RandomState(3).permutation(N)
    shuffled, ptask = run_post(fx, perm)
    for k, v in shuffled.items():
        assert same_bits(v, full[k][perm]), k
    assert np.array_equal(npy(ptask.succ_objid_lst), fx["out64_succ_objid"])
    for drive in ("ik", "pos"):
        pre, _ = run_pre(fx, drive=drive, rnd=True)
        assert 0 < pre["reset"].sum() < N
        ppre, _ = run_pre(fx, perm, drive=drive, rnd=True)
        for k in PER_ENV:
            assert same_bits(ppre[k], pre[k][perm]), (drive, k)
        for k in ("pos_act_all", "dof_state_all"):              # the permuted batch rewrites the flat tensors to the same bits
            assert same_bits(ppre[k], pre[k]), (drive, k)
        for e in list(range(0, N, 7)) + [2, 68, 69]:            # 2, 7 and 42 sit next to a base limit
            one, _ = run_pre(fx, [e], drive=drive, rnd=True)
            for k in PER_ENV:
                assert same_bits(one[k], pre[k][e:e + 1]), (drive, k, e)
            assert same_bits(one["pos_act_all"][dfm[e, :ND]], pre["pos_act_all"][dfm[e, :ND]]), (drive, e)
            if drive == "ik":
                post1, _ = run_post(fx, [e])
                for k, v in post1.items():
                    assert same_bits(v, full[k][e:e + 1]), (k, e)
    small = load("mobile_franka_ref_small")
    sfull, _ = run_post(small)
    spre, _ = run_pre(small)
    for e in range(5):
        one, _ = run_post(small, [e])
        for k, v in one.items():
            assert same_bits(v, sfull[k][e:e + 1]), (k, e)
        one, _ = run_pre(small, [e])
        for k in PER_ENV:
            assert same_bits(one[k], spre[k][e:e + 1]), (k, e)


def test_a_nan_stays_inside_its_environment():
    fx = load("mobile_franka_ref_70")
    N = 70
    live = np.nonzero(~fx["out64_ik_train_reset"])[0]
    va, vj = int(live[3]), int(live[len(live) // 2])            # two environments that go on, in different blocks
    assert va != vj and abs(va - vj) >= 8
    clean, _ = run_pre(fx)
    act = fx["actions"].copy()
    act[va, 1] = np.nan                                       # one base action
    jac = fx["jac"].copy()
    jac[vj, int(fx["rtip"]) - 1, 4, NBASE + 2] = np.nan         # one arm entry of a tip link's Jacobian
    got, _ = run_pre(fx, actions=act, jac=jac)
    others = np.ones(N, dtype=bool)
    others[[va, vj]] = False
    for k in PER_ENV:
        assert same_bits(got[k][others], clean[k][others]), k
    for k in ("reset", "reset_succ", "progress", "success", "epis_max_step", "epis_max_rew"):        # the flags do not see the drive
        assert same_bits(got[k], clean[k]), k
    assert not np.isnan(got["pos_act"][others]).any()
    # the base action reaches the base targets and, through dpose, the arm; the fingers have their own action
    assert np.isnan(got["pos_act"][va, :ND - 2]).all() and same_bits(got["pos_act"][va, ND - 2:], clean["pos_act"][va, ND - 2:])
    # the Jacobian reaches the arm alone
    assert np.isnan(got["pos_act"][vj, NBASE:ND - 2]).all()
    assert same_bits(got["pos_act"][vj, :NBASE], clean["pos_act"][vj, :NBASE]) and same_bits(got["pos_act"][vj, ND - 2:], clean["pos_act"][vj, ND - 2:])
    # the base's own Jacobian columns are never read: NaN there changes nothing
    jac = fx["jac"].copy()
    jac[:, :, :, :NBASE] = np.nan
    got, _ = run_pre(fx, jac=jac)
    for k in PER_ENV + ("pos_act_all", "dof_state_all"):
        assert same_bits(got[k], clean[k]), k
    # 'pos': a NaN base action stays in the base targets
    clean, _ = run_pre(fx, drive="pos")
    act = fx["actions_pos"].copy()
    act[va, 2] = np.nan
    got, _ = run_pre(fx, drive="pos", actions=act)
    others[vj] = True
    for k in PER_ENV:
        assert same_bits(got[k][others], clean[k][others]), k
    assert np.isnan(got["pos_act"][va, :NBASE]).all() and same_bits(got["pos_act"][va, NBASE:], clean["pos_act"][va, NBASE:])


def test_sixteen_environments_per_block_give_the_bits_of_four():
    """Every other test here runs at N <= 70, where the post kernel takes 4 environments per block and the control kernel 8.  The 70
    fixture 118 times over (N = 8260: both take 16, the last block holds 4) must give, in environment e, the bits of environment
    e mod 70 of the plain fixture: begin_step ('ik', train, random_reset), then end_step on the rows it rewrote."""
    fx = load("mobile_franka_ref_70")
    reps, B, D = 118, fx["rigid_body_all"].shape[0], fx["dof_state_all"].shape[0]
    rep = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))   # noqa: E731
    big = dict(fx)
    for k in ("rigid_body_all", "dof_state_all", "pos_act_all_before", "root", "obj_id", "part_bbox_init", "part_axis_dir_init", "joint_lo",
              "joint_hi", "before_progress", "before_epis_max_rew", "before_epis_max_step", "actions", "jac", "u"):
        big[k] = rep(fx[k])
    for k, rows in (("rigid_body_mask", B), ("dof_state_mask", D)):     # copy j reads and writes its own rows
        big[k] = np.concatenate([fx[k] + j * rows for j in range(reps)]).astype(np.int32)
    res = []
    for f in (fx, big):
        pre, task = run_pre(f, rnd=True)
        task.end_step(t(f["rigid_body_all"]), t(pre["dof_state_all"]), t(pre["root"]))
        res.append((pre, post_outputs(task), npy(task.succ_objid_lst)))
    (pre, post, flags), (bpre, bpost, bflags) = res
    assert bpre["reset"].shape == (70 * reps,) and 0 < pre["reset"].sum() < 70
    for k in PER_ENV + ("pos_act_all", "dof_state_all", "rew"):
        assert same_bits(bpre[k], rep(pre[k])), k
    for k, v in post.items():
        assert same_bits(bpost[k], rep(v)), k
    assert np.array_equal(bflags, flags)


def test_eight_environments_per_block_set_by_the_lds_cap_give_the_bits_of_four():
    """helpers.lds_cap_check: at M = 60 an environment costs 4352 B (nrb = 17, nd = 12), so 8 per block are what the 48 KB hold; the test
    above reaches 16 through the grid rule alone."""
    fx = load("mobile_franka_ref_70")
    helpers.lds_cap_check(fx, make_task(fx), 13)


# ------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("name,drive", [("mobile_franka_ref_70", "ik"), ("mobile_franka_ref_70", "pos"), ("mobile_franka_ref_small", "ik")])
def test_actions_as_a_column_view_of_a_wider_buffer(name, drive):
    fx = load(name)
    N = fx["root"].shape[0]
    A = 10 if drive == "ik" else 11
    clean, _ = run_pre(fx, drive=drive)
    task = make_task(fx, drive=drive)
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))
    task.epis_max_rew.copy_(t(fx["before_epis_max_rew"]))
    task.epis_max_step.copy_(t(fx["before_epis_max_step"]))
    width = A + 7                                             # odd: the rows' alignment walks through all four residues
    buf = torch.full((N, width), SENTINEL, device=DEV)
    buf[:, 4:4 + A] = t(fx["actions" if drive == "ik" else "actions_pos"])
    before = npy(buf).copy()
    view = buf[:, 4:4 + A]
    assert view.stride(0) == width > A and not view.is_contiguous()
    dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"]), t(fx["pos_act_all_before"])
    task.begin_step(view, t(fx["jac"]), dof_all, root, pa_all, u=t(fx["u"]))
    assert same_bits(npy(task.pos_act), clean["pos_act"]) and same_bits(npy(pa_all), clean["pos_act_all"])
    assert same_bits(npy(task.reset_buf), clean["reset"]) and same_bits(npy(root), clean["root"]) and same_bits(npy(dof_all), clean["dof_state_all"])
    assert same_bits(npy(buf), before)


# ------------------------------------------------------------------------------------------- 4. several steps in a row
def control_bound(fx, idx, before_q, want_pos_act):
    """Per environment: a float32 Cholesky solve is backward stable, |du| <= 64 eps cond(A) |u| (tests/test_gpu_grasp_cube.py), with
    A from the arm's columns, plus 8 eps |target| for the rounding of qpos + u and of the targets; the base targets (three products,
    two sums, one more sum, on numbers below 1) add at most 8 eps max(1, |target|)."""
    jl, jr = int(fx["ltip"]) - 1, int(fx["rtip"]) - 1
    J = (fx["jac"][idx, jl, :, NBASE:ND - 2].astype(np.float64) + fx["jac"][idx, jr, :, NBASE:ND - 2]) / 2
    cond = np.linalg.cond(J @ J.transpose(0, 2, 1) + 0.0025 * np.eye(6))
    move = np.abs(want_pos_act - before_q).max(axis=1)
    return 64 * EPS * cond * np.maximum(move, 1e-3) + 8 * EPS * np.abs(want_pos_act).max() \
        + 8 * EPS * max(1.0, float(np.abs(want_pos_act[:, :NBASE]).max()))


def test_three_steps_in_a_row_follow_the_restated_task():
    """Three begin_step / end_step rounds around a trivial simulator (DOF position <- its target), the test of
    tests/test_gpu_open_drawer.py with the mobile robot.  Each round is compared with the float64 restatement evaluated on the state
    the round started from, so rounding does not accumulate.  Bounds: those stated there (observation row and box 64 eps P / l, reward
    and extras 20 times that, rewritten root rows 8 eps, rewritten DOF rows equal) and control_bound for the joint targets."""
    fx = load("mobile_franka_ref_small")
    N = 5
    dfm = fx["dof_state_mask"]
    task = make_task(fx, random_reset=True)
    rng = np.random.RandomState(12)
    rb_all, dof_all, root, pa_all = (t(fx[k]) for k in ("rigid_body_all", "dof_state_all", "root", "pos_act_all_before"))
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    task.end_step(rb_all, dof_all, root)
    task.epis_max_rew.copy_(t(fx["before_epis_max_rew"]))
    task.epis_max_step.copy_(t(fx["before_epis_max_step"]))
    jl, jr = int(fx["ltip"]) - 1, int(fx["rtip"]) - 1
    R = MF.base_matrix(fx["robot_default_root"])
    flags = fx["out64_succ_objid"].copy()
    n_reset = n_live = 0
    for step in range(3):
        state = dict(rew=npy(task.rew_buf), success=npy(task.success), progress=npy(task.progress_buf),
                     epis_max_rew=npy(task.epis_max_rew), epis_max_step=npy(task.epis_max_step))
        before = dict(root=npy(root), dof=npy(dof_all), pa=npy(pa_all), rds=npy(task.robot_dof_state))
        act = rng.uniform(-1, 1, size=(N, 10)).astype(np.float32)
        u = rng.uniform(0, 1, size=(N, 4)).astype(np.float32)
        _, reset = task.begin_step(t(act), t(fx["jac"]), dof_all, root, pa_all, u=t(u))
        tgt = MF.control(act, before["rds"], fx["jac"], jl, jr, fx["dof_lo"], fx["dof_hi"], float(fx["dt"]), "ik", R)
        want = G.bookkeeping(state, tgt, fx["default_dof_pos"], int(fx["explore_step"]), 200, True)
        assert np.array_equal(npy(reset), want["reset"]) and np.array_equal(npy(task.reset_succ), want["reset_succ"]), step
        assert np.array_equal(npy(task.progress_buf), want["progress"]) and np.array_equal(npy(task.success), want["success"]), step
        assert np.array_equal(npy(task.epis_max_step), want["epis_max_step"]), step
        assert same_bits(npy(task.epis_max_rew), want["epis_max_rew"].astype(np.float32)), step
        n_reset += int(want["reset"].sum())
        n_live += int((~want["reset"]).sum())
        w_root, w_dof, w_pa = OD.reset(want["reset"], want["pos_act"], dfm, before["root"], before["dof"], before["pa"], 0, 1,
                                       fx["robot_default_root"], fx["obj_default_root"], fx["default_dof_pos"], fx["joint_lo"], u)
        bound = control_bound(fx, np.arange(N), before["rds"][:, :, 0], want["pos_act"])
        err = np.abs(npy(task.pos_act).astype(np.float64) - want["pos_act"]).max(axis=1)
        record_margin(f"mobile_franka steps {step}: pos_act |hip - fp64| / bound", float((err / bound).max()), 1.0)
        assert (err <= bound).all(), (step, float((err / bound).max()))
        assert same_bits(npy(pa_all)[dfm[:, :ND]], npy(task.pos_act))
        assert np.abs(npy(root).astype(np.float64) - w_root).max() <= 8 * EPS, step
        assert np.array_equal(npy(dof_all), w_dof.astype(np.float32)), step
        # the trivial simulator
        m = t(dfm[:, :ND].astype(np.int64))
        dof_all[m, 0] = pa_all[m]
        task.end_step(rb_all, dof_all, root)
        assert np.array_equal(npy(task.progress_buf), want["progress"] + 1), step
        ref = OD.post(fx["rigid_body_all"], npy(dof_all), npy(root), fx["rigid_body_mask"], dfm, 1, int(fx["ltip"]), int(fx["rtip"]),
                      fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"], fx["dof_lo"], fx["dof_hi"],
                      fx["obj_id"], flags, fx["part_slot"], fx["part_C"])
        flags = ref["succ_objid"]
        got = post_outputs(task)
        P = max(1.0, float(np.abs(ref["part_bbox"]).max()), float(np.abs(ref["normal_state"][:, :3]).max()))
        shortest = float(ref["normal_state"][:, 25:28].min())
        for k, mult in (("normal_state", 1), ("part_bbox", 1), ("extras", 20), ("rew", 20)):
            bound = 64 * EPS * P / shortest * mult
            err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
            record_margin(f"mobile_franka steps {step}: {k} |hip - fp64| / bound", err / bound, 1.0)
            assert err <= bound, (step, k, err, bound)
        assert np.array_equal(got["success"], ref["success"]) and np.array_equal(got["is_reached"], ref["is_reached"]), step
        assert np.array_equal(npy(task.succ_objid_lst), flags), step
    assert n_reset > 0 and n_live > 0


# ------------------------------------------------------------------------------------------- 5. the cube task
@pytest.mark.parametrize("drive", ["ik", "pos"])
def test_grasp_cube_with_a_mobile_robot(drive):
    """GraspCubeTensors around the 70 fixture's robots: their 17 bodies and, as the cube, each environment's target link.  Joint
    targets within control_bound of the float64 restatement; part poses those of mesh_bodies + [17]: positions are copies, rotations
    quat_to_mat C in fewer than 16 operations on numbers <= 1 (16 eps)."""
    from partmanip_amd.tasks import GraspCubeTensors
    fx = load("mobile_franka_ref_70")
    N = 70
    rb = fx["rigid_body_all"][fx["rigid_body_mask"][:, :NRB + 1]]
    dof = fx["dof_state_all"][fx["dof_state_mask"][:, :ND]]
    act = fx["actions" if drive == "ik" else "actions_pos"]
    robot = make_robot(fx, N, drive)
    task = GraspCubeTensors(N, DEV, {"explore_step": 40}, float(fx["dt"]), num_bodies=NRB + 1, robot=robot)
    assert task.part_body.tolist() == MESH + [NRB] and task.num_actions == act.shape[1] and task.num_obs["normal_state"] == 19 + 2 * ND
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    task.end_step(t(rb), t(dof), t(fx["root"]))
    task.epis_max_rew.copy_(t(fx["before_epis_max_rew"]))
    task.epis_max_step.copy_(t(fx["before_epis_max_step"]))
    rot, pos = task.compute_scene_pose()
    assert same_bits(npy(pos), rb[:, MESH + [NRB], :3])
    C = np.concatenate([fx["part_C"][:11], np.eye(3, dtype=np.float32)[None]]).astype(np.float64)
    want_R = np.einsum("bpij,pjk->bpik", G.quat_to_mat(rb[:, MESH + [NRB], 3:7].astype(np.float64)), C)
    assert np.abs(npy(rot).astype(np.float64) - want_R).max() <= 16 * EPS
    state = dict(rew=npy(task.rew_buf), success=npy(task.success), progress=npy(task.progress_buf), epis_max_rew=npy(task.epis_max_rew),
                 epis_max_step=npy(task.epis_max_step))
    pos_act, reset = task.begin_step(t(act), t(dof), t(fx["jac"]))
    tgt = MF.control(act, dof, fx["jac"], int(fx["ltip"]) - 1, int(fx["rtip"]) - 1, fx["dof_lo"], fx["dof_hi"], float(fx["dt"]), drive,
                     MF.base_matrix(fx["robot_default_root"]))
    want = G.bookkeeping(state, tgt, fx["default_dof_pos"], 40, 200, True)
    assert np.array_equal(npy(reset), want["reset"]) and 0 < want["reset"].sum() < N
    assert np.array_equal(npy(task.progress_buf), want["progress"]) and np.array_equal(npy(task.epis_max_step), want["epis_max_step"])
    bound = control_bound(fx, np.arange(N), dof[:, :, 0], want["pos_act"])
    err = np.abs(npy(pos_act).astype(np.float64) - want["pos_act"]).max(axis=1)
    record_margin(f"mobile_franka grasp_cube {drive}: pos_act |hip - fp64| / bound", float((err / bound).max()), 1.0)
    assert (err <= bound).all(), float((err / bound).max())
    # the same launch as under OpenDrawerTensors: the environments that go on there and here get the same target bits
    pre, _ = run_pre(fx, drive=drive)
    both = ~want["reset"] & ~pre["reset"]
    assert both.sum() >= 8 and same_bits(npy(pos_act)[both], pre["pos_act"][both])
