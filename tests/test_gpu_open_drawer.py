"""The open_drawer task step on the GPU: partmanip_amd.tasks.OpenDrawerTensors (pm_open_drawer_post_f32, pm_open_drawer_reset_f32 and
pm_franka_control_f32; csrc/task_open_drawer.hip) against the REFERENCE's own task code (fixtures of
tests/golden/make_open_drawer_golden.py) and against the numpy restatement of the contract (tests/open_drawer_ref.py).

Tolerance of the parity tests (the rule of tests/test_gpu_grasp_cube.py): e_ref = max |out32 - out64| of a fixture's output group is
what the reference's own float32 run loses against its float64 run; the kernel must stay within 4 e_ref of out64.  Flags and integers
must be equal; a group with e_ref = 0 (rows that are copies of constants) must be equal.  Where a test compares states the fixtures do
not cover against the float64 restatement, the bound is stated at the comparison.
Observed 2026-10-18 on 1x MI355X: every group within 1.01 e_ref (profiles/open_drawer_margins.json)."""
import functools

import numpy as np
import pytest
import torch

from tests import grasp_cube_ref as G
from tests import open_drawer_ref as OD
from tests import helpers
from tests.helpers import load, npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
within = functools.partial(helpers.within, prefix="open_drawer ")
SENTINEL = -777.25
EPS = float(np.finfo(np.float32).eps)
GROUPS = ("normal_state", "part_bbox", "rew", "pose_R", "pose_T")
RUNS = (("ik_train", "ik", "train", False), ("ik_test_rand", "ik", "test", True), ("pos_train_rand", "pos", "train", True),
        ("pos_test", "pos", "test", False))
FIXTURES = ["open_drawer_ref_small", "open_drawer_ref_70"]


def make_task(fx, idx=None, drive="ik", random_reset=False, masks=None):
    """A task over the environments idx (any order; default all) of a fixture; the flat state tensors are shared."""
    from partmanip_amd.tasks import OpenDrawerTensors
    idx = np.arange(fx["root"].shape[0]) if idx is None else np.asarray(idx)
    rbm, dfm = masks if masks is not None else (fx["rigid_body_mask"], fx["dof_state_mask"])
    cfg = {"robot": {"driveMode": drive, "dof": fx["default_dof_pos"].tolist(), "root": fx["robot_default_root"].tolist()},
           "explore_step": int(fx["explore_step"]), "maxEpisodeLength": 200, "random_reset": random_reset}
    task = OpenDrawerTensors(len(idx), DEV, cfg, float(fx["dt"]), rbm[idx], dfm[idx], fx["obj_id"][idx], fx["part_bbox_init"][idx],
                             fx["part_axis_dir_init"][idx], fx["joint_lo"][idx], fx["joint_hi"][idx], int(fx["num_objs"]),
                             num_rigid_bodies=fx["rigid_body_all"].shape[0], num_dof_states=fx["dof_state_all"].shape[0],
                             obj_default_root=fx["obj_default_root"])
    task.succ_objid_lst.copy_(t(fx["before_succ_objid"]))
    return task


def post_outputs(task):
    return dict(normal_state=npy(task.obs_buf["normal_state"]), part_bbox=npy(task.part_bbox), rew=npy(task.rew_buf), extras=npy(task._extras),
                success=npy(task.success), is_reached=npy(task.is_reached), pose_R=npy(task.pose_R), pose_T=npy(task.pose_T),
                robot_dof_state=npy(task.robot_dof_state), part_dof_state=npy(task.part_dof_state))


def run_post(fx, idx=None, rb=None, dof=None, root=None, bbox=None, masks=None):
    idx = np.arange(fx["root"].shape[0]) if idx is None else np.asarray(idx)
    task = make_task(fx, idx, masks=masks)
    if bbox is not None:
        task.part_bbox_init.copy_(t(bbox[idx]))
    task.end_step(t(fx["rigid_body_all"] if rb is None else rb), t(fx["dof_state_all"] if dof is None else dof),
                  t((fx["root"] if root is None else root)[idx]))
    return post_outputs(task), task


# ------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity_after_physics(name):
    fx = load(name)
    task = make_task(fx)
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    obs, rew, _, extras = task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))
    rot, pos = task.compute_scene_pose()
    got = dict(normal_state=npy(obs["normal_state"]), part_bbox=npy(task.part_bbox), rew=npy(rew), pose_R=npy(rot), pose_T=npy(pos))
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
    assert same_bits(npy(task.robot_dof_state), fx["dof_state_all"][fx["dof_state_mask"][:, :9]])
    assert same_bits(npy(task.part_dof_state), fx["dof_state_all"][fx["dof_state_mask"][:, 9]])
    assert np.array_equal(npy(task.progress_buf), fx["before_progress"])
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))       # sticky: a second step clears nothing
    assert np.array_equal(npy(task.succ_objid_lst), fx["out64_succ_objid"])


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity_before_physics(name):
    fx = load(name)
    N, D = fx["root"].shape[0], fx["dof_state_all"].shape[0]
    dfm = fx["dof_state_mask"]
    for run, drive, mode, rnd in RUNS:
        task = make_task(fx, drive=drive, random_reset=rnd)
        task.train_test_flag = mode
        if mode == "test":
            task.max_episode_length = int(fx["max_episode_length_test"])
        task.progress_buf.copy_(t(fx["before_progress"] - 1))
        task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))
        task.epis_max_rew.copy_(t(fx["before_epis_max_rew"]))
        task.epis_max_step.copy_(t(fx["before_epis_max_step"]))
        rew = task.rew_buf.clone()
        dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"]), t(fx["pos_act_all_before"])
        out_pa, reset = task.begin_step(t(fx["actions" if drive == "ik" else "actions_pos"]), t(fx["jac"]), dof_all, root, pa_all,
                                        u=t(fx["u"]))
        assert out_pa is pa_all
        o = lambda k, p=64: fx[f"out{p}_{run}_{k}"]             # noqa: E731
        for k, got in (("pos_act_all", pa_all), ("root", root), ("dof_state_all", dof_all)):
            within(f"{name} {run}", k, npy(got), o(k, 32), o(k))
        rs = o("reset")
        assert np.array_equal(npy(reset), rs) and np.array_equal(npy(task.progress_buf), o("after_progress")), run
        assert np.array_equal(npy(task.success), o("after_success")) and np.array_equal(npy(task.epis_max_step), o("after_epis_max_step"))
        emr = torch.where(reset, torch.full_like(rew, -100.0),
                          torch.maximum(rew, t(fx["before_epis_max_rew"])) if mode == "train" else t(fx["before_epis_max_rew"]))
        assert same_bits(npy(task.epis_max_rew), npy(emr))
        # what the reference leaves alone holds its value bit for bit: rows of environments that go on, a cabinet's other joints,
        # the target entries of everything that is not a robot DOF
        keep_dof = np.ones(D, dtype=bool)
        keep_dof[dfm[rs].reshape(-1)] = False
        assert keep_dof.sum() > 0 and same_bits(npy(dof_all)[keep_dof], fx["dof_state_all"][keep_dof]), run
        assert same_bits(npy(root)[~rs], fx["root"][~rs]), run
        keep_pa = np.ones(D, dtype=bool)
        keep_pa[dfm[:, :9].reshape(-1)] = False
        assert keep_pa.sum() >= N and same_bits(npy(pa_all)[keep_pa], fx["pos_act_all_before"][keep_pa]), run
        # the compact tensors carry the rewritten rows
        assert same_bits(npy(task.robot_dof_state), npy(dof_all)[dfm[:, :9]]) and same_bits(npy(task.part_dof_state), npy(dof_all)[dfm[:, 9]])
        assert same_bits(npy(pa_all)[dfm[:, :9]], npy(task.pos_act))
        slot = task._counters[2 * task._slot:2 * task._slot + 2].cpu().numpy()
        assert int(slot[0]) == int(fx["out64_success"].sum()) and int(slot[1]) == int(rs.sum())
        if mode == "train":
            assert np.array_equal(npy(task.reset_succ), o("reset_succ"))
            assert np.array_equal(npy(task.extras["succ_rate"]), o("succ_rate").reshape(1))
        if not rnd:                                           # without random_reset a given u changes nothing
            assert same_bits(npy(root)[rs][:, 1, :7], np.broadcast_to(fx["obj_default_root"], (int(rs.sum()), 7)))


def test_begin_step_draws_its_own_u_inside_the_reset_ranges():
    fx = load("open_drawer_ref_70")
    task = make_task(fx, random_reset=True)
    task.train_test_flag, task.max_episode_length = "test", 0                       # every environment starts over
    task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]))
    dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"]), t(fx["pos_act_all_before"])
    _, reset = task.begin_step(t(fx["actions"]), t(fx["jac"]), dof_all, root, pa_all)
    assert bool(reset.all())
    obj = npy(root)[:, 1].astype(np.float64)
    d = obj[:, :3] - fx["obj_default_root"][:3]
    assert np.abs(d).max() <= 0.05 + 1e-6 and d.min() < -0.01 and d.max() > 0.01 and len(np.unique(d)) > 100
    ang = np.arctan2(-obj[:, 6], obj[:, 5])                     # (0, 0, 1, 0) x (0, 0, sin a, cos a) = (0, 0, cos a, -sin a)
    assert np.abs(ang).max() <= np.pi / 12 + 1e-5 and ang.min() < -0.05 and ang.max() > 0.05
    np.testing.assert_allclose(np.linalg.norm(obj[:, 3:7], axis=1), 1, rtol=0, atol=4 * EPS)
    assert (obj[:, 7:] == 0).all() and (obj[:, 3:5] == 0).all()


# ------------------------------------------------------------------------------------------- 2. independence
def test_every_environment_alone_in_the_batch_and_in_a_permuted_batch_gives_the_same_bits():
    fx = load("open_drawer_ref_70")
    N = 70
    full, _ = run_post(fx)
    perm = np.random.RandomState(3).permutation(N)
    shuffled, ptask = run_post(fx, perm)
    for k, v in shuffled.items():
        assert same_bits(v, full[k][perm]), k
    assert np.array_equal(npy(ptask.succ_objid_lst), fx["out64_succ_objid"])
    for e in list(range(0, N, 7)) + [68, 69]:
        one, _ = run_post(fx, [e])
        for k, v in one.items():
            assert same_bits(v, full[k][e:e + 1]), (k, e)
    small = load("open_drawer_ref_small")
    sfull, _ = run_post(small)
    for e in range(5):
        one, _ = run_post(small, [e])
        for k, v in one.items():
            assert same_bits(v, sfull[k][e:e + 1]), (k, e)
    # before physics: the permuted batch rewrites the flat tensors to the same bits
    res = []
    for idx in (np.arange(N), perm):
        task = make_task(fx, idx, random_reset=True)
        task.progress_buf.copy_(t(fx["before_progress"][idx] - 1))
        task.end_step(t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"][idx]))
        task.epis_max_rew.copy_(t(fx["before_epis_max_rew"][idx]))
        task.epis_max_step.copy_(t(fx["before_epis_max_step"][idx]))
        dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"][idx]), t(fx["pos_act_all_before"])
        task.begin_step(t(fx["actions"][idx]), t(fx["jac"][idx]), dof_all, root, pa_all, u=t(fx["u"][idx]))
        inv = np.argsort(idx)
        res.append((npy(dof_all), npy(pa_all), npy(root)[inv], npy(task.reset_buf)[inv], npy(task.pos_act)[inv]))
    assert 0 < res[0][3].sum() < N
    for a, b in zip(*res):
        assert same_bits(a, b)


def test_a_nan_stays_inside_its_environment():
    fx = load("open_drawer_ref_70")
    N, victim = 70, 33
    clean, _ = run_post(fx)
    others = np.arange(N) != victim
    bbox = fx["part_bbox_init"].copy()
    bbox[victim, 3, 1] = np.nan                               # one coordinate of one handle corner
    rb = fx["rigid_body_all"].copy()
    rb[fx["rigid_body_mask"][victim, int(fx["ltip"])], 4] = np.nan                   # one quaternion entry of a tip row
    for kw, nan_keys in ((dict(bbox=bbox), ("rew", "part_bbox")), (dict(rb=rb), ("rew",))):
        got, task = run_post(fx, **kw)
        for k in clean:
            assert same_bits(got[k][others], clean[k][others]), k
        for k in nan_keys:
            assert np.isnan(got[k][victim]).any(), k
        assert not got["success"][victim] and not np.isnan(got["rew"][others]).any()
        assert np.array_equal(npy(task.succ_objid_lst), fx["out64_succ_objid"])


def test_eight_environments_per_block_set_by_the_lds_cap_give_the_bits_of_four():
    """helpers.lds_cap_check: at M = 60 an environment costs 4096 B (nrb = 13, nd = 9), so 8 per block are what the 48 KB hold; no other
    test here reaches a block size that the cap forces."""
    fx = load("open_drawer_ref_70")
    helpers.lds_cap_check(fx, make_task(fx), 13)


def test_a_part_slot_outside_the_gathered_rows_gives_nan_rows_and_touches_nothing_else():
    """part_slot entries -1 and nrb + 2 between valid ones: those parts' pose rows are NaN in every environment (the kernel never forms
    their address), every other row and every other output has the bits of the run without them."""
    fx = load("open_drawer_ref_small")
    task = make_task(fx)
    nrb = task.robot.num_rigid_body
    eye = torch.eye(3, device=DEV)[None]
    good = helpers.open_drawer_post_op(fx, task, 1, task.part_slot, task.part_C)
    bad_at, slot = (3, 8), task.part_slot.tolist()
    keep = [k for k in range(15) if k not in bad_at]
    slot.insert(3, -1), slot.insert(8, nrb + 2)
    part_C = torch.cat([task.part_C[:3], eye, task.part_C[3:7], eye, task.part_C[7:]]).contiguous()
    got = helpers.open_drawer_post_op(fx, task, 1, torch.tensor(slot, dtype=torch.int32, device=DEV), part_C)
    assert [slot[k] for k in keep] == task.part_slot.tolist() and not np.isnan(good["pose_R"]).any()
    for k, v in good.items():
        if k in ("pose_R", "pose_T"):
            assert np.isnan(got[k][:, bad_at]).all(), k
            assert same_bits(got[k][:, keep], v), k
        else:
            assert same_bits(got[k], v), k


# ------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("off", [1, 2, 3])
def test_column_views_leave_everything_else_alone(off):
    from partmanip_amd import ops
    fx = load("open_drawer_ref_70")
    N = 70
    full, task = run_post(fx)
    r = task.robot
    width = 3 + 47 + 2 + 8 + 3                                # odd: the rows' alignment walks through all four residues
    buf = torch.full((N * width + 8,), SENTINEL, device=DEV)
    view = buf[off:off + N * width].view(N, width)
    ns, ex = view[:, 3:50], view[:, 52:60]
    args = (t(fx["rigid_body_all"]), t(fx["dof_state_all"]), t(fx["root"]), task.rigid_body_mask, task.dof_state_mask, 1, r.ltip_rb_index,
            r.rtip_rb_index, task.part_bbox_init, task.part_axis_dir_init, task.part_joint_lower_limits, task.part_joint_upper_limits,
            r.dof_lower_limits_tensor, r.dof_upper_limits_tensor)
    ops.open_drawer_post(*args, normal_state=ns, extras=ex)
    assert same_bits(npy(ns), full["normal_state"]) and same_bits(npy(ex), full["extras"])
    mask = torch.ones(N, width, dtype=torch.bool, device=DEV)
    mask[:, 3:50] = mask[:, 52:60] = False
    assert bool((view[mask] == SENTINEL).all()) and bool((buf[:off] == SENTINEL).all()) and bool((buf[off + N * width:] == SENTINEL).all())
    # null outputs are skipped: an output alone gives the bits of the full call
    rew = torch.full((N,), SENTINEL, device=DEV)
    ops.open_drawer_post(*args, rew=rew)
    assert same_bits(npy(rew), full["rew"])
    pose_T = torch.full((N, 13, 3), SENTINEL, device=DEV)
    flags = torch.zeros(3, dtype=torch.bool, device=DEV)
    ops.open_drawer_post(*args, part_slot=task.part_slot, part_C=task.part_C, pose_T=pose_T, obj_id=task.obj_id, succ_objid=flags)
    assert same_bits(npy(pose_T), full["pose_T"])
    assert np.array_equal(npy(flags), np.bincount(fx["obj_id"][fx["out64_success"]], minlength=3) > 0)
    bb = torch.full((N, 8, 3), SENTINEL, device=DEV)
    ops.open_drawer_post(*args, part_bbox=bb)
    assert same_bits(npy(bb), full["part_bbox"])
    ops.open_drawer_post(*args)                               # nothing asked for: nothing written, no error


def test_masks_whose_robot_rows_are_scattered_give_the_same_bits():
    fx = load("open_drawer_ref_70")
    B, D = fx["rigid_body_all"].shape[0], fx["dof_state_all"].shape[0]
    rng = np.random.RandomState(5)
    pb, pd = rng.permutation(B), rng.permutation(D)            # row r moves to pb[r]
    rb, dof = np.empty_like(fx["rigid_body_all"]), np.empty_like(fx["dof_state_all"])
    rb[pb], dof[pd] = fx["rigid_body_all"], fx["dof_state_all"]
    masks = (pb[fx["rigid_body_mask"]].astype(np.int32), pd[fx["dof_state_mask"]].astype(np.int32))
    assert (np.diff(masks[0][:, :13], axis=1) != 1).any()
    full, _ = run_post(fx)
    got, _ = run_post(fx, rb=rb, dof=dof, masks=masks)
    for k, v in got.items():
        assert same_bits(v, full[k]), k
    # and the reset writes through them: the scattered tensors end as the permuted contiguous ones
    res = []
    for masks_, dof0, pa0 in ((None, fx["dof_state_all"], fx["pos_act_all_before"]), (masks, dof, None)):
        task = make_task(fx, random_reset=True, masks=masks_)
        task.train_test_flag, task.max_episode_length = "test", int(fx["max_episode_length_test"])
        task.progress_buf.copy_(t(fx["before_progress"] - 1))
        task.end_step(t(fx["rigid_body_all"] if masks_ is None else rb), t(dof0), t(fx["root"]))
        pa = fx["pos_act_all_before"].copy()
        if masks_ is not None:
            pa[pd] = fx["pos_act_all_before"]
        dof_all, root, pa_all = t(dof0), t(fx["root"]), t(pa)
        task.begin_step(t(fx["actions"]), t(fx["jac"]), dof_all, root, pa_all, u=t(fx["u"]))
        res.append((npy(dof_all), npy(pa_all), npy(root)))
    assert same_bits(res[1][0][pd], res[0][0]) and same_bits(res[1][1][pd], res[0][1]) and same_bits(res[1][2], res[0][2])


# ------------------------------------------------------------------------------------------- 4. several steps in a row
def test_reset_starts_every_environment_over():
    fx = load("open_drawer_ref_small")
    task = make_task(fx)
    task.progress_buf.fill_(7)
    dof_all, root, pa_all = t(fx["dof_state_all"]), t(fx["root"]), t(fx["pos_act_all_before"])
    task.reset(dof_all, root, pa_all)
    ones = np.ones(5, dtype=bool)
    pos_act = np.broadcast_to(fx["default_dof_pos"], (5, 9))
    w_root, w_dof, w_pa = OD.reset(ones, pos_act, fx["dof_state_mask"], fx["root"], fx["dof_state_all"], fx["pos_act_all_before"], 0, 1,
                                   fx["robot_default_root"], fx["obj_default_root"], fx["default_dof_pos"], fx["joint_lo"], dtype=np.float32)
    assert same_bits(npy(root), w_root) and same_bits(npy(dof_all), w_dof) and same_bits(npy(pa_all), w_pa)
    assert int(task.progress_buf.abs().sum()) == 0 and not bool(task.reset_buf.any()) and float(task.epis_max_rew.max()) == -100.0


def test_three_steps_in_a_row_follow_the_restated_task():
    """Three begin_step / end_step rounds around a trivial simulator (DOF position <- its target).  Each round is compared with the
    float64 restatement evaluated on the state the round started from, so rounding does not accumulate.  Bounds: a value of the post
    step is a chain of fewer than 64 float32 operations on numbers of magnitude <= P = max(1, |position|), and the handle's unit
    vectors divide differences of such numbers by the shortest handle edge l: |error| <= 64 eps P / l for the observation row and
    the box; the reward multiplies the unit vectors' error by at most 5 + (1 + |base|) <= 20 -> 20 times that.  Joint targets: the
    bound of tests/test_gpu_grasp_cube.py (a backward-stable 6 x 6 Cholesky solve, 64 eps cond |u|, plus 8 eps |target|).  The rewritten
    root rows are sums and products of at most 8 operations on numbers <= 1: 8 eps.  Rewritten DOF rows are constants: equal."""
    fx = load("open_drawer_ref_small")
    N, nd = 5, 9
    dfm = fx["dof_state_mask"]
    task = make_task(fx, random_reset=True)
    rng = np.random.RandomState(12)
    rb_all, dof_all, root, pa_all = (t(fx[k]) for k in ("rigid_body_all", "dof_state_all", "root", "pos_act_all_before"))
    task.progress_buf.copy_(t(fx["before_progress"] - 1))
    task.end_step(rb_all, dof_all, root)
    task.epis_max_rew.copy_(t(fx["before_epis_max_rew"]))
    task.epis_max_step.copy_(t(fx["before_epis_max_step"]))
    jl, jr = int(fx["ltip"]) - 1, int(fx["rtip"]) - 1
    flags = fx["out64_succ_objid"].copy()
    n_reset = 0
    for step in range(3):
        state = dict(rew=npy(task.rew_buf), success=npy(task.success), progress=npy(task.progress_buf),
                     epis_max_rew=npy(task.epis_max_rew), epis_max_step=npy(task.epis_max_step))
        before = dict(root=npy(root), dof=npy(dof_all), pa=npy(pa_all), rds=npy(task.robot_dof_state))
        act = rng.uniform(-1, 1, size=(N, 7)).astype(np.float32)
        u = rng.uniform(0, 1, size=(N, 4)).astype(np.float32)
        _, reset = task.begin_step(t(act), t(fx["jac"]), dof_all, root, pa_all, u=t(u))
        tgt = G.control(act, before["rds"], fx["jac"], jl, jr, fx["dof_lo"], fx["dof_hi"], float(fx["dt"]), "ik")
        want = G.bookkeeping(state, tgt, fx["default_dof_pos"], int(fx["explore_step"]), 200, True)
        assert np.array_equal(npy(reset), want["reset"]) and np.array_equal(npy(task.reset_succ), want["reset_succ"]), step
        assert np.array_equal(npy(task.progress_buf), want["progress"]) and np.array_equal(npy(task.success), want["success"]), step
        assert np.array_equal(npy(task.epis_max_step), want["epis_max_step"]), step
        assert same_bits(npy(task.epis_max_rew), want["epis_max_rew"].astype(np.float32)), step
        n_reset += int(want["reset"].sum())
        w_root, w_dof, w_pa = OD.reset(want["reset"], want["pos_act"], dfm, before["root"], before["dof"], before["pa"], 0, 1,
                                       fx["robot_default_root"], fx["obj_default_root"], fx["default_dof_pos"], fx["joint_lo"], u)
        J = (fx["jac"][:, jl, :, :nd - 2].astype(np.float64) + fx["jac"][:, jr, :, :nd - 2]) / 2
        cond = np.linalg.cond(J @ J.transpose(0, 2, 1) + 0.0025 * np.eye(6))
        move = np.abs(want["pos_act"] - before["rds"][:, :, 0]).max(axis=1)
        bound = 64 * EPS * cond * np.maximum(move, 1e-3) + 8 * EPS * np.abs(want["pos_act"]).max()
        err = np.abs(npy(task.pos_act).astype(np.float64) - want["pos_act"]).max(axis=1)
        record_margin(f"open_drawer steps {step}: pos_act |hip - fp64| / bound", float((err / bound).max()), 1.0)
        assert (err <= bound).all(), (step, float((err / bound).max()))
        assert same_bits(npy(pa_all)[dfm[:, :nd]], npy(task.pos_act))
        assert np.abs(npy(root).astype(np.float64) - w_root).max() <= 8 * EPS, step
        assert np.array_equal(npy(dof_all), w_dof.astype(np.float32)), step
        # the trivial simulator
        m = t(dfm[:, :nd].astype(np.int64))
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
            record_margin(f"open_drawer steps {step}: {k} |hip - fp64| / bound", err / bound, 1.0)
            assert err <= bound, (step, k, err, bound)
        assert np.array_equal(got["success"], ref["success"]) and np.array_equal(got["is_reached"], ref["is_reached"]), step
        assert np.array_equal(npy(task.succ_objid_lst), flags), step
    assert n_reset > 0
