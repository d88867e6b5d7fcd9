"""The kinematic articulation on the GPU: pm_articulation_step_f32 (csrc/articulation.hip) through ops.articulation_step,
kinematics.Articulation and kinematics.KinematicSim, against the tests' own float64 evaluation of the contract
(tests/kinematics_ref.py: homogeneous matrices and Rodrigues' formula, no quaternion products, no ancestor masks).

Tolerance.  Per quantity, e_ref = the worst error of the reference's own float32 run against its float64 run on the same inputs is
what the formulas lose in float32; the kernel must stay within 4 e_ref of the float64 run (the project's convention).  The kernel walks
the chain of frames in float64 and forms the Jacobian and the velocities in float32 from the rounded frames.  For the quaternion norm the quantity is | |q| - 1 |, the reference's being
that of the quaternion read off its float32 rotation matrix.  Every observed / allowed pair is recorded (tests/helpers.record_margin;
tools/margins_summary.py folds them into profiles/kinematics_margins.json).  Everything else is an equality: zeros outside the
ancestor mask, bit-identity between runs and batch sizes, sentinels, error codes."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import grasp_cube_ref as G
from tests import helpers
from tests import kinematics_ref as K
from tests import mobile_franka_ref as MF
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
URDF = dict(fixed=os.path.join(GOLDEN, "franka_panda_sdf.urdf"), mobile=os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf"))
SENTINEL = -777.25
DT = 1.0 / 60.0
BRANCHY = """<robot name="branchy">
  <link name="root"/><link name="a"/><link name="a1"/><link name="a2"/><link name="b"/><link name="b1"/><link name="c"/>
  <joint name="ra" type="revolute"><parent link="root"/><child link="a"/><origin xyz="0.1 0.2 0.3" rpy="0.4 -0.5 0.6"/>
    <axis xyz="1 1 0"/><limit lower="-2" upper="2" velocity="1"/></joint>
  <joint name="aa1" type="prismatic"><parent link="a"/><child link="a1"/><origin xyz="0 0.3 0" rpy="1.2 0 0"/><axis xyz="0 1 2"/>
    <limit lower="-0.3" upper="0.3" velocity="1"/></joint>
  <joint name="a1a2" type="fixed"><parent link="a1"/><child link="a2"/><origin xyz="0.2 0 0.1" rpy="0 0.7 0"/></joint>
  <joint name="rb" type="continuous"><parent link="root"/><child link="b"/><origin xyz="-0.2 0 0" rpy="0 0 -1.1"/><axis xyz="0 0 -1"/></joint>
  <joint name="bb1" type="revolute"><parent link="b"/><child link="b1"/><origin xyz="0 0 0.4" rpy="-0.3 0.2 0.1"/><axis xyz="1 0 0"/>
    <limit lower="-1" upper="1" velocity="1"/></joint>
  <joint name="ac" type="revolute"><parent link="a"/><child link="c"/><origin xyz="0 -0.1 0.1"/><axis xyz="0 1 0"/>
    <limit lower="-1" upper="1" velocity="1"/></joint>
</robot>"""


@functools.lru_cache(maxsize=None)
def tree_of(name):
    from partmanip_amd.urdf import KinematicTree, load_urdf
    if name == "branchy":
        return load_urdf(BRANCHY)
    if name == "chain64":                                     # the staging limit: 64 bodies, 64 revolute DOFs, the root's joint included
        rng = np.random.default_rng(64)
        ax = rng.normal(size=(64, 3))
        return KinematicTree([f"b{i}" for i in range(64)], [f"j{i}" for i in range(64)], np.arange(64) - 1, np.ones(64, dtype=np.int32),
                             rng.uniform(-0.05, 0.05, (64, 3)), rng.uniform(-1, 1, (64, 3)), ax / np.linalg.norm(ax, axis=1, keepdims=True),
                             [(-1.0, 1.0, 2.0)] * 64, np.zeros(64, dtype=bool))
    return load_urdf(URDF[name])


@functools.lru_cache(maxsize=None)
def case(name, N, seed=5):
    """Seeded inputs (float32 values) and the reference's float64 and float32 runs, computed once and never modified."""
    tree = tree_of(name)
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(tree.lower, -3.0), np.minimum(tree.upper, 3.0)
    q = (lo + rng.uniform(0.02, 0.98, (N, tree.num_dofs)) * (hi - lo)).astype(np.float32)
    qd = rng.normal(size=(N, tree.num_dofs)).astype(np.float32)
    base = np.concatenate([rng.uniform(-0.5, 0.5, (N, 3)), rng.normal(size=(N, 4)) * 1.3], axis=1).astype(np.float32)
    out = dict(q=q, qd=qd, base=base, o64=K.fk(tree, q, qd, base), o32=K.fk(tree, q, qd, base, dtype=np.float32))
    for v in (q, qd, base, *out["o64"].values(), *out["o32"].values()):
        v.setflags(write=False)
    return out


def articulation(name, N):
    from partmanip_amd.kinematics import Articulation
    return Articulation(tree_of(name), N, DEV)


def hold(name, key, err, e_ref):
    print(f"{name} {key}: e_ref = {e_ref:.3e}; observed = {err:.3e}" + (f" = {err / e_ref:.2f} e_ref" if e_ref > 0 else ""))
    if e_ref > 0:
        record_margin(f"kinematics {name}: {key} / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    return err <= 4 * e_ref, (name, key, err, e_ref)


def compare(name, rb, jac, o64, o32):
    """Every quantity of the accuracy rule; all are printed and recorded before the first one is asserted."""
    rb, jac = np.asarray(rb, dtype=np.float64), np.asarray(jac, dtype=np.float64)
    worst = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - b).max())      # noqa: E731
    res = [hold(name, "positions", worst(rb[..., :3], o64["pos"]), worst(o32["pos"], o64["pos"])),
           hold(name, "rotation matrices", worst(K.quat_matrix(rb[..., 3:7], np.float64), o64["R"]), worst(o32["R"], o64["R"])),
           hold(name, "| |q| - 1 |", float(np.abs(np.linalg.norm(rb[..., 3:7], axis=-1) - 1).max()),
                float(np.abs(np.linalg.norm(o32["quat"].astype(np.float64), axis=-1) - 1).max())),
           hold(name, "velocities", worst(rb[..., 7:], o64["vel"]), worst(o32["vel"], o64["vel"])),
           hold(name, "jacobian", worst(jac, o64["jac"]), worst(o32["jac"], o64["jac"]))]
    for ok, what in res:
        assert ok, what


def dof_tensor(c):
    return t(np.stack([c["q"], c["qd"]], axis=-1))


# ------------------------------------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("name", ["fixed", "mobile"])
def test_frankas_match_the_float64_reference(name, N):
    c, tree = case(name, N), tree_of(name)
    dof = dof_tensor(c)
    before = dof.clone()
    rb, jac = articulation(name, N).forward(dof, t(c["base"]))
    assert same_bits(npy(dof), npy(before))                   # pure forward kinematics only reads the joint state
    rb, jac = npy(rb), npy(jac)
    compare(f"{name} N={N}", rb, jac, c["o64"], c["o32"])
    outside = np.array([[(int(tree.anc_mask[b]) >> d) & 1 == 0 for d in range(tree.num_dofs)] for b in range(1, tree.num_bodies)])
    assert outside.any() and np.all(jac.transpose(0, 2, 1, 3)[:, :, outside].view(np.uint32) == 0)       # +0.0, bit for bit
    assert np.all(c["o64"]["jac"].transpose(0, 2, 1, 3)[:, :, outside] == 0)                              # found by walking the parents


@pytest.mark.parametrize("name, N", [("branchy", 9), ("chain64", 5)])
def test_branching_tree_and_the_64_by_64_chain_match_the_reference(name, N):
    c, tree = case(name, N), tree_of(name)
    assert name != "chain64" or (tree.num_bodies, tree.num_dofs) == (64, 64)
    assert name != "branchy" or sorted(set(tree.jtype.tolist())) == [0, 1, 2]
    rb, jac = articulation(name, N).forward(dof_tensor(c), t(c["base"]))
    compare(f"{name} N={N}", npy(rb), npy(jac), c["o64"], c["o32"])


# ------------------------------------------------------------------------------------------- 2. properties
def test_an_environment_alone_equals_itself_inside_a_batch_and_calls_repeat_bit_for_bit():
    c = case("mobile", 70)
    rb, jac = articulation("mobile", 70).forward(dof_tensor(c), t(c["base"]))
    rb2, jac2 = articulation("mobile", 70).forward(dof_tensor(c), t(c["base"]))
    assert same_bits(npy(rb), npy(rb2)) and same_bits(npy(jac), npy(jac2))
    one = dict(q=c["q"][5:6], qd=c["qd"][5:6])
    rb1, jac1 = articulation("mobile", 1).forward(dof_tensor(one), t(c["base"][5:6]))
    assert same_bits(npy(rb)[5:6], npy(rb1)) and same_bits(npy(jac)[5:6], npy(jac1))
    rb1, jac1 = articulation("mobile", 1).forward(dof_tensor(one), t(c["base"][5]))       # one pose for all: stride 0
    assert same_bits(npy(rb)[5:6], npy(rb1)) and same_bits(npy(jac)[5:6], npy(jac1))


@pytest.mark.parametrize("reps, eb", [(59, 8), (118, 16)])
def test_more_environments_per_block_give_the_same_bits(reps, eb):
    """70 environments take 4 per block; 70 x 59 = 4130 take 8 (517 blocks) and 70 x 118 = 8260 take 16 (517 blocks), the last block
    partial in both: the launch rule of task_common.h at 1596 B of LDS per environment (32 would not fit 48 KB).  Same
    environments, same bits."""
    c = case("fixed", 70)
    rb, jac = articulation("fixed", 70).forward(dof_tensor(c), t(c["base"]))
    N = 70 * reps
    assert -(-N // eb) >= 512 > -(-N // (2 * eb)) and N % eb
    big = dict(q=np.tile(c["q"], (reps, 1)), qd=np.tile(c["qd"], (reps, 1)))
    rbN, jacN = articulation("fixed", N).forward(dof_tensor(big), t(np.tile(c["base"], (reps, 1))))
    assert torch.equal(rbN.view(reps, 70, 13, 13).view(torch.int32), rb.view(torch.int32).expand(reps, 70, 13, 13))
    assert torch.equal(jacN.view(reps, 70, 12, 6, 9).view(torch.int32), jac.view(torch.int32).expand(reps, 70, 12, 6, 9))


# ------------------------------------------------------------------------------------------- 3. the drive
def drive_case(N=6, seed=9):
    tree = tree_of("fixed")
    rng = np.random.default_rng(seed)
    lo, hi = tree.lower.astype(np.float32), tree.upper.astype(np.float32)
    q = (lo + rng.uniform(0.1, 0.9, (N, 9)) * (hi - lo)).astype(np.float32)
    qd = rng.normal(size=(N, 9)).astype(np.float32)
    tg = (q + rng.normal(size=(N, 9)) * 0.2 * (hi - lo)).astype(np.float32)          # some beyond the limits, some beyond vmax dt
    return tree, q, qd, tg, lo, hi


def run_drive(q, qd, tg, vmax=None, reset=None, dt=DT):
    art = articulation("fixed", q.shape[0])
    dof = t(np.stack([q, qd], axis=-1))
    rb = torch.full((q.shape[0], 13, 13), SENTINEL, device=DEV)
    jac = torch.full((q.shape[0], 12, 6, 9), SENTINEL, device=DEV)
    art.step(dof, t(np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.float32)), targets=t(tg), reset=None if reset is None else t(reset),
             vmax=None if vmax is None else t(vmax), dt=dt, rigid_body=rb, jacobian=jac)
    return npy(dof), npy(rb), npy(jac)


def test_drive_tracks_exactly_without_vmax_and_clamps_to_the_limits():
    tree, q, qd, tg, lo, hi = drive_case()
    dof, rb, jac = run_drive(q, qd, tg)
    qn, qdn = K.drive(q, tg, lo, hi, None, np.float32(DT), dtype=np.float32)
    assert (tg > hi).any() and (tg < lo).any()
    inside = (tg >= lo) & (tg <= hi)
    assert same_bits(dof[..., 0][inside], tg[inside]) and np.all((dof[..., 0] >= lo) & (dof[..., 0] <= hi))
    assert same_bits(dof[..., 0], qn.astype(np.float32)) and same_bits(dof[..., 1], ((dof[..., 0] - q) / np.float32(DT)).astype(np.float32))
    o64 = K.fk(tree, dof[..., 0], dof[..., 1], [0, 0, 0, 0, 0, 0, 1])
    o32 = K.fk(tree, dof[..., 0], dof[..., 1], [0, 0, 0, 0, 0, 0, 1], dtype=np.float32)
    compare("drive exact", rb, jac, o64, o32)                 # the bodies and velocities are those of the NEW joint state


def test_drive_rate_limit_reset_and_velocity_column():
    tree, q, qd, tg, lo, hi = drive_case()
    vmax = tree.velocity.astype(np.float32)
    reset = np.array([0, 1, 0, 0, 1, 0], dtype=bool)
    dof, rb, jac = run_drive(q, qd, tg, vmax=vmax, reset=reset)
    qn, qdn = K.drive(q, tg, lo, hi, vmax, np.float32(DT), reset=reset, dtype=np.float32)
    step = np.abs(dof[..., 0] - q)
    assert (np.abs(tg - q) > vmax * np.float32(DT)).any() and np.all(step[~reset] <= vmax * np.float32(DT) * (1 + 1e-6) + 1e-7)
    assert same_bits(dof[..., 0], qn.astype(np.float32)) and same_bits(dof[..., 1], qdn.astype(np.float32))
    assert same_bits(dof[~reset][..., 1], ((dof[..., 0] - q) / np.float32(DT)).astype(np.float32)[~reset])
    assert np.all(dof[reset][..., 1] == 0) and same_bits(dof[reset][..., 0], np.clip(tg, lo, hi)[reset])
    assert np.all(rb[reset][..., 7:] == 0) and np.abs(rb[~reset][..., 7:]).max() > 0


def test_nan_target_stays_in_its_environment_and_no_targets_leave_the_state_alone():
    tree, q, qd, tg, lo, hi = drive_case()
    clean = run_drive(q, qd, tg)
    bad = tg.copy()
    bad[2, 3] = np.nan
    dof, rb, jac = run_drive(q, qd, bad)
    keep = np.arange(6) != 2
    assert all(same_bits(a[keep], b[keep]) for a, b in zip((dof, rb, jac), clean))
    assert np.isnan(dof[2, 3]).all() and np.isfinite(np.delete(dof[2], 3, axis=0)).all()
    assert np.isnan(rb[2, 4:, :3]).any() and np.isfinite(rb[2, :4, :7]).all()          # bodies below joint 4 (DOF 3) follow it
    outside = np.array([[(int(tree.anc_mask[b]) >> d) & 1 == 0 for d in range(9)] for b in range(1, 13)])
    assert np.all(jac[2].transpose(1, 0, 2)[:, outside].view(np.uint32) == 0)              # zeros stay zeros beside the NaN
    art = articulation("fixed", 6)
    state = t(np.stack([q, qd], axis=-1))
    before = npy(state).copy()
    art.forward(state, t(np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.float32)))
    assert same_bits(npy(state), before)


# ------------------------------------------------------------------------------------------- 4. layouts
def test_robot_rows_inside_a_wider_tensor_leave_the_other_rows_and_the_tail_alone():
    N = 7
    c = case("fixed", N, seed=6)
    art = articulation("fixed", N)
    dense, jac0 = art.forward(dof_tensor(c), t(c["base"]))
    buf = torch.full((N * 14 * 13 + 64,), SENTINEL, device=DEV)
    wide = buf[:N * 14 * 13].view(N, 14, 13)
    jbuf = torch.full((N * 12 * 6 * 9 + 64,), SENTINEL, device=DEV)
    rb, jac = art.forward(dof_tensor(c), t(c["base"]), rigid_body=wide, jacobian=jbuf[:N * 648].view(N, 12, 6, 9))
    assert same_bits(npy(wide[:, :13]), npy(dense)) and same_bits(npy(jac), npy(jac0))
    assert np.all(npy(wide[:, 13]) == SENTINEL) and np.all(npy(buf[N * 14 * 13:]) == SENTINEL) and np.all(npy(jbuf[N * 648:]) == SENTINEL)


def test_flat_tensors_with_row_tables_give_the_dense_values_and_keep_the_gaps():
    N = 6
    c = case("mobile", N, seed=7)
    art = articulation("mobile", N)
    nb, nd = 16, 12
    dense, jac0 = art.forward(dof_tensor(c), t(c["base"]))
    gaps_rb, gaps_dof = [2, 0, 5, 1, 3, 4], [1, 3, 0, 2, 0, 4]                          # cabinets of different sizes between the robots
    rb_row0 = np.cumsum([2] + [nb + g for g in gaps_rb[:-1]]).astype(np.int32)
    dof_row0 = np.cumsum([1] + [nd + g for g in gaps_dof[:-1]]).astype(np.int32)
    order = np.array([3, 0, 5, 1, 4, 2])                                                 # and the environments not in row order
    rb_row0, dof_row0 = rb_row0[order], dof_row0[order]
    B, D = int(rb_row0.max()) + nb + 3, int(dof_row0.max()) + nd + 2
    flat_rb = torch.full((B, 13), SENTINEL, device=DEV)
    flat_dof = torch.full((D, 2), SENTINEL, device=DEV)
    rows = (t(dof_row0).long()[:, None] + torch.arange(nd, device=DEV)[None]).reshape(-1)
    flat_dof[rows] = dof_tensor(c).reshape(-1, 2)
    dof_before = npy(flat_dof).copy()
    _, jac = art.forward(flat_dof, t(c["base"]), rigid_body=flat_rb, rb_row0=t(rb_row0), dof_row0=t(dof_row0))
    got = npy(flat_rb)
    mine = np.zeros(B, dtype=bool)
    for e in range(N):
        assert same_bits(got[rb_row0[e]:rb_row0[e] + nb], npy(dense)[e]), e
        mine[rb_row0[e]:rb_row0[e] + nb] = True
    assert (~mine).sum() >= 10 and np.all(got[~mine] == SENTINEL) and same_bits(npy(jac), npy(jac0))
    assert same_bits(npy(flat_dof), dof_before)
    # the drive through the tables: the gaps of dof_state stay, the robots' rows take the targets
    tg = np.clip(c["q"] + 0.01, tree_of("mobile").lower.astype(np.float32), tree_of("mobile").upper.astype(np.float32)).astype(np.float32)
    art.step(flat_dof, t(c["base"]), targets=t(tg), dt=DT, rigid_body=flat_rb, rb_row0=t(rb_row0), dof_row0=t(dof_row0))
    after = npy(flat_dof)
    rows = npy(rows)
    untouched = np.ones(D, dtype=bool)
    untouched[rows] = False
    assert np.all(after[untouched] == SENTINEL) and same_bits(after[rows, 0], tg.reshape(-1))


def test_every_invalid_argument_is_refused_before_any_launch():
    from partmanip_amd._lib import lib
    N = 3
    art = articulation("fixed", N)
    c = case("fixed", N)
    dof, base, tg = dof_tensor(c), t(c["base"]), t(c["q"])
    rb = torch.full((N, 13, 13), SENTINEL, device=DEV)
    jac = torch.full((N, 12, 6, 9), SENTINEL, device=DEV)
    p = lambda x: 0 if x is None else x.data_ptr()             # noqa: E731
    good = dict(parent=p(art.parent), jtype=p(art.jtype), dof=p(art.dof), origin_q=p(art.origin_q), origin_t=p(art.origin_t),
                axis=p(art.axis), anc_mask=p(art.anc_mask), dof_lo=p(art.dof_lower), dof_hi=p(art.dof_upper), vmax=0, dt=DT,
                base_pose=p(base), base_stride=7, dof_state=p(dof), dof_rows=N * 9, targets=p(tg), tgt_stride=9, reset=0, rb_row0=0,
                rb_stride=13, rb_rows=N * 13, dof_row0=0, dof_stride=9, N=N, nb=13, nd=9, rigid_body=p(rb), jac=p(jac), stream=0)
    bad = [dict(parent=0), dict(jtype=0), dict(dof=0), dict(origin_q=0), dict(origin_t=0), dict(axis=0), dict(anc_mask=0), dict(dof_lo=0),
           dict(dof_hi=0), dict(base_pose=0), dict(dof_state=0), dict(N=0), dict(nb=0), dict(nb=65), dict(nd=0), dict(nd=65),
           dict(base_stride=6), dict(tgt_stride=8), dict(rb_stride=12), dict(dof_stride=8), dict(dt=0.0), dict(dt=-DT),
           dict(dt=float("nan")), dict(rb_rows=N * 13 - 1), dict(dof_rows=N * 9 - 1)]
    before = npy(dof).copy()
    for change in bad:
        assert lib.pm_articulation_step_f32(*{**good, **change}.values()) == -1, change
    torch.cuda.synchronize()
    assert np.all(npy(rb) == SENTINEL) and np.all(npy(jac) == SENTINEL) and same_bits(npy(dof), before)
    assert lib.pm_articulation_step_f32(*{**good, "dt": 0.0, "targets": 0}.values()) == 0       # dt is not read without targets
    assert lib.pm_articulation_step_f32(*good.values()) == 0
    torch.cuda.synchronize()
    assert np.isfinite(npy(rb)).all() and same_bits(npy(dof)[..., 0], c["q"])


# ------------------------------------------------------------------------------------------- 5. the closed loop
def loop_reference(tree, robot, q0, act, steps, dtype):
    """begin_step's drive -> the articulation -> again, in the reference: (q, fk of the last state, fk of the first)."""
    lo, hi = npy(robot.dof_lower_limits_tensor).astype(dtype), npy(robot.dof_upper_limits_tensor).astype(dtype)
    q = np.broadcast_to(np.asarray(q0, dtype=dtype), (act.shape[0], tree.num_dofs)).copy()
    qd = np.zeros_like(q)
    base = [0, 0, 0, 0, 0, 0, 1]
    jl, jr = robot.ltip_rb_index - 1, robot.rtip_rb_index - 1
    first = out = K.fk(tree, q, qd, base, dtype=dtype)
    for _ in range(steps):
        state = np.stack([q, qd], axis=-1)
        if robot.mobile:
            tg = MF.control(act, state, out["jac"], jl, jr, lo, hi, DT, "ik", np.eye(3), dtype=dtype)
        else:
            tg = G.control(act, state, out["jac"], jl, jr, lo, hi, DT, "ik", dtype=dtype)
        q, qd = K.drive(q, tg, lo, hi, None, dtype(DT), dtype=dtype)
        out = K.fk(tree, q, qd, base, dtype=dtype)
    return q, out, first


def tip_mid(pos, robot):
    return (pos[:, robot.ltip_rb_index] + pos[:, robot.rtip_rb_index]) / 2


@pytest.mark.parametrize("name, axis", [("fixed", 0), ("fixed", 2), ("mobile", 0)])
def test_closed_loop_moves_the_tip_where_the_action_says(name, axis):
    from partmanip_amd.kinematics import KinematicSim
    from partmanip_amd.tasks import Franka, GraspCubeTensors, MobileFranka
    N, steps = 4, 20
    tree = tree_of(name)
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:      # the default pose of the reference's task cfg
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)[name]}, "explore_step": 40, "maxEpisodeLength": 200}
    robot = (MobileFranka if name == "mobile" else Franka)(cfg["robot"], DT, N, DEV, **tree.robot_kwargs())
    nb = tree.num_bodies
    task = GraspCubeTensors(N, DEV, cfg, DT, num_bodies=nb + 1, robot=robot)
    sim = KinematicSim(tree, N, DEV, DT, base_pose=(0, 0, 0, 0, 0, 0, 1), num_bodies=nb + 1, num_actors=2)
    cube = torch.tensor([0.6, 0.5, 0.025], device=DEV)        # out of reach: the cube is the caller's, and nothing here moves it
    sim.rigid_body[:, nb, :3] = cube
    sim.root[:, 1, :3] = cube
    act = np.zeros((N, robot.num_actions), dtype=np.float32)
    act[:, robot.num_base_dofs + axis] = 1.0                  # 0.005 per step along the axis; a zero base action
    actions = t(act)
    rb, dof, jac = sim.set_dof_state(robot.default_dof_pos)
    start = npy(rb).copy()
    for _ in range(steps):
        pos_act, reset = task.begin_step(actions, dof, jac)
        assert not bool(reset.any())
        rb, dof, jac = sim.step(pos_act, reset)
        task.end_step(rb, dof, sim.root)
    got = npy(rb)
    q0 = npy(robot.default_dof_pos)
    _, o64, first = loop_reference(tree, robot, q0, act, steps, np.float64)
    _, o32, _ = loop_reference(tree, robot, q0, act, steps, np.float32)
    assert np.abs(start[:, :nb, :3] - first["pos"]).max() < 1e-5 and same_bits(got[:, nb], start[:, nb])
    res = [hold(f"closed loop {name} axis {axis}", "tip midpoint", float(np.abs(tip_mid(got, robot)[:, :3] - tip_mid(o64["pos"], robot)).max()),
                float(np.abs(tip_mid(o32["pos"], robot).astype(np.float64) - tip_mid(o64["pos"], robot)).max()))]
    # plain sense, from the float64 prototype of this loop (0.0912 / 0.0968 / 0.0947 of 0.100 along; <= 0.002 off; <= 0.004 rad).  No -y on
    # the mobile default pose: a joint of it sits exactly on its lower limit and the clamp bends the motion (0.30 rad of tip rotation)
    moved = (tip_mid(got, robot)[:, :3] - tip_mid(start, robot)[:, :3]).astype(np.float64)
    off = np.delete(moved, axis, axis=1)
    Rt = K.quat_matrix(got[:, robot.ltip_rb_index, 3:7], np.float64) @ K.quat_matrix(start[:, robot.ltip_rb_index, 3:7], np.float64).transpose(0, 2, 1)
    angle = np.arccos(np.clip((np.trace(Rt, axis1=1, axis2=2) - 1) / 2, -1, 1))
    print(f"closed loop {name} axis {axis}: along {moved[:, axis].min():.4f}, off {np.abs(off).max():.4f}, rotation {angle.max():.4f} rad")
    assert moved[:, axis].min() >= 0.085
    if name == "fixed":
        assert np.abs(off).max() <= 0.005 and angle.max() <= 0.01
    # compute_scene_pose of the last step: the reference's body poses times the part matrices
    rot, pos = task.compute_scene_pose()
    parts = npy(task.part_body)
    C = npy(task.part_C).astype(np.float64)
    R64 = np.concatenate([o64["R"], np.broadcast_to(np.eye(3), (N, 1, 3, 3))], axis=1)[:, parts] @ C
    R32 = np.concatenate([o32["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (N, 1, 3, 3))], axis=1)[:, parts].astype(np.float64) @ C
    T64 = np.concatenate([o64["pos"], np.broadcast_to(npy(cube).astype(np.float64), (N, 1, 3))], axis=1)[:, parts]
    T32 = np.concatenate([o32["pos"].astype(np.float64), np.broadcast_to(npy(cube).astype(np.float64), (N, 1, 3))], axis=1)[:, parts]
    assert parts.tolist() == (list(tree.mesh_bodies()) if name == "mobile" else list(range(10)) + [11]) + [nb]
    res += [hold(f"closed loop {name} axis {axis}", "pose_R", float(np.abs(npy(rot) - R64).max()), float(np.abs(R32 - R64).max())),
            hold(f"closed loop {name} axis {axis}", "pose_T", float(np.abs(npy(pos) - T64).max()), float(np.abs(T32 - T64).max()))]
    for ok, what in res:
        assert ok, what
