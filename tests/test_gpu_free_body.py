"""The free body's step on the GPU: pm_free_body_step_f32 (csrc/free_body.hip) through ops.free_body_step, against the numpy statement
of its four rules (tests/free_body_ref.py), at N = 67 (more than a wave, more than a block of 64) and N = 1, dt = 1 / 60.

Tolerance: test_gpu_kinematics.py's rule.  Per rule and quantity e_ref = the worst error of the statement's float32 run against its
float64 run; the kernel must stay within 4 e_ref of the float64 run (a quantity the contract keeps or copies has e_ref = 0 and must
come out exactly).  Every observed / allowed pair is recorded (helpers.record_margin; tools/margins_summary.py folds the lines into
profiles/free_body_margins.json).  Everything else is an equality: flags, the latch, bits between runs, orders, batch sizes and layouts,
sentinels, error codes."""
import functools

import numpy as np
import pytest
import torch

from tests import free_body_ref as FB
from tests import helpers
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
SENTINEL = -777.25
DT = 1.0 / 60.0
N67 = 67
NB, NA, LT, RT, OBJ = 5, 3, 1, 3, 1                           # bodies per environment, actors, the tips' bodies, the body's actor
PARAMS = dict(reset_range=0.15, rest_z=0.025, fall_speed=0.3)
DEFAULT_POSE = np.array([0.01, -0.02, 0.025, 0.1, -0.2, 0.3, 0.9], dtype=np.float32)
DEFAULT_POSE[3:] /= np.linalg.norm(DEFAULT_POSE[3:].astype(np.float64))


@functools.lru_cache(maxsize=None)
def scene(N=N67, seed=7):
    """Seeded float32 inputs in which neighbouring environments take different rules: e % 6 = 0 reset, 1 reset + hold (reset wins),
    2 hold with the latch clear, 3 hold with the latch set, 4 and 5 released (one above rest_z by less than a step's fall or more, one
    at or under it), latch set or clear.  Computed once and never modified."""
    rng = np.random.default_rng(seed)
    tips = (rng.normal(size=(N, 2, 13)) * 0.3).astype(np.float32)
    tips[:, :, 3:7] = (rng.normal(size=(N, 2, 4)) * 1.3).astype(np.float32)             # not unit: the contract divides by the norm
    body = np.concatenate([rng.uniform(-0.3, 0.3, (N, 3)), rng.normal(size=(N, 4)), rng.normal(size=(N, 6))], axis=1).astype(np.float32)
    e = np.arange(N)
    body[e % 6 == 4, 2] = (0.025 + rng.uniform(0.0005, 0.02, N))[e % 6 == 4]             # fall_speed dt = 0.005: some reach rest_z
    body[e % 6 == 5, 2] = (0.025 - rng.uniform(0.0, 0.01, N))[e % 6 == 5]
    body[5, 2] = np.float32(0.025)                            # exactly at rest
    grip = np.concatenate([rng.uniform(-0.05, 0.05, (N, 3)), rng.normal(size=(N, 4)), np.zeros((N, 1))], axis=1).astype(np.float32)
    grip[:, 3:7] /= np.linalg.norm(grip[:, 3:7], axis=1, keepdims=True)
    grip[:, 7] = ((e % 6 == 3) | (e % 12 == 0) | (e % 12 == 4) | (e % 12 == 11)).astype(np.float32)
    hold = np.isin(e % 6, (1, 2, 3))
    reset = np.isin(e % 6, (0, 1))
    u = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    for v in (tips, body, grip, hold, reset, u):
        v.setflags(write=False)
    s = dict(N=N, tips=tips, body=body, grip=grip, hold=hold, reset=reset, u=u)
    for name, dtype in (("w64", np.float64), ("w32", np.float32)):
        s[name] = FB.step(tips[:, 0], tips[:, 1], body, grip, hold, reset, DEFAULT_POSE, u, dt=DT, dtype=dtype, **PARAMS)
    assert sorted(set(s["w64"][2])) == [1, 2, 3, 4]
    return s


def dense_rows(N):
    first = np.arange(N) * NB
    return np.stack([first + LT, first + RT], axis=1).astype(np.int32), (first + NB - 1).astype(np.int32)


def launch(s, env=None, layout="dense", u="given", **over):
    """The scene's environments `env` through ops.free_body_step: (body rows (n, 13), root, grip, rigid_body), all numpy.  layout
    'flat': the same rows scattered over a flat (B, 13) tensor, each environment's three rows apart and in reverse order."""
    from partmanip_amd import ops
    env = np.arange(s["N"]) if env is None else np.asarray(env)
    n = len(env)
    if layout == "dense":
        rb = np.full((n, NB, 13), SENTINEL, dtype=np.float32)
        tip_rows, body_row = dense_rows(n)
    else:
        rb = np.full((7 * n + 3, 13), SENTINEL, dtype=np.float32)
        first = 7 * (n - 1 - np.arange(n)) + 2
        tip_rows, body_row = np.stack([first + 4, first], axis=1).astype(np.int32), (first + 2).astype(np.int32)
    flat = rb.reshape(-1, 13)
    flat[tip_rows[:, 0]], flat[tip_rows[:, 1]] = s["tips"][env, 0], s["tips"][env, 1]
    root = np.full((n, NA, 13), SENTINEL, dtype=np.float32)
    root[:, OBJ] = s["body"][env]
    rb0, root0 = rb.copy(), root.copy()
    rb_t, root_t, grip_t = t(rb), t(root), t(s["grip"][env])
    kw = dict(PARAMS, **over)
    ops.free_body_step(rb_t, t(tip_rows), t(body_row), root_t, OBJ, t(s["hold"][env]), t(s["reset"][env]), grip_t, t(DEFAULT_POSE), DT,
                       u=t(s["u"][env]) if u == "given" else None, **kw)
    rb, root, grip = npy(rb_t), npy(root_t), npy(grip_t)
    # only the body's row, root[e, OBJ] and grip change: every other row keeps its bits, sentinels and tips alike
    other = np.ones(rb.reshape(-1, 13).shape[0], dtype=bool)
    other[body_row] = False
    assert same_bits(rb.reshape(-1, 13)[other], rb0.reshape(-1, 13)[other])
    keep = np.ones(NA, dtype=bool)
    keep[OBJ] = False
    assert same_bits(root[:, keep], root0[:, keep])
    rows = rb.reshape(-1, 13)[body_row]
    assert same_bits(rows, root[:, OBJ])                      # the two copies hold identical bits
    return rows, root, grip, rb


def margin(name, key, got, w32, w64):
    e_ref = float(np.abs(w32.astype(np.float64) - w64).max()) if w64.size else 0.0
    err = float(np.abs(np.asarray(got, dtype=np.float64) - w64).max()) if w64.size else 0.0
    print(f"{name} {key}: e_ref = {e_ref:.3e}; observed = {err:.3e}" + (f" = {err / e_ref:.2f} e_ref" if e_ref > 0 else ""))
    if e_ref > 0:
        record_margin(f"free body {name}: {key} / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    return err <= 4 * e_ref, (name, key, err, e_ref)


QUANTITIES = (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("linear velocity", slice(7, 10)), ("angular velocity", slice(10, 13)))
RULES = ((FB.RESET, "1 reset"), (FB.LATCH, "2 latch"), (FB.CARRY, "3 carry"), (FB.FREE, "4 released"))


def compare(s, rows, grip, w64, w32, tag=""):
    res = []
    for case, name in RULES:
        m = w64[2] == case
        assert m.any(), name
        for key, sl in QUANTITIES:
            res.append(margin(name + tag, key, rows[m][:, sl], w32[0][m][:, sl], w64[0][m][:, sl]))
        res.append(margin(name + tag, "grip rel_t", grip[m, :3], w32[1][m, :3], w64[1][m, :3]))
        res.append(margin(name + tag, "grip rel_q", grip[m, 3:7], w32[1][m, 3:7], w64[1][m, 3:7]))
    assert np.array_equal(grip[:, 7], w64[1][:, 7].astype(np.float32))                   # the latch: an equality
    for ok, what in res:
        assert ok, what


# ------------------------------------------------------------------------------------------- 1. the four rules
def test_every_rule_matches_its_float64_statement():
    s = scene()
    rows, root, grip, _ = launch(s)
    compare(s, rows, grip, s["w64"], s["w32"])
    w64 = s["w64"]
    kept = np.isin(w64[2], (FB.LATCH, FB.FREE))
    assert same_bits(rows[kept][:, [0, 1, 3, 4, 5, 6]], s["body"][kept][:, [0, 1, 3, 4, 5, 6]])      # a kept value keeps its bits
    assert same_bits(rows[w64[2] == FB.LATCH, 2], s["body"][w64[2] == FB.LATCH, 2])
    assert same_bits(rows[w64[2] == FB.CARRY, 10:], s["tips"][w64[2] == FB.CARRY, 0, 10:])           # the left tip's angular velocity
    assert not np.any(rows[w64[2] != FB.CARRY, 10:]) and not np.any(rows[np.isin(w64[2], (FB.RESET, FB.LATCH)), 7:])
    free = w64[2] == FB.FREE
    z0, z1 = s["body"][free, 2], rows[free, 2]
    assert (z1 >= np.float32(0.025))[z0 > np.float32(0.025)].all() and (z1 == np.float32(0.025)).any() and (z1 < z0).any()
    assert same_bits(z1[z0 <= np.float32(0.025)], z0[z0 <= np.float32(0.025)]) and not np.any(rows[free][z0 <= np.float32(0.025), 9])
    assert same_bits(grip[~(w64[2] == FB.LATCH), :7], s["grip"][~(w64[2] == FB.LATCH), :7])          # rel is written by the latch only


def test_fall_speed_zero_leaves_a_released_body_where_it_is():
    s = scene()
    rows, _, grip, _ = launch(s, fall_speed=0.0)
    free = s["w64"][2] == FB.FREE
    assert same_bits(rows[free, :7], s["body"][free, :7]) and not np.any(rows[free, 7:]) and not np.any(grip[free, 7])
    assert not np.signbit(rows[free, 7:]).any()               # the velocity is +0


# ------------------------------------------------------------------------------------------- 2. reset
def test_reset_without_u_is_the_default_pose_and_with_u_stays_in_range():
    s = scene()
    rows, _, grip, _ = launch(s, u=None)
    r = s["reset"]
    assert same_bits(rows[r, :7], np.broadcast_to(DEFAULT_POSE, (r.sum(), 7))) and not np.any(rows[r, 7:]) and not np.any(grip[r, 7])
    other, _, _, _ = launch(s)
    assert same_bits(other[~r], rows[~r])                     # u is read by resetting environments only
    # every environment resets, over a seeded u that holds both ends of [0, 1)
    N = 67
    rng = np.random.default_rng(3)
    u = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    u[0], u[1] = 0.0, np.float32(1.0) - np.float32(2.0 ** -24)
    s2 = dict(s, N=N, u=u, reset=np.ones(N, dtype=bool))
    rows, _, _, _ = launch(s2)
    want64 = FB.step(s["tips"][:, 0], s["tips"][:, 1], s["body"], s["grip"], s["hold"], s2["reset"], DEFAULT_POSE, u, dt=DT, **PARAMS)
    want32 = FB.step(s["tips"][:, 0], s["tips"][:, 1], s["body"], s["grip"], s["hold"], s2["reset"], DEFAULT_POSE, u, dt=DT, dtype=np.float32,
                     **PARAMS)
    res = [margin("reset over u", key, rows[:, sl], want32[0][:, sl], want64[0][:, sl]) for key, sl in QUANTITIES]
    for ok, what in res:
        assert ok, what
    d = rows[:, :2].astype(np.float64) - DEFAULT_POSE[:2]
    assert (np.abs(d) <= 0.15 + 2.0 ** -24).all() and np.abs(d).max() > 0.14 and same_bits(rows[:, 2], np.full(N, DEFAULT_POSE[2]))
    assert not np.any(rows[:, 7:])


# ------------------------------------------------------------------------------------------- 3. independence
def test_repeated_permuted_alone_and_flat_runs_give_the_same_bits():
    s = scene()
    rows, root, grip, _ = launch(s)
    rows2, root2, grip2, _ = launch(s)
    assert same_bits(rows, rows2) and same_bits(root, root2) and same_bits(grip, grip2)
    perm = np.random.default_rng(1).permutation(s["N"])
    rp, _, gp, _ = launch(s, env=perm)
    assert same_bits(rp, rows[perm]) and same_bits(gp, grip[perm])
    for e in (0, 1, 2, 3, 4, 5, 63, 64, 66):                  # N = 1: every rule, the wave's seam, the last
        r1, _, g1, _ = launch(s, env=[e])
        assert same_bits(r1[0], rows[e]) and same_bits(g1[0], grip[e]), e
    rf, _, gf, _ = launch(s, layout="flat")                  # flat rows, scattered and in reverse order
    assert same_bits(rf, rows) and same_bits(gf, grip)


def test_a_carried_body_keeps_its_grip_exactly_over_50_steps():
    from partmanip_amd import ops
    N = N67
    rng = np.random.default_rng(9)
    tip_rows, body_row = dense_rows(N)
    rb = np.zeros((N, NB, 13), dtype=np.float32)
    rb[..., 6] = 1
    root = np.zeros((N, NA, 13), dtype=np.float32)
    root[:, OBJ, :3] = rng.uniform(-0.1, 0.1, (N, 3))
    root[:, OBJ, 3:7] = rng.normal(size=(N, 4))
    rb_t, root_t, grip_t = t(rb), t(root), torch.zeros(N, 8, device=DEV)
    hold, reset = torch.ones(N, dtype=torch.bool, device=DEV), torch.zeros(N, dtype=torch.bool, device=DEV)
    args = (t(tip_rows), t(body_row), root_t, OBJ, hold, reset, grip_t, t(DEFAULT_POSE), DT)
    first = None
    for step in range(51):
        tips = (rng.normal(size=(N, 2, 13)) * 0.3).astype(np.float32)                   # the hand moves and turns every step
        rb_t[:, LT], rb_t[:, RT] = t(tips[:, 0]), t(tips[:, 1])
        ops.free_body_step(rb_t, *args)
        if step == 0:
            first = npy(grip_t).copy()
            assert (first[:, 7] == 1).all() and same_bits(npy(root_t)[:, OBJ, :7], root[:, OBJ, :7])
        else:
            assert same_bits(npy(grip_t), first), step        # the latch is written once: nothing to drift
    # and the last pose is the hand frame o grip, as the statement gives it from the FIRST step's grip
    last = np.concatenate([tips[:, 0], tips[:, 1]], axis=0).reshape(2, N, 13)
    w64 = FB.step(last[0], last[1], npy(root_t)[:, OBJ], first, np.ones(N, bool), np.zeros(N, bool), DEFAULT_POSE, None, dt=DT, **PARAMS)
    w32 = FB.step(last[0], last[1], npy(root_t)[:, OBJ], first, np.ones(N, bool), np.zeros(N, bool), DEFAULT_POSE, None, dt=DT,
                  dtype=np.float32, **PARAMS)
    got = npy(root_t)[:, OBJ]
    res = [margin("after 50 carried steps", key, got[:, sl], w32[0][:, sl], w64[0][:, sl]) for key, sl in QUANTITIES[:2]]
    for ok, what in res:
        assert ok, what


def test_a_nan_stays_in_its_environment():
    s = scene()
    rows, _, grip, _ = launch(s)
    tips, body = s["tips"].copy(), s["body"].copy()
    tips[2, 1, 0] = np.nan                                    # a latching environment: its right tip's position
    tips[3, 0, 4] = np.nan                                    # a carried one: the hand's quaternion
    body[4, 2] = np.nan                                       # a released one: its own height
    got, _, g2, _ = launch(dict(s, tips=tips, body=body))
    hit = np.zeros(s["N"], dtype=bool)
    hit[[2, 3, 4]] = True
    assert same_bits(got[~hit], rows[~hit]) and same_bits(g2[~hit], grip[~hit])
    assert np.isnan(g2[2, :3]).all() and g2[2, 7] == 1 and same_bits(got[2, :7], s["body"][2, :7])
    assert np.isnan(got[3, :7]).all()
    assert np.isnan(got[4, 2]) and got[4, 9] == 0 and same_bits(got[4, [0, 1, 3, 4, 5, 6]], s["body"][4, [0, 1, 3, 4, 5, 6]])


# ------------------------------------------------------------------------------------------- 4. refusals
def test_every_invalid_argument_is_refused_and_an_out_of_range_row_stores_nothing():
    from partmanip_amd import ops
    from partmanip_amd._lib import lib as clib
    s = scene()
    N = s["N"]
    tip_rows, body_row = dense_rows(N)
    rb0 = np.full((N, NB, 13), SENTINEL, dtype=np.float32)
    rb0[:, LT], rb0[:, RT] = s["tips"][:, 0], s["tips"][:, 1]
    root0 = np.full((N, NA, 13), SENTINEL, dtype=np.float32)
    root0[:, OBJ] = s["body"]
    rb, root, grip = t(rb0), t(root0), t(s["grip"])
    keep = [t(tip_rows), t(body_row), t(s["hold"]), t(s["reset"]), t(DEFAULT_POSE), t(s["u"])]
    p = lambda x: x.data_ptr()                                 # noqa: E731
    good = dict(rigid_body=p(rb), rb_rows=N * NB, tip_rows=p(keep[0]), body_row=p(keep[1]), root=p(root), na=NA, obj_actor=OBJ,
                hold=p(keep[2]), reset=p(keep[3]), grip=p(grip), default_pose=p(keep[4]), u=p(keep[5]), reset_range=0.15, dt=DT,
                rest_z=0.025, fall_speed=0.3, N=N, stream=0)
    bad = [{k: 0} for k in ("rigid_body", "rb_rows", "tip_rows", "body_row", "root", "na", "hold", "reset", "grip", "default_pose", "N", "dt")]
    bad += [dict(obj_actor=-1), dict(obj_actor=NA), dict(rb_rows=2 ** 31), dict(rb_rows=-1), dict(N=-1), dict(dt=-DT), dict(dt=float("nan")),
            dict(fall_speed=-0.1), dict(fall_speed=float("nan")), dict(reset_range=-0.1), dict(reset_range=float("nan")),
            dict(rest_z=float("nan"))]
    for change in bad:
        assert clib.pm_free_body_step_f32(*{**good, **change}.values()) == -1, change
    torch.cuda.synchronize()
    assert same_bits(npy(rb), rb0) and same_bits(npy(root), root0) and same_bits(npy(grip), s["grip"])
    # the wrapper's own checks
    for change, err in ((dict(dt=0.0), ValueError), (dict(fall_speed=-1.0), ValueError), (dict(obj_actor=NA), ValueError),
                        (dict(grip=grip[:, :7].contiguous()), ValueError), (dict(u=keep[5][:, :2].contiguous()), ValueError),
                        (dict(tip_rows=keep[0].long()), ValueError), (dict(hold=keep[2].float()), ValueError),
                        (dict(root=root.cpu()), RuntimeError)):
        kw = dict(rigid_body=rb, tip_rows=keep[0], body_row=keep[1], root=root, obj_actor=OBJ, hold=keep[2], reset=keep[3], grip=grip,
                  default_pose=keep[4], dt=DT, u=keep[5], **PARAMS)
        kw.update(change)
        with pytest.raises(err):
            ops.free_body_step(**kw)
    # environments the kernel must skip: a tip row or the body's row outside [0, rb_rows).  Everyone else is computed as before.
    want, _, want_grip, _ = launch(s)
    tr, br = tip_rows.copy(), body_row.copy()
    tr[0, 0], tr[1, 1], tr[2, 0], br[3], br[4], br[65] = N * NB, -1, 2 ** 31 - 1, N * NB, -5, -(2 ** 31)
    skipped = [0, 1, 2, 3, 4, 65]
    ops.free_body_step(rb, t(tr), t(br), root, OBJ, keep[2], keep[3], grip, keep[4], DT, u=keep[5], **PARAMS)
    got_rb, got_root, got_grip = npy(rb), npy(root), npy(grip)
    for e in range(N):
        if e in skipped:
            assert same_bits(got_rb[e], rb0[e]) and same_bits(got_root[e], root0[e]) and same_bits(got_grip[e], s["grip"][e]), e
        else:
            assert same_bits(got_rb[e, NB - 1], want[e]) and same_bits(got_root[e, OBJ], want[e]) and same_bits(got_grip[e], want_grip[e]), e
