"""Contact blocking, everything that needs no GPU: the restatement of tests/guarded_step_ref.py on the push and the grasp fixtures
(what the rule does, and the condition under which the GPU tests may assert a cut as an equality), the selection rule on hand-made
rows, the slot_body derivation, and the refusals of the C entries, ops.articulation_sweep, StepGuard and KinematicEnv."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import contact_episode as CE
from tests import guarded_step_ref as GS
from tests import kinematic_episode as E
from tests.test_capi_symbols import header_functions

PUSH_STEPS = 46


@functools.lru_cache(maxsize=None)
def push(S):
    """(float64 run, float32 run replaying its actions) of the guarded push episode at S parts per step."""
    r64 = GS.push_episode(PUSH_STEPS, S=S)
    return r64, GS.push_episode(PUSH_STEPS, S=S, dtype=np.float32, actions=[s["action"][None] for s in r64])


# ------------------------------------------------------------------------------------------- the restatement
def test_candidates_end_at_the_drive_rule_and_stay_inside_the_limits():
    rng = np.random.RandomState(5)
    lo, hi = np.full(4, -1.0), np.full(4, 1.0)
    q, t = rng.uniform(-1.2, 1.2, size=(3, 4)), rng.uniform(-2, 2, size=(3, 4))
    vmax, dt = np.full(4, 3.0), np.float32(1 / 60)
    from tests import kinematics_ref as K
    for S in (1, 4, 8):
        for reset in (None, np.array([False, True, False])):
            c = GS.candidates(q, t, lo, hi, vmax, dt, reset, S)
            assert c.shape == (S + 1, 3, 4) and (c >= -1).all() and (c <= 1).all()
            assert np.array_equal(c[-1], K.drive(q, t, lo, hi, vmax, dt, reset=reset)[0]) and np.array_equal(c[0], np.clip(q, -1, 1))
            assert np.array_equal(K.clamp(c, lo, hi), c)      # clamp is idempotent: executing a candidate as a target gives the candidate
    c32 = GS.candidates(q.astype(np.float32), t.astype(np.float32), lo, hi, vmax, dt, None, 8, dtype=np.float32)
    assert c32.dtype == np.float32 and np.abs(c32 - GS.candidates(q, t, lo, hi, vmax, dt, None, 8)).max() < 1e-6
    t[1, 2] = np.nan
    c = GS.candidates(q, t, lo, hi, vmax, dt, None, 4)
    assert not np.isnan(c[0]).any() and np.isnan(c[1:, 1, 2]).all() and not np.isnan(np.delete(c.reshape(5, -1), 6, axis=1)).any()


# ------------------------------------------------------------------------------------------- the selection rule
def test_selection_rule_on_hand_made_rows():
    nan = np.nan
    rows = np.array([[0.5, 0.4, 0.3, 0.2, 0.1],               # free motion above the margin
                     [0.5, 0.3, 0.1, -0.1, -0.2],             # first contact at k = 3
                     [-0.3, -0.2, -0.1, 0.05, 0.2],           # separation from inside: admitted all the way
                     [-0.3, -0.2, -0.25, 0.1, 0.2],           # ... until it would go deeper again
                     [-0.02, -0.02, -0.02, -0.02, -0.02],     # a plateau at the truncation: moving along is admitted
                     [0.5, 0.4, nan, 0.4, 0.5],               # a NaN in the middle
                     [nan, 0.4, 0.3, 0.2, 0.1],               # a NaN start: the candidates above the margin are admissible
                     [nan, -0.1, -0.1, 0.2, 0.3],             # a NaN start below the margin: nothing compares
                     [0.1, 0.0, 0.1, 0.2, 0.3],               # AT the margin counts as contact
                     [0.5, 0.3, 0.1, -0.1, -0.2]])
    want = [4, 2, 4, 1, 4, 1, 4, 0, 0, 2]
    assert GS.select(rows, 0.0).tolist() == want
    forced = np.zeros(10, dtype=bool)
    forced[[1, 5, 7]] = True                                  # reset or free environments take the whole step
    assert GS.select(rows, 0.0, forced).tolist() == [4 if f else w for w, f in zip(want, forced)]
    assert GS.select(rows[[0, 1]], 0.35).tolist() == [1, 0]   # a wider margin
    assert GS.select(rows[:, :2], 0.0).tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0, 1]      # S = 1


# ------------------------------------------------------------------------------------------- the push fixture
def test_unguarded_push_goes_through_the_cube():
    un = GS.push_episode(60)
    depth = -min(float(s["body_dist"][2]) for s in un)
    print(f"unguarded: the right finger ends {1e3 * -un[-1]['body_dist'][2]:.2f} mm inside the cube (deepest {1e3 * depth:.2f} mm)")
    assert abs(-un[-1]["body_dist"][2] - 0.0150) < 1e-4 and CE.CUBE_TRUNC == 0.02      # 15.0 mm; the grid truncates at 20 mm


@pytest.mark.parametrize("S, parts, rest_mm", [(4, 1, 0.365), (8, 2, 0.365), (16, 5, 0.073)])
def test_guarded_push_stops_short_of_the_cube(S, parts, rest_mm):
    r64, r32 = push(S)
    cuts = [(i, s["steps"]) for i, s in enumerate(r64) if s["steps"] < S]
    rest = float(r64[-1]["body_dist"].min())
    print(f"S = {S}: first cut at log index {cuts[0][0]} to {cuts[0][1]} of {S}, rest distance {1e3 * rest:.3f} mm")
    assert cuts[0] == (41, parts) and all(c == 0 for _, c in cuts[1:]) and [i for i, _ in cuts] == list(range(41, PUSH_STEPS))
    assert abs(1e3 * rest - rest_mm) < 5e-4 and all(s["body_dist"].min() > 0 for s in r64)
    if S == 8:
        D = r64[41]["sweep_dist"]
        assert abs(D[2] - 0.00036) < 1e-5 and abs(D[3] + 0.00022) < 1e-5            # the two distances that decide the cut


@pytest.mark.parametrize("S", [4, 8, 16])
def test_every_deciding_distance_is_clear_of_float32_round_off(S):
    """For every step and every candidate up to the first inadmissible one: its distance differs from the margin (0) by more than
    100 x what the float32 run loses there, and where it is at or below the margin it differs as much from its predecessor.  So
    the float32 run, and the kernel, which equals a float32 composition bit for bit, take the same decisions."""
    r64, r32 = push(S)
    worst = np.inf
    for a, b in zip(r64, r32):
        assert a["steps"] == b["steps"]
        D, e = a["sweep_dist"], np.abs(b["sweep_dist"].astype(np.float64) - a["sweep_dist"])
        for k in range(1, min(a["steps"] + 1, S) + 1):
            gaps = [abs(D[k])] + ([abs(D[k] - D[k - 1])] if D[k] <= 0 else [])
            err = max(e[k], e[k - 1])
            if err > 0:
                worst = min(worst, min(gaps) / err)
            assert min(gaps) > 100 * err, (S, k, D[k - 1:k + 1], err)
    print(f"S = {S}: the closest decision is {worst:.0f} x the float32 error away")


# ------------------------------------------------------------------------------------------- the grasp fixture
def test_the_contact_grasp_episode_is_never_cut():
    S = 8
    log = GS.grasp_episode(E.MAX_EPISODE_LENGTH, S=S)
    plain = CE.run_reference(E.MAX_EPISODE_LENGTH, stop_after_hold=40)
    onset = next(i for i, s in enumerate(log) if s["hold"])
    success = next(i for i, s in enumerate(log) if s["success"])
    nearest = min(float(s["sweep_dist"].min()) for s in log[:onset])
    print(f"hold from log index {onset}, success at step {success + 1}; nearest candidate before the latch {1e3 * nearest:.2f} mm")
    assert all(s["steps"] == S for s in log) and onset == 50 == CE.hold_onset(plain) and success + 1 == 84
    assert nearest > 0.0015
    for a, b in zip(log, plain):                              # the guard changes nothing: the cube and the flags of the unguarded run
        assert np.array_equal(a["cube"], b["cube"]) and a["success"] == b["success"] and a["hold"] == b["hold"]


# ------------------------------------------------------------------------------------------- host logic
def test_slot_body_derivation():
    from partmanip_amd.envs import guard_slot_body, scene_row_table
    from partmanip_amd.tasks.grasp_cube import default_part_body
    assert guard_slot_body(13, part_body=default_part_body(14)).tolist() == list(range(10)) + [11, -1]
    assert guard_slot_body(13, part_body=[3, 13, 14, -1, 0]).tolist() == [3, -1, -1, -1, 0]
    rb_row0, obj_rb_row0 = np.array([0, 15, 35]), np.array([13, 28, 48])
    rows = scene_row_table([0, 4, 12], rb_row0, obj_rb_row0, [2, 7, 1])
    sb = guard_slot_body(13, scene_rows=rows, rb_row0=rb_row0)
    assert sb.dtype == np.int32 and sb.tolist() == [0, 4, 12] + [-1] * 7
    dense = np.array([[0, 5, 13], [14, 19, 27]])              # a dense (N, 14, 13) tensor: the cube is the row after the robot's 13
    assert guard_slot_body(13, scene_rows=dense, rb_row0=[0, 14]).tolist() == [0, 5, -1]
    with pytest.raises(ValueError, match="same slots"):
        guard_slot_body(13, scene_rows=np.array([[0, 5], [14, 20]]), rb_row0=[0, 14])
    with pytest.raises(ValueError, match="scene_rows / rb_row0"):
        guard_slot_body(13, scene_rows=dense, rb_row0=[0])


def test_header_ctypes_table_and_library_agree():
    from partmanip_amd import _lib
    P_, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert header_functions()["pm_articulation_sweep_f32"] == ("int", 51) and header_functions()["pm_articulation_sweep_groups_f32"] == ("int", 58)
    step = _lib.SIGNATURES["pm_articulation_step_f32"][1]
    pts = _lib.SIGNATURES["pm_mesh_sdf_points_f32"][1]
    args = _lib.SIGNATURES["pm_articulation_sweep_f32"][1]
    chain = [P_] * 9 + [F, P_, L, P_, L, P_, L, P_, P_, L, I, I, I]
    assert chain[:6] == step[:6] and args[:22] == chain and args[22:27] == pts[:5]
    assert args[27:] == [P_, P_, I, I, I, P_, L, P_, P_, P_, I, P_, I, I, P_, P_, I, I, F, P_, P_, P_, P_, P_]
    gargs = _lib.SIGNATURES["pm_articulation_sweep_groups_f32"][1]
    assert gargs == args[:27] + [P_, I, I, P_, I, P_, I] + args[27:]
    assert hasattr(_lib.lib, "pm_articulation_sweep_f32") and hasattr(_lib.lib, "pm_articulation_sweep_groups_f32")
    assert _lib.ABI_VERSION == 163 == _lib.lib.pm_version()


def test_every_einval_condition_is_refused_before_a_launch():
    """Any non-NULL pointer will do: a call that is refused launches and reads nothing."""
    from partmanip_amd._lib import lib
    one = 1
    good = dict(parent=one, jtype=one, dof=one, origin_q=one, origin_t=one, axis=one, dof_lo=one, dof_hi=one, vmax=None, dt=1 / 60, base_pose=one,
                base_stride=0, dof_state=one, dof_rows=27, targets=one, tgt_stride=9, reset=None, dof_row0=None, dof_stride=9, N=3, nb=13,
                nd=9, fields=one, part_off=one, part_shape=one, part_bbox_min=one, part_voxel_size=one, pose_R=one, pose_T=one, M=12, p0=11,
                p1=12, pts=one, pts_env_stride=0, carrier=one, pt_id=None, chunk_sphere=None, NP=384, seg_off=one, NS=3, cull=1,
                slot_body=one, slot_C=one, MC=12, S=8, block_margin=0.0, free_env=None, sweep_dist=one, steps=one, targets_out=one,
                stream=None)
    call = lambda **kw: lib.pm_articulation_sweep_f32(*dict(good, **kw).values())         # noqa: E731
    items = list(good.items())
    ggood = dict(items[:27] + [("grid_slot", one), ("NG", 6), ("NG_shared", 2), ("group_off", one), ("G", 2), ("env_group", one),
                               ("max_group_grids", 3)] + items[27:])
    ggood.update(M=5, p0=2, p1=5, MC=5)
    gcall = lambda **kw: lib.pm_articulation_sweep_groups_f32(*dict(ggood, **kw).values())   # noqa: E731
    for name in ("parent", "jtype", "dof", "origin_q", "origin_t", "axis", "dof_lo", "dof_hi", "base_pose", "dof_state", "targets", "fields",
                 "part_off", "part_shape", "part_bbox_min", "part_voxel_size", "pose_R", "pose_T", "pts", "carrier", "seg_off", "slot_body",
                 "slot_C", "sweep_dist", "steps", "targets_out"):
        assert call(**{name: None}) == -1 and gcall(**{name: None}) == -1, name
    bad = [dict(N=0), dict(nb=0), dict(nb=65), dict(nd=0), dict(nd=65), dict(base_stride=6), dict(dof_rows=26), dict(dof_stride=8), dict(dt=0.0),
           dict(dt=float("nan")), dict(tgt_stride=8), dict(M=0), dict(p0=-1), dict(p0=2, p1=2), dict(NP=0), dict(NP=2 ** 30 + 1), dict(NS=0),
           dict(pts_env_stride=1151), dict(MC=-1), dict(MC=13), dict(S=0), dict(S=64), dict(block_margin=float("nan")),
           dict(nb=64, nd=64, dof_rows=192, dof_stride=64, tgt_stride=64, S=14)]                  # 15 candidates of 64 bodies: LDS
    for kw in bad:
        assert call(**kw) == -1, kw
        assert gcall(**kw) == -1, kw
    assert call(p1=13) == -1
    for kw in (dict(grid_slot=None), dict(group_off=None), dict(env_group=None), dict(NG=0), dict(NG_shared=-1), dict(NG_shared=7), dict(G=-1),
               dict(max_group_grids=-1), dict(p1=6), dict(M=32769)):
        assert gcall(**kw) == -1, kw


@pytest.fixture(scope="module")
def cpu():
    """The contact episode's tables as CPU tensors: every check of ops.articulation_sweep comes before it looks for a device."""
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.kinematics import Articulation
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    tree, bp, dof0 = E.scene()
    art = Articulation(tree, 2, "cpu")
    tsdf = TSDFfromMesh(2, 0.5, 10, "cpu", sdf_dicts=CE.grids())
    pts, carrier, segments = CE.sensing_points()
    sensor = ContactSensor(tsdf, pts, carrier, segments, targets=(11, 12))
    return dict(art=art, sensor=sensor, tsdf=tsdf, nd=tree.num_dofs, base=torch.tensor(np.float32(bp)))


def sweep(c, **kw):
    s, nd = c["sensor"], c["nd"]
    a = dict(dof_state=torch.zeros(2, nd, 2), targets=torch.zeros(2, nd), dt=1 / 60, pose_R=torch.zeros(2, 12, 3, 3), pose_T=torch.zeros(2, 12, 3),
             slot_body=list(range(11)) + [-1], substeps=8, seg_off=s._seg_off)
    a.update({k: kw.pop(k) for k in list(kw) if k in a})
    tables, R, T, groups = s.tsdf._point_tables(a["pose_R"], a["pose_T"])
    return c["art"].sweep(a["dof_state"], c["base"], a["targets"], a["dt"], *tables, R, T, s._pts, s._carrier, a["seg_off"], a["slot_body"],
                          a["substeps"], p0=11, p1=12, pt_id=s._pt_id, chunk_sphere=s.chunk_sphere, **groups, **kw)


def test_ops_wrapper_checks_come_before_the_device(cpu):
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # good arguments reach the device check
        sweep(cpu)
    for kw, what in ((dict(targets=None), "targets"), (dict(targets=torch.zeros(2, 8)), "targets"), (dict(dt=0.0), "dt"),
                     (dict(substeps=0), "substeps"), (dict(substeps=64), "substeps"), (dict(margin=float("nan")), "margin"),
                     (dict(seg_off=None), "seg_off"), (dict(slot_body=[0] * 11), "slot_body"), (dict(slot_body=[13] + [-1] * 11), "slot_body"),
                     (dict(slot_body=[-2] + [-1] * 11), "slot_body"), (dict(slot_body=np.zeros(12)), "slot_body"),
                     (dict(slot_C=torch.zeros(13, 3, 3)), "slot_C"), (dict(slot_C=torch.zeros(12, 9)), "slot_C"),
                     (dict(reset=torch.zeros(3, dtype=torch.bool)), "reset"), (dict(free=torch.zeros(2)), "free"),
                     (dict(pose_R=torch.zeros(3, 12, 3, 3), pose_T=torch.zeros(3, 12, 3)), "environments of the articulation"),
                     (dict(sweep_dist=torch.zeros(2, 8)), "sweep_dist"), (dict(steps=torch.zeros(2)), "steps"),
                     (dict(targets_out=torch.zeros(2, 8)), "targets_out"), (dict(dof_state=torch.zeros(2, 8, 2)), "dof_state")):
        with pytest.raises(ValueError, match=what):
            sweep(cpu, **kw)


def test_step_guard_and_env_refusals(cpu):
    from partmanip_amd.contact import StepGuard
    s = cpu["sensor"]
    for kw, what in ((dict(slot_body=[-1] * 11), "slot_body"), (dict(slot_body=[-2] + [-1] * 11), "slot_body"), (dict(substeps=0), "substeps"),
                     (dict(substeps=64), "substeps"), (dict(margin=float("nan")), "margin"), (dict(slot_C=np.zeros((13, 3, 3))), "slot_C")):
        a = dict(slot_body=[0] * 11 + [-1])
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            StepGuard(s, **a)
    g = StepGuard(s, list(range(11)) + [-1], np.zeros((12, 3, 3), dtype=np.float32), substeps=4, margin=0.001)
    assert g.substeps == 4 and g.margin == 0.001 and g.sweep_dist is None and g.slot_body.dtype == torch.int32
    from partmanip_amd.envs import KinematicEnv
    with pytest.raises(ValueError, match="resolve='block': needs contact="):
        KinematicEnv(None, None, resolve="block")
    with pytest.raises(ValueError, match="resolve: expected"):
        KinematicEnv(None, None, contact=s, resolve="slide")
