"""A numpy restatement of the swept contact test (include/partmanip_hip.h, pm_articulation_sweep_f32, steps 1 to 7) composed from the
tests' own references -- kinematics_ref.drive / fk, grasp_cube_ref.post, mesh_sdf_points_ref.restate -- in a chosen dtype, and the
two episodes the guard is judged on, over the fixture of tests/contact_episode.py (golden Franka, 3 x 128 sensing points, the 5 cm
cube's grid):

  push_episode    the tips' midpoint is driven at cube + (0, 0.03, 0) with the gripper open and hold never set: unguarded the right
                  finger ends up inside the cube, guarded it stops short of it;
  grasp_episode   contact_episode.run_reference's scripted contact grasp with the guard in the loop, which must not change it.

Host checks: tests/test_guarded_step_host.py; yardstick of tests/test_gpu_guarded_env.py."""
import numpy as np

from tests import contact_episode as CE
from tests import free_body_ref as FB
from tests import grasp_cube_ref as G
from tests import kinematic_episode as E
from tests import kinematics_ref as K
from tests import mesh_sdf_points_ref as RF

PUSH_OFFSET = (0.0, 0.03, 0.0)


def candidates(q, t, lo, hi, vmax, dt, reset, S, dtype=np.float64):
    """Steps 1 and 2: (S + 1, N, nd) joint states from q (N, nd) to the drive rule's end state, one rounding per operation."""
    f = dtype
    q, lo, hi = (np.asarray(a, dtype=f) for a in (q, lo, hi))
    with np.errstate(invalid="ignore"):
        qn = K.drive(q, t, lo, hi, vmax, dt, reset=reset, dtype=f)[0]
        out = [K.clamp(q, lo, hi)]
        for k in range(1, S):
            a = f(k) / f(S)
            out.append(K.clamp(q + a * (qn - q), lo, hi))
    return np.stack(out + [qn])


def select(D, margin, forced=None):
    """Steps 5 and 6 on distance rows D (N, S + 1): candidate k >= 1 is admissible iff D_k > margin or D_k >= D_{k-1} (a NaN is
    not); steps = the largest K with candidates 1 .. K all admissible; S where `forced` (N) is set."""
    D = np.asarray(D)
    S = D.shape[1] - 1
    with np.errstate(invalid="ignore"):
        adm = (D[:, 1:] > margin) | (D[:, 1:] >= D[:, :-1])
    steps = np.where(adm.all(axis=1), S, np.argmin(adm, axis=1)).astype(np.int32)
    return steps if forced is None else np.where(np.asarray(forced, dtype=bool), S, steps).astype(np.int32)


class Fixture:
    """The grasp_cube scene of contact_episode in dtype: observe() is one observation (fk, post, the point query)."""

    def __init__(self, dtype=np.float64):
        self.f = f = dtype
        self.tree, bp, dof0 = E.scene()
        c = lambda a: np.asarray(a, dtype=f)                   # noqa: E731
        self.lo, self.hi = c(np.float32(self.tree.lower)), c(np.float32(self.tree.upper))
        kw = self.tree.robot_kwargs()
        self.lt, self.rt, self.nb = kw["ltip_rb_index"], kw["rtip_rb_index"], self.tree.num_bodies
        self.part_body, self.part_C = CE.part_tables(self.nb + 1)
        self.pts, self.carrier, self.segments = CE.sensing_points()
        self.target = [None] * CE.CUBE_SLOT + [CE.cube_grid()]
        self.own = [[(CE.CUBE_SLOT, CE.CUBE_SLOT)]]
        self.default, self.base = c(np.float32(dof0)), c(np.float32(bp))
        self.cube0 = c(np.float32(E.CUBE_POSE))
        self.dt = np.float32(E.DT)

    def observe(self, q, qd, cube):
        """(fk, rigid-body rows, post, body distances (3,)) of one environment's state."""
        f = self.f
        out = K.fk(self.tree, q, qd, self.base, dtype=f)
        rb = np.concatenate([K.rigid_rows(out), cube[:, None]], axis=1)
        root = np.zeros((1, 2, 13), dtype=f)
        root[:, 1] = cube
        p = G.post(rb, np.stack([q, qd], axis=-1), root, 1, self.lt, self.rt, self.lo, self.hi, E.GOAL, E.GOAL_THRESH, E.CUBE_POSE[:3],
                   self.part_body, self.part_C, dtype=f)
        body = RF.restate(self.target, p["pose_R"], p["pose_T"], self.pts, self.carrier, own=self.own, segments=self.segments,
                          dtype=f)["seg_min"][0]
        return out, rb, p, body

    def sweep(self, q, cube, targets, reset, free, S, margin):
        """Steps 1 to 7 for one environment: dict(sweep_dist (S + 1,), steps, targets (1, nd), cand (S + 1, 1, nd)).  The scene
        pose of a candidate is post's on the candidate's body rows and the cube as it stands (a slot the robot does not place)."""
        f = self.f
        cand = candidates(q, targets, self.lo, self.hi, None, self.dt, reset, S, dtype=f)
        zero = np.zeros_like(q)
        D = np.asarray([self.observe(qk, zero, cube)[3].min() for qk in cand], dtype=f)       # numpy's min: a NaN wins
        steps = int(select(D[None], f(np.float32(margin)), np.asarray(reset, dtype=bool) | np.asarray(free, dtype=bool))[0])
        return dict(sweep_dist=D, steps=steps, targets=cand[steps], cand=cand)


def push_action(tip, cube):
    """The push script: translate the tips' midpoint towards cube + PUSH_OFFSET, gripper open."""
    a = np.zeros((tip.shape[0], 7), dtype=np.float32)
    a[:, :3] = np.clip((np.asarray(cube, dtype=np.float64) + np.asarray(PUSH_OFFSET) - np.asarray(tip, dtype=np.float64)) / 0.005, -1, 1)
    a[:, 6] = 1.0
    return a


def _episode(steps, dtype, S, margin, action, contact_hold, stop_after_success=None, actions=None):
    """kinematic_episode's loop with an optional guard (S None: none).  Entry t of the log is step t + 1: steps (parts taken, S when
    unguarded: None), sweep_dist, body_dist (3,) after the step, q, cube, hold (the flag the step was taken with), reached, success."""
    fx = Fixture(dtype)
    f = dtype
    q, qd = fx.default[None].copy(), np.zeros((1, fx.tree.num_dofs), dtype=f)
    cube = np.zeros((1, 13), dtype=f)
    cube[:, :7] = fx.cube0
    grip = np.zeros((1, 8), dtype=f)
    out, rb, p, body = fx.observe(q, qd, cube)
    hold = np.zeros(1, dtype=bool)
    touch = body <= f(np.float32(CE.MARGIN))
    if contact_hold:
        hold = np.asarray([touch[1] and touch[2]])
    st = dict(rew=p["rew"], success=p["success"], progress=np.zeros(1, dtype=np.int64), epis_max_rew=np.full(1, -100.0, dtype=f),
              epis_max_step=np.zeros(1, dtype=np.int64))
    log, done = [], None
    for t in range(steps):
        tip = (rb[:, fx.lt, :3] + rb[:, fx.rt, :3]) / 2
        a = actions[t] if actions is not None else action(tip, cube[:, :3], p["is_reached"], grip[:, 7] != 0)
        targets = G.control(a, np.stack([q, qd], axis=-1), out["jac"], fx.lt - 1, fx.rt - 1, fx.lo, fx.hi, fx.dt, "ik", dtype=f)
        bk = G.bookkeeping(st, targets, fx.default, E.EXPLORE_STEP, E.MAX_EPISODE_LENGTH, True)
        reset = bk["reset"]
        sw = None
        pos_act = bk["pos_act"]
        if S is not None:
            sw = fx.sweep(q, cube, pos_act, reset, hold, S, margin)
            pos_act = sw["targets"]
        q, qd = K.drive(q, pos_act, fx.lo, fx.hi, None, fx.dt, reset=reset, dtype=f)
        tips = K.rigid_rows(K.fk(fx.tree, q, qd, fx.base, dtype=f))
        cube, grip, _ = FB.step(tips[:, fx.lt], tips[:, fx.rt], cube, grip, hold, reset, fx.cube0, None, 0.15, E.DT, 0.025, 0.0, dtype=f,
                                f32_inputs=False)
        held = hold.copy()
        out, rb, p, body = fx.observe(q, qd, cube)
        if contact_hold:
            touch = body <= f(np.float32(CE.MARGIN))
            hold = np.asarray([touch[1] and touch[2]])
        st = dict(rew=p["rew"], success=p["success"], progress=bk["progress"] + 1, epis_max_rew=bk["epis_max_rew"],
                  epis_max_step=bk["epis_max_step"])
        log.append(dict(steps=None if sw is None else sw["steps"], sweep_dist=None if sw is None else sw["sweep_dist"], body_dist=body.copy(),
                        q=q[0].copy(), cube=cube[0].copy(), hold=bool(held[0]), reached=bool(p["is_reached"][0]),
                        success=bool(p["success"][0]), reset=bool(reset[0]), action=np.asarray(a)[0].copy()))
        if done is None and p["success"][0]:
            done = t
        if stop_after_success is not None and done is not None and t >= done + stop_after_success:
            break
    return log


def push_episode(steps, S=None, margin=0.0, dtype=np.float64, actions=None):
    """The push script, hold never set; S None: unguarded.  actions: None (the script closes its own loop) or a list of (1, 7)
    actions to replay (the float32 run replays the float64 run's, so that the two differ by round-off alone)."""
    return _episode(steps, dtype, S, margin, lambda tip, cube, reached, latched: push_action(tip, cube), False, actions=actions)


def grasp_episode(steps, S=None, margin=0.0, dtype=np.float64):
    """contact_episode.run_reference's episode (the contact predicate sets hold) with the guard in the loop, up to one step after
    success."""
    return _episode(steps, dtype, S, margin, E.script_action, True, stop_after_success=1)
