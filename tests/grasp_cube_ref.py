"""numpy restatement of the grasp_cube task step, written from the contract in include/partmanip_hip.h (pm_grasp_cube_post_f32,
pm_franka_control_f32) and sharing no code with partmanip_amd: used in float64 against the reference's fixtures
(tests/test_grasp_cube_host.py) and for the bookkeeping of several steps in a row (tests/test_gpu_grasp_cube.py).

Every function takes and returns numpy arrays; `dtype` chooses the arithmetic (float64 for the checks, float32 where a test wants
the reference's own precision).  The IK solve uses numpy.linalg.solve (LU), not the kernel's Cholesky."""
import numpy as np

IND = np.array([[0, 1], [0, 2], [1, 2], [1, 0], [2, 0], [2, 1]] * 4)
EXTRAS = ("reaching_reward", "close_reward", "rot_reward", "reaching_goal_reward", "obj_movement", "raw_reward", "obj_height",
          "obj_up_flag")
POSE_LO = np.array([-0.15, -0.15, 0.0, -1, -1, -1, -1], dtype=np.float64)
POSE_HI = np.array([0.15, 0.15, 0.4, 1, 1, 1, 1], dtype=np.float64)


def quat_to_mat(q):
    """(..., 4) in the order (i, j, k, r), two_s = 2 / sum q^2, no normalisation -> (..., 3, 3)."""
    i, j, k, r = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = 2.0 / (((i * i + j * j) + k * k) + r * r)
    m = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def candidates(q):
    """The 24 candidate rotations (N, 24, 3, 3) of the contract and their traces (N, 24)."""
    R = quat_to_mat(q)
    two = R[:, :, IND].transpose(0, 2, 1, 3).copy()           # (N, 24, 3 rows, 2 columns)
    two[:, :12, 0] *= -1
    two[:, 6:18, 1] *= -1
    third = np.cross(two[..., 0], two[..., 1], axis=-1)
    cand = np.concatenate([two, third[..., None]], axis=-1)
    return cand, cand[..., 0, 0] + cand[..., 1, 1] + cand[..., 2, 2]


def deambiguity_rotation(q):
    cand, tr = candidates(q)
    return cand[np.arange(len(q)), np.argmax(tr, axis=1)]      # argmax: the first of equal maxima


def scale(x, lo, hi):
    return 2 * (x - lo) / (hi - lo) - 1


def norm(v):
    return np.sqrt((v * v).sum(-1))


def post(rigid_body, dof_state, root, obj_actor, ltip, rtip, dof_lo, dof_hi, goal, goal_thresh, obj_default_pos, part_body, part_C,
         dtype=np.float64):
    c = lambda a: np.asarray(a, dtype=dtype)                   # noqa: E731
    rb, dof, root = c(rigid_body), c(dof_state), c(root)
    lo, hi, dlo, dhi = c(POSE_LO), c(POSE_HI), c(dof_lo), c(dof_hi)
    N = rb.shape[0]
    L, Rt = rb[:, ltip], rb[:, rtip]
    tip = (L + Rt) / 2
    gl = norm(L[:, :3] - Rt[:, :3])
    obj = root[:, obj_actor]
    tip_s = scale(tip[:, :7], lo, hi)
    obj_s = scale(obj[:, :3], lo[:3], hi[:3])
    o = deambiguity_rotation(obj[:, 3:7])
    qn = scale(dof[:, :, 0], dlo, dhi)
    qv = dof[:, :, 1]
    out = dict(normal_state=np.concatenate([tip_s, obj_s, o.reshape(N, 9), qn, qv], axis=1),
               proprio=np.concatenate([tip_s, qn, qv], axis=1))
    dist = norm(tip[:, :3] - obj[:, :3])
    reached = dist < 0.02
    reaching = -dist
    close = np.where(reached, c(0.1) - gl, c(0.1) * (gl - c(0.1)))
    h = quat_to_mat(tip[:, 3:7])
    down = -h[:, 2, 2]
    p1 = (np.abs(h[:, :, 0] * o[:, :, 0]) + np.abs(h[:, :, 1] * o[:, :, 1])).sum(-1)
    p2 = (np.abs(h[:, :, 0] * o[:, :, 1]) + np.abs(h[:, :, 1] * o[:, :, 0])).sum(-1)
    rot = down + np.maximum(p1, p2) - 3
    dgoal = norm(obj[:, :3] - c(goal))
    rgoal = np.maximum(c(0.2) - dgoal, 0) * reached
    succ = (dgoal <= goal_thresh) & reached
    rew = reaching + c(0.5) * rot + 5 * close + 20 * rgoal + 3 * succ
    out.update(rew=rew.astype(dtype), success=succ, is_reached=reached)
    out["extras"] = np.stack([reaching, close, rot, rgoal, norm(obj[:, :3] - c(obj_default_pos)), rew, obj[:, 2],
                              (obj[:, 2] > 0.1).astype(dtype)], axis=1).astype(dtype)
    pb = np.asarray(part_body)
    out["pose_T"] = rb[:, pb, :3]
    Rm = quat_to_mat(rb[:, pb, 3:7])
    out["pose_R"] = Rm if part_C is None else np.einsum("bpij,pjk->bpik", Rm, c(part_C))
    return out


def control(actions, dof_state, jac, jl, jr, dof_lo, dof_hi, dt, drive_mode, dtype=np.float64):
    """Joint targets (N, nd) before any reset."""
    c = lambda a: np.asarray(a, dtype=dtype)                   # noqa: E731
    a, q, lo, hi = c(actions), c(dof_state)[:, :, 0], c(dof_lo), c(dof_hi)
    nd = q.shape[1]
    na = nd - 2
    t = np.empty_like(q)
    if drive_mode == "ik":
        J = (c(jac)[:, jl, :, :na] + c(jac)[:, jr, :, :na]) / 2
        A = J @ J.transpose(0, 2, 1) + np.eye(6, dtype=dtype) * c(0.05 ** 2)
        u = (J.transpose(0, 2, 1) @ np.linalg.solve(A, (a[:, :6] * c(0.005))[..., None]))[..., 0]
        t[:, :na] = q[:, :na] + u
        t[:, na:] = q[:, na:] + (a[:, 6:7] * c(dt) / 5)
    elif drive_mode == "pos":
        t[:, :na] = q[:, :na] + a[:, :na] * c(dt) * 20
        t[:, na:] = q[:, na:] + a[:, na:na + 1] * c(dt)
    else:
        raise ValueError(drive_mode)
    return np.maximum(np.minimum(t, hi), lo)


def bookkeeping(state, targets, default_dof_pos, explore_step, max_episode_length, train):
    """state: dict of rew, success, progress, epis_max_rew, epis_max_step (numpy, not modified) -> the dict after the step with
    pos_act, reset, reset_succ (None in test mode), n_succ, n_reset, succ_rate added."""
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    rew, succ, prog = s["rew"], s["success"].astype(bool), s["progress"].astype(np.int64)
    ems, emr = s["epis_max_step"].astype(np.int64), s["epis_max_rew"]
    if train:
        ems = np.where(rew < emr, ems, prog)
        emr = np.maximum(rew, emr)
        reset = (prog >= ems + explore_step) | succ
        reset_succ = succ.copy()
    else:
        reset = prog >= max_episode_length
        reset_succ = None
    n_succ, n_reset = int(succ.sum()), int(reset.sum())
    pos_act = np.where(reset[:, None], np.asarray(default_dof_pos, dtype=targets.dtype)[None], targets)
    return dict(rew=rew, success=succ & ~reset, progress=np.where(reset, 0, prog), epis_max_rew=np.where(reset, -100, emr).astype(emr.dtype),
                epis_max_step=np.where(reset, 0, ems), pos_act=pos_act, reset=reset, reset_succ=reset_succ, n_succ=n_succ,
                n_reset=n_reset, succ_rate=np.float32(n_succ) / np.float32(max(n_reset, 1)))
