"""numpy restatement of the mobile Franka's drive, written from the contract in include/partmanip_hip.h
(pm_franka_control_mobile_f32) and sharing no code with partmanip_amd: used in float64 against the reference's fixtures
(tests/golden/make_mobile_franka_golden.py, tests/test_mobile_franka_host.py) and for several steps in a row
(tests/test_gpu_mobile_franka.py).  The episode bookkeeping is tests/grasp_cube_ref.bookkeeping and everything after physics and the
reset scatter are tests/open_drawer_ref.post / reset: they do not know how many DOFs or bodies the robot has.

`wrong` evaluates one of three deliberately wrong drives, so that the fixtures can show that each mobile-specific term is visible in
them: "no_transpose" turns the base action by base_R where the contract says base_R^T, "keep_dpose" leaves the base motion in the
pose error, "first_columns" takes the Jacobian columns [0, nd - 2 - nbase) where the contract says [nbase, nd - 2)."""
import numpy as np

from tests import grasp_cube_ref as G
from tests import open_drawer_ref as OD

WRONG = ("no_transpose", "keep_dpose", "first_columns")
NBASE = 3


def base_matrix(robot_default_root, dtype=np.float64):
    """base_R = quat_to_mat of the default root quaternion (x, y, z, w as stored: read as (i, j, k, r))."""
    return G.quat_to_mat(np.asarray(robot_default_root, dtype=dtype)[3:7])


def unclamped(actions, dof_state, jac, jl, jr, dt, drive_mode, base_R, nbase=NBASE, dtype=np.float64, wrong=None):
    """Joint targets (N, nd) before the clamp and before any reset."""
    assert wrong is None or wrong in WRONG
    c = lambda a: np.asarray(a, dtype=dtype)                   # noqa: E731
    a, q, R = c(actions), c(dof_state)[:, :, 0], c(base_R)
    nd = q.shape[1]
    na = nd - 2 - nbase
    t = np.empty_like(q)
    db = a[:, :3] * c(0.005)
    t[:, :nbase] = q[:, :nbase] + db @ (R.T if wrong == "no_transpose" else R)      # row e: R^T db[e]
    b = a[:, nbase:]
    if drive_mode == "ik":
        assert a.shape[1] == 7 + nbase
        dpose = b[:, :6] * c(0.005)
        if wrong != "keep_dpose":
            dpose[:, :3] -= db
        cols = slice(0, na) if wrong == "first_columns" else slice(nbase, nd - 2)
        J = (c(jac)[:, jl, :, cols] + c(jac)[:, jr, :, cols]) / 2
        A = J @ J.transpose(0, 2, 1) + np.eye(6, dtype=dtype) * c(0.05 ** 2)
        t[:, nbase:nd - 2] = q[:, nbase:nd - 2] + (J.transpose(0, 2, 1) @ np.linalg.solve(A, dpose[..., None]))[..., 0]
        t[:, nd - 2:] = q[:, nd - 2:] + b[:, 6:7] * c(dt) / 5
    elif drive_mode == "pos":
        assert a.shape[1] == nd - 1
        t[:, nbase:nd - 2] = q[:, nbase:nd - 2] + b[:, :na] * c(dt) * 20
        t[:, nd - 2:] = q[:, nd - 2:] + b[:, na:na + 1] * c(dt)
    else:
        raise ValueError(drive_mode)
    return t


def control(actions, dof_state, jac, jl, jr, dof_lo, dof_hi, dt, drive_mode, base_R, nbase=NBASE, dtype=np.float64, wrong=None):
    """Joint targets (N, nd), clamped, before any reset."""
    t = unclamped(actions, dof_state, jac, jl, jr, dt, drive_mode, base_R, nbase, dtype, wrong)
    return np.maximum(np.minimum(t, np.asarray(dof_hi, dtype=dtype)), np.asarray(dof_lo, dtype=dtype))


def post(fx, dtype=np.float64):
    """Everything after physics on a fixture (tests/open_drawer_ref.post)."""
    return OD.post(fx["rigid_body_all"], fx["dof_state_all"], fx["root"], fx["rigid_body_mask"], fx["dof_state_mask"], int(fx["obj_actor"]),
                   int(fx["ltip"]), int(fx["rtip"]), fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"],
                   fx["dof_lo"], fx["dof_hi"], fx["obj_id"], fx["before_succ_objid"], fx["part_slot"], fx["part_C"], dtype=dtype)


def begin_step(fx, after, drive, train, rnd, dtype=np.float64, wrong=None):
    """Restated begin_step on a fixture, `after` = post(fx): (bookkeeping dict, targets before the resets, root, dof_state_all,
    pos_act_all)."""
    jl, jr = int(fx["ltip"]) - 1, int(fx["rtip"]) - 1
    R = base_matrix(fx["robot_default_root"], dtype)
    tgt = control(fx["actions" if drive == "ik" else "actions_pos"], after["robot_dof_state"], fx["jac"], jl, jr, fx["dof_lo"], fx["dof_hi"],
                  float(fx["dt"]), drive, R, dtype=dtype, wrong=wrong)
    before = dict(rew=after["rew"], success=after["success"], progress=fx["before_progress"],
                  epis_max_rew=fx["before_epis_max_rew"].astype(dtype), epis_max_step=fx["before_epis_max_step"])
    s = G.bookkeeping(before, tgt, fx["default_dof_pos"].astype(dtype), int(fx["explore_step"]),
                      200 if train else int(fx["max_episode_length_test"]), train)
    root, dof, pa = OD.reset(s["reset"], s["pos_act"], fx["dof_state_mask"], fx["root"], fx["dof_state_all"], fx["pos_act_all_before"], 0,
                             int(fx["obj_actor"]), fx["robot_default_root"], fx["obj_default_root"], fx["default_dof_pos"],
                             fx["joint_lo"], fx["u"] if rnd else None, dtype=dtype)
    return s, tgt, root, dof, pa
