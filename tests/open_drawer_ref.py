"""numpy restatement of the open_drawer task step, written from the contract in include/partmanip_hip.h (pm_open_drawer_post_f32,
pm_open_drawer_reset_f32) and sharing no code with partmanip_amd: used in float64 against the reference's fixtures
(tests/test_open_drawer_host.py) and for several steps in a row (tests/test_gpu_open_drawer.py).  The joint targets and the episode
bookkeeping are those of tests/grasp_cube_ref.py (control, bookkeeping): the drawer task uses the same launch for them."""
import numpy as np

from tests.grasp_cube_ref import norm, quat_to_mat, scale

EXTRAS = ("is_open", "is_open_notgrasp", "reaching_reward", "close_reward", "rot_reward", "joint_state_reward", "raw_reward",
          "is_grasped")
OBJ_DEFAULT_ROOT = np.array([-0.6, 0, 0.5, 0, 0, 1, 0], dtype=np.float64)
T_RANGE, R_RANGE, SUC_PROP = 0.05, np.pi / 12, 0.5


def quat_rotate(q, v):
    """v (2 w^2 - 1) + 2 w (q x v) + 2 q (q . v), q = (x, y, z, w) not normalised."""
    w, qv = q[..., 3:4], q[..., :3]
    return v * (2 * w * w - 1) + np.cross(qv, v) * w * 2 + qv * (qv * v).sum(-1, keepdims=True) * 2


def quat_mul(a, b):
    x1, y1, z1, w1 = (a[..., i] for i in range(4))
    x2, y2, z2, w2 = (b[..., i] for i in range(4))
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return np.stack([qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2), qq - zz + (z1 + y1) * (w2 - x2),
                     qq - ww + (z1 - y1) * (y2 - z2)], axis=-1)


def dot(a, b):
    return (a * b).sum(-1)


def post(rigid_body_all, dof_state_all, root, rigid_body_mask, dof_state_mask, obj_actor, ltip, rtip, bbox_init, axis_dir, joint_lo,
         joint_hi, dof_lo, dof_hi, obj_id, succ_objid_before, part_slot, part_C, suc_prop=SUC_PROP, dtype=np.float64):
    c = lambda a: np.asarray(a, dtype=dtype)                   # noqa: E731
    g = c(rigid_body_all)[np.asarray(rigid_body_mask)]         # (N, nrb + 2, 13)
    d = c(dof_state_all)[np.asarray(dof_state_mask)]           # (N, nd + 1, 2)
    obj = c(root)[:, obj_actor]
    N, nd = d.shape[0], d.shape[1] - 1
    L, Rt = g[:, ltip], g[:, rtip]
    tip = (L + Rt) / 2
    gl = norm(L[:, :3] - Rt[:, :3])
    q = d[:, nd, 0]
    bbox = (c(bbox_init) + q[:, None, None] * c(axis_dir)[:, None, :]) @ quat_to_mat(obj[:, 3:7]).transpose(0, 2, 1) + obj[:, None, :3]
    h_out, h_long, h_short = bbox[:, 0] - bbox[:, 4], bbox[:, 1] - bbox[:, 0], bbox[:, 3] - bbox[:, 0]
    mid = (bbox[:, 0] + bbox[:, 6]) / 2
    l_out, l_long, l_short = norm(h_out), norm(h_long), norm(h_short)
    h_out, h_long, h_short = h_out / l_out[:, None], h_long / l_long[:, None], h_short / l_short[:, None]
    qn = scale(d[:, :nd, 0], c(dof_lo), c(dof_hi))
    out = dict(normal_state=np.concatenate([tip, mid, h_out, h_short, h_long, l_out[:, None], l_long[:, None], l_short[:, None], qn,
                                            d[:, :nd, 1], q[:, None]], axis=1), part_bbox=bbox)
    delta = tip[:, :3] - mid
    r_out = np.abs(dot(delta, h_out)) < l_out / 2
    short_l, short_r = dot(L[:, :3] - mid, h_short), dot(Rt[:, :3] - mid, h_short)
    r_short = short_l * short_r < 0
    r_long = np.abs(dot(delta, h_long)) < l_long / 2
    reached = r_out & r_short & r_long
    reaching = -norm(delta) + c(0.1) * (r_out | r_short | r_long)
    eye = np.eye(3, dtype=dtype)
    axes = [quat_rotate(tip[:, 3:7], np.broadcast_to(eye[k], (N, 3))) for k in range(3)]
    down, sep, grip = axes
    rot = dot(-grip, h_out) + np.maximum(dot(sep, h_short), dot(-sep, h_short)) + np.maximum(dot(down, h_long), dot(-down, h_long)) - 3
    close = (c(0.1) - gl) * reached + c(0.1) * (gl - c(0.1)) * ~reached
    grasp = reached & (gl < l_short + c(0.01)) & (rot > c(-0.2))
    lo, hi = c(joint_lo), c(joint_hi)
    frac = (q - lo) / hi
    jsr = grasp * (c(0.1) + np.minimum(frac, c(suc_prop)))
    open_ng = frac > c(0.1)
    base = reaching + c(0.5) * rot + 5 * close + 5 * jsr
    succ = grasp & (q - lo >= c(suc_prop) * hi)
    rew = (base + np.abs(base) * rot + 2 * succ).astype(dtype)
    flags = np.array(succ_objid_before, dtype=bool, copy=True)
    flags[np.asarray(obj_id)[succ]] = True
    out.update(rew=rew, success=succ, is_reached=reached, succ_objid=flags, robot_dof_state=d[:, :nd], part_dof_state=d[:, nd],
               reach_flags=np.stack([r_out, r_short, r_long], axis=1), gripper_length=gl, short_length=l_short,
               short_product=short_l * short_r, half_margins=np.stack([np.abs(dot(delta, h_out)) - l_out / 2,
                                                                       np.abs(dot(delta, h_long)) - l_long / 2], axis=1),
               open_fraction=frac, travel=q - lo)
    out["extras"] = np.stack([(grasp & open_ng).astype(dtype), open_ng.astype(dtype), reaching, close, rot, jsr, rew,
                              grasp.astype(dtype)], axis=1).astype(dtype)
    ps = np.asarray(part_slot)
    out["pose_T"] = g[:, ps, :3]
    Rm = quat_to_mat(g[:, ps, 3:7])
    out["pose_R"] = Rm if part_C is None else np.einsum("bpij,pjk->bpik", Rm, c(part_C))
    return out


def reset(reset_flags, pos_act, dof_state_mask, root, dof_state_all, pos_act_all, robot_actor, obj_actor, robot_default_root,
          obj_default_root, default_dof_pos, joint_lo, u=None, dtype=np.float64):
    """The state half of reset_idx on copies: returns (root, dof_state_all, pos_act_all)."""
    c = lambda a: np.array(a, dtype=dtype, copy=True)          # noqa: E731
    root, dof, pa = c(root), c(dof_state_all), c(pos_act_all)
    m = np.asarray(dof_state_mask)
    nd = m.shape[1] - 1
    pa[m[:, :nd]] = np.asarray(pos_act, dtype=dtype)
    ids = np.nonzero(np.asarray(reset_flags))[0]
    root[ids, :, 7:] = 0
    root[ids, robot_actor, :7] = c(robot_default_root)
    root[ids, obj_actor, :7] = c(obj_default_root)
    if u is not None:
        uu = np.asarray(u, dtype=dtype)[ids]
        t, r = np.asarray(T_RANGE, dtype=dtype), np.asarray(R_RANGE, dtype=dtype)
        root[ids, obj_actor, :3] += uu[:, :3] * t * 2 - t
        ang = uu[:, 3] * r * 2 - r
        rnd = np.stack([np.zeros_like(ang), np.zeros_like(ang), np.sin(ang), np.cos(ang)], axis=-1)
        root[ids, obj_actor, 3:7] = quat_mul(np.broadcast_to(c(obj_default_root)[3:7], rnd.shape), rnd)
    dof[m[ids, :nd], 0] = c(default_dof_pos)
    dof[m[ids, nd], 0] = np.asarray(joint_lo, dtype=dtype)[ids]
    dof[m[ids], 1] = 0
    return root, dof, pa
