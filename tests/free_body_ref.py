"""numpy statement of the free body's step, written from the contract in include/partmanip_hip.h (pm_free_body_step_f32) for the tests
only: rotation matrices for the hand frame and the scalar / vector form of the quaternion product, over all environments at once.  It
shares no code with partmanip_amd or the kernel.  `dtype` chooses the arithmetic: float64 for the checks, float32 for the reference's
own error.  Values the contract keeps (a pose that stays, the left tip's angular velocity, the default pose) are copied, not computed."""
import numpy as np

RESET, LATCH, CARRY, FREE = 1, 2, 3, 4


def qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions: the rotation b, then a."""
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], axis=-1)


def unit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def matrix(q):
    """Unit (x, y, z, w) -> (..., 3, 3)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def case_of(hold, reset, grip):
    hold, reset, latched = np.asarray(hold, dtype=bool), np.asarray(reset, dtype=bool), np.asarray(grip)[:, 7] != 0
    return np.where(reset, RESET, np.where(hold & ~latched, LATCH, np.where(hold, CARRY, FREE)))


def step(tip_l, tip_r, body, grip, hold, reset, default_pose, u, reset_range, dt, rest_z, fall_speed, dtype=np.float64, f32_inputs=True):
    """tip_l, tip_r, body (N, 13) float32 rows (body = root[:, obj_actor]), grip (N, 8) -> (row (N, 13), grip (N, 8), case (N)) in
    dtype.  dt, reset_range, rest_z and fall_speed are taken as the float32 numbers the C entry receives.  f32_inputs=False takes
    the arrays as they come (a closed loop that stays in dtype from step to step)."""
    c = (lambda a: np.asarray(a, dtype=np.float32).astype(dtype)) if f32_inputs else (lambda a: np.asarray(a, dtype=dtype))   # noqa: E731
    L, R, b, g, d0 = c(tip_l), c(tip_r), c(body), c(grip), c(default_pose)
    dt, rng, zr, fs = (dtype(np.float32(v)) for v in (dt, reset_range, rest_z, fall_speed))
    N = b.shape[0]
    case = case_of(hold, reset, grip)
    row, gout = b.copy(), g.copy()
    row[:, 7:] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (L[:, :3] + R[:, :3]) / 2
        qh = unit(L[:, 3:7])
        RH = matrix(qh)
        # 1. reset
        r = case == RESET
        pose = np.broadcast_to(d0, (N, 7)).copy()
        if u is not None:
            uu = c(u)
            pose[:, :2] = d0[:2] + (2 * uu[:, :2] - 1) * rng
            th = 2 * dtype(np.pi) * uu[:, 2] - dtype(np.pi)
            yaw = np.stack([np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype), np.sin(th), np.cos(th)], axis=1)
            pose[:, 3:] = qmul(np.broadcast_to(d0[3:], (N, 4)), yaw)
        row[r, :7] = pose[r]
        gout[r, 7] = 0
        # 2. latch
        m = case == LATCH
        conj = qh * np.array([-1, -1, -1, 1], dtype=dtype)
        rel_t = np.einsum("nji,nj->ni", RH, b[:, :3] - p)
        rel_q = qmul(conj, b[:, 3:7])
        gout[m, :3], gout[m, 3:7], gout[m, 7] = rel_t[m], rel_q[m], 1
        # 3. carry
        k = case == CARRY
        cn = p + np.einsum("nij,nj->ni", RH, g[:, :3])
        qn = unit(qmul(qh, g[:, 3:7]))
        row[k, :3], row[k, 3:7] = cn[k], qn[k]
        row[k, 7:10] = ((cn - b[:, :3]) / dt)[k]
        row[k, 10:] = L[k, 10:]
        # 4. released
        f = case == FREE
        sink = f & (b[:, 2] > zr)
        zn = np.maximum(zr, b[:, 2] - fs * dt)
        row[sink, 2] = zn[sink]
        row[sink, 9] = ((zn - b[:, 2]) / dt)[sink]
        gout[f, 7] = 0
    return row, gout, case
