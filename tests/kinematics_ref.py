"""numpy evaluation of the kinematic articulation's contract (include/partmanip_hip.h, pm_articulation_step_f32) for the tests only:
4 x 4 homogeneous matrices and Rodrigues' formula, the origin rotations rebuilt from the tree's `rpy`, the ancestors found by walking
the parents.  It reads a KinematicTree's arrays and shares no code with partmanip_amd/urdf.py or the kernel (no quaternion
products, no ancestor masks).  `dtype` chooses the arithmetic: float64 for the checks, float32 for the reference's own error."""
import numpy as np

FIXED, REVOLUTE, PRISMATIC = 0, 1, 2


def rpy_matrix(rpy):
    """Fixed-axis roll-pitch-yaw, R = Rz(yaw) Ry(pitch) Rx(roll), float64."""
    r, p, y = (float(v) for v in rpy)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def quat_matrix(q, dtype):
    """Unit-normalised (x, y, z, w) -> (..., 3, 3)."""
    q = np.asarray(q, dtype=dtype)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def matrix_quat(R):
    """(..., 3, 3) -> (x, y, z, w) by the largest-pivot rule, in R's dtype; not renormalised, so | |q| - 1 | shows what R has lost."""
    R = np.asarray(R)
    flat = R.reshape(-1, 3, 3)
    out = np.empty((flat.shape[0], 4), dtype=R.dtype)
    one, quarter = R.dtype.type(1), R.dtype.type(0.25)
    for n, m in enumerate(flat):
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = np.sqrt(tr + one) * 2
            out[n] = ((m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, quarter * s)
        else:
            i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
            j, k = (i + 1) % 3, (i + 2) % 3
            s = np.sqrt(one + m[i, i] - m[j, j] - m[k, k]) * 2
            v = np.empty(4, dtype=R.dtype)
            v[i], v[j], v[k], v[3] = quarter * s, (m[j, i] + m[i, j]) / s, (m[k, i] + m[i, k]) / s, (m[k, j] - m[j, k]) / s
            out[n] = v
    return out.reshape(R.shape[:-2] + (4,))


def _hom(R, t, dtype):
    R, t = np.asarray(R), np.asarray(t)
    T = np.zeros(np.broadcast_shapes(R.shape[:-2], t.shape[:-1]) + (4, 4), dtype=dtype)
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = R, t, 1
    return T


def rodrigues(axis, theta, dtype):
    """Rotation by theta (N) about the unit axis (3): I + sin K + (1 - cos) K^2, (N, 3, 3)."""
    a = np.asarray(axis, dtype=dtype)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dtype)
    th = np.asarray(theta, dtype=dtype)[:, None, None]
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def ancestors(tree, b):
    """The bodies on b's path to the root whose joint moves, b included."""
    out = []
    while b >= 0:
        if tree.jtype[b] != FIXED:
            out.append(b)
        b = int(tree.parent[b])
    return out


def fk(tree, q, qd, base_pose, dtype=np.float64):
    """q, qd (N, nd), base_pose (7) or (N, 7) -> dict of pos (N, nb, 3), R (N, nb, 3, 3), jac (N, nb - 1, 6, nd), vel (N, nb, 6) =
    (linear, angular) = J qd, quat (N, nb, 4) = matrix_quat(R), all in dtype."""
    q, qd = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    N, nb, nd = q.shape[0], tree.num_bodies, tree.num_dofs
    bp = np.broadcast_to(np.asarray(base_pose, dtype=dtype), (N, 7))
    Tb = _hom(quat_matrix(bp[:, 3:], dtype), bp[:, :3], dtype)
    T, Tj = [None] * nb, [None] * nb                          # the body frames; the joint frames (parent o origin) before the joint moves
    for b in range(nb):
        p = int(tree.parent[b])
        To = _hom(rpy_matrix(tree.origin_rpy[b]).astype(dtype), np.asarray(tree.origin_t[b], dtype=dtype), dtype)
        Tj[b] = (Tb if p < 0 else T[p]) @ To
        d = int(tree.dof[b])
        if tree.jtype[b] == REVOLUTE:
            M = _hom(rodrigues(tree.axis[b], q[:, d], dtype), np.zeros(3, dtype=dtype), dtype)
        elif tree.jtype[b] == PRISMATIC:
            M = _hom(np.eye(3, dtype=dtype), q[:, d, None] * np.asarray(tree.axis[b], dtype=dtype)[None], dtype)
        else:
            M = np.eye(4, dtype=dtype)
        T[b] = Tj[b] @ M
    T = np.stack(T, axis=1)
    pos, R = T[:, :, :3, 3], T[:, :, :3, :3]
    J = np.zeros((N, nb, 6, nd), dtype=dtype)
    for b in range(nb):
        for jb in ancestors(tree, b):
            d = int(tree.dof[jb])
            a = Tj[jb][:, :3, :3] @ np.asarray(tree.axis[jb], dtype=dtype)
            if tree.jtype[jb] == REVOLUTE:
                J[:, b, :3, d] = np.cross(a, pos[:, b] - Tj[jb][:, :3, 3])
                J[:, b, 3:, d] = a
            else:
                J[:, b, :3, d] = a
    vel = np.einsum("nbrd,nd->nbr", J, qd)
    return dict(pos=pos, R=R, jac=J[:, 1:], vel=vel, quat=matrix_quat(R))


def clamp(v, lo, hi):
    """NaN passes through, as torch.clamp with scalar bounds."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.maximum(np.minimum(v, hi), lo))


def drive(q, t, lo, hi, vmax, dt, reset=None, dtype=np.float64):
    """The contract's drive: (q', qd') from positions q (N, nd) and targets t."""
    q, t, lo, hi = (np.asarray(a, dtype=dtype) for a in (q, t, lo, hi))
    dt = dtype(dt)
    if vmax is None:
        qn = t
    else:
        m = np.asarray(vmax, dtype=dtype) * dt
        qn = q + clamp(t - q, -m, m)
    qn = clamp(qn, lo, hi)
    qd = (qn - q) / dt
    if reset is not None:
        r = np.asarray(reset, dtype=bool)[:, None]
        qn, qd = np.where(r, clamp(t, lo, hi), qn), np.where(r, dtype(0), qd)
    return qn, qd


def rigid_rows(out):
    """The (N, nb, 13) rigid-body rows of an fk() result."""
    return np.concatenate([out["pos"], out["quat"], out["vel"]], axis=-1)
