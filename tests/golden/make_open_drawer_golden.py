"""Dev-machine generator of the open_drawer task-step fixtures (tests/test_open_drawer_host.py, tests/test_gpu_open_drawer.py): runs
the REFERENCE's own open_drawer.compute_observations, franka.update_state, open_drawer.compute_reward, hand_base.pre_physics_step and
open_drawer.reset_idx on the CPU, once in float32 and once in float64.

    python tests/golden/make_open_drawer_golden.py /path/to/reference

As in make_grasp_cube_golden.py the reference's modules are loaded by file path with stand-in isaacgym modules written here
(tensor_clamp, quat_conjugate, quat_mul and quat_rotate after Isaac Gym's public formulas, a gym whose every method does nothing) and
PYTORCH_JIT=0; task and robot are built with object.__new__ and their attributes set by hand.  The index tables are built the way
open_drawer.py:58-70 builds them.  With random_reset the reference draws torch.rand twice inside reset_idx, (n, 3) then (n,), n the
number of resetting environments: torch.rand is patched for that call so that it hands out the rows of the fixture's `u` (N, 4)
that belong to the resetting environments.

Writes open_drawer_ref_small.npz (N = 5) and open_drawer_ref_70.npz (N = 70): nrb = 13, nd = 9, three object types with (bodies,
DOFs) = (3, 1), (5, 3), (4, 2), environment i of type i mod 3.  Contents: the inputs, out32_* / out64_* per output group of the post
step, and for each of the four pre-physics runs RUNS (drive, mode, random_reset) the groups <run>_pos_act_all, <run>_root,
<run>_dof_state_all with the flags and counters.  The conditions the fixtures must meet (asserted here and again on the committed
files by tests/test_open_drawer_host.py) are in check_conditions."""
import os
os.environ["PYTORCH_JIT"] = "0"                               # before torch is imported
import importlib.util  # noqa: E402
import sys  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import open_drawer_ref as OD  # noqa: E402

NRB, ND, NA, NL, LTIP, RTIP, ROBOT_ACTOR, OBJ_ACTOR = 13, 9, 2, 12, 10, 12, 0, 1
DT = 1.0 / 60.0
DOF_LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0], dtype=np.float32)
DOF_HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04], dtype=np.float32)
DEFAULT_DOF = np.array([0.3, -0.4, -0.3, -2.2, -0.1, 2.0, -0.5, 0.04, 0.04], dtype=np.float32)
ROBOT_ROOT = np.array([0.3, -0.1, 0.05, 0, 0, 0.6, 0.8], dtype=np.float32)
OBJ_ROOT = np.array([-0.6, 0, 0.5, 0, 0, 1, 0], dtype=np.float32)
# object types: (bodies, DOFs, target link, target handle, target joint)
TYPES = ((3, 1, 1, 2, 0), (5, 3, 2, 4, 2), (4, 2, 3, 1, 1))
NUM_OBJS = 3
# what an environment shows, by type and by its index within the type (see make_inputs); only type 0 ever succeeds
KINDS = ((0, 4, 0, 6), (1, 5, 2, 1), (3, 7, 3, 1))
EXPLORE_STEP, MAX_EPISODE_LENGTH_TEST = 40, 60
CASES = (("open_drawer_ref_small", 5, 6101), ("open_drawer_ref_70", 70, 6102))
RUNS = (("ik_train", "ik", "train", False), ("ik_test_rand", "ik", "test", True), ("pos_train_rand", "pos", "train", True),
        ("pos_test", "pos", "test", False))
MARGIN = 1e-4
FLOAT_GROUPS = ("normal_state", "part_bbox", "rew", "extras", "pose_R", "pose_T")
RUN_FLOAT_GROUPS = ("pos_act_all", "root", "dof_state_all", "after_epis_max_rew")
RUN_INT_KEYS = ("reset", "after_progress", "after_success", "after_epis_max_step")


def part_defaults():
    C = np.zeros((13, 3, 3), dtype=np.float32)
    C[:, 0, 0] = 1
    C[:11, 1, 2] = -1
    C[:11, 2, 1] = 1
    C[10, 1, 2] = 1
    C[11] = C[12] = np.eye(3)
    return np.array(list(range(10)) + [NRB - 2, NRB, NRB + 1], dtype=np.int32), C


def build_masks(N):
    """open_drawer.py:58-70 with obj_lstid = i mod 3."""
    dof_mask = np.zeros((N, ND + 1), dtype=np.int64)
    rb_mask = np.zeros((N, NRB + 2), dtype=np.int64)
    dof_count = rigid_count = 0
    for i in range(N):
        nb, ndof, link, handle, joint = TYPES[i % 3]
        dof_mask[i, :ND] = np.arange(dof_count, dof_count + ND)
        dof_mask[i, -1] = dof_count + ND + joint
        rb_mask[i, :NRB] = np.arange(rigid_count, rigid_count + NRB)
        rb_mask[i, -2] = rigid_count + NRB + link
        rb_mask[i, -1] = rigid_count + NRB + handle
        dof_count += ND + ndof
        rigid_count += NRB + nb
    return rb_mask, dof_mask, rigid_count, dof_count


def unit(rng, *shape):
    v = rng.normal(size=shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return OD.quat_to_mat(q[None])[0], q


def rotvec(axis, ang):
    """Rodrigues: the rotation by ang about the unit vector axis."""
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def mat_to_quat(R):
    """(x, y, z, w) of a rotation matrix, the branch of the largest diagonal term."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def make_inputs(N, seed):
    rng = np.random.RandomState(seed)
    rb_mask, dof_mask, B, D = build_masks(N)
    rb = np.zeros((B, 13))
    rb[:, :3] = rng.uniform(-0.8, 0.8, size=(B, 3))
    q = rng.normal(size=(B, 4))
    rb[:, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    rb[:, 7:] = rng.normal(size=(B, 6)) * 0.3
    dof = np.zeros((D, 2))
    dof[:, 0] = rng.uniform(0.0, 0.3, size=D)                 # the cabinets' other joints; the robot's rows are set below
    dof[:, 1] = rng.normal(size=D) * 0.5
    mid, span = (DOF_LO + DOF_HI) / 2.0, (DOF_HI - DOF_LO) / 2.0
    dof[dof_mask[:, :ND], 0] = mid + span * rng.uniform(-0.9, 0.9, size=(N, ND))
    root = np.zeros((N, NA, 13))
    root[:, ROBOT_ACTOR, :7] = ROBOT_ROOT + rng.normal(size=(N, 7)) * 0.01
    root[:, :, 7:] = rng.normal(size=(N, NA, 6)) * 0.1
    bbox = np.zeros((N, 8, 3))
    axis = np.zeros((N, 3))
    lo = rng.uniform(0.0, 0.02, size=N)
    hi = rng.uniform(0.15, 0.4, size=N)
    kind = np.array([KINDS[i % 3][(i // 3) % 4] for i in range(N)])
    for i in range(N):
        k = kind[i]
        Ro, qo = rand_rot(rng)
        pos = OBJ_ROOT[:3] + rng.uniform(-0.05, 0.05, size=3)
        root[i, OBJ_ACTOR, :3], root[i, OBJ_ACTOR, 3:7] = pos, qo
        # the handle box in the object's frame: right-handed frame (o, l, s), half sizes, centre
        F, _ = rand_rot(rng)
        o, l, s = F[:, 0], F[:, 1], F[:, 2]
        ho, hl, hs = rng.uniform(0.015, 0.03), rng.uniform(0.05, 0.1), rng.uniform(0.012, 0.02)
        c0 = rng.uniform(-0.2, 0.2, size=3)
        b0 = c0 + o * ho - l * hl - s * hs
        b4 = b0 - 2 * ho * o
        bbox[i] = [b0, b0 + 2 * hl * l, b0 + 2 * hl * l + 2 * hs * s, b0 + 2 * hs * s, b4, b4 + 2 * hl * l, b4 + 2 * hl * l + 2 * hs * s,
                   b4 + 2 * hs * s]
        ax = o + rng.normal(size=3) * 0.1
        axis[i] = ax / np.linalg.norm(ax)
        frac = {0: rng.uniform(0.55, 0.9), 1: rng.uniform(0.15, 0.45), 2: rng.uniform(0.01, 0.08), 3: rng.uniform(0.15, 0.8),
                4: rng.uniform(0.01, 0.08), 5: rng.uniform(0.15, 0.9), 6: rng.uniform(0.6, 0.9), 7: rng.uniform(0.01, 0.08)}[k]
        qj = lo[i] + frac * hi[i]
        dof[dof_mask[i, ND], 0] = qj
        ow, lw, sw = Ro @ o, Ro @ l, Ro @ s
        centre = Ro @ (c0 + qj * axis[i]) + pos
        # where the tool centre sits in the handle frame, as fractions of the lengths (reached: |.| < 0.5), and the short offset
        fo, fl = rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35)
        ts = rng.uniform(-0.003, 0.003)
        gap = rng.uniform(0.026, 2 * hs + 0.008)              # grasped: below the handle's width + 0.01
        aligned = True
        if k == 3:
            if (i // 3) % 8 < 4:
                gap = 2 * hs + 0.01 + rng.uniform(0.005, 0.03)    # reached, gripper too wide
            else:
                aligned = False                               # reached, hand turned away
        if k == 4:
            fo = rng.choice([-1, 1]) * rng.uniform(0.7, 1.5)   # past the handle along `out` only
        if k == 5:
            ts = rng.choice([-1, 1]) * (gap / 2 + rng.uniform(0.01, 0.03))     # both tips on one side along `short`, and past `long`
            fl = rng.choice([-1, 1]) * rng.uniform(0.7, 1.2)
        if k == 6:
            fl = rng.choice([-1, 1]) * rng.uniform(0.7, 1.2)   # past the handle along `long` only
        if k == 7:
            fo, fl = rng.uniform(2, 6), rng.uniform(1.5, 3)    # far away: only the two tips still straddle the handle
        tcp = centre + fo * 2 * ho * ow + fl * 2 * hl * lw + ts * sw
        d = sw + rng.normal(size=3) * 0.05
        d /= np.linalg.norm(d)
        rb[rb_mask[i, LTIP], :3], rb[rb_mask[i, RTIP], :3] = tcp + d * gap / 2, tcp - d * gap / 2
        # the hand: x = down = +-long, y = sep = +-short, z = grip = -out, turned by a small angle
        H = np.stack([lw, sw, -ow], axis=1)
        if np.linalg.det(H) < 0:
            H[:, 0] = -H[:, 0]
        if rng.randint(2):
            H[:, :2] = -H[:, :2]
        H = rotvec(unit(rng), rng.uniform(0.02, 0.2) if aligned else rng.uniform(0.8, 2.5)) @ H
        qh = mat_to_quat(H)
        ql = qh + rng.normal(size=4) * 0.02
        qr = qh + rng.normal(size=4) * 0.02
        rb[rb_mask[i, LTIP], 3:7], rb[rb_mask[i, RTIP], 3:7] = ql / np.linalg.norm(ql), qr / np.linalg.norm(qr)
    jac = np.zeros((N, NL, 6, ND))                             # only the two tip links are ever read; zeros keep the file small
    jac[:, [LTIP - 1, RTIP - 1]] = rng.normal(size=(N, 2, 6, ND))
    part_slot, part_C = part_defaults()
    u_step = (np.cumsum(kind != 0) % 2).astype(np.int64)       # live episodes alternate between timed out and running
    progress = np.where(u_step == 1, rng.randint(61, 100, size=N), rng.randint(1, 100, size=N)).astype(np.int64)
    u = rng.uniform(0.02, 0.45, size=(N, 4))                   # pairs (2 j, 2 j + 1) alternate sides of 0.5, column by column
    flip = (np.arange(N)[:, None] // 2 + np.arange(4)[None, :]) % 2 == 1
    u[flip] = 1 - u[flip]
    succ_before = np.array([False, False, True])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)   # noqa: E731
    return dict(rigid_body_all=f(rb), dof_state_all=f(dof), root=f(root), rigid_body_mask=i32(rb_mask), dof_state_mask=i32(dof_mask),
                obj_id=i32(np.arange(N) % 3), num_objs=np.int64(NUM_OBJS), part_bbox_init=f(bbox), part_axis_dir_init=f(axis),
                joint_lo=f(lo), joint_hi=f(hi), jac=f(jac), actions=f(rng.uniform(-1, 1, size=(N, 7))),
                actions_pos=f(rng.uniform(-1, 1, size=(N, 8))), dof_lo=DOF_LO, dof_hi=DOF_HI, default_dof_pos=DEFAULT_DOF,
                robot_default_root=ROBOT_ROOT, obj_default_root=OBJ_ROOT, dt=np.float64(DT), part_slot=part_slot, part_C=part_C,
                ltip=np.int64(LTIP), rtip=np.int64(RTIP), obj_actor=np.int64(OBJ_ACTOR), explore_step=np.int64(EXPLORE_STEP),
                max_episode_length_test=np.int64(MAX_EPISODE_LENGTH_TEST), before_progress=progress, kind=kind.astype(np.int64),
                before_succ_objid=succ_before, u=f(u), pos_act_all_before=f(rng.uniform(-9, -8, size=D)),
                u_rew=f(rng.uniform(0.05, 1.0, size=N)), u_sign=rng.randint(0, 2, size=N).astype(np.int64), u_step=u_step)


def bookkeeping_before(inp, rew64):
    """epis_max_rew well away from the reward on either side; epis_max_step so that timeouts and live episodes both occur."""
    prog = inp["before_progress"]
    emr = (rew64 + np.where((inp["u_sign"] == 1) | (inp["u_step"] == 1), 1.0, -1.0) * inp["u_rew"]).astype(np.float32)
    ems = np.where(inp["u_step"] == 1, np.maximum(prog - EXPLORE_STEP - 3, 0), np.maximum(prog - 5, 0)).astype(np.int64)
    return emr, ems


def load_reference(root):
    class AnyGym:
        def __getattr__(self, name):
            return lambda *a, **k: None

    ig = types.ModuleType("isaacgym")
    ig.gymapi, ig.gymtorch, tu = types.ModuleType("isaacgym.gymapi"), types.ModuleType("isaacgym.gymtorch"), types.ModuleType("isaacgym.torch_utils")
    ig.gymtorch.unwrap_tensor = lambda t: t
    tu.tensor_clamp = lambda t, lo, hi: torch.max(torch.min(t, hi), lo)
    tu.quat_conjugate = lambda a: torch.cat((-a[..., :3], a[..., 3:]), dim=-1)

    def quat_mul(a, b):
        x1, y1, z1, w1 = a.unbind(-1)
        x2, y2, z2, w2 = b.unbind(-1)
        ww = (z1 + x1) * (x2 + y2)
        yy = (w1 - y1) * (w2 + z2)
        zz = (w1 + y1) * (w2 - z2)
        xx = ww + yy + zz
        qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
        return torch.stack([qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2), qq - zz + (z1 + y1) * (w2 - x2),
                            qq - ww + (z1 - y1) * (y2 - z2)], dim=-1)

    def quat_rotate(q, v):
        shape = q.shape
        q_w, q_vec = q[:, -1], q[:, :3]
        a = v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1)
        b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
        c = q_vec * torch.bmm(q_vec.view(shape[0], 1, 3), v.view(shape[0], 3, 1)).squeeze(-1) * 2.0
        return a + b + c

    tu.quat_mul, tu.quat_rotate = quat_mul, quat_rotate
    ig.torch_utils = tu
    utils, tasks = types.ModuleType("utils"), types.ModuleType("tasks")
    utils.TSDFVolume = utils.gen_camera_pose = utils.TSDFfromMesh = None
    utils.__path__, tasks.__path__ = [], []
    sys.modules.update({"isaacgym": ig, "isaacgym.gymapi": ig.gymapi, "isaacgym.gymtorch": ig.gymtorch, "isaacgym.torch_utils": tu,
                        "utils": utils, "tasks": tasks})
    mods = {}
    for name, rel in (("utils.torch_jit_utils", "utils/torch_jit_utils.py"), ("tasks.load_robot", "tasks/load_robot.py"),
                      ("tasks.hand_base", "tasks/hand_base.py"), ("tasks.open_drawer", "tasks/open_drawer.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods, AnyGym()


def build_task(mods, gym, inp, dt, drive_mode, train_test, max_episode_length, random_reset):
    """An open_drawer task and its franka robot without their constructors; tensors of dtype dt."""
    N = inp["root"].shape[0]
    T = lambda a: torch.from_numpy(np.array(a)).to(dt)        # noqa: E731
    robot = object.__new__(mods["tasks.load_robot"].franka)
    robot.gym, robot.device, robot.num_envs, robot.dt, robot.driveMode, robot.mobile = gym, "cpu", N, float(inp["dt"]), drive_mode, False
    robot.num_dofs, robot.num_rigid_body, robot.ltip_rb_index, robot.rtip_rb_index = ND, NRB, LTIP, RTIP
    robot.dof_lower_limits_tensor, robot.dof_upper_limits_tensor = T(inp["dof_lo"]), T(inp["dof_hi"])
    robot.default_dof_pos, robot.default_root = T(inp["default_dof_pos"]), T(inp["robot_default_root"])
    robot.action_tensor = torch.zeros(N, ND, dtype=dt)
    robot.jacobian_tensor = T(inp["jac"])
    task = object.__new__(mods["tasks.open_drawer"].open_drawer)
    task.gym, task.sim, task.device, task.num_envs, task.robot = gym, None, "cpu", N, robot
    task.rigid_body_tensor_all, task.dof_state_tensor_all, task.root_tensor = T(inp["rigid_body_all"]), T(inp["dof_state_all"]), T(inp["root"])
    task.rigid_body_mask = torch.from_numpy(inp["rigid_body_mask"].astype(np.int64))
    task.dof_state_mask = torch.from_numpy(inp["dof_state_mask"].astype(np.int64))
    task.obj_actor, task.obs_buf, task.extras = OBJ_ACTOR, {}, {}
    task.part_bbox_init, task.part_axis_dir_init = T(inp["part_bbox_init"]), T(inp["part_axis_dir_init"])
    task.part_joint_lower_limits, task.part_joint_upper_limits = T(inp["joint_lo"]), T(inp["joint_hi"])
    task.obj_lstid_lst = torch.from_numpy(inp["obj_id"].astype(np.int64))
    task.suc_prop = 0.5
    task.succ_objid_lst = torch.from_numpy(inp["before_succ_objid"].copy())
    task.obj_default_root = T(inp["obj_default_root"])
    task.random_reset, task.reset_t_range, task.reset_r_range = random_reset, 0.05, np.pi / 12
    task.progress_buf = torch.from_numpy(inp["before_progress"].copy())
    task.train_test_flag, task.explore_step, task.max_episode_length = train_test, EXPLORE_STEP, max_episode_length
    task.success = torch.zeros(N, dtype=torch.bool)
    task.pos_act = torch.zeros(N, ND, dtype=dt)
    task.pos_act_all = T(inp["pos_act_all_before"])
    task.global_indices = torch.arange(N * 2, dtype=torch.int32).view(N, -1)
    task.reset_buf = torch.zeros(N, dtype=torch.long)
    task.reset_succ = torch.zeros(N, dtype=torch.bool)
    task.rew_buf = torch.zeros(N, dtype=dt)
    return task


def run_reference(mods, gym, inp, dt, emr_ems=None):
    """One post step, then the pre-physics runs RUNS; returns numpy outputs."""
    out = {}
    n = lambda t: t.detach().numpy().copy()                   # noqa: E731
    task = build_task(mods, gym, inp, dt, "ik", "train", 200, False)
    task.compute_observations()
    out["normal_state"], out["part_bbox"] = n(task.obs_buf["normal_state"]), n(task.part_bbox)
    task.compute_reward(None)
    out["rew"], out["success"], out["is_reached"] = n(task.rew_buf), n(task.success), n(task.extras["is_reached"])
    out["extras"] = np.stack([n(task.extras[k]).astype(out["rew"].dtype) for k in OD.EXTRAS], axis=1)
    out["succ_objid"] = n(task.extras["success_objnum"])
    qm = mods["utils.torch_jit_utils"].quat_to_mat
    g = task.rigid_body_tensor[:, torch.from_numpy(inp["part_slot"].astype(np.int64))]
    out["pose_T"] = n(g[:, :, :3])
    out["pose_R"] = n(torch.matmul(qm(g[:, :, 3:7]), torch.from_numpy(inp["part_C"]).to(dt).unsqueeze(0)))
    if emr_ems is None:
        return out
    rew, succ = task.rew_buf.clone(), task.success.clone()
    for name, drive, mode, rnd in RUNS:
        t2 = build_task(mods, gym, inp, dt, drive, mode, 200 if mode == "train" else MAX_EPISODE_LENGTH_TEST, rnd)
        t2.compute_observations()
        t2.rew_buf, t2.success = rew.clone(), succ.clone()
        t2.epis_max_rew, t2.epis_max_step = torch.from_numpy(emr_ems[0].copy()).to(dt), torch.from_numpy(emr_ems[1].copy())
        act = torch.from_numpy(inp["actions" if drive == "ik" else "actions_pos"]).to(dt)
        u = torch.from_numpy(inp["u"]).to(dt)
        real_rand = torch.rand

        def fixture_rand(shape, *a, **k):
            ids = torch.nonzero(t2.reset_buf).squeeze(-1)
            return u[ids, :3].clone() if len(shape) == 2 else u[ids, 3].clone()

        torch.rand = fixture_rand
        try:
            t2.pre_physics_step(act)
        finally:
            torch.rand = real_rand
        o = {"pos_act_all": n(t2.pos_act_all), "root": n(t2.root_tensor), "dof_state_all": n(t2.dof_state_tensor_all),
             "reset": n(t2.reset_buf).astype(bool), "after_progress": n(t2.progress_buf), "after_success": n(t2.success),
             "after_epis_max_rew": n(t2.epis_max_rew), "after_epis_max_step": n(t2.epis_max_step)}
        if mode == "train":
            o["reset_succ"], o["succ_rate"] = n(t2.reset_succ), n(t2.extras["succ_rate"]).astype(np.float32)
        out.update({name + "_" + k: v for k, v in o.items()})
    return out


def restated(fx, dtype=np.float64):
    return OD.post(fx["rigid_body_all"], fx["dof_state_all"], fx["root"], fx["rigid_body_mask"], fx["dof_state_mask"], int(fx["obj_actor"]),
                   int(fx["ltip"]), int(fx["rtip"]), fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"],
                   fx["dof_lo"], fx["dof_hi"], fx["obj_id"], fx["before_succ_objid"], fx["part_slot"], fx["part_C"], dtype=dtype)


def check_conditions(fx):
    """The conditions of the fixtures; fx: the dict that is (or was) written to the .npz."""
    N = fx["root"].shape[0]
    assert N != 3 and N % 4 != 0 and N % 8 != 0                # partial last block at every environments-per-block the launcher picks
    rbm, dfm = fx["rigid_body_mask"], fx["dof_state_mask"]
    assert rbm.shape == (N, NRB + 2) and dfm.shape == (N, ND + 1) and rbm.dtype == np.int32 and dfm.dtype == np.int32
    want_rb, want_df, B, D = build_masks(N)
    assert np.array_equal(rbm, want_rb) and np.array_equal(dfm, want_df)
    assert fx["rigid_body_all"].shape == (B, 13) and fx["dof_state_all"].shape == (D, 2) and fx["root"].shape == (N, NA, 13)
    assert np.array_equal(fx["obj_id"], np.arange(N) % 3)
    assert len(set(np.diff(rbm[:, 0]).tolist())) == 3 and (dfm[:, -1] - dfm[:, ND - 1] != 1).any()   # irregular strides; not the first joint
    ref = restated(fx)
    m = lambda v, thr=0.0: float(np.abs(np.asarray(v) - thr).min())          # noqa: E731
    # threshold margins
    assert m(ref["half_margins"]) >= MARGIN and m(ref["short_product"]) >= MARGIN
    assert m(ref["gripper_length"] - (ref["short_length"] + 0.01)) >= MARGIN
    assert m(ref["extras"][:, 4], -0.2) >= MARGIN and m(ref["open_fraction"], 0.1) >= MARGIN
    assert m(ref["travel"] - 0.5 * fx["joint_hi"].astype(np.float64)) >= MARGIN
    # float32 and float64 reference agree on every flag and integer
    for k in ("success", "is_reached", "succ_objid"):
        assert np.array_equal(fx["out32_" + k], fx["out64_" + k]), k
    for j in (0, 1, 7):
        assert np.array_equal(fx["out32_extras"][:, j], fx["out64_extras"][:, j]), j
    for name, drive, mode, rnd in RUNS:
        for k in RUN_INT_KEYS + (("reset_succ", "succ_rate") if mode == "train" else ()):
            assert np.array_equal(fx[f"out32_{name}_{k}"], fx[f"out64_{name}_{k}"]), (name, k)
    # flag coverage
    ex = fx["out64_extras"]
    grasp, is_open, open_ng = ex[:, 7] != 0, ex[:, 0] != 0, ex[:, 1] != 0
    for name, flag in (("is_reached", fx["out64_is_reached"]), ("is_grasped", grasp), ("success", fx["out64_success"]), ("is_open", is_open),
                       ("open_notgrasp_without_grasp", open_ng & ~grasp)):
        assert flag.sum() * 8 >= N and (~flag).any(), name
    assert (~open_ng).any()
    # reach sub-flags: each false somewhere while another holds; a counted bonus would differ from the logical one often enough
    rf = ref["reach_flags"]
    for j in range(3):
        assert (~rf[:, j] & rf[:, [c for c in range(3) if c != j]].any(axis=1)).any(), j
    assert (rf.sum(axis=1) >= 2).sum() * 8 >= N
    # sticky object flags: a type that never succeeds and had no flag, and a flag set beforehand on a type without success now
    succ_types = set(fx["obj_id"][fx["out64_success"]].tolist())
    before = fx["before_succ_objid"]
    assert any(not before[t] and t not in succ_types for t in range(NUM_OBJS))
    assert any(before[t] and t not in succ_types for t in range(NUM_OBJS)) and succ_types
    want = before.copy()
    want[list(succ_types)] = True
    assert np.array_equal(fx["out64_succ_objid"], want)
    # resets
    reset, succ = fx["out64_ik_train_reset"], fx["out64_success"]
    assert (reset & succ).any() and (reset & ~succ).any() and (~reset).any()
    for name, drive, mode, rnd in RUNS:
        r = fx[f"out64_{name}_reset"]
        assert r.any() and (~r).any(), name
        if rnd:                                               # u of the resetting environments spans both signs of yaw and translation
            uu = fx["u"][r]
            assert (uu < 0.5).any(axis=0).all() and (uu > 0.5).any(axis=0).all(), name
    assert np.abs(fx["out64_rew"] - fx["before_epis_max_rew"]).min() >= 0.04
    assert (fx["u"] >= 0).all() and (fx["u"] < 1).all()
    q = fx["dof_state_all"][dfm[:, :ND], 0]
    assert (q >= fx["dof_lo"]).all() and (q <= fx["dof_hi"]).all() and np.abs(fx["actions"]).max() <= 1
    for k in FLOAT_GROUPS:
        assert fx["out32_" + k].dtype == np.float32 and fx["out64_" + k].dtype == np.float64, k
    for name, *_ in RUNS:
        for k in RUN_FLOAT_GROUPS:
            assert fx[f"out32_{name}_{k}"].dtype == np.float32 and fx[f"out64_{name}_{k}"].dtype == np.float64, (name, k)


def main(reference_root):
    mods, gym = load_reference(reference_root)
    for name, N, seed in CASES:
        inp = make_inputs(N, seed)
        torch.set_default_dtype(torch.float64)
        rew64 = run_reference(mods, gym, inp, torch.float64)["rew"]
        emr, ems = bookkeeping_before(inp, rew64)
        o64 = run_reference(mods, gym, inp, torch.float64, (emr, ems))
        torch.set_default_dtype(torch.float32)
        o32 = run_reference(mods, gym, inp, torch.float32, (emr, ems))
        fx = {k: v for k, v in inp.items() if not k.startswith("u_")}
        fx.update(before_epis_max_rew=emr, before_epis_max_step=ems)
        fx.update({"out32_" + k: v for k, v in o32.items()})
        fx.update({"out64_" + k: v for k, v in o64.items()})
        check_conditions(fx)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **fx)
        e = {k: float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in ("normal_state", "rew", "pose_R", "ik_train_pos_act_all",
                                                                                  "ik_test_rand_root")}
        print(f"{name}: {os.path.getsize(path)} bytes; reached {int(o64['is_reached'].sum())}, success {int(o64['success'].sum())}, "
              f"reset {int(o64['ik_train_reset'].sum())} / {N}; e_ref {e}")


if __name__ == "__main__":
    main(sys.argv[1])
