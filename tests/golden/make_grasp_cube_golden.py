"""Dev-machine generator of the grasp_cube task-step fixtures (tests/test_grasp_cube_host.py, tests/test_gpu_grasp_cube.py): runs
the REFERENCE's own compute_observations, update_state, compute_reward, compute_scene_pose, control / solve_ik, pre_physics_step
and reset_idx on the CPU, once in float32 and once in float64.

    python tests/golden/make_grasp_cube_golden.py /path/to/reference

The reference's task modules import isaacgym and their own `utils` / `tasks` packages at the top, so stand-in modules go into
sys.modules (isaacgym.torch_utils with tensor_clamp, quat_mul, quat_conjugate; a gym whose every method does nothing) and
utils/torch_jit_utils.py, tasks/load_robot.py, tasks/hand_base.py and tasks/grasp_cube.py are loaded by file path with PYTORCH_JIT=0
(scripting fails on names the stand-in lacks).  Task and robot are built with object.__new__ and their attributes set by hand.  The
float64 pass runs under torch.set_default_dtype(torch.float64) because deambiguity_rotation creates its own eye; `exit` is
shadowed in the loaded hand_base for compute_scene_pose, which starts with exit(1).

Writes grasp_cube_ref_small.npz (N = 5) and grasp_cube_ref_64.npz (N = 64), nb = 14, nd = 9: the inputs, out32_* / out64_* per
output group, and the bookkeeping buffers before (before_*) and after (in the out groups).  The conditions the fixtures must meet
(asserted here and again on the committed files by tests/test_grasp_cube_host.py) are in check_conditions."""
import os
os.environ["PYTORCH_JIT"] = "0"                               # before torch is imported
import importlib.util  # noqa: E402
import sys  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import grasp_cube_ref as G  # noqa: E402

NB, ND, NA, NL, LTIP, RTIP, OBJ_ACTOR = 14, 9, 2, 12, 10, 12, 1
DT = 1.0 / 60.0
DOF_LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0], dtype=np.float32)
DOF_HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04], dtype=np.float32)
DEFAULT_DOF = np.array([0.3, -0.4, -0.3, -2.2, -0.1, 2.0, -0.5, 0.04, 0.04], dtype=np.float32)
GOAL, GOAL_THRESH, OBJ_DEFAULT = np.array([0, 0, 0.2], dtype=np.float32), 0.025, np.array([0, 0, 0.025], dtype=np.float32)
EXPLORE_STEP, MAX_EPISODE_LENGTH_TEST = 40, 60
CASES = (("grasp_cube_ref_small", 5, 5101), ("grasp_cube_ref_64", 64, 5102))
GAP, MARGIN = 1e-3, 1e-4


def part_defaults():
    C = np.zeros((12, 3, 3), dtype=np.float32)
    C[:, 0, 0] = 1
    C[:11, 1, 2] = -1
    C[:11, 2, 1] = 1
    C[10, 1, 2] = 1
    C[11] = np.eye(3)
    return np.array(list(range(10)) + [NB - 3, NB - 1], dtype=np.int32), C


def unit(rng, *shape):
    v = rng.normal(size=shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_inputs(N, seed):
    rng = np.random.RandomState(seed)
    rb = np.zeros((N, NB, 13))
    rb[..., :3] = rng.uniform(-0.5, 0.5, size=(N, NB, 3))
    q = rng.normal(size=(N, NB, 4))
    rb[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    rb[..., 7:] = rng.normal(size=(N, NB, 6)) * 0.3
    kind = np.arange(N) % 4                                   # 0: success, 1: reached only, 2: far & on the table, 3: far & lifted
    rng.shuffle(kind)
    obj = np.zeros((N, 3))
    obj[:, :2] = rng.uniform(-0.14, 0.14, size=(N, 2))
    obj[:, 2] = np.where(kind == 3, rng.uniform(0.12, 0.3, size=N), rng.uniform(0.02, 0.09, size=N))
    s = kind == 0
    obj[s] = GOAL + unit(rng, int(s.sum())) * rng.uniform(0.002, 0.02, size=(int(s.sum()), 1))
    tip = obj + unit(rng, N) * np.where(kind <= 1, rng.uniform(0.002, 0.015, size=N), rng.uniform(0.05, 0.3, size=N))[:, None]
    half = unit(rng, N) * rng.uniform(0.005, 0.04, size=(N, 1))
    rb[:, LTIP, :3], rb[:, RTIP, :3] = tip + half, tip - half
    qr = rb[:, LTIP, 3:7] + rng.normal(size=(N, 4)) * 0.02    # the two tips share the hand's orientation up to noise
    rb[:, RTIP, 3:7] = qr / np.linalg.norm(qr, axis=-1, keepdims=True)
    root = np.zeros((N, NA, 13))
    root[:, 0, :7] = [0, -0.5, 0, 0, 0, 0.707, 0.707]
    root[:, 1, :3] = obj
    for b in range(N):                                        # object quaternions with a clear best candidate
        while True:
            qq = rng.normal(size=4)
            qq /= np.linalg.norm(qq)
            tr = np.sort(G.candidates(qq[None])[1][0])
            if tr[-1] - tr[-2] >= 2 * GAP:
                break
        root[b, 1, 3:7] = qq
    root[:, 1, 7:] = rng.normal(size=(N, 6)) * 0.1
    rb[:, NB - 1] = root[:, 1]
    dof = np.zeros((N, ND, 2))
    mid, span = (DOF_LO + DOF_HI) / 2.0, (DOF_HI - DOF_LO) / 2.0
    dof[..., 0] = mid + span * rng.uniform(-0.9, 0.9, size=(N, ND))
    dof[..., 1] = rng.normal(size=(N, ND)) * 0.5
    jac = rng.normal(size=(N, NL, 6, ND))
    part_body, part_C = part_defaults()
    u_step = (np.cumsum(kind != 0) % 2).astype(np.int64)       # live episodes alternate between timed out and running
    progress = np.where(u_step == 1, rng.randint(45, 100, size=N), rng.randint(1, 100, size=N)).astype(np.int64)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    return dict(rigid_body=f(rb), dof_state=f(dof), root=f(root), jac=f(jac), actions=f(rng.uniform(-1, 1, size=(N, 7))),
                actions_pos=f(rng.uniform(-1, 1, size=(N, 8))), dof_lo=DOF_LO, dof_hi=DOF_HI, default_dof_pos=DEFAULT_DOF,
                dt=np.float64(DT), goal=GOAL, goal_thresh=np.float64(GOAL_THRESH), obj_default_pos=OBJ_DEFAULT, part_body=part_body,
                part_C=part_C, ltip=np.int64(LTIP), rtip=np.int64(RTIP), obj_actor=np.int64(OBJ_ACTOR),
                explore_step=np.int64(EXPLORE_STEP), max_episode_length_test=np.int64(MAX_EPISODE_LENGTH_TEST),
                before_progress=progress, kind=kind.astype(np.int64),
                u_rew=f(rng.uniform(0.05, 1.0, size=N)), u_sign=rng.randint(0, 2, size=N).astype(np.int64),
                u_step=u_step)


def bookkeeping_before(inp, rew64):
    """epis_max_rew well away from the reward on either side; epis_max_step so that timeouts (an earlier, better step more than
    explore_step ago) and live episodes both occur."""
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
        return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], dim=-1)

    tu.quat_mul = quat_mul
    ig.torch_utils = tu
    utils, tasks = types.ModuleType("utils"), types.ModuleType("tasks")
    utils.TSDFVolume = utils.gen_camera_pose = utils.TSDFfromMesh = None
    utils.__path__, tasks.__path__ = [], []
    sys.modules.update({"isaacgym": ig, "isaacgym.gymapi": ig.gymapi, "isaacgym.gymtorch": ig.gymtorch, "isaacgym.torch_utils": tu,
                        "utils": utils, "tasks": tasks})
    mods = {}
    for name, rel in (("utils.torch_jit_utils", "utils/torch_jit_utils.py"), ("tasks.load_robot", "tasks/load_robot.py"),
                      ("tasks.hand_base", "tasks/hand_base.py"), ("tasks.grasp_cube", "tasks/grasp_cube.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    mods["tasks.hand_base"].exit = lambda *a: None            # compute_scene_pose starts with exit(1)
    return mods, AnyGym()


def build_task(mods, gym, inp, dt, drive_mode, train_test, max_episode_length):
    """A grasp_cube task and its franka robot without their constructors; tensors of dtype dt."""
    N = inp["rigid_body"].shape[0]
    T = lambda a: torch.from_numpy(np.array(a)).to(dt)        # noqa: E731
    robot = object.__new__(mods["tasks.load_robot"].franka)
    robot.gym, robot.device, robot.num_envs, robot.dt, robot.driveMode, robot.mobile = gym, "cpu", N, float(inp["dt"]), drive_mode, False
    robot.num_dofs, robot.ltip_rb_index, robot.rtip_rb_index = ND, LTIP, RTIP
    robot.dof_lower_limits_tensor, robot.dof_upper_limits_tensor = T(inp["dof_lo"]), T(inp["dof_hi"])
    robot.default_dof_pos = T(inp["default_dof_pos"])
    robot.default_root = T(inp["root"][0, 0, :7])
    robot.action_tensor = torch.zeros(N, ND, dtype=dt)
    robot.jacobian_tensor = T(inp["jac"])
    task = object.__new__(mods["tasks.grasp_cube"].grasp_cube)
    task.gym, task.sim, task.device, task.num_envs, task.robot = gym, None, "cpu", N, robot
    task.pose_lower_limit, task.pose_upper_limit = T(G.POSE_LO), T(G.POSE_HI)
    task.rigid_body_tensor, task.dof_state_tensor, task.root_tensor = T(inp["rigid_body"]), T(inp["dof_state"]), T(inp["root"])
    task.obj_actor, task.learn_input_mode, task.add_proprio_obs, task.obs_buf, task.extras = OBJ_ACTOR, "normal_state", True, {}, {}
    task.goal_thresh, task.success_pos = float(inp["goal_thresh"]), T(inp["goal"])[None, :]
    task.obj_default_root = torch.cat([T(inp["obj_default_pos"]), T(np.array([0, 0, 0, 1.0]))])
    task.coordinate_transform_matrix = T(inp["part_C"][:11])
    task.progress_buf = torch.from_numpy(inp["before_progress"].copy())
    task.train_test_flag, task.explore_step, task.max_episode_length, task.random_reset = train_test, EXPLORE_STEP, max_episode_length, False
    task.success = torch.zeros(N, dtype=torch.bool)
    task.pos_act = torch.zeros(N, ND, dtype=dt)
    task.pos_act_all = torch.zeros(N * ND, dtype=dt)
    task.dof_state_mask = torch.arange(N * ND).reshape(N, -1)
    task.global_indices = torch.arange(N * 2, dtype=torch.int32).view(N, -1)
    task.reset_buf = torch.zeros(N, dtype=torch.long)
    task.reset_succ = torch.zeros(N, dtype=torch.bool)
    return task


def run_reference(mods, gym, inp, dt, emr_ems=None):
    """One post step, then one pre step in train mode, one in test mode and the 'pos' drive; returns numpy outputs."""
    out = {}
    n = lambda t: t.detach().numpy().copy()                   # noqa: E731
    task = build_task(mods, gym, inp, dt, "ik", "train", 200)
    task.compute_observations()
    out["normal_state"], out["proprio"] = n(task.obs_buf["normal_state"][:, :19 + 2 * ND]), n(task.obs_buf["proprio_state"])
    task.compute_reward(None)
    out["rew"], out["success"], out["is_reached"] = n(task.rew_buf), n(task.success), n(task.extras["is_reached"])
    out["extras"] = np.stack([n(task.extras[k]).astype(out["rew"].dtype) for k in G.EXTRAS], axis=1)
    rot, pos = task.compute_scene_pose()
    out["pose_R"], out["pose_T"] = n(rot), n(pos)
    if emr_ems is None:
        return out
    after_post = dict(rew=task.rew_buf.clone(), success=task.success.clone())
    for mode, mel in (("train", 200), ("test", MAX_EPISODE_LENGTH_TEST)):
        t2 = build_task(mods, gym, inp, dt, "ik", mode, mel)
        t2.robot.update_state(t2.rigid_body_tensor, t2.dof_state_tensor)
        t2.rew_buf, t2.success = after_post["rew"].clone(), after_post["success"].clone()
        t2.epis_max_rew, t2.epis_max_step = torch.from_numpy(emr_ems[0].copy()).to(dt), torch.from_numpy(emr_ems[1].copy())
        if mode == "train":
            out["pos_act_ik"] = n(t2.robot.control(torch.from_numpy(inp["actions"]).to(dt)))
        t2.pre_physics_step(torch.from_numpy(inp["actions"]).to(dt))
        k = "" if mode == "train" else "test_"
        out[k + "pos_act"], out[k + "reset"] = n(t2.pos_act), n(t2.reset_buf).astype(bool)
        out[k + "after_progress"], out[k + "after_success"] = n(t2.progress_buf), n(t2.success)
        out[k + "after_epis_max_rew"], out[k + "after_epis_max_step"] = n(t2.epis_max_rew), n(t2.epis_max_step)
        if mode == "train":
            out["reset_succ"], out["succ_rate"] = n(t2.reset_succ), n(t2.extras["succ_rate"]).astype(np.float32)
            out["n_succ"], out["n_reset"] = np.int64(after_post["success"].sum()), np.int64(t2.reset_buf.sum())
    t3 = build_task(mods, gym, inp, dt, "pos", "train", 200)
    t3.robot.update_state(t3.rigid_body_tensor, t3.dof_state_tensor)
    out["pos_act_pos"] = n(t3.robot.control(torch.from_numpy(inp["actions_pos"]).to(dt)))
    return out


INT_KEYS = ("success", "is_reached", "reset", "reset_succ", "after_progress", "after_success", "after_epis_max_step", "n_succ", "n_reset",
            "succ_rate", "test_reset", "test_after_progress", "test_after_success", "test_after_epis_max_step")


def check_conditions(fx):
    """The conditions of the fixtures; fx: the dict that is (or was) written to the .npz."""
    N = fx["rigid_body"].shape[0]
    assert N != 3                                             # the reference's torch.cross picks the batch axis at N = 3
    assert fx["rigid_body"].shape[1:] == (NB, 13) and fx["dof_state"].shape[1:] == (ND, 2)
    tr = np.sort(G.candidates(fx["root"][:, OBJ_ACTOR, 3:7].astype(np.float64))[1], axis=1)
    assert (tr[:, -1] - tr[:, -2]).min() >= GAP
    ref = G.post(fx["rigid_body"], fx["dof_state"], fx["root"], OBJ_ACTOR, LTIP, RTIP, fx["dof_lo"], fx["dof_hi"], fx["goal"],
                 float(fx["goal_thresh"]), fx["obj_default_pos"], fx["part_body"], fx["part_C"])
    dist, height = -ref["extras"][:, 0], ref["extras"][:, 6]
    dgoal = np.linalg.norm(fx["root"][:, OBJ_ACTOR, :3].astype(np.float64) - fx["goal"], axis=1)
    for v, thr in ((dist, 0.02), (dgoal, float(fx["goal_thresh"])), (dgoal, 0.2), (height, 0.1)):
        assert np.abs(v - thr).min() >= MARGIN, (np.abs(v - thr).min(), thr)
    assert fx["out64_is_reached"].sum() * 4 >= N and fx["out64_success"].sum() * 4 >= N
    reset, succ = fx["out64_reset"], fx["out64_success"]
    assert (reset & succ).any() and (reset & ~succ).any() and (~reset).any()
    assert fx["out64_test_reset"].any() and (~fx["out64_test_reset"]).any()
    q = fx["dof_state"][:, :, 0]
    assert (q >= fx["dof_lo"]).all() and (q <= fx["dof_hi"]).all() and np.abs(fx["actions"]).max() <= 1
    assert abs(float(fx["dt"]) - 1 / 60) < 1e-12
    assert np.abs(fx["out64_rew"] - fx["before_epis_max_rew"]).min() >= 0.04
    for k in INT_KEYS:                                        # float32 and float64 reference agree on every flag and integer
        assert np.array_equal(fx["out32_" + k], fx["out64_" + k]), k
    for k in ("normal_state", "proprio", "rew", "extras", "pose_R", "pose_T", "pos_act", "pos_act_ik", "pos_act_pos", "after_epis_max_rew"):
        assert fx["out32_" + k].dtype == np.float32 and fx["out64_" + k].dtype == np.float64, k


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
        e = {k: float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in ("normal_state", "rew", "pose_R", "pos_act_ik")}
        print(f"{name}: {os.path.getsize(path)} bytes; reached {int(o64['is_reached'].sum())}, success {int(o64['success'].sum())}, "
              f"reset {int(o64['reset'].sum())} / {N}; e_ref {e}")


if __name__ == "__main__":
    main(sys.argv[1])
