"""partmanip_amd.envs.KinematicEnv on the GPU: the scripted grasp_cube episode of tests/kinematic_episode.py through env.step against
its float64 run, the observation rows, the mobile robot, open_drawer on the synthetic cabinets of tests/cabinet_fixtures.py, and
`ppo` / `dagger` / train.py running on it.

Tolerance of the episode: test_gpu_kinematics.py's rule on a closed loop.  e_ref = the error of the composed references' float32 run
against their float64 run at the step compared; the environment's cube stays within 4 e_ref of the float64 run there.  The step
compared is the success step, or the last step before any flag (is_reached, hold, success, reset) differs between the three runs.
Everything else is an equality."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cabinet_fixtures as CF
from tests import helpers
from tests import kinematic_episode as E
from tests.helpers import npy, record_margin, same_bits
from tests.test_gpu_run_loop import _ppo_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MOBILE_URDF = os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf")
DT = E.DT
N67 = 67
t = functools.partial(helpers.t, device=DEV)


def grasp_env(N, **kw):
    from partmanip_amd.envs import make_grasp_cube_env
    tree, bp, dof = E.scene()
    kw.setdefault("free_body_pose", E.CUBE_POSE)
    return make_grasp_cube_env(dict(E.CFG, **kw.pop("cfg", {})), N, DEV, tree, DT, base_pose=bp, dof=dof, **kw)


def run_script(env, steps, stop_after_success=1):
    """The script of tests/kinematic_episode.py through env.step: per step the flags and the cube of every environment (numpy)."""
    task, sim = env.task, env.sim
    r = task.robot
    env.reset()
    assert int(task.progress_buf.abs().sum()) == 0
    log, done = [], None
    for i in range(steps):
        rb = npy(sim.rigid_body)
        tip = (rb[:, r.ltip_rb_index, :3].astype(np.float64) + rb[:, r.rtip_rb_index, :3]) / 2
        a = E.script_action(tip, npy(sim.root)[:, 1, :3], npy(task.is_reached), npy(sim.grip)[:, 7] != 0)
        hold = npy(env._hold).copy()
        obs, rew, reset, extras = env.step(t(a))
        log.append(dict(cube=npy(sim.root)[:, 1].copy(), body=npy(sim.rigid_body)[:, -1].copy(), grip=npy(sim.grip).copy(),
                        reached=npy(task.is_reached).copy(), success=npy(task.success).copy(), reset=npy(reset).copy(), hold=hold,
                        rew=npy(rew).copy()))
        if done is None and log[-1]["success"].all():
            done = i
        if done is not None and i >= done + stop_after_success:
            break
    return log


# ------------------------------------------------------------------------------------------- 1. the scripted episode
@pytest.fixture(scope="module")
def references():
    return E.run_reference(E.MAX_EPISODE_LENGTH), E.run_reference(E.MAX_EPISODE_LENGTH, dtype=np.float32)


@pytest.mark.parametrize("N", [N67, 1])
def test_scripted_episode_reaches_success_and_resets(N, references):
    r64, r32 = references
    env = grasp_env(N)
    log = run_script(env, E.MAX_EPISODE_LENGTH)
    succ = [i for i, s in enumerate(log) if s["success"].all()]
    assert succ, "the scripted episode did not reach success"
    s0 = succ[0]
    print(f"N = {N}: success after step {s0 + 1} (float64 reference: {next(i for i, s in enumerate(r64) if s['success']) + 1})")
    for s in log:                                             # every environment runs the same scene: the same bits
        assert all(same_bits(s[k], np.broadcast_to(s[k][:1], s[k].shape)) for k in ("cube", "grip", "rew"))
        assert same_bits(s["cube"], s["body"])
    flags = lambda s, one: tuple(bool(s[k][0]) if one else bool(s[k]) for k in ("reached", "hold", "success", "reset"))      # noqa: E731
    agree = 0
    while agree < min(len(log), len(r64), len(r32)) and flags(log[agree], True) == flags(r64[agree], False) == flags(r32[agree], False):
        agree += 1
    at = min(s0, agree - 1)
    print(f"flags agree between the environment and the two reference runs for {agree} steps; compared after step {at + 1}")
    assert at >= 50                                           # well into the carried phase (the latch is set at step 50)
    res = []
    for key, sl in (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("linear velocity", slice(7, 10)), ("angular velocity", slice(10, 13))):
        w64, w32 = r64[at]["cube"][sl], r32[at]["cube"][sl].astype(np.float64)
        e_ref, err = float(np.abs(w32 - w64).max()), float(np.abs(log[at]["cube"][0, sl].astype(np.float64) - w64).max())
        print(f"episode N={N}, cube {key} after step {at + 1}: e_ref = {e_ref:.3e}; observed = {err:.3e}")
        if e_ref > 0:
            record_margin(f"kinematic env episode N={N}: cube {key} / e_ref", err / e_ref, 4.0, e_ref=e_ref, step=at + 1)
        res.append((err <= 4 * e_ref, (key, err, e_ref)))
    # the step after success: reset is set and the cube is back at its default pose, bit for bit, at rest, unlatched
    after = log[s0 + 1]
    assert after["reset"].all() and not after["success"].any()
    want = np.zeros(13, dtype=np.float32)
    want[:7] = E.CUBE_POSE
    assert same_bits(after["cube"], np.broadcast_to(want, (N, 13))) and not after["grip"][:, 7].any()
    for ok, what in res:
        assert ok, what


def test_with_hold_off_the_cube_never_moves_and_success_stays_false():
    env = grasp_env(3, hold=False)
    log = run_script(env, 90)
    assert len(log) == 90 and not any(s["success"].any() for s in log) and any(s["reached"].all() for s in log)
    assert all(same_bits(s["cube"], log[0]["cube"]) and not s["grip"].any() for s in log)
    assert same_bits(log[0]["cube"][0, :7], np.asarray(E.CUBE_POSE, dtype=np.float32))


def test_kinematic_sim_without_free_body_still_refuses_hold():
    from partmanip_amd.kinematics import KinematicSim
    tree, bp, dof = E.scene()
    sim = KinematicSim(tree, 2, DEV, DT, num_bodies=14, num_actors=2)
    rb0 = npy(sim.rigid_body).copy()
    with pytest.raises(ValueError, match="hold needs"):
        sim.step(torch.zeros(2, 9, device=DEV), hold=torch.ones(2, dtype=torch.bool, device=DEV))
    assert same_bits(npy(sim.rigid_body)[:, 13], rb0[:, 13])   # the caller's row: untouched, as before
    fb = KinematicSim(tree, 2, DEV, DT, free_body=True, tips=(10, 12))
    cube = npy(fb.root)[:, 1].copy()
    fb.forward(), fb.set_dof_state(t(dof.astype(np.float32)))
    assert same_bits(npy(fb.root)[:, 1], cube) and same_bits(npy(fb.rigid_body)[:, 13], cube)        # they re-pose the robot only


# ------------------------------------------------------------------------------------------- 2. observations
def finger_pc(N, parts, num_points=256):
    from partmanip_amd import meshio
    from partmanip_amd.mesh2pc import PCfromMesh
    mesh = meshio.load_mesh(os.path.join(GOLDEN, "finger.stl"))
    return PCfromMesh(N, DEV, num_points=num_points, meshes=[mesh] * parts)


def test_every_declared_mode_has_its_width_and_the_cloud_row_ends_in_the_proprio_row():
    from partmanip_amd.envs import pc_observer
    N = 5
    pc = finger_pc(N, 12)
    ob = pc_observer(pc)
    env = grasp_env(N, observers={"mesh_pc": ob, "mesh_pc2": pc_observer(pc, sel=ob.sel)}, add_proprio_obs=True)
    assert env.num_obs == {"normal_state": 37, "proprio_state": 25, "mesh_pc": 3 * 256 + 25, "mesh_pc2": 3 * 256 + 25}
    assert env.num_envs == N and env.num_actions == 7 and env.max_episode_length == E.MAX_EPISODE_LENGTH
    rng = np.random.default_rng(0)
    obs = env.reset()
    last = None
    for step in range(4):
        assert set(obs) == set(env.num_obs)
        for mode, w in env.num_obs.items():
            assert tuple(obs[mode].shape) == (N, w) and obs[mode].dtype == torch.float32 and torch.isfinite(obs[mode]).all(), mode
        for mode in ("mesh_pc", "mesh_pc2"):
            assert torch.equal(obs[mode][:, -25:], obs["proprio_state"]), mode
        want = pc.query_pc(*env.task.compute_scene_pose(), sel=ob.sel).reshape(N, -1)
        assert torch.equal(obs["mesh_pc"][:, :3 * 256], want) and torch.equal(obs["mesh_pc2"][:, :3 * 256], want)
        assert torch.equal(obs["proprio_state"][:, :7], obs["normal_state"][:, :7])
        if last is not None:                                  # the previous observation is still intact after a step
            assert all(torch.equal(last[0][k], last[1][k]) for k in last[0])
        last = (obs, {k: v.clone() for k, v in obs.items()})
        obs, rew, reset, extras = env.step(t(rng.uniform(-1, 1, (N, 7)).astype(np.float32)))
        assert rew.shape == (N,) and reset.shape == (N,) and all(v.dim() == 1 for v in extras.values())
    assert not torch.equal(last[0]["normal_state"], obs["normal_state"])
    env.train_test_flag = "test"
    assert env.task.train_test_flag == "test" and env.train_test_flag == "test"
    pose = env.save_scene_pose()
    assert pose["rot"].shape == (N, 12, 3, 3) and pose["pos"].shape == (N, 12, 3)


def test_tsdf_and_depth_observers_fill_their_rows():
    from partmanip_amd import camera, meshio
    from partmanip_amd.depth2tsdf import TSDFVolume
    from partmanip_amd.envs import depth_pc_observer
    from partmanip_amd.mesh2depth import DepthFromMesh
    N = 2
    mesh = meshio.load_mesh(os.path.join(GOLDEN, "finger.stl"))
    cam_pose, cam_intr, im_h, im_w = camera.shipped_rig({"look_at": [0.0, 0.0, 0.1], "radius": 0.6})
    cam = DepthFromMesh(N, DEV, cam_pose, cam_intr, im_h, im_w, meshes=[mesh] * 12)
    vol = TSDFVolume(DEV, 2, 50, (-1, -1, 0.0))
    vol.register_camera(cam_pose, cam_intr, im_h, im_w, N)
    env = grasp_env(N, observers={"depth_pc": depth_pc_observer(cam, vol, num_points=64)})
    assert env.num_obs["depth_pc"] == 192
    obs = env.reset()
    obs, _, _, _ = env.step(torch.zeros(N, 7, device=DEV))
    want = vol.depth2pc(cam.render(*env.task.compute_scene_pose()), K=64).reshape(N, -1)
    assert torch.equal(obs["depth_pc"], want)


# ------------------------------------------------------------------------------------------- 3. the mobile robot
def test_mobile_robot_steps_with_ten_actions():
    from partmanip_amd.envs import make_grasp_cube_env
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:
        dof = json.load(f)["mobile"]
    N = 5
    cfg = dict(E.CFG, robot={"driveMode": "ik", "mobile": True})
    env = make_grasp_cube_env(cfg, N, DEV, MOBILE_URDF, DT, dof=dof)
    assert env.num_actions == 10 and env.num_obs["normal_state"] == 19 + 24 and env.num_obs["proprio_state"] == 7 + 24
    assert env.sim.rigid_body.shape == (N, 17, 13)
    obs = env.reset()
    q0 = npy(env.sim.dof_state).copy()
    a = np.zeros((N, 10), dtype=np.float32)
    a[:, 0], a[:, 3] = 1.0, -1.0
    for _ in range(3):
        obs, rew, reset, extras = env.step(t(a))
    assert tuple(obs["normal_state"].shape) == (N, 43) and torch.isfinite(obs["normal_state"]).all() and torch.isfinite(rew).all()
    q1 = npy(env.sim.dof_state)
    assert (q1[:, 0, 0] > q0[:, 0, 0]).all() and not np.array_equal(q1[:, 3:10], q0[:, 3:10])     # the base slid, the arm moved


# ------------------------------------------------------------------------------------------- 4. open_drawer
def test_open_drawer_env_a_held_drawer_opens_through_env_step(tmp_path):
    from partmanip_amd.envs import make_open_drawer_env
    from partmanip_amd.tasks.open_drawer import load_drawer_assets
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)["mobile"]}, "explore_step": 40, "maxEpisodeLength": 200, "random_reset": False}
    assets = load_drawer_assets([CF.write_cabinet(tmp_path, kind, i) for i, kind in enumerate(("B", "A"))], scale=0.5)
    N = 4
    out = {}
    for hold in ("always", False, True):
        env = make_open_drawer_env(cfg, N, DEV, MOBILE_URDF, assets, DT, hold=hold)
        assert env.num_actions == 10 and env.num_obs == {"normal_state": 29 + 24, "proprio_state": 7 + 24}
        obs = env.reset()
        assert tuple(obs["normal_state"].shape) == (N, 53) and tuple(obs["proprio_state"].shape) == (N, 31)
        bb = npy(env.task.part_bbox).astype(np.float64)
        pull = bb[:, 0] - bb[:, 4]
        pull /= np.linalg.norm(pull, axis=1, keepdims=True)
        a = np.zeros((N, 10), dtype=np.float32)
        a[:, 3:6] = pull                                      # a unit `ik` action along the handle's outward direction
        q = [npy(env.task.part_dof_state)[:, 0].copy()]
        for _ in range(20):
            obs, rew, reset, extras = env.step(t(a))
            assert not bool(reset.any())
            q.append(npy(env.task.part_dof_state)[:, 0].copy())
        out[hold] = (np.stack(q), npy(extras["is_open_notgrasp"]), npy(env.task.part_joint_upper_limits))
    q, open_ng, upper = out["always"]
    assert (np.diff(q, axis=0) >= 0).all() and (q[-1] - q[0] > 0.1 * upper).all() and (q[-1] < upper).all() and (open_ng > 0).all()
    for hold in (False, True):                                # the gripper is nowhere near the handle: the predicate never holds
        q, open_ng, _ = out[hold]
        assert all(same_bits(q[i], q[0]) for i in range(len(q))) and not open_ng.any()


# ------------------------------------------------------------------------------------------- 5. training
def _train_env(N, cloud=False, add_proprio=False):
    from partmanip_amd.envs import pc_observer
    kw = dict(cfg={"maxEpisodeLength": 6})
    if cloud:
        kw.update(observers={"mesh_pc": pc_observer(finger_pc(N, 12, num_points=1024))}, add_proprio_obs=add_proprio)
    return grasp_env(N, **kw)


@pytest.mark.parametrize("kind", ["mlp", "pointnet"])
def test_ppo_runs_on_the_kinematic_env(kind, tmp_path):
    from partmanip_amd.algorithms import ppo
    from partmanip_amd.feeder import ScreenLogger
    if kind == "mlp":
        net, mode = dict(name="MLP", hid_dim=[64, 64], activation="tanh"), "normal_state"
    else:
        net, mode = dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=True), "mesh_pc"
    env = _train_env(16, cloud=kind == "pointnet")
    logger = ScreenLogger(str(tmp_path), "g", "n", quiet=True)
    run = ppo(env, _ppo_cfg(net, mode, 16, 4, kind == "mlp"), logger)
    before = torch.cat([p.detach().reshape(-1).clone() for p in run.actor_critic.parameters()])
    run.run()
    after = torch.cat([p.detach().reshape(-1) for p in run.actor_critic.parameters()])
    assert run.curr_iter == 2 and run.total_envsteps == 128
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    for k in ("Train/surrogate_loss", "Train/value_function_loss", "Train/kl", "Progress/learn_time", "Val/succ_rate_mean",
              "Train/reaching_reward_mean", "Train/obj_height_mean"):
        assert k in run.log_dict and np.isfinite(float(run.log_dict[k])), k
    assert os.path.exists(os.path.join(logger.save_ckpt_dir, "model_2.pth"))


def test_dagger_runs_on_the_kinematic_env(tmp_path, monkeypatch):
    from partmanip_amd.algorithms import dagger, ppo
    from partmanip_amd.feeder import ScreenLogger
    monkeypatch.chdir(tmp_path)
    np.save("teacher_reward.npy", np.linspace(0, 1, 300).astype(np.float32))
    env = _train_env(16, cloud=True, add_proprio=True)
    tlog = ScreenLogger(str(tmp_path), "t", "n", quiet=True)
    tea = ppo(env, _ppo_cfg(dict(name="MLP", hid_dim=[64, 64], activation="tanh"), "normal_state", 16, 2, False), tlog)
    tea.save(1)
    cfg = dict(num_envs=16, obs_mode="mesh_pc",
               model=dict(action_std=0.1, action_activate="tanh", clipAction=1.0,
                          network=dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=False)),
               max_iterations=2, n_steps=1, n_updates=2, n_minibatches=2, device=DEV, buf_size=4, reward_reset=True,
               add_proprio_obs=True, offline_data_pth=None, eval_round=1, eval_frequence=2, save_frequence=2,
               test_only=False, save_pose=False, save_video=False, lr_schedule="linear_decay", lr=1e-4,
               teacher=os.path.join(tlog.save_ckpt_dir, "model_1.pth"), resume=None, pretrain=None, sampler="random")
    logger = ScreenLogger(str(tmp_path), "d", "n", quiet=True)
    run = dagger(env, cfg, logger)
    run.run()
    assert run.curr_iter == 2 and run.storage.cur_buf_size == 32
    assert np.isfinite(float(run.log_dict["Train/dagger_loss"]))
    assert os.path.exists(os.path.join(logger.save_ckpt_dir, "model_2.pth"))
    assert env.task.dagger_reward_reset is not None and env.dagger_reward_reset is env.task.dagger_reward_reset


def test_train_py_env_kinematic_command_line(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--env", "kinematic", "--taskcfg", "grasp_cube", "--algocfg", "ppo",
                          "--kinematic.urdf", os.path.join("tests", "golden", "franka_panda_sdf.urdf"), "--kinematic.scene",
                          os.path.join("tests", "golden", "kinematic_grasp_scene.json"), "--exp_name", "kin", "--algo.num_envs", "16",
                          "--algo.n_steps", "4", "--algo.max_iterations", "2", "--algo.n_minibatches", "2", "--log.log_root", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Train/surrogate_loss" in out.stdout and "Learning iteration 2" in out.stdout
