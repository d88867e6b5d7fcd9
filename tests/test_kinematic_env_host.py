"""Host checks of the kinematic environment (no GPU): the scripted grasp_cube episode composed from the tests' own float64 references
(tests/kinematic_episode.py) must reach `success`, which is a condition on the stated rules and not on any kernel; train.py's
argument errors; KinematicSim's refusals.  The ctypes table against the header is tests/test_capi_symbols.py's."""
import os

import numpy as np
import pytest
import torch

from tests import kinematic_episode as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def episode():
    return E.run_reference(E.MAX_EPISODE_LENGTH)


def test_scripted_episode_reaches_success_within_the_episode_length(episode):
    """Measured here in float64 with the one-step-late predicate: is_reached at step 49, the latch at step 50, success at step 84 of
    200 (the issue's own check, with hold taken right after the robot's move, saw 82)."""
    succ = [i for i, s in enumerate(episode) if s["success"]]
    print(f"first success after step {succ[0] + 1 if succ else None}; steps run {len(episode)}")
    assert succ and succ[0] + 1 <= E.MAX_EPISODE_LENGTH
    s = episode[succ[0]]
    assert s["reached"] and s["grip"][7] == 1 and np.linalg.norm(s["cube"][:3] - np.asarray(E.GOAL)) <= E.GOAL_THRESH
    assert not any(x["reset"] for x in episode[:succ[0] + 1])              # one episode: no exploration reset on the way
    first_hold = next(i for i, x in enumerate(episode) if x["hold"])
    assert episode[first_hold - 1]["reached"] and not episode[first_hold - 1]["hold"]      # the predicate is one step late
    assert episode[first_hold]["grip"][7] == 1 and np.array_equal(episode[first_hold]["cube"][:7], episode[first_hold - 1]["cube"][:7])
    rel = episode[first_hold]["grip"]
    assert all(np.array_equal(x["grip"], rel) for x in episode[first_hold:succ[0] + 1])   # written once


def test_the_step_after_success_resets_the_cube_to_its_default_pose(episode):
    after = episode[-1]
    assert episode[-2]["success"] and after["reset"] and not after["success"]
    assert np.array_equal(after["cube"][:7], np.asarray(np.float32(E.CUBE_POSE), dtype=np.float64)) and not after["cube"][7:].any()
    assert after["grip"][7] == 0


def test_without_the_rule_the_cube_never_moves_and_success_stays_false():
    log = E.run_reference(100, hold_on=False)
    assert len(log) == 100 and not any(s["success"] for s in log) and any(s["reached"] for s in log)
    assert all(np.array_equal(s["cube"], log[0]["cube"]) for s in log)


def test_float32_run_of_the_episode_succeeds_too():
    log = E.run_reference(E.MAX_EPISODE_LENGTH, dtype=np.float32)
    assert any(s["success"] for s in log)


# ------------------------------------------------------------------------------------------- train.py's arguments
def _cfg(argv):
    from partmanip_amd.config import process_cfgs
    return process_cfgs(argv, root=ROOT)


def test_train_py_env_argument_errors():
    import train
    cfg = _cfg([])
    assert cfg["env"] == "feeder" and set(cfg["kinematic"]) == {"urdf", "scene", "dt"} and cfg["kinematic"]["urdf"] is None
    with pytest.raises(ValueError, match=r"--kinematic\.urdf"):
        train.build_env(_cfg(["--env", "kinematic", "--taskcfg", "grasp_cube", "--algocfg", "ppo"]))
    with pytest.raises(NotImplementedError, match="make_open_drawer_env"):
        train.build_env(_cfg(["--env", "kinematic", "--taskcfg", "open_drawer", "--algocfg", "ppo", "--kinematic.urdf", E.URDF]))
    with pytest.raises(ValueError, match="'feeder' or 'kinematic'"):
        train.build_env(_cfg(["--env", "gym"]))
    with pytest.raises(NotImplementedError, match="observers="):
        train.build_env(_cfg(["--env", "kinematic", "--taskcfg", "grasp_cube", "--algocfg", "ppo_pointnet", "--kinematic.urdf", E.URDF]))


# ------------------------------------------------------------------------------------------- KinematicSim's refusals
def test_kinematic_sim_refusals(monkeypatch):
    """The constructor's checks come before any launch; with the robot's launch stubbed out (there is no device here) step() shows
    that `hold` is still refused without free_body= / objects= and that free_body= does go to the free-body entry."""
    from partmanip_amd import ops
    from partmanip_amd.kinematics import KinematicSim
    tree, bp, dof = E.scene()
    with pytest.raises(ValueError, match="tips"):
        KinematicSim(tree, 2, "cpu", E.DT, free_body=True)
    with pytest.raises(ValueError, match="objects="):
        KinematicSim(tree, 2, "cpu", E.DT, tips=(10, 12))
    with pytest.raises(ValueError, match="num_bodies"):
        KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 12), num_bodies=tree.num_bodies)
    with pytest.raises(ValueError, match="fall_speed"):
        KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 12), fall_speed=-1.0)
    with pytest.raises(ValueError, match="tips"):
        KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 13))
    monkeypatch.setattr(ops, "articulation_step", lambda *a, **k: None)
    sim = KinematicSim(tree, 2, "cpu", E.DT, num_bodies=14, num_actors=2)
    pos_act, hold = torch.zeros(2, tree.num_dofs), torch.ones(2, dtype=torch.bool)
    with pytest.raises(ValueError, match="hold needs"):
        sim.step(pos_act, hold=hold)
    with pytest.raises(ValueError, match="u needs"):
        sim.step(pos_act, u=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="free_body="):
        sim.reset_free_body()
    fb = KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 12), free_body_pose=E.CUBE_POSE)
    assert fb.rigid_body.shape == (2, 14, 13) and fb.root.shape == (2, 2, 13) and fb.grip.shape == (2, 8)
    assert fb.free_body_row.tolist() == [13, 27] and fb.tip_rows.tolist() == [[10, 12], [24, 26]]
    assert torch.equal(fb.root[:, 1, :7], fb.rigid_body[:, 13, :7]) and fb.root[0, 1, :3].tolist() == [np.float32(v) for v in E.CUBE_POSE[:3]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fb.step(pos_act, hold=hold)
    flat = KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 12), rb_row0=[3, 20], dof_row0=[0, 9])
    assert flat.free_body_row.tolist() == [16, 33] and flat.tip_rows.tolist() == [[13, 15], [30, 32]] and flat.rigid_body.shape[0] == 34
    with pytest.raises(ValueError, match="overlap"):
        KinematicSim(tree, 2, "cpu", E.DT, free_body=True, tips=(10, 12), rb_row0=[0, 13], dof_row0=[0, 9])
