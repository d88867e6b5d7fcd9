"""KinematicEnv(contact=, grasp='contact') on the GPU: the extras, that sensing observes and does not act, the refusals, and the
scripted grasp_cube episode of tests/contact_episode.py with the contact predicate against its float64 composition.

Tolerance of the episode: the standing rule.  e_ref = what the composed references' float32 run loses against their float64 run at
the observation compared (the one that sets `hold`); the environment's two finger distances stay within 4 e_ref of the float64 run
there.  The onset step is an equality -- tests/test_mesh_sdf_points_host.py shows on the CPU that at that observation and the one
before it both finger distances are further from contact_margin than 100 x the float32 error, so round-off cannot move it.
contact_margin is KinematicEnv's default, 0.002."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import cabinet_fixtures as CF
from tests import contact_episode as CE
from tests import helpers
from tests import kinematic_episode as E
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = E.GOLDEN
t = functools.partial(helpers.t, device=DEV)


def make_sensor(N, names=CE.NAMES):
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.mesh2pc import PCfromMesh
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    tsdf = TSDFfromMesh(N, 0.5, 10, DEV, sdf_dicts=CE.grids())
    pc = PCfromMesh(N, DEV, num_points=CE.POINTS, part_pcs=CE.part_clouds())
    return ContactSensor.from_cloud(tsdf, pc, CE.SLOTS, targets=(CE.CUBE_SLOT, CE.CUBE_SLOT + 1), names=names), pc


def grasp_env(N, **kw):
    from partmanip_amd.envs import make_grasp_cube_env
    tree, bp, dof = E.scene()
    return make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, free_body_pose=E.CUBE_POSE, **kw)


def script_step(env):
    task, sim, r = env.task, env.sim, env.task.robot
    rb = npy(sim.rigid_body)
    tip = (rb[:, r.ltip_rb_index, :3].astype(np.float64) + rb[:, r.rtip_rb_index, :3]) / 2
    a = E.script_action(tip, npy(sim.root)[:, 1, :3], npy(task.is_reached), npy(sim.grip)[:, 7] != 0)
    hold = npy(env._hold).copy()
    obs, rew, reset, extras = env.step(t(a))
    return hold, extras


# ------------------------------------------------------------------------------------------- extras
def test_extras_keys_shapes_and_the_penetration_rule():
    N = 3
    sensor, _ = make_sensor(N)
    env = grasp_env(N, contact=sensor)
    env.reset()
    plain = grasp_env(N)
    plain.reset()
    deepest = 0.0
    for i in range(56):
        _, extras = script_step(env)
        cd, ic, pen = extras["contact_dist"], extras["in_contact"], extras["penetration"]
        assert tuple(cd.shape) == (N, 3) and cd.dtype == torch.float32 and tuple(ic.shape) == (N, 3) and ic.dtype == torch.bool
        assert tuple(pen.shape) == (N,) and pen.dtype == torch.float32
        assert torch.equal(ic, cd <= 0.002) and same_bits(npy(pen), np.maximum(0, -npy(cd).min(axis=1)).astype(np.float32))
        assert same_bits(npy(cd), np.broadcast_to(npy(cd)[:1], (N, 3)))                     # one scene in every environment
        deepest = max(deepest, float(pen.max()))
    _, px = script_step(plain)
    assert set(extras) == set(px) | {"contact_dist", "in_contact", "penetration"}
    print(f"deepest penetration of the gap-rule episode's first 56 steps: {deepest:.4f} m")
    assert deepest > 0.002 and bool(ic[:, 1:].all())          # the kinematic fingers do pass into the cube: that is what is reported


def test_sensing_observes_and_does_not_act():
    """Ten steps of seeded actions with and without contact=: observation rows, rewards and flags are the same bits."""
    from partmanip_amd.envs import pc_observer
    N = 3
    sensor, pc = make_sensor(N)
    sel = torch.arange(0, 12 * CE.POINTS, 7, dtype=torch.int32, device=DEV)
    runs = []
    for kw in ({}, {"contact": sensor}):
        env = grasp_env(N, observers={"mesh_pc": pc_observer(pc, sel=sel)}, add_proprio_obs=True, **kw)
        rng = np.random.default_rng(5)
        obs = env.reset()
        log = [{k: npy(v).copy() for k, v in obs.items()}]
        for _ in range(10):
            obs, rew, reset, extras = env.step(t(rng.uniform(-1, 1, size=(N, 7)).astype(np.float32)))
            log.append(dict({k: npy(v).copy() for k, v in obs.items()}, rew=npy(rew).copy(), reset=npy(reset).copy(),
                            success=npy(env.task.success).copy(), reached=npy(env.task.is_reached).copy(), hold=npy(env._hold).copy(),
                            task_extras={k: npy(v).copy() for k, v in extras.items() if k not in ("contact_dist", "in_contact", "penetration")}))
        runs.append(log)
    for a, b in zip(*runs):
        assert set(a) == set(b)
        for k in a:
            if k == "task_extras":
                assert all(same_bits(a[k][j], b[k][j]) for j in a[k]), k
            else:
                assert same_bits(a[k], b[k]), k
    assert not same_bits(runs[0][1]["normal_state"], runs[0][-1]["normal_state"])


# ------------------------------------------------------------------------------------------- refusals
def test_contact_grasp_refusals(tmp_path):
    from partmanip_amd.envs import make_open_drawer_env
    from partmanip_amd.tasks.open_drawer import load_drawer_assets
    with pytest.raises(ValueError, match="needs contact="):
        grasp_env(2, grasp="contact")
    with pytest.raises(ValueError, match="'lfinger' and 'rfinger'"):
        grasp_env(2, grasp="contact", contact=make_sensor(2, names=None)[0])
    with pytest.raises(ValueError, match="'lfinger' and 'rfinger'"):
        grasp_env(2, grasp="contact", contact=make_sensor(2, names=("hand", "left", "rfinger"))[0])
    with pytest.raises(ValueError, match="grasp: expected"):
        grasp_env(2, grasp="touch")
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)["mobile"]}, "explore_step": 40, "maxEpisodeLength": 200, "random_reset": False}
    assets = load_drawer_assets([CF.write_cabinet(tmp_path, kind, i) for i, kind in enumerate(("B", "A"))], scale=0.5)
    with pytest.raises(ValueError, match="target link differs per cabinet"):
        make_open_drawer_env(cfg, 2, DEV, os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf"), assets, E.DT, grasp="contact",
                             contact=make_sensor(2)[0])


# ------------------------------------------------------------------------------------------- the episode
def test_scripted_episode_latches_on_finger_contact():
    """Measured on the CPU (float64 and float32 compositions alike): both fingers come within 0.002 of the cube at the observation
    after step 50 (0.00156 and 0.00172; 0.0048 and 0.0051 one step earlier), so step 51 is the first taken with hold set -- the
    same step as under the gap rule in this scene."""
    N = 2
    r64, r32 = CE.run_reference(E.MAX_EPISODE_LENGTH), CE.run_reference(E.MAX_EPISODE_LENGTH, dtype=np.float32)
    on64, on32 = CE.hold_onset(r64), CE.hold_onset(r32)
    assert on64 is not None and on64 == on32
    sensor, _ = make_sensor(N)
    env = grasp_env(N, contact=sensor, grasp="contact")
    env.reset()
    holds, dists = [], []
    for i in range(on64 + 3):
        hold, extras = script_step(env)
        holds.append(hold)
        dists.append(npy(extras["contact_dist"]).copy())
    onset = next(i for i, h in enumerate(holds) if h.any())
    print(f"hold first set for step {onset + 1} on the device, {on64 + 1} in the float64 composition")
    assert onset == on64 and all(h.all() for h in holds[onset:]) and not any(h.any() for h in holds[:onset])
    at = onset - 1                                            # the observation that set it
    e_ref = float(np.abs(r32[at]["body_dist"][1:].astype(np.float64) - r64[at]["body_dist"][1:]).max())   # the two fingers' own fp32 error
    for body in (1, 2):
        w64 = float(r64[at]["body_dist"][body])
        err = float(np.abs(dists[at][:, body].astype(np.float64) - w64).max())
        print(f"{CE.NAMES[body]} distance after step {at + 1}: fp64 {w64:.6f}, e_ref = {e_ref:.3e}, observed error {err:.3e}")
        record_margin(f"contact: grasp episode {CE.NAMES[body]} distance at the hold observation / e_ref", err / max(e_ref, 1e-300), 4.0,
                      e_ref=e_ref, step=at + 1)
        assert e_ref > 0 and err <= 4 * e_ref, (body, err, e_ref)
    gap = E.run_reference(E.MAX_EPISODE_LENGTH)
    gap_on = next(i for i, s in enumerate(gap) if s["hold"])
    record_margin("contact: hold onset step under the contact predicate (observed) and the gap predicate (tol)", onset + 1, gap_on + 1)
    assert bool(env.sim.grip[:, 7].ne(0).all())               # the cube is latched to the gripper
