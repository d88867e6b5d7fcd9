"""Contact blocking on the GPU through the host layers: KinematicSim.step(guard=), contact.StepGuard and
KinematicEnv(resolve='block'), on the fixture of tests/contact_episode.py and the cabinets of tests/cabinet_fixtures.py.

What is an equality and why.  The executed joint state is the accepted candidate bit for bit (the sweep's definition), and so is the
next observation's nearest distance.  The step and the fraction of the push episode's first cut are equalities with the float64
restatement of tests/guarded_step_ref.py: tests/test_guarded_step_host.py shows on the CPU that every distance that decides a cut
there is further from the margin, and from its predecessor, than 100 x the float32 run's error.  The one tolerance is the standing
rule: the rest distance stays within 4 x the restatement's own float32 error of its float64 value."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import cabinet_fixtures as CF
from tests import contact_episode as CE
from tests import guarded_step_ref as GS
from tests import helpers
from tests import kinematic_episode as E
from tests import mesh_tsdf_parts as P
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
S = 8
PUSH_STEPS = 46                                               # the first cut comes at log index 41


def make_sensor(N):
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.mesh2pc import PCfromMesh
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    tsdf = TSDFfromMesh(N, 0.5, 10, DEV, sdf_dicts=CE.grids())
    pc = PCfromMesh(N, DEV, num_points=CE.POINTS, part_pcs=CE.part_clouds())
    return ContactSensor.from_cloud(tsdf, pc, CE.SLOTS, targets=(CE.CUBE_SLOT, CE.CUBE_SLOT + 1), names=CE.NAMES)


def grasp_env(N, **kw):
    from partmanip_amd.envs import make_grasp_cube_env
    tree, bp, dof = E.scene()
    return make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, free_body_pose=E.CUBE_POSE, **kw)


def tips(env):
    r, rb = env.task.robot, npy(env.sim.rigid_body)
    return (rb[:, r.ltip_rb_index, :3].astype(np.float64) + rb[:, r.rtip_rb_index, :3]) / 2


def executed_state_holds(env, extras, guarded):
    """dof_state holds the bits of the accepted candidate, and the observation after the step sees the accepted candidate's
    distance, in the environments `guarded` (N) bool (neither reset nor held on this step)."""
    g = env._guard
    q = npy(env.sim.dof_state.reshape(-1, 2)[env.sim._dof_index, 0] if env.sim.flat else env.sim.dof_state[..., 0]).reshape(npy(g.targets).shape)
    d, st = npy(g.sweep_dist), npy(g.steps)
    now = npy(extras["contact_dist"].min(dim=1)[0])
    assert same_bits(q[guarded], npy(g.targets)[guarded])
    assert same_bits(now[guarded], d[np.arange(len(st)), st][guarded]), (now, d, st)
    assert same_bits(npy(extras["blocked"]), st < g.substeps) and same_bits(npy(extras["step_fraction"]), (st / np.float32(g.substeps)).astype(np.float32))


# ------------------------------------------------------------------------------------------- the sim and the guard
def test_sim_step_with_a_guard_executes_the_accepted_candidate():
    """The grasp_cube env with hold=False (nothing is ever held) and a margin wide enough to cut steps: the push script brings the
    fingers to the cube, then seeded actions move them about it."""
    N = 3
    env = grasp_env(N, contact=make_sensor(N), resolve="block", block_substeps=4, block_margin=0.01, hold=False)
    env.reset()
    rng = np.random.default_rng(11)
    cut, near = 0, 1.0
    for i in range(52):
        a = GS.push_action(tips(env), npy(env.sim.root)[:, 1, :3])
        if i >= 38:
            a[:, :3] = np.clip(a[:, :3] + rng.uniform(-1, 1, size=(N, 3)), -1, 1)
        obs, rew, reset, extras = env.step(t(a))
        executed_state_holds(env, extras, ~npy(reset))
        cut += int(npy(extras["blocked"]).sum())
        near = min(near, float(npy(env._guard.sweep_dist).min()))
    print(f"{cut} of {52 * N} steps were cut; nearest candidate {1e3 * near:.2f} mm; last distances {npy(env._guard.sweep_dist).tolist()}")
    assert cut > 0 and near < 0.01 and float(extras["contact_dist"].min()) < 1


def test_refusals_and_untouched_defaults():
    from partmanip_amd.contact import StepGuard
    with pytest.raises(ValueError, match="needs contact="):
        grasp_env(2, resolve="block")
    with pytest.raises(ValueError, match="resolve: expected"):
        grasp_env(2, contact=make_sensor(2), resolve="push")
    sensor = make_sensor(2)
    with pytest.raises(ValueError, match="substeps"):
        StepGuard(sensor, [-1] * 12, substeps=64)
    with pytest.raises(ValueError, match="slot_body"):
        StepGuard(sensor, [-1] * 11)
    guard = StepGuard(sensor, [0] * 11 + [-1])
    env = grasp_env(2, contact=sensor)
    env.reset()
    with pytest.raises(ValueError, match="set_scene"):
        env.sim.step(env.task.pos_act, guard=guard)
    assert env._guard is None and "blocked" not in env.step(t(np.zeros((2, 7), dtype=np.float32)))[3]


# ------------------------------------------------------------------------------------------- the push script
@functools.lru_cache(maxsize=None)
def push_reference():
    r64 = GS.push_episode(PUSH_STEPS, S=S)
    r32 = GS.push_episode(PUSH_STEPS, S=S, dtype=np.float32, actions=[s["action"][None] for s in r64])
    return r64, r32


def push_run(N, steps, reverse_after=None, **kw):
    env = grasp_env(N, contact=make_sensor(N), hold=False, **kw)
    env.reset()
    log = []
    for i in range(steps):
        a = GS.push_action(tips(env), npy(env.sim.root)[:, 1, :3])
        obs, rew, reset, extras = env.step(t(a))
        log.append({k: npy(v).copy() for k, v in extras.items() if k in ("contact_dist", "penetration", "blocked", "step_fraction")})
    if reverse_after:
        a[:, :3] = -a[:, :3]
        extras = env.step(t(a))[3]
        log.append({k: npy(extras[k]).copy() for k in ("contact_dist", "penetration", "blocked", "step_fraction")})
    return env, log


def test_push_script_stops_at_first_contact():
    N = 2
    r64, r32 = push_reference()
    first64 = next(i for i, s in enumerate(r64) if s["steps"] < S)
    assert first64 == next(i for i, s in enumerate(r32) if s["steps"] < S) and r64[first64]["steps"] == r32[first64]["steps"]
    _, plain = push_run(N, 60)
    deepest = max(float(s["penetration"].max()) for s in plain)
    print(f"unguarded: deepest penetration {1e3 * deepest:.2f} mm")
    assert deepest > 0.010                                    # the precondition: unguarded, the finger goes more than 10 mm in
    env, log = push_run(N, PUSH_STEPS, reverse_after=True, resolve="block", block_substeps=S)
    back, log = log[-1], log[:-1]
    first = next(i for i, s in enumerate(log) if s["blocked"].any())
    print(f"first cut at log index {first} (float64: {first64}), fraction {log[first]['step_fraction'].tolist()} "
          f"(float64: {r64[first64]['steps']} of {S})")
    assert first == first64 and log[first]["blocked"].all()
    assert same_bits(log[first]["step_fraction"], np.full(N, r64[first64]["steps"] / S, dtype=np.float32))
    assert all((s["penetration"] == 0).all() for s in log)
    assert all((s["step_fraction"] == 0).all() for s in log[first + 1:])
    rest64, rest32 = float(r64[-1]["body_dist"].min()), float(r32[-1]["body_dist"].min())
    e_ref = abs(rest32 - rest64)
    err = float(np.abs(log[-1]["contact_dist"].min(axis=1).astype(np.float64) - rest64).max())
    print(f"rest distance: fp64 {rest64:.7f}, e_ref = {e_ref:.3e}, observed error {err:.3e}")
    record_margin("guarded step: push episode rest distance |hip - fp64| / e_ref", err / max(e_ref, 1e-300), 4.0, e_ref=e_ref, S=S)
    assert e_ref > 0 and err <= 4 * e_ref, (err, e_ref)
    assert not back["blocked"].any() and (back["step_fraction"] == 1).all()       # separation is admitted


# ------------------------------------------------------------------------------------------- the grasp episode is left alone
def test_contact_grasp_episode_is_the_same_with_the_guard():
    """The scripted contact grasp never comes within the margin before it latches, and held steps are not guarded: observation
    rows, rewards, flags and the cube carry the bits of the run without resolve=, up to the step after success."""
    N = 2
    runs = []
    for kw in ({}, {"resolve": "block", "block_substeps": S}):
        env = grasp_env(N, contact=make_sensor(N), grasp="contact", **kw)
        obs = env.reset()
        log = []
        for i in range(E.MAX_EPISODE_LENGTH):
            a = E.script_action(tips(env), npy(env.sim.root)[:, 1, :3], npy(env.task.is_reached), npy(env.sim.grip)[:, 7] != 0)
            obs, rew, reset, extras = env.step(t(a))
            log.append(dict({k: npy(v).copy() for k, v in obs.items()}, rew=npy(rew).copy(), reset=npy(reset).copy(),
                            success=npy(env.task.success).copy(), reached=npy(env.task.is_reached).copy(), hold=npy(env._hold).copy(),
                            cube=npy(env.sim.root)[:, 1].copy(), blocked=npy(extras["blocked"]).copy() if kw else None))
            if log[-1]["success"].all():
                break
        runs.append(log)
    plain, guarded = runs
    print(f"success after step {len(plain)} without the guard, {len(guarded)} with it")
    assert len(plain) == len(guarded) and plain[-1]["success"].all() and len(plain) < E.MAX_EPISODE_LENGTH
    for a, b in zip(plain, guarded):
        assert all(same_bits(a[k], b[k]) for k in a if k != "blocked")
        assert not b["blocked"].any()


# ------------------------------------------------------------------------------------------- open_drawer
def box_grid(half, voxel, trunc):
    n = int(np.ceil((2 * half + 2 * trunc) / voxel)) + 10
    idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1)
    pts = (idx - n // 2) * voxel
    sdf = np.clip(P._box_sdf(pts, np.full(3, half)), -trunc, trunc).astype(np.float32)
    return {'sdf': sdf, 'bbox_min': pts.reshape(-1, 3).min(axis=0).astype(np.float32), 'voxel_size': voxel}


def test_open_drawer_steps_with_the_guard(tmp_path):
    """Two cabinets, the mobile Franka, the task's 13 posed parts: the hand and the fingers sense a coarse box grid about the target
    link and one about the handle (5 cm cells, a 1.2 m band: they reach the hand from where the cabinet stands).  A few seeded steps: the executed state is the accepted candidate where nothing is held."""
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.envs import make_open_drawer_env
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    from partmanip_amd.tasks.open_drawer import load_drawer_assets
    N = 3
    with open(os.path.join(E.GOLDEN, "kinematics_default_dof.json")) as f:
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)["mobile"]}, "explore_step": 40, "maxEpisodeLength": 200, "random_reset": False}
    assets = load_drawer_assets([CF.write_cabinet(tmp_path, kind, i) for i, kind in enumerate(("B", "A"))], scale=0.5)
    urdf = os.path.join(E.GOLDEN, "franka_panda_sdf_mobile.urdf")
    dummy = CE.grids()[0]
    tsdf = TSDFfromMesh(N, 0.5, 10, DEV, sdf_dicts=[dummy] * 11 + [box_grid(0.4, 0.05, 1.2), box_grid(0.1, 0.05, 1.2)])
    pcs = CE.part_clouds()
    sensor = ContactSensor(tsdf, np.concatenate([pcs[s] for s in CE.SLOTS]), np.repeat(CE.SLOTS, CE.POINTS), [CE.POINTS] * 3, targets=(11, 13),
                           names=CE.NAMES)
    keys = None
    for kw in ({}, {"resolve": "block", "block_substeps": 4, "block_margin": 0.5}):
        env = make_open_drawer_env(cfg, N, DEV, urdf, assets, E.DT, contact=sensor, **kw)
        env.reset()
        rng = np.random.default_rng(23)
        near = []
        for i in range(6):
            held = npy(env._hold).copy()
            obs, rew, reset, extras = env.step(t(rng.uniform(-1, 1, size=(N, env.task.num_actions)).astype(np.float32)))
            if kw:
                executed_state_holds(env, extras, ~held & ~npy(reset))
                near.append(float(npy(env._guard.sweep_dist).min()))
        if kw:
            assert set(extras) == keys | {"blocked", "step_fraction"}
            assert env._guard.slot_body.tolist()[:11] == env.task.part_slot.tolist()[:11] and env._guard.slot_body.tolist()[11:] == [-1, -1]
            print(f"nearest candidate distance per step: {near}; parts taken at the last step {npy(env._guard.steps).tolist()}")
            assert min(near) < 1                              # the coarse grids reach the hand: the distances compared are distances
        else:
            keys = set(extras)
            assert "blocked" not in keys
