"""Posed mesh point cloud on the GPU: partmanip_amd.mesh2pc.PCfromMesh (pm_mesh_pc_query_f32, csrc/mesh_pc.hip) against the
REFERENCE's own query_pc (fixtures of tests/golden/make_mesh_pc_golden.py) and against a numpy float32 evaluation of the stated
association, bit for bit.

Tolerance of the parity test: e_ref = max |out32 - out64| of the fixture is what the reference's own float32 run loses against its
float64 run; the kernel must stay within 4 e_ref of out64 (this project's margin convention).  Everything else is exact: the
contract fixes the association and the rounding of every operation, so the uint32 views must be equal.
Observed 2026-10-17 on 1x MI355X: e_ref = 1.58e-8 / 1.97e-8 (small / 1024 fixture), max |hip - out64| = 1.00 / 1.07 e_ref
(profiles/mesh_pc_margins.json)."""
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_bake_ref as MB
from tests import helpers
from tests.helpers import GOLDEN, ROOT, bits, load, record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
FINGER = os.path.join(GOLDEN, "finger.stl")
SENTINEL = -777.25


def ref32(pts, part_of, R, T, sel):
    """numpy float32, one rounding per operation, in the contract's association; sel (K,), (B, K) or None -> (B, K, 3).  A point
    whose q is outside [0, Q) or whose part is outside [0, M) is NaN."""
    B, M = R.shape[:2]
    Q = len(pts)
    q = np.arange(Q) if sel is None else np.asarray(sel, dtype=np.int64)
    q = np.broadcast_to(q, (B, q.shape[-1]))
    okq = (q >= 0) & (q < Q)
    qc = np.where(okq, q, 0)
    p = part_of.astype(np.int64)[qc]
    ok = okq & (p >= 0) & (p < M)
    pc = np.where(ok, p, 0)
    x = pts.astype(np.float32)[qc]                                                      # (B, K, 3)
    Rs = R.astype(np.float32)[np.arange(B)[:, None], pc]                                # (B, K, 3, 3)
    Ts = T.astype(np.float32)[np.arange(B)[:, None], pc]
    v = ((x[..., None, 0] * Rs[..., 0] + x[..., None, 1] * Rs[..., 1]) + x[..., None, 2] * Rs[..., 2]) + Ts
    assert v.dtype == np.float32
    return np.where(ok[..., None], v, np.float32(np.nan))


def scene(B, M, p, seed):
    """Seeded part clouds (M, p, 3) and poses; a PCfromMesh over them."""
    from partmanip_amd.mesh2pc import PCfromMesh
    from tests.mesh_tsdf_parts import random_poses
    rng = np.random.RandomState(seed)
    pcs = rng.uniform(-0.07, 0.07, size=(M, p, 3)).astype(np.float32)
    R, T = random_poses(seed + 1, B, M)
    return PCfromMesh(B, DEV, num_points=p, part_pcs=pcs), pcs, R, T


# ------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ["mesh_pc_ref_small", "mesh_pc_ref_1024"])
def test_reference_parity(name):
    from partmanip_amd.mesh2pc import PCfromMesh
    fx = load(name)
    b, (m, p, _) = fx["R"].shape[0], fx["part_pcs"].shape
    pc = PCfromMesh(b, DEV, num_points=p, part_pcs=fx["part_pcs"])
    torch.manual_seed(int(fx["seed"]))
    got = pc.query_pc(t(fx["R"]), t(fx["T"]))
    assert tuple(got.shape) == (b, p, 3) and got.dtype == torch.float32
    assert pc.last_sel.dtype == torch.int32 and np.array_equal(pc.last_sel.cpu().numpy(), fx["perm"][:p])
    e_ref = float(np.abs(fx["out32"].astype(np.float64) - fx["out64"]).max())
    assert e_ref > 0
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - fx["out64"]).max())
    print(f"{name}: e_ref = {e_ref:.3e}; max |hip - out64| = {err:.3e} = {err / e_ref:.2f} e_ref")
    record_margin(f"{name}: max |hip - out64| / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    assert err <= 4 * e_ref
    want = ref32(fx["part_pcs"].reshape(-1, 3), np.arange(m * p, dtype=np.int32) // p, fx["R"], fx["T"], fx["perm"][:p])
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------- 2. bit-exactness
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("M", [1, 12, 70])                   # 70 parts: the poses no longer fit the kernel's LDS table
def test_bit_exact_over_shapes_and_selections(B, M):
    p = 64
    pc, pcs, R, T = scene(B, M, p, 100 + B + M)
    pts, part_of = pcs.reshape(-1, 3), np.arange(M * p, dtype=np.int32) // p
    Rd, Td = t(R), t(T)
    rng = np.random.RandomState(5)
    for K in (61, 64):
        shared = rng.randint(0, M * p, size=K).astype(np.int32)
        per_env = rng.randint(0, M * p, size=(B, K)).astype(np.int32)
        for sel in (shared, per_env):
            got = pc.query_pc(Rd, Td, sel=t(sel))
            assert tuple(got.shape) == (B, K, 3)
            assert np.array_equal(bits(got), bits(ref32(pts, part_of, R, T, sel))), (K, sel.shape)
        # a per-environment selection that is a column slice of a wider table (row stride > K)
        wide = t(np.concatenate([per_env, per_env[:, ::-1]], axis=1))
        got = pc.query_pc(Rd, Td, sel=wide[:, :K])
        assert np.array_equal(bits(got), bits(ref32(pts, part_of, R, T, per_env)))
    got = pc.query_pc(Rd, Td, select='all')
    assert tuple(got.shape) == (B, M * p, 3) and pc.last_sel is None
    assert np.array_equal(bits(got), bits(ref32(pts, part_of, R, T, None)))


def test_all_points_of_three_parts():
    pc, pcs, R, T = scene(37, 3, 64, 131)
    got = pc.query_pc(t(R), t(T), select='all')
    assert tuple(got.shape) == (37, 3 * 64, 3)
    assert np.array_equal(bits(got), bits(ref32(pcs.reshape(-1, 3), np.arange(192, dtype=np.int32) // 64, R, T, None)))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("K", [61, 64])
def test_out_views_at_every_row_alignment_leave_the_tail_alone(off, K):
    B, M, p = 37, 12, 64
    pc, pcs, R, T = scene(B, M, p, 140)
    sel = np.random.RandomState(6).randint(0, M * p, size=K).astype(np.int32)
    width = 3 * K + 5                                        # odd: the rows' alignment walks through all four residues
    buf = torch.full((B * width + 8,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + B * width].view(B, width)
    got = pc.query_pc(t(R), t(T), out=view, sel=t(sel))
    assert got.data_ptr() == view.data_ptr() and tuple(got.shape) == (B, K, 3)
    want = ref32(pcs.reshape(-1, 3), np.arange(M * p, dtype=np.int32) // p, R, T, sel)
    assert np.array_equal(bits(view[:, :3 * K]), bits(want.reshape(B, -1)))
    assert bool((view[:, 3 * K:] == SENTINEL).all()) and bool((buf[:off] == SENTINEL).all())
    assert bool((buf[off + B * width:] == SENTINEL).all())
    # one environment: the row stride of a one-row view is arbitrary (n + 5, n + 5 and 1 here) and must reach the kernel as n
    n, R1, T1 = 3 * K, t(R[:1]), t(T[:1])
    want1 = pc.query_pc(R1, T1, sel=t(sel))
    wide, flat, col = (torch.full(s, SENTINEL, device=DEV) for s in ((1, n + 5), (n + 5,), (n + 5, 1)))
    for base, out in ((wide, wide[:, :n]), (flat, flat[None]), (col, col.t())):
        got = pc.query_pc(R1, T1, out=out, sel=t(sel))
        assert got.data_ptr() == base.data_ptr() and np.array_equal(bits(got), bits(want1))
        assert bool((base.reshape(-1)[n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------- 3. guards
def test_bad_indices_and_bad_poses_become_nan_and_nothing_else_changes():
    from partmanip_amd import ops
    B, M, p, K = 5, 12, 64, 61
    pc, pcs, R, T = scene(B, M, p, 150)
    Q = M * p
    pts, part_of = pcs.reshape(-1, 3), np.arange(Q, dtype=np.int32) // p
    sel = np.random.RandomState(7).randint(0, Q, size=(B, K)).astype(np.int32)
    Rd, Td = t(R), t(T)
    clean = pc.query_pc(Rd, Td, sel=t(sel)).clone()
    assert not torch.isnan(clean).any()
    bad = sel.copy()
    bad[0, 3], bad[2, 0], bad[4, K - 1], bad[1, 17] = -1, Q, Q, -1      # one step outside, never farther
    victim = int(sel[3, 5])                                              # a point some selection really uses
    bad_part = part_of.copy()
    bad_part[victim] = M
    got = ops.mesh_pc_query(pc.pts, t(bad_part), Rd, Td, t(bad)).view(B, K, 3)
    expect_nan = (bad < 0) | (bad >= Q) | (np.where((bad >= 0) & (bad < Q), bad, 0) == victim)
    assert expect_nan[3, 5] and expect_nan.sum() >= 5
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.broadcast_to(expect_nan[..., None], g.shape))
    assert np.array_equal(bits(g)[~expect_nan], bits(clean)[~expect_nan])
    assert np.array_equal(bits(g)[~expect_nan], bits(ref32(pts, bad_part, R, T, bad))[~expect_nan])
    # a NaN in one part's pose of one environment: exactly the points of that part in that environment
    Rn = R.copy()
    Rn[2, 7, 1, 1] = np.nan
    g = pc.query_pc(t(Rn), Td, sel=t(sel)).cpu().numpy()
    hit = np.zeros((B, K), dtype=bool)
    hit[2] = part_of[sel[2]] == 7
    assert hit.sum() >= 1
    assert np.array_equal(np.isnan(g).any(axis=-1), hit)
    assert np.array_equal(bits(g)[~hit], bits(clean)[~hit])


# ------------------------------------------------------------------------------------------- 4. farthest-point selection
def test_fps_selection_is_the_oracle_fps_of_the_full_cloud():
    from oracle import ref_cpu
    from partmanip_amd.mesh2pc import PCfromMesh
    from tests.mesh_tsdf_parts import random_poses
    B, M, p, K = 5, 3, 40, 16
    pcs = np.random.RandomState(160).uniform(-0.07, 0.07, size=(M, p, 3)).astype(np.float32)
    R, T = random_poses(161, B, M)
    pc = PCfromMesh(B, DEV, num_points=K, part_pcs=pcs)
    full = pc.query_pc(t(R), t(T), select='all').clone()
    got = pc.query_pc(t(R), t(T), select='fps')
    idx = pc.last_sel
    assert tuple(got.shape) == (B, K, 3) and tuple(idx.shape) == (B, K) and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), ref_cpu.fps(full.cpu().numpy(), K))
    want = torch.gather(full, 1, idx.long().unsqueeze(-1).expand(B, K, 3))
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------- 5. repeatability
def test_two_calls_give_the_same_bits():
    pc, pcs, R, T = scene(37, 12, 64, 170)
    sel = t(np.random.RandomState(8).randint(0, 768, size=(37, 64)).astype(np.int32))
    a = pc.query_pc(t(R), t(T), sel=sel).clone()
    b = pc.query_pc(t(R), t(T), sel=sel)
    assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------- 6. construction from files
def test_construction_from_mesh_files(tmp_path):
    from partmanip_amd import meshio
    from partmanip_amd.mesh2pc import PCfromMesh, random_poses
    rng = np.random.RandomState(61)
    boxes = [MB.box_mesh(rng.uniform(0.0101, 0.0249, size=3), rng.uniform(-0.005, 0.005, size=3)) for _ in range(9)]
    torus = MB.torus_mesh(nu=24, nv=12)
    finger = meshio.load_mesh(FINGER)
    vis = tmp_path / "assets" / "franka_description" / "meshes" / "visual"
    vis.mkdir(parents=True)
    (tmp_path / "assets" / "objs" / "cube").mkdir(parents=True)
    for i in range(8):
        meshio.save_obj(str(vis / f"link{i}.obj"), *boxes[i])
    meshio.save_obj(str(vis / "hand.obj"), *torus)
    shutil.copy(FINGER, vis / "finger.stl")
    meshio.save_obj(str(tmp_path / "assets" / "objs" / "cube" / "cube.obj"), *boxes[8])
    pc = PCfromMesh(4, DEV, asset_root=str(tmp_path))
    assert pc.part_num == 12 and tuple(pc.part_pc.shape) == (12, 1024, 3) and pc.part_pc.dtype == torch.float32
    got = pc.part_pc.cpu().numpy()
    assert not np.array_equal(got[9], got[10])               # the two fingers: one file, two seeds
    for i, (v, f) in enumerate(boxes[:8] + [torus, finger, finger, boxes[8]]):
        v, f = meshio.load_mesh(str(vis / "hand.obj")) if i == 8 else (v, f)     # what the object read: the written file
        d = MB.evaluate(got[i], v, f)["d"].max()
        assert d <= 2.0 ** -22 * float(np.abs(v).max()), (i, d)
    R, T = random_poses(4, 12, torch.Generator(device=DEV).manual_seed(2), DEV)
    cloud = pc.query_pc(R, T)
    assert tuple(cloud.shape) == (4, 1024, 3) and bool(torch.isfinite(cloud).all())


# ------------------------------------------------------------------------------------------- 7. the feeder
def test_feeder_serves_posed_mesh_clouds_and_ppo_trains_on_them(tmp_path):
    from partmanip_amd.algorithms import ppo
    from partmanip_amd.feeder import FeederEnv, ScreenLogger
    from partmanip_amd.mesh2pc import PCfromMesh, random_poses
    N, P = 8, 1024
    pc = PCfromMesh(N, DEV, num_points=P, part_pcs=load("mesh_pc_ref_1024")["part_pcs"])
    env = FeederEnv(N, {'depth_pc': 3 * P + 7}, 10, DEV, seed=11, max_episode_length=5, pc_source=pc)
    obs = env.reset()['depth_pc']
    assert tuple(obs.shape) == (N, 3 * P + 7)
    R, T = env.last_pc_poses
    sel = pc.last_sel
    direct = pc.query_pc(R, T, sel=sel)
    assert np.array_equal(bits(obs[:, :3 * P]), bits(direct.reshape(N, -1)))
    g = torch.Generator(device=DEV).manual_seed(11)                     # the feeder's own draws, in its order
    R2, T2 = random_poses(N, 12, g, DEV)
    sel2 = torch.randperm(12 * P, device=DEV, generator=g)[:P].to(torch.int32)
    tail = torch.randn(N, 7, device=DEV, generator=g)
    assert torch.equal(R, R2) and torch.equal(T, T2) and torch.equal(sel, sel2) and torch.equal(obs[:, 3 * P:], tail)
    assert float(obs[:, :3 * P].abs().max()) < 1.0           # scene-sized, not U([-1.5, 1.5])
    # without a source nothing changes
    a, b = FeederEnv(N, {'depth_pc': 3 * P + 7}, 10, DEV, seed=11), FeederEnv(N, {'depth_pc': 3 * P + 7}, 10, DEV, seed=11, pc_source=None)
    assert torch.equal(a.reset()['depth_pc'], b.reset()['depth_pc'])
    # one PPO iteration over the mesh clouds
    cfg = dict(num_envs=N, obs_mode='depth_pc', succ_value=None,
               model=dict(action_std=0.5, action_activate="tanh", clipAction=1.0,
                          network=dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=True)),
               max_iterations=1, n_steps=2, n_updates=1, n_minibatches=2, device=DEV, eval_round=1, eval_frequence=1,
               save_frequence=1, test_only=False, save_pose=False, save_video=False, lr_schedule="linear_decay",
               lr=1e-4, desired_kl=0.1, epsilon_clip=0.2, gamma=0.99, lam=0.95,
               tricks=dict(mini_adv_norm=True, whole_adv_norm=True, use_state_norm=False,
                           use_clipped_value_loss=True, use_grad_clip=True, max_grad_norm=0.5),
               sampler="random", resume=None)
    run = ppo(env, cfg, ScreenLogger(str(tmp_path), "g", "n", quiet=True))
    before = torch.cat([q.detach().reshape(-1).clone() for q in run.actor_critic.parameters()])
    run.run()
    after = torch.cat([q.detach().reshape(-1) for q in run.actor_critic.parameters()])
    assert run.curr_iter == 1 and bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    assert np.isfinite(float(run.log_dict["Train/surrogate_loss"]))


# ------------------------------------------------------------------------------------------- 8. the timing tool
def test_timing_tool_tiny():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_mesh_pc.py"), "--tiny"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    row = res["sizes"][0]
    for k in ("random", "all", "fps"):
        assert row["hip_ms"][k] > 0, k
    assert row["torch_ms"] > 0 and row["share_of_output_bandwidth_floor"]["all"] > 0
