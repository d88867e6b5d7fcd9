"""Mesh-TSDF observation on the GPU: partmanip_amd.mesh2sdf.TSDFfromMesh (pm_mesh_tsdf_query_f32) against the REFERENCE's own
volumes (fixtures of tests/golden/make_mesh_tsdf_golden.py: the reference run in fp32 and in fp64 on the same inputs) and
against the fp64 restatement of tests/mesh_tsdf_parts.py.

Tolerance: e_ref = max |ref32 - ref64| of the fixture is what the reference itself loses to fp32; the HIP path must stay within
4 e_ref of ref64 (this project's margin convention; the reference's bmm and the kernel round the 3x3 product in different
orders, so the maxima of the two fp32 error populations differ by a small factor)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_tsdf_parts as P
from tests.helpers import GOLDEN, ROOT, record_margin, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = P.RES ** 3


def family(name):
    fx = P.load_family(name, GOLDEN)
    parts = P.fixture_parts("cut" if name == "mesh_tsdf_cut" else "cont")
    assert [P.parts_digest([d]) for d in parts] == list(fx["part_sha"]), "regenerated part grids differ from the fixture's"
    return fx, parts


def make(parts, B, res=P.RES, size=P.SIZE):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    return TSDFfromMesh(B, size, res, DEV, sdf_dicts=parts, vox_origin=list(P.ORIGIN))


def cont_e_ref():
    fx = P.load_family("mesh_tsdf_cont", GOLDEN)
    return float(max(np.abs(fx["scene32"] - fx["scene64"]).max(), np.abs(fx["obj32"] - fx["obj64"]).max()))


def dev(a):
    return t(a).to(DEV)


# ------------------------------------------------------------------------------------------- 4. the continuous family
def test_cont_family_matches_the_reference():
    fx, parts = family("mesh_tsdf_cont")
    e_ref = cont_e_ref()
    print(f"e_ref = {e_ref:.3e}")
    assert 0 < e_ref < 1e-5
    obj = make(parts, 2)
    R, T = dev(fx["pose_R"]), dev(fx["pose_T"])
    full = obj.query_tsdf(R, T).cpu().numpy()
    scene, ob = (v.cpu().numpy() for v in obj.query_tsdf_seperately(R, T))
    assert full.shape == scene.shape == ob.shape == (2, 50, 50, 50)
    for name, got, want in (("query_tsdf", full, np.minimum(fx["scene64"], fx["obj64"])), ("scene", scene, fx["scene64"]),
                            ("obj", ob, fx["obj64"])):
        print(f"{name}: max |hip - ref64| = {np.abs(got - want).max():.3e} = {np.abs(got - want).max() / e_ref:.2f} e_ref")
        np.testing.assert_allclose(got, want, rtol=0, atol=4 * e_ref, err_msg=name)
    assert np.array_equal(np.minimum(scene, ob), full)                     # bit for bit, as in the reference
    assert np.array_equal(obj.query_tsdf_parallel(R, T).cpu().numpy(), full)


def test_cont_family_after_initialize_sdf_matches_the_reference():
    fx, parts = family("mesh_tsdf_cont_init")
    e_ref = float(np.abs(fx["ref32"] - fx["ref64"]).max())
    print(f"e_ref = {e_ref:.3e}")
    assert 0 < e_ref < 1e-5
    obj = make(parts, 1)
    obj.initialize_sdf(dev(fx["pred"]))
    got = obj.query_tsdf(dev(fx["pose_R"]), dev(fx["pose_T"])).cpu().numpy()
    print(f"max |hip - ref64| = {np.abs(got - fx['ref64']).max():.3e} = {np.abs(got - fx['ref64']).max() / e_ref:.2f} e_ref")
    np.testing.assert_allclose(got, fx["ref64"], rtol=0, atol=4 * e_ref)


# ------------------------------------------------------------------------------------------- 5. the cut family
def test_cut_family_differs_from_the_reference_only_on_the_valid_box_border():
    fx, parts = family("mesh_tsdf_cut")
    e_ref = cont_e_ref()
    obj = make(parts, 4)
    got = obj.query_tsdf(dev(fx["pose_R"]), dev(fx["pose_T"])).cpu().numpy()
    err = np.abs(got - fx["ref64"])
    differ = err > 4 * e_ref
    _, margin = P.restate(parts, fx["pose_R"], fx["pose_T"])
    margin = margin.reshape(got.shape)
    away = ~differ
    print(f"differing voxels: {int(differ.sum())} of {differ.size}; max error elsewhere {err[away].max():.3e} = "
          f"{err[away].max() / e_ref:.2f} e_ref; border margins of the differing: {margin[differ].tolist()}")
    record_margin("cut: voxels differing from ref64 by more than 4 e_ref", int(differ.sum()), 10)
    assert differ.size == 500000 and differ.sum() <= 10
    assert np.all(margin[differ] < 1e-3)


# ------------------------------------------------------------------------------------------- 6. bit-for-bit properties
def test_brick_skip_is_conservative():
    for fam, B in (("mesh_tsdf_cont", 2), ("mesh_tsdf_cut", 4)):
        fx, parts = family(fam)
        obj = make(parts, B)
        R, T = dev(fx["pose_R"]), dev(fx["pose_T"])
        on = obj.query_tsdf(R, T, brick_skip=True)
        off = obj.query_tsdf(R, T, brick_skip=False)
        assert torch.equal(on, off)
    # a sheared, scaled (non-orthonormal) R and a far-away part: still the same bits
    R2 = R.clone()
    R2[:, ::2] = R2[:, ::2] * 1.7 + 0.3
    T2 = T.clone()
    T2[:, 3] += 1.0e3
    assert torch.equal(obj.query_tsdf(R2, T2, brick_skip=True), obj.query_tsdf(R2, T2, brick_skip=False))


def test_strided_output_lands_in_an_observation_buffer_and_leaves_the_tail_alone():
    fx, parts = family("mesh_tsdf_cont")
    obj = make(parts, 2)
    R, T = dev(fx["pose_R"]), dev(fx["pose_T"])
    want = obj.query_tsdf(R, T)
    buf = torch.full((2, N + 17), float("nan"), device=DEV)
    got = obj.query_tsdf(R, T, out=buf)
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (2, 50, 50, 50)
    assert torch.equal(got, want) and torch.equal(buf[:, :N], want.reshape(2, -1))
    assert torch.isnan(buf[:, N:]).all()
    buf2 = torch.full((2, N + 17), float("nan"), device=DEV)
    obj.query_tsdf(R, T, out=buf2[:, :N])
    assert torch.equal(buf2[:, :N], want.reshape(2, -1)) and torch.isnan(buf2[:, N:]).all()
    with pytest.raises(ValueError):
        obj.query_tsdf(R, T, out=buf[:, :N - 1])
    # one environment: the row stride of a one-row view is arbitrary (N + 5, N + 5 and 1 here) and must reach the kernel as N
    want1 = obj.query_tsdf(R[:1], T[:1])
    assert not torch.isnan(want1).any()
    wide, flat, col = (torch.full(s, float("nan"), device=DEV) for s in ((1, N + 5), (N + 5,), (N + 5, 1)))
    for base, out in ((wide, wide[:, :N]), (flat, flat[None]), (col, col.t())):
        got = obj.query_tsdf(R[:1], T[:1], out=out)
        assert got.data_ptr() == base.data_ptr() and torch.equal(got.view(torch.int32), want1.view(torch.int32))
        assert torch.isnan(base.reshape(-1)[N:]).all()


def test_repeatable_and_stream_independent():
    fx, parts = family("mesh_tsdf_cont")
    obj = make(parts, 2)
    R, T = dev(fx["pose_R"]), dev(fx["pose_T"])
    a = obj.query_tsdf(R, T).clone()
    b = obj.query_tsdf(R, T)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = obj.query_tsdf(R, T)
    side.synchronize()
    assert torch.equal(a, c)


@pytest.mark.parametrize("B", [1, 37])
def test_batch_sizes_against_the_restatement(B):
    parts = P.fixture_parts("cont")
    e_ref = cont_e_ref()
    R, T = P.random_poses(4000 + B, B)
    want, _ = P.restate(parts, R, T)
    got = make(parts, B).query_tsdf(dev(R), dev(T)).cpu().numpy()
    print(f"B = {B}: max |hip - restatement| = {np.abs(got - want).max():.3e} = {np.abs(got - want).max() / e_ref:.2f} e_ref")
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * e_ref)


@pytest.mark.parametrize("res", [10, 32])
def test_resolutions_that_are_no_multiple_of_the_brick_edge(res):
    """1 cm voxels as in the fixtures (size = res cm), so the parts' clamp equals sdf_trunc and the volume stays continuous."""
    parts = P.fixture_parts("cont")
    e_ref = cont_e_ref()
    size = res * 0.01
    R, T = P.random_poses(5000 + res, 3)
    T = (T * np.float32(size / P.SIZE)).astype(np.float32)
    want, _ = P.restate(parts, R, T, res=res, size=size)
    obj = make(parts, 3, res=res, size=size)
    got = obj.query_tsdf(dev(R), dev(T))
    assert tuple(got.shape) == (3, res, res, res)
    assert torch.equal(got, obj.query_tsdf(dev(R), dev(T), brick_skip=False))
    got = got.cpu().numpy()
    assert (got < 1.0).mean() > 0.2
    print(f"res = {res}: max |hip - restatement| = {np.abs(got - want).max():.3e} = {np.abs(got - want).max() / e_ref:.2f} e_ref")
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * e_ref)


# ------------------------------------------------------------------------------------------- 7. non-finite pose
def test_non_finite_pose_poisons_its_environment_only():
    parts = P.fixture_parts("cont")
    R, T = P.random_poses(6001, 3)
    obj = make(parts, 3)
    clean = obj.query_tsdf(dev(R), dev(T)).clone()
    T2 = T.copy()
    T2[1, 4, 2] = np.nan
    got = obj.query_tsdf(dev(R), dev(T2))
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


# ------------------------------------------------------------------------------------------- 8. end to end into the student
def test_volume_written_into_the_observation_buffer_feeds_conv3dnet():
    from partmanip_amd.algo_utils import ActorCritic
    from tests.golden import cases
    c = cases.CONV3D_CASES["conv3d_proprio"]
    B, pr = c["B"], c["proprio"]
    ac = ActorCritic(N + pr, c["out"], dict(action_std=0.5, action_activate="tanh", clipAction=1.0,
                                            network=dict(name="Conv3DNet", activation="tanh")), pr).to(DEV)
    ac.actor.load_state_dict({k: t(v.copy()) for k, v in cases.conv3d_state(c).items()})
    ac.flat()
    parts = P.fixture_parts("cont")
    R, T = P.random_poses(7001, B)
    obj = make(parts, B)
    proprio = torch.randn(B, pr, generator=torch.Generator().manual_seed(3)).to(DEV)
    obs = torch.empty(B, N + pr, device=DEV)
    obs[:, N:] = proprio
    obj.query_tsdf(dev(R), dev(T), out=obs[:, :N])
    direct = ac.actor.hip_forward(obs).clone()
    vol = obj.query_tsdf(dev(R), dev(T))
    cat = torch.cat((vol.reshape(B, -1), proprio), dim=1)
    assert torch.equal(obs, cat)
    assert torch.equal(ac.actor.hip_forward(cat), direct)
    assert torch.isfinite(direct).all()


# ------------------------------------------------------------------------------------------- 9. the timer
def test_timer_tool_runs_to_its_json_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_mesh_tsdf.py"), "--tiny"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    row = res["sizes"][0]
    assert row["B"] == 4 and row["hip_ms"] > 0 and row["torch_ms"] > 0 and row["hip_share_of_floor"] > 0
