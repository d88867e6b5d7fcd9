"""Mesh bake on the GPU: TSDFfromMesh.mesh2sdf (pm_mesh_sdf_bake_f32, csrc/mesh_bake.hip) against the fp64 restatement of
tests/mesh_bake_ref.py and against analytic distances.

Parity with the reference's own bake is UNPINNED (fp64 restatement + analytic known answers): kaolin, trimesh and ManifoldPlus
cannot be installed here, so the reference's bake cannot be run to make fixtures; tests/test_mesh_bake_host.py proves the
restatement against known answers on the CPU before it judges the kernel here.

Tolerance: e_ref = max |fp32 numpy evaluation of the restatement - its fp64 evaluation| over the same voxels is what a plain fp32
evaluation of the contract loses; the kernel must stay within 4 e_ref of fp64 (this project's margin convention).  Signs are
compared wherever fp64 itself is decided: |d64| > 4 e_ref on closed meshes, ||w64| - 0.5| >= 0.05 on the open one, and the
share of voxels so excluded is capped.  Every observed figure is recorded beside its bound (tests/helpers.record_margin)."""
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_bake_ref as M
from tests import mesh_tsdf_parts as P
from tests.helpers import GOLDEN, ROOT, record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FINGER = os.path.join(GOLDEN, "finger.stl")


def baker():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    return TSDFfromMesh(1, 0.5, 50, DEV, sdf_dicts=P.make_parts(7, "cut"), bake=True)


def gpu_bake(v, f, tri_cull=True):
    d = baker().mesh2sdf(vertices=v, faces=f, tri_cull=tri_cull)
    shape, tables, bbox_min = M.grid_layout(v)
    assert d["sdf"].shape == shape and d["sdf"].dtype == np.float32
    assert np.array_equal(np.asarray(d["bbox_min"]), bbox_min) and d["voxel_size"] == 0.002
    assert np.all(np.isfinite(d["sdf"])) and np.abs(d["sdf"]).max() <= np.float32(M.TRUNC)
    return d["sdf"], tables


@functools.lru_cache(maxsize=None)
def finger_mesh():
    from partmanip_amd import meshio
    return meshio.load_mesh(FINGER)


@functools.lru_cache(maxsize=None)
def finger_eval(dtype):
    v, f = finger_mesh()
    _, tables, _ = M.grid_layout(v)
    return M.evaluate(M.grid_points(tables), v, f, dtype=dtype)


def check_against_fp64(name, got, r64, r32, decided, cap):
    """got / r64 / r32 over the same voxels.  Magnitude and value within 4 e_ref; sign identical wherever `decided` (None: wherever
    |d64| > 4 e_ref)."""
    # e_ref on the clamped magnitude: where fp32 and fp64 agree on the sign this IS |sdf32 - sdf64|, and it stays meaningful on the
    # open mesh, where an fp32 winding number next to 0.5 may flip a sign (a difference of 2 |d| that says nothing about precision)
    e_ref = float(np.abs(np.minimum(r32["d"].astype(np.float64), M.TRUNC) - np.minimum(r64["d"], M.TRUNC)).max())
    assert 0 < e_ref < 1e-6, e_ref
    got = got.astype(np.float64)
    mag_err = float(np.abs(np.abs(got) - np.minimum(r64["d"], M.TRUNC)).max())
    print(f"{name}: e_ref = {e_ref:.3e}; max ||hip| - min(d64, trunc)| = {mag_err:.3e} = {mag_err / e_ref:.2f} e_ref")
    record_margin(f"{name}: max magnitude error / e_ref", mag_err / e_ref, 4.0, e_ref=e_ref)
    np.testing.assert_allclose(np.abs(got), np.minimum(r64["d"], M.TRUNC), rtol=0, atol=4 * e_ref, err_msg=name + " magnitude")
    if decided is None:
        decided = r64["d"] > 4 * e_ref
    excluded = float(1.0 - decided.mean())
    wrong = int(((got < 0) != (r64["sdf"] < 0))[decided].sum())
    print(f"{name}: sign compared on {int(decided.sum())} of {decided.size} voxels (excluded share {excluded:.5f}, cap {cap}); "
          f"wrong signs: {wrong}")
    record_margin(f"{name}: share of voxels excluded from the sign comparison", excluded, cap)
    record_margin(f"{name}: wrong signs among the compared voxels", wrong, 0)
    assert excluded <= cap
    assert wrong == 0
    np.testing.assert_allclose(got[decided], r64["sdf"][decided], rtol=0, atol=4 * e_ref, err_msg=name + " signed value")
    return e_ref


# ------------------------------------------------------------------------------------------- 1. box, analytic
def test_box_whole_grid_against_the_analytic_distance():
    v, f = M.box_mesh()
    got, tables = gpu_bake(v, f)
    pts = M.grid_points(tables)
    r64, r32 = M.evaluate(pts, v, f), M.evaluate(pts, v, f, dtype=np.float32)
    e_ref = float(np.abs(r32["sdf"].astype(np.float64) - r64["sdf"]).max())
    v64 = v.astype(np.float64)
    c, h = (v64.max(0) + v64.min(0)) / 2, (v64.max(0) - v64.min(0)) / 2
    d = P._box_sdf(pts.astype(np.float64) - c, h)
    want = np.clip(d, -M.TRUNC, M.TRUNC)
    g = got.reshape(-1).astype(np.float64)
    err = float(np.abs(g - want).max())
    print(f"box, {g.size} voxels: e_ref = {e_ref:.3e}; max |hip - analytic| = {err:.3e} = {err / e_ref:.2f} e_ref")
    assert 0 < e_ref < 1e-6
    record_margin("box: max |hip - analytic| / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    near = np.abs(d) < e_ref
    assert np.array_equal((g < 0)[~near], (d < 0)[~near]), "a sign differs away from the surface"
    assert near.mean() < 1e-3
    np.testing.assert_allclose(g, want, rtol=0, atol=4 * e_ref)
    assert 0.02 < np.mean(g < 0) < 0.5 and np.mean(g == np.float32(M.TRUNC)) > 0.01


# ------------------------------------------------------------------------------------------- 2. finger.stl, closed, whole grid
def test_finger_whole_grid_against_fp64():
    v, f = finger_mesh()
    got, _ = gpu_bake(v, f)
    assert got.shape == (51, 67, 54)
    r64, r32 = finger_eval(np.float64), finger_eval(np.float32)
    check_against_fp64("finger", got.reshape(-1), r64, r32, None, 1e-3)
    assert np.mean(got < 0) > 0.003


# ------------------------------------------------------------------------------------------- 3. hand.obj, open, sampled
def test_hand_sample_against_fp64():
    from partmanip_amd import meshio
    v, f = meshio.load_mesh(M.hand_obj())
    got, tables = gpu_bake(v, f)
    assert got.shape == (72, 86, 143)
    cand = np.random.RandomState(41).permutation(got.size)[:12000]                # seeded candidates, in seeded order
    c64 = M.evaluate(M.grid_points(tables, cand), v, f)
    near = np.flatnonzero(c64["d"] < M.TRUNC)[:2048]
    assert len(near) == 2048, "fewer than 2048 of the 12000 candidates lie inside the truncation band"
    rest = np.setdiff1d(np.arange(len(cand)), near, assume_unique=True)[:2048]
    pick = np.sort(np.concatenate([near, rest]))
    assert len(pick) == 4096
    idx = cand[pick]
    r64 = {k: a[pick] for k, a in c64.items()}
    r32 = M.evaluate(M.grid_points(tables, idx), v, f, dtype=np.float32)
    decided = np.abs(np.abs(r64["w"]) - 0.5) >= 0.05
    check_against_fp64("hand", got.reshape(-1)[idx], r64, r32, decided, 0.01)
    assert np.mean(got < 0) > 0.01


# ------------------------------------------------------------------------------------------- 4. torus, 20 000 triangles
def test_torus_sample_against_fp64_whole_grid_against_analytic_and_cull_bit_identity():
    v, f = M.torus_mesh()
    assert len(f) == 20000
    got, tables = gpu_bake(v, f)
    assert got.shape == (151, 151, 70)
    idx = np.sort(np.random.RandomState(42).choice(got.size, size=2048, replace=False))
    pts = M.grid_points(tables, idx)
    r64, r32 = M.evaluate(pts, v, f), M.evaluate(pts, v, f, dtype=np.float32)
    e_ref = check_against_fp64("torus sample", got.reshape(-1)[idx], r64, r32, None, 1e-3)
    H = M.torus_chord_bound()
    own = float(np.abs(r64["sdf"] - np.clip(M.torus_sdf(pts), -M.TRUNC, M.TRUNC)).max())
    print(f"torus: fp64 restatement vs analytic on the sample {own:.3e}, bound H = {H:.3e}")
    assert own <= H
    want = np.clip(M.torus_sdf(M.grid_points(tables)), -M.TRUNC, M.TRUNC)
    err = float(np.abs(got.reshape(-1).astype(np.float64) - want).max())
    print(f"torus, whole grid {got.size}: max |hip - analytic| = {err:.3e}, bound H + 4 e_ref = {H + 4 * e_ref:.3e}")
    record_margin("torus whole grid: max |hip - analytic| / (H + 4 e_ref)", err / (H + 4 * e_ref), 1.0, H=H, e_ref=e_ref)
    np.testing.assert_allclose(got.reshape(-1), want, rtol=0, atol=H + 4 * e_ref)
    off, _ = gpu_bake(v, f, tri_cull=False)
    assert np.array_equal(got.view(np.uint32), off.view(np.uint32)), "tri_cull changed bits"


def test_cull_is_bit_identical_on_the_open_mesh_and_the_finger():
    from partmanip_amd import meshio
    for path in (FINGER, M.hand_obj()):
        v, f = meshio.load_mesh(path)
        on, _ = gpu_bake(v, f, tri_cull=True)
        off, _ = gpu_bake(v, f, tri_cull=False)
        assert np.array_equal(on.view(np.uint32), off.view(np.uint32)), path


# ------------------------------------------------------------------------------------------- 5. degenerate faces, repeatability
def test_degenerate_faces_change_nothing_and_bakes_repeat():
    v, fa, fb = M.degenerate_mesh()
    a, _ = gpu_bake(v, fa)
    b, _ = gpu_bake(v, fb)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.mean(a < 0) > 0.02
    a2, _ = gpu_bake(v, fa)
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    tv, tf = M.torus_mesh(nu=24, nv=16)
    t1, _ = gpu_bake(tv, tf)
    t2, _ = gpu_bake(tv, tf)
    assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32))


# ------------------------------------------------------------------------------------------- 6. end to end
E2E_TORUS = dict(R=0.0151, r=0.0063, nu=16, nv=16)


def e2e_meshes():
    """The twelve parts' meshes in the reference's order (finger twice): seeded boxes for the links and the cube, one coarse torus
    for the hand, the real finger."""
    rng = np.random.RandomState(61)
    boxes = []
    for _ in range(9):
        half = rng.uniform(0.0101, 0.0249, size=3)
        centre = rng.uniform(-0.005, 0.005, size=3)
        boxes.append(M.box_mesh(half, centre))
    torus = M.torus_mesh(**E2E_TORUS)
    names = [f"link{i}.obj" for i in range(8)] + ["hand.obj", "finger.stl", "finger.stl", "cube.obj"]
    meshes = boxes[:8] + [torus, finger_mesh(), finger_mesh(), boxes[8]]
    for name, (v, _) in zip(names, meshes):
        r = M.range_over_voxel(v)
        assert np.all(np.abs(r - np.round(r)) > 1e-3), (name, r)
    return names, meshes


def test_end_to_end_bake_save_reload_and_query(tmp_path):
    from partmanip_amd import meshio, ops
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    names, meshes = e2e_meshes()
    vis = tmp_path / "assets" / "franka_description" / "meshes" / "visual"
    vis.mkdir(parents=True)
    (tmp_path / "assets" / "objs" / "cube").mkdir(parents=True)
    for name, (v, f) in zip(names[:9], meshes[:9]):
        meshio.save_obj(str(vis / name), v, f)
    shutil.copy(FINGER, vis / "finger.stl")
    meshio.save_obj(str(tmp_path / "assets" / "objs" / "cube" / "cube.obj"), *meshes[11])
    B = 2
    ops.TIMER.enable("mesh_sdf_bake")
    try:
        first = TSDFfromMesh(B, 0.5, 50, DEV, bake=True, asset_root=str(tmp_path))
        assert len(ops.TIMER.events["mesh_sdf_bake"]) == 11                 # the finger is baked once
        files = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*.npy"))
        sdf_dir = os.path.join("assets", "franka_description", "sdf", "visual")
        assert files == sorted([os.path.join(sdf_dir, n) for n in [f"link{i}.npy" for i in range(8)] + ["hand.npy", "finger.npy"]]
                               + [os.path.join("assets", "objs", "cube", "sdf.npy")])
        ops.TIMER.enable("mesh_sdf_bake")
        second = TSDFfromMesh(B, 0.5, 50, DEV, bake=True, asset_root=str(tmp_path))
        assert len(ops.TIMER.events["mesh_sdf_bake"]) == 0, "the second construction baked again"
        third = TSDFfromMesh(B, 0.5, 50, DEV, asset_root=str(tmp_path))      # and the files serve an object without bake=True
    finally:
        ops.TIMER.disable()
    d = np.load(tmp_path / sdf_dir / "finger.npy", allow_pickle=True).item()
    assert sorted(d) == ["bbox_min", "sdf", "voxel_size"]
    assert d["sdf"].dtype == np.float32 and d["sdf"].shape == (51, 67, 54)
    assert d["bbox_min"].dtype == np.float32 and d["bbox_min"].shape == (3,) and d["voxel_size"] == 0.002
    assert first.part_num == second.part_num == 12 and torch.equal(first.sdf_field, second.sdf_field)
    assert torch.equal(first.sdf_field, third.sdf_field)

    # the observation over the baked grids against the fp64 composition: fp64 bakes sampled by the fp64 query restatement
    parts64, parts32 = [], []
    for name, (v, f) in zip(names, meshes):
        if name == "finger.stl":
            shape, _, bbox_min = M.grid_layout(v)
            s64, s32 = finger_eval(np.float64)["sdf"].reshape(shape), finger_eval(np.float32)["sdf"].reshape(shape)
        else:
            shape, tables, bbox_min = M.grid_layout(v)
            pts = M.grid_points(tables)
            s64 = M.evaluate(pts, v, f)["sdf"].reshape(shape)
            s32 = M.evaluate(pts, v, f, dtype=np.float32)["sdf"].reshape(shape)
        parts64.append({'sdf': s64, 'bbox_min': bbox_min, 'voxel_size': 0.002})
        parts32.append({'sdf': s32.astype(np.float64), 'bbox_min': bbox_min, 'voxel_size': 0.002})
    for got, w in zip(second.sdf_dict_list, parts64):
        assert got["sdf"].shape == w["sdf"].shape and np.array_equal(got["bbox_min"], w["bbox_min"])
    R, T = P.random_poses(6201, B)
    want, margin = P.restate(parts64, R, T)
    via32, _ = P.restate(parts32, R, T)
    # the composition's own fp32 loss: what the fp32-evaluated bakes change in the volume, plus what the reference's fp32 query
    # loses on fp32 grids (e_ref of tests/test_gpu_mesh_tsdf.py, from the reference's own fp32 and fp64 runs)
    fx = P.load_family("mesh_tsdf_cont", GOLDEN)
    e_query = float(max(np.abs(fx["scene32"] - fx["scene64"]).max(), np.abs(fx["obj32"] - fx["obj64"]).max()))
    e_bake = float(np.abs(via32 - want).max())
    e_comp = e_bake + e_query
    got = second.query_tsdf(torch.from_numpy(R).to(DEV), torch.from_numpy(T).to(DEV)).cpu().numpy().astype(np.float64)
    away = (margin >= 1e-3).reshape(got.shape)
    err = float(np.abs(got - want)[away].max())
    print(f"end to end: e_bake = {e_bake:.3e}, e_query = {e_query:.3e}; max |hip - fp64 composition| = {err:.3e} = "
          f"{err / e_comp:.2f} e_comp; border voxels excluded {int((~away).sum())} of {away.size}")
    record_margin("end to end: max |hip - fp64 composition| / e_comp", err / e_comp, 4.0, e_bake=e_bake, e_query=e_query)
    record_margin("end to end: share of border voxels excluded", float((~away).mean()), 0.01)
    assert (~away).mean() < 0.01 and (want[away] < 1.0).mean() > 0.05
    np.testing.assert_allclose(got[away], want[away], rtol=0, atol=4 * e_comp)


# ------------------------------------------------------------------------------------------- 7. the timer
def test_timer_tool_runs_to_its_json_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_mesh_bake.py"), "--tiny"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    row = res["cases"][0]
    assert row["triangles"] > 0 and row["hip_ms"] > 0 and row["torch_ms"] > 0 and row["pairs_per_s"] > 0
    assert 0 < row["share_of_valu_floor"] <= 1.5
