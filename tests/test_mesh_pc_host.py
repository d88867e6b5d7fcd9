"""Posed mesh point cloud (partmanip_amd.mesh2pc.PCfromMesh, pm_mesh_pc_query_f32), everything that needs no GPU: the surface
sampler meshio.sample_surface, the fixtures made from the reference's own query_pc (tests/golden/make_mesh_pc_golden.py), the C
ABI's argument checks and the host logic on the 'cpu' device.

Bounds.  On the surface: a sample is the float32 rounding of an fp64 point of its triangle, so it lies within half an ulp per
coordinate of the surface, 2^-24 max|v| per coordinate; the bound is 2^-22 max|v| (that with a factor 4).  Area-proportional: Pearson's
chi-square over 8 contiguous equal-area face bins against the 0.999 quantile at 7 degrees of freedom, 24.32."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mesh_bake_ref as MB
from tests.helpers import GOLDEN, load

FINGER = os.path.join(GOLDEN, "finger.stl")
FIXTURES = ("mesh_pc_ref_small", "mesh_pc_ref_1024")


def restate64(part_pcs, R, T, sel):
    """The query in fp64, written from its description: point q of part p under (R[b, p], T[b, p]) is R x + T."""
    m, p, _ = part_pcs.shape
    pts = part_pcs.reshape(-1, 3).astype(np.float64)[sel]
    part = (np.arange(m * p) // p)[sel]
    Rs, Ts = R.astype(np.float64)[:, part], T.astype(np.float64)[:, part]             # (b, K, 3, 3), (b, K, 3)
    return np.einsum("bkji,ki->bkj", Rs, pts) + Ts


def finger():
    from partmanip_amd import meshio
    return meshio.load_mesh(FINGER)


def draw(count=4096, seed=7):
    from partmanip_amd import meshio
    v, f = finger()
    pts, fi = meshio.sample_surface(v, f, count, torch.Generator().manual_seed(seed))
    return v, f, pts, fi


def areas_cdf(v, f):
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    return area, np.cumsum(area)


# ------------------------------------------------------------------------------------------- 1. the sampler
def test_samples_lie_on_the_surface():
    v, f, pts, fi = draw()
    assert pts.dtype == np.float32 and pts.shape == (4096, 3) and fi.dtype == np.int64 and fi.shape == (4096,)
    bound = 2.0 ** -22 * float(np.abs(v).max())
    d = MB.evaluate(pts, v, f)["d"]
    print(f"finger, 4096 samples: max distance to the surface {d.max():.3e}, bound {bound:.3e} (max|v| = {np.abs(v).max():.4f})")
    assert d.max() <= bound


def test_samples_are_area_proportional():
    v, f, pts, fi = draw()
    area, cdf = areas_cdf(v, f)
    edges = np.searchsorted(cdf, cdf[-1] * np.arange(1, 8) / 8.0, side="left") + 1      # 8 contiguous runs of faces of ~equal area
    bins = np.searchsorted(edges, fi, side="right")
    lo = np.concatenate([[0], edges])
    hi = np.concatenate([edges, [len(f)]])
    expect = np.array([area[a:b].sum() for a, b in zip(lo, hi)]) / cdf[-1] * len(fi)
    got = np.bincount(bins, minlength=8)
    chi2 = float(((got - expect) ** 2 / expect).sum())
    print(f"chi-square over 8 equal-area face bins: {chi2:.2f} (0.999 quantile at 7 dof: 24.32); counts {got.tolist()}")
    assert expect.min() > 100 and chi2 < 24.32


def test_sampler_is_seeded_and_its_weights_are_barycentric():
    from partmanip_amd import meshio
    v, f, pts, fi = draw()
    _, _, pts2, fi2 = draw()
    assert np.array_equal(pts.view(np.uint32), pts2.view(np.uint32)) and np.array_equal(fi, fi2)
    _, _, pts3, _ = draw(seed=8)
    assert not np.array_equal(pts, pts3)
    tri = v.astype(np.float64)[f[fi]]
    e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pts.astype(np.float64) - tri[:, 0]
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    a, b = (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det
    tol = 1e-5                                               # float32 rounding of the point over a millimetre-sized edge
    assert a.min() >= -tol and b.min() >= -tol and (a + b).max() <= 1 + tol
    # the uniforms behind the draw: no CDF boundary within 1e-9 * total of any u0 * total (the face pick is not a coin toss)
    u = torch.rand(4096, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64).numpy()
    _, cdf = areas_cdf(v, f)
    t = u[:, 0] * cdf[-1]
    gap = np.abs(t[:, None] - cdf[None, :]).min()
    print(f"minimum |u0 total - cdf boundary| / total = {gap / cdf[-1]:.2e}")
    assert gap > 1e-9 * cdf[-1]
    assert np.array_equal(fi, np.searchsorted(cdf, t, side="right"))
    with pytest.raises(ValueError):
        meshio.sample_surface(v, np.zeros((0, 3), dtype=np.int64), 8, torch.Generator().manual_seed(0))
    flat = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)                # collinear: no area
    with pytest.raises(ValueError):
        meshio.sample_surface(flat, np.array([[0, 1, 2]]), 8, torch.Generator().manual_seed(0))


def test_zero_area_faces_are_never_picked():
    from partmanip_amd import meshio
    v, fa, fb = MB.degenerate_mesh()                         # a box + a double-corner face + a collinear sliver
    kept = meshio.drop_double_corner_faces(v, fa)
    area, _ = areas_cdf(v, kept)
    assert (area == 0).sum() == 1
    # zero-area faces at the front, in the middle and at the end of the list
    sliver = kept[area == 0]
    faces = np.concatenate([sliver, kept[:5], sliver, kept[5:]], axis=0)
    pts, fi = meshio.sample_surface(v, faces, 20000, torch.Generator().manual_seed(3))
    area2, _ = areas_cdf(v, meshio.drop_double_corner_faces(v, faces))
    assert (area2[fi] > 0).all()
    assert len(np.unique(fi)) == 12                          # every real face is reached


# ------------------------------------------------------------------------------------------- 2. the fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_equals_the_fp64_restatement(name):
    fx = load(name)
    b, (m, p, _) = fx["R"].shape[0], fx["part_pcs"].shape
    assert m == 12 and fx["perm"].shape == (m * p,) and fx["out64"].shape == (b, p, 3) and fx["out32"].dtype == np.float32
    torch.manual_seed(int(fx["seed"]))
    assert np.array_equal(torch.randperm(m * p).numpy(), fx["perm"])       # the reference's subset under the seed
    want = restate64(fx["part_pcs"], fx["R"], fx["T"], fx["perm"][:p])
    err = float(np.abs(want - fx["out64"]).max())
    e_ref = float(np.abs(fx["out32"].astype(np.float64) - fx["out64"]).max())
    print(f"{name}: max |restatement - out64| = {err:.2e}; e_ref = max |out32 - out64| = {e_ref:.3e}")
    assert err <= 1e-15
    assert 0 < e_ref < 1e-6
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 256 * 1024


# ------------------------------------------------------------------------------------------- 3. the entry point
def test_entry_point_rejects_bad_arguments_before_any_launch():
    from partmanip_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION >= 155
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first

    def call(pts=p, part_of=p, Q=128, R=p, T=p, B=2, M=3, sel=p, sel_stride=0, K=16, out=p, out_stride=48):
        return lib.pm_mesh_pc_query_f32(pts, part_of, Q, R, T, B, M, sel, sel_stride, K, out, out_stride, None)
    assert call(pts=None) == -1 and call(part_of=None) == -1 and call(R=None) == -1 and call(T=None) == -1 and call(out=None) == -1
    assert call(B=0) == -1 and call(M=0) == -1 and call(Q=0) == -1 and call(K=0) == -1 and call(B=-2) == -1
    assert call(B=65535 * 16 + 1) == -1
    assert call(out_stride=47) == -1
    assert call(sel=None, K=16) == -1                        # identity needs K == Q
    assert call(sel_stride=15) == -1 and call(sel_stride=-1) == -1


# ------------------------------------------------------------------------------------------- 4. host logic on 'cpu'
def test_query_pc_refuses_cpu_tensors_and_wrong_shapes():
    from partmanip_amd import ops
    from partmanip_amd.mesh2pc import PCfromMesh, random_poses
    fx = load("mesh_pc_ref_small")
    pc = PCfromMesh(3, "cpu", num_points=64, part_pcs=fx["part_pcs"])
    assert pc.part_num == 12 and tuple(pc.part_pc.shape) == (12, 64, 3) and tuple(pc.pts.shape) == (768, 3)
    assert pc.part_of.dtype == torch.int32 and pc.part_of.tolist() == [i // 64 for i in range(768)]
    assert tuple(pc.all_pc.shape) == (36, 64, 3) and torch.equal(pc.all_pc[12:24], pc.part_pc)
    R, T = random_poses(3, 12, torch.Generator().manual_seed(1), "cpu")
    assert R.dtype == torch.float32 and tuple(R.shape) == (3, 12, 3, 3) and tuple(T.shape) == (3, 12, 3)
    eye = torch.eye(3).expand(3, 12, 3, 3)
    assert (R @ R.transpose(-1, -2) - eye).abs().max() < 1e-5 and T.abs().max() <= 0.25
    assert torch.linalg.det(R).sub(1).abs().max() < 1e-5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_pc_query(pc.pts, pc.part_of, R, T)
    for bad_R, bad_T in ((R[:, :11], T), (R, T[:, :11]), (R.reshape(3, 12, 9), T), (R, T[:2]), (R.double(), T.double())):
        with pytest.raises(ValueError):
            pc.query_pc(bad_R, bad_T)
    for bad_out in (torch.empty(3 * 192), torch.empty(2, 192), torch.empty(3, 191)):    # 1-D, wrong row count, too few columns
        with pytest.raises(ValueError, match="out"):
            pc.query_pc(R, T, out=bad_out)                   # the out view is checked before the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T, out=torch.empty(3, 192))
    with pytest.raises(ValueError):
        PCfromMesh(1, "cpu", part_pcs=np.zeros((12, 64, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        PCfromMesh(1, "cpu", num_points=8, meshes=[(np.zeros((3, 3), dtype=np.float32), np.array([[0, 1, 2]]))])


def test_feeder_without_pc_source_is_unchanged_and_checks_point_num():
    from partmanip_amd.feeder import FeederEnv
    from partmanip_amd.mesh2pc import PCfromMesh
    obs = {"normal_state": 53, "depth_pc": 3072 + 7}
    a, b = FeederEnv(4, obs, 10, "cpu", seed=3), FeederEnv(4, obs, 10, "cpu", seed=3, pc_source=None)
    for x, y in zip(a.reset().values(), b.reset().values()):
        assert torch.equal(x, y)
    pc = PCfromMesh(4, "cpu", num_points=64, part_pcs=load("mesh_pc_ref_small")["part_pcs"])
    with pytest.raises(ValueError, match="point_num"):
        FeederEnv(4, obs, 10, "cpu", seed=3, pc_source=pc)
