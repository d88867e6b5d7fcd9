"""Mesh bake (TSDFfromMesh.mesh2sdf, pm_mesh_sdf_bake_f32), everything that needs no GPU: the C ABI entry, the mesh readers, the
fp64 restatement of tests/mesh_bake_ref.py against known answers, the fp32 grid layout and the host logic on the 'cpu' device.

Parity with the reference's own bake is UNPINNED (fp64 restatement + analytic known answers): the reference bakes with kaolin
(CUDA only), trimesh and ManifoldPlus, none of which can be installed here, so no fixture of its output exists.  The yardstick
is the restatement, and this module is the proof that the yardstick itself is sound: it reproduces the analytic box distance to
1e-12, its winding-number sign equals an independent ray-parity sign on every closed mesh, and it stays within the tessellation
bound of the analytic torus."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import mesh_bake_ref as M
from tests.helpers import GOLDEN, ROOT
from tests.mesh_tsdf_parts import _box_sdf

FINGER = os.path.join(GOLDEN, "finger.stl")


def fixtures():
    from partmanip_amd import meshio
    dv, dfa, _ = M.degenerate_mesh()
    return {"box": M.box_mesh(), "torus": M.torus_mesh(), "degenerate": (dv, dfa), "finger": meshio.load_mesh(FINGER),
            "hand": meshio.load_mesh(M.hand_obj())}


# ------------------------------------------------------------------------------------------- 1. the entry point
def test_entry_point_is_exported_declared_and_typed():
    from partmanip_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "partmanip_hip.h")).read()
    for name, ret in (("pm_mesh_sdf_bake_f32", "int"), ("pm_mesh_sdf_bake_workspace_bytes", "size_t")):
        assert hasattr(so, name)
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), hdr)
    res, args = _lib.SIGNATURES["pm_mesh_sdf_bake_f32"]
    assert res is ctypes.c_int and len(args) == 15 and args[0] is ctypes.c_void_p and args[5] is ctypes.c_float
    assert args[13] is ctypes.c_size_t
    assert _lib.ABI_VERSION >= 154
    assert _lib.lib.pm_mesh_sdf_bake_workspace_bytes(0) == 0 and _lib.lib.pm_mesh_sdf_bake_workspace_bytes(624) >= 624 * 9 * 4


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from partmanip_amd._lib import lib
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first

    def call(tri=p, F=12, X=8, Y=8, Z=8, vs=0.002, trunc=0.04, sdf=p, ws=p, nbytes=None):
        nbytes = lib.pm_mesh_sdf_bake_workspace_bytes(max(F, 1)) if nbytes is None else nbytes
        return lib.pm_mesh_sdf_bake_f32(tri, F, X, Y, Z, vs, 0.0, 0.0, 0.0, trunc, 1, sdf, ws, nbytes, None)
    assert call(tri=None) == -1 and call(sdf=None) == -1 and call(ws=None) == -1
    assert call(F=0) == -1 and call(F=-3) == -1
    assert call(X=0) == -1 and call(Y=-1) == -1 and call(Z=0) == -1
    assert call(vs=0.0) == -1 and call(vs=-0.002) == -1 and call(trunc=0.0) == -1
    assert call(X=2048, Y=1024, Z=1024) == -1                # 2^31 cells
    assert call(nbytes=16) == -1


# ------------------------------------------------------------------------------------------- 2. the mesh readers
def test_obj_reader_forms(tmp_path):
    from partmanip_amd import meshio
    path = tmp_path / "forms.obj"
    path.write_text("# comment\nmtllib x.mtl\no thing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ns off\nusemtl m\n"
                    "f 1 2 3\nf 1/1 2/1 3/1\nf 1/1/1 2/1/1 4/1/1\nf 1//1 3//1 4//1\nf -4 -3 -2\nv 0.5 0.5 1\nf 1 2 3 4 5\n")
    v, f = meshio.load_mesh(str(path))
    assert v.dtype == np.float32 and f.dtype == np.int64 and v.shape == (5, 3)
    assert f.tolist() == [[0, 1, 2], [0, 1, 2], [0, 1, 3], [0, 2, 3], [0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    with pytest.raises(ValueError):
        meshio.load_mesh(str(tmp_path / "mesh.ply"))


def test_binary_and_ascii_stl_give_the_same_merged_mesh(tmp_path):
    from partmanip_amd import meshio
    v, f = M.box_mesh()
    tri = v[f]
    ascii_path, bin_path, solid_path = tmp_path / "a.stl", tmp_path / "b.stl", tmp_path / "c.stl"
    with open(ascii_path, "w") as fh:
        fh.write("solid box\n")
        for t in tri:
            fh.write("facet normal 0 0 0\n outer loop\n")
            for c in t:
                fh.write("  vertex %.9g %.9g %.9g\n" % tuple(float(x) for x in c))
            fh.write(" endloop\nendfacet\n")
        fh.write("endsolid box\n")
    for path, head in ((bin_path, b"binary"), (solid_path, b"solid but binary all the same")):
        with open(path, "wb") as fh:
            fh.write(head.ljust(80, b" ") + struct.pack("<I", len(tri)))
            for t in tri:
                fh.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *[float(x) for x in t.reshape(-1)], 0))
    got = [meshio.load_mesh(str(p)) for p in (ascii_path, bin_path, solid_path)]
    for gv, gf in got:
        assert gv.shape == (8, 3) and gf.shape == (12, 3)
        np.testing.assert_array_equal(gv, got[0][0])
        np.testing.assert_array_equal(gf, got[0][1])
        np.testing.assert_array_equal(gv[gf], tri)           # the same triangles, corner for corner


def test_real_meshes():
    from partmanip_amd import meshio
    v, f = meshio.load_mesh(FINGER)
    assert v.shape == (318, 3) and f.shape == (624, 3)
    assert set(M.edge_use_counts(f).tolist()) == {2}         # closed manifold: every edge shared by two faces
    assert len(meshio.drop_double_corner_faces(v, f)) == 624
    v, f = meshio.load_mesh(M.hand_obj())
    assert f.shape == (7078, 3) and len(meshio.drop_double_corner_faces(v, f)) == 7078
    assert os.path.getsize(FINGER) == 31284 and os.path.getsize(M.hand_obj()) == 483975


def test_double_corner_faces_are_dropped_by_position():
    from partmanip_amd import meshio
    v, fa, fb = M.degenerate_mesh()
    kept = meshio.drop_double_corner_faces(v, fa)
    assert len(fa) == 14 and len(kept) == 13                 # the repeated-vertex face goes, the collinear sliver stays
    np.testing.assert_array_equal(kept, M.clean_faces(v, fa))
    np.testing.assert_array_equal(kept[:12], fb)


# ------------------------------------------------------------------------------------------- 3. the restatement is sound
def test_no_range_is_near_an_integer_number_of_voxels():
    for name, (v, _) in fixtures().items():
        r = M.range_over_voxel(v)
        assert np.all(np.abs(r - np.round(r)) > 1e-3), (name, r)
    assert M.grid_layout(M.torus_mesh()[0])[0] == (151, 151, 70)
    assert M.grid_layout(fixtures()["finger"][0])[0] == (51, 67, 54)
    assert M.grid_layout(fixtures()["hand"][0])[0] == (72, 86, 143)


def test_restatement_reproduces_the_analytic_box_on_the_full_grid():
    v, f = M.box_mesh()
    shape, tables, _ = M.grid_layout(v)
    pts = M.grid_points(tables)
    r = M.evaluate(pts, v, f, parity=True)
    v64 = v.astype(np.float64)
    c, h = (v64.max(0) + v64.min(0)) / 2, (v64.max(0) - v64.min(0)) / 2
    want = np.clip(_box_sdf(pts.astype(np.float64) - c, h), -M.TRUNC, M.TRUNC)
    err = np.abs(r["sdf"] - want).max()
    print(f"box, {len(pts)} voxels: max |restatement - analytic| = {err:.3e}")
    assert err <= 1e-12
    assert np.abs(np.abs(r["w"]) - np.round(np.abs(r["w"]))).max() < 1e-9
    np.testing.assert_array_equal(np.abs(r["w"]) >= 0.5, r["inside_parity"])        # every voxel
    assert 0.02 < np.mean(r["sdf"] < 0) < 0.5


def _sample(n_cells, n, seed):
    return np.sort(np.random.RandomState(seed).choice(n_cells, size=n, replace=False))


def test_winding_sign_equals_ray_parity_and_torus_stays_within_its_chord_bound():
    v, f = M.torus_mesh()
    shape, tables, _ = M.grid_layout(v)
    idx = _sample(int(np.prod(shape)), 1500, 31)
    pts = M.grid_points(tables, idx)
    r = M.evaluate(pts, v, f, parity=True)
    assert np.abs(np.abs(r["w"]) - np.round(np.abs(r["w"]))).max() < 1e-9
    np.testing.assert_array_equal(np.abs(r["w"]) >= 0.5, r["inside_parity"])
    assert 20 < int(r["inside_parity"].sum()) < 1400
    H = M.torus_chord_bound()
    assert 1.37e-4 < H < 1.39e-4
    want = np.clip(M.torus_sdf(pts), -M.TRUNC, M.TRUNC)
    err = np.abs(r["sdf"] - want).max()
    print(f"torus, {len(pts)} voxels: max |restatement - analytic| = {err:.3e}, bound H = {H:.3e}")
    assert err <= H


def test_winding_sign_equals_ray_parity_on_the_finger():
    v, f = fixtures()["finger"]
    shape, tables, _ = M.grid_layout(v)
    idx = _sample(int(np.prod(shape)), 20000, 32)
    r = M.evaluate(M.grid_points(tables, idx), v, f, parity=True)
    dev = np.abs(np.abs(r["w"]) - np.round(np.abs(r["w"]))).max()
    print(f"finger: winding numbers within {dev:.2e} of an integer; inside share {np.mean(r['inside_parity']):.3f}")
    assert dev < 1e-6
    np.testing.assert_array_equal(np.abs(r["w"]) >= 0.5, r["inside_parity"])
    assert int(r["inside_parity"].sum()) > 50


def test_degenerate_faces_do_not_change_the_restatement():
    v, fa, fb = M.degenerate_mesh()
    shape, tables, _ = M.grid_layout(v)
    idx = _sample(int(np.prod(shape)), 4000, 33)
    pts = M.grid_points(tables, idx)
    a, b = M.evaluate(pts, v, fa), M.evaluate(pts, v, fb)
    assert np.all(np.isfinite(a["sdf"])) and np.all(np.isfinite(a["w"]))
    np.testing.assert_array_equal(a["sdf"], b["sdf"])


# ------------------------------------------------------------------------------------------- 4. grid layout in fp32
def test_grid_layout_equals_the_reference_expressions_in_torch_fp32():
    from partmanip_amd.mesh2sdf import bake_grid_layout
    trunc, vs = 4 * (0.5 / 50), 0.002
    for name, (v, _) in fixtures().items():
        vertices = torch.FloatTensor(v).reshape(1, -1, 3)                                   # mesh2sdf.py:207, 213-223
        obj_center = (vertices.max(dim=1)[0] + vertices.min(dim=1)[0]) / 2
        max_range = vertices.max(dim=1)[0] - vertices.min(dim=1)[0] + 2 * trunc
        volume_shape = torch.ceil(max_range / vs)
        size_x, size_y, size_z = int(volume_shape[0, 0]), int(volume_shape[0, 1]), int(volume_shape[0, 2])
        corners = torch.tensor([[0, 0, 0], [size_x - 1, size_y - 1, size_z - 1]])
        query_points = (corners - volume_shape // 2) * vs + obj_center
        shape, centre, bbox_min = bake_grid_layout(v, trunc, vs)
        assert shape == (size_x, size_y, size_z), name
        assert centre.dtype == bbox_min.dtype == torch.float32
        assert torch.equal(centre, obj_center[0]) and torch.equal(bbox_min, query_points[0]), name
        # ... and the yardstick's numpy float32 restatement of the same expressions, bit for bit, every voxel coordinate
        shape2, tables, bb2 = M.grid_layout(v, trunc, vs)
        assert shape2 == shape and np.array_equal(bb2, bbox_min.numpy()), name
        assert np.array_equal(np.array([tb[-1] for tb in tables]), query_points[1].numpy()), name
        for a in range(3):
            want = (torch.arange(shape[a]) - (volume_shape // 2)[0, a]) * vs + obj_center[0, a]
            assert np.array_equal(tables[a], want.numpy()), (name, a)


# ------------------------------------------------------------------------------------------- 5. host logic on 'cpu'
def _asset_root(tmp_path):
    from partmanip_amd import meshio
    import shutil
    vis = tmp_path / "assets" / "franka_description" / "meshes" / "visual"
    vis.mkdir(parents=True)
    (tmp_path / "assets" / "objs" / "cube").mkdir(parents=True)
    v, f = M.box_mesh()
    for name in [f"link{i}.obj" for i in range(8)] + ["hand.obj"]:
        meshio.save_obj(str(vis / name), v, f)
    shutil.copy(FINGER, vis / "finger.stl")
    meshio.save_obj(str(tmp_path / "assets" / "objs" / "cube" / "cube.obj"), v, f)
    return tmp_path


def test_bake_false_keeps_the_errors_and_bake_true_has_no_cpu_path(tmp_path):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    root = _asset_root(tmp_path)
    with pytest.raises(NotImplementedError, match="kaolin") as e:
        TSDFfromMesh(1, 0.5, 50, "cpu", asset_root=str(root))
    assert "bake=True" in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TSDFfromMesh(1, 0.5, 50, "cpu", asset_root=str(root), bake=True)
    assert not [p for p in root.rglob("*.npy")], "a failed bake must not leave a file"
    assert not (root / "assets" / "franka_description" / "sdf").exists()
    from tests.mesh_tsdf_parts import make_parts
    t = TSDFfromMesh(1, 0.5, 10, "cpu", sdf_dicts=make_parts(7, "cut"), bake=True)
    with pytest.raises(NotImplementedError):
        t.preprocess_mesh("a.obj", "b.obj")                  # ManifoldPlus stays out of scope
    v, f = M.box_mesh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.mesh2sdf(vertices=v, faces=f)
    t0 = TSDFfromMesh(1, 0.5, 10, "cpu", sdf_dicts=make_parts(7, "cut"))
    with pytest.raises(NotImplementedError, match="bake=True"):
        t0.mesh2sdf("a.obj")


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from partmanip_amd import ops
    tri = torch.zeros(12, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_sdf_bake(tri, (8, 8, 8), 0.002, (0.0, 0.0, 0.0), 0.04)
