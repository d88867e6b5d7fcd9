"""Mesh-TSDF observation, everything that needs no GPU: the fp64 restatement of tests/mesh_tsdf_parts.py against the REFERENCE's
own fp64 volumes (fixtures of tests/golden/make_mesh_tsdf_golden.py), the C ABI entry, and the host logic of
partmanip_amd.mesh2sdf.TSDFfromMesh built on the 'cpu' device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_tsdf_parts as P
from tests.helpers import GOLDEN, ROOT


def family(name):
    fx = P.load_family(name, GOLDEN)
    parts = P.fixture_parts("cut" if name == "mesh_tsdf_cut" else "cont")
    assert [P.parts_digest([d]) for d in parts] == list(fx["part_sha"]), "regenerated part grids differ from the fixture's"
    return fx, parts


# ------------------------------------------------------------------------------------------- 1. restatement vs reference
def test_restatement_matches_reference_fp64_cont():
    fx, parts = family("mesh_tsdf_cont")
    assert fx["scene64"].dtype == np.float64 and fx["scene64"].shape == (2, 50, 50, 50)
    scene, _ = P.restate(parts, fx["pose_R"], fx["pose_T"], p1=P.N_PARTS - 1)
    obj, _ = P.restate(parts, fx["pose_R"], fx["pose_T"], p0=P.N_PARTS - 1)
    full, _ = P.restate(parts, fx["pose_R"], fx["pose_T"])
    assert np.abs(scene - fx["scene64"]).max() <= 1e-12
    assert np.abs(obj - fx["obj64"]).max() <= 1e-12
    assert np.abs(full - np.minimum(fx["scene64"], fx["obj64"])).max() <= 1e-12
    q = np.minimum(fx["scene64"], fx["obj64"])
    assert 0.2 < np.mean(q == 1.0) < 0.6 and np.mean(q < 0) > 0.1          # far, near-surface and inside are all exercised


def test_restatement_matches_reference_fp64_after_initialize_sdf():
    fx, parts = family("mesh_tsdf_cont_init")
    np.testing.assert_array_equal(fx["pred"], P.seeded_pred(3103))
    base = fx["pred"].astype(np.float64) * (4 * P.SIZE / P.RES)
    vol, _ = P.restate(parts, fx["pose_R"], fx["pose_T"], base=base)
    assert np.abs(vol - fx["ref64"]).max() <= 1e-12


def test_restatement_matches_reference_fp64_cut():
    fx, parts = family("mesh_tsdf_cut")
    assert fx["ref64"].shape == (4, 50, 50, 50)
    vol, margin = P.restate(parts, fx["pose_R"], fx["pose_T"])
    away = (margin > 1e-9).reshape(vol.shape)
    assert away.mean() > 0.999
    assert np.abs(vol - fx["ref64"])[away].max() <= 1e-12


# ------------------------------------------------------------------------------------------- 2. the entry point exists
def test_entry_point_is_exported_declared_and_typed():
    from partmanip_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "pm_mesh_tsdf_query_f32")
    hdr = open(os.path.join(ROOT, "include", "partmanip_hip.h")).read()
    assert re.search(r"\bint\s+pm_mesh_tsdf_query_f32\s*\(", hdr)
    res, args = _lib.SIGNATURES["pm_mesh_tsdf_query_f32"]
    assert res is ctypes.c_int and len(args) == 23 and args[1] is ctypes.c_void_p and args[20] is ctypes.c_long
    assert _lib.ABI_VERSION >= 153


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from partmanip_amd._lib import lib
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first

    def call(B=1, M=12, p0=0, p1=12, res=50, stride=125000, ptr=p):
        return lib.pm_mesh_tsdf_query_f32(ptr, p, p, p, p, p, p, B, M, p0, p1, res, 0.01, 0.0, 0.0, 0.0, 0.04, p, 0, p, stride, 1, None)
    assert call(p0=3, p1=3) == -1 and call(p0=5, p1=4) == -1 and call(p1=13) == -1
    assert call(res=0) == -1 and call(res=-5) == -1
    assert call(stride=124999) == -1
    assert call(ptr=None) == -1 and call(B=0) == -1


def test_module_imports_without_a_gpu():
    import partmanip_amd.mesh2sdf as m
    assert hasattr(m.TSDFfromMesh, "query_tsdf") and hasattr(m.TSDFfromMesh, "query_tsdf_seperately")
    assert hasattr(m.TSDFfromMesh, "query_tsdf_parallel") and hasattr(m.TSDFfromMesh, "initialize_sdf")


# ------------------------------------------------------------------------------------------- 3. host logic on 'cpu'
def small_parts():
    return P.make_parts(7, "cut", n_parts=12)


def test_file_loader_reads_the_reference_paths_in_the_reference_order(tmp_path):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    parts = small_parts()
    franka = tmp_path / "assets" / "franka_description" / "sdf" / "visual"
    franka.mkdir(parents=True)
    (tmp_path / "assets" / "objs" / "cube").mkdir(parents=True)
    names = [f"link{i}" for i in range(8)] + ["hand", "finger"]
    for name, d in zip(names, parts[:10]):
        np.save(franka / (name + ".npy"), d)
    np.save(tmp_path / "assets" / "objs" / "cube" / "sdf.npy", parts[11])
    t = TSDFfromMesh(2, 0.5, 50, "cpu", asset_root=str(tmp_path))
    assert t.part_num == 12 and len(t.sdf_dict_list) == 12
    want = parts[:10] + [parts[9], parts[11]]               # link0..7, hand, finger, finger, cube
    for got, w in zip(t.sdf_dict_list, want):
        np.testing.assert_array_equal(got["sdf"], w["sdf"])
        np.testing.assert_array_equal(got["bbox_min"], w["bbox_min"])
    # an absent pre-stored grid is the kaolin bake: out of scope, and said so
    os.remove(franka / "link3.npy")
    with pytest.raises(NotImplementedError, match="kaolin"):
        TSDFfromMesh(2, 0.5, 50, "cpu", asset_root=str(tmp_path))


def test_out_of_scope_methods_raise():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    parts = small_parts()
    t = TSDFfromMesh(1, 0.5, 10, "cpu", sdf_dicts=parts)
    for call in (lambda: t.visualize(None, 0.0, None, "x"), lambda: t.extract_surface_points_from_volume(None, "x"),
                 lambda: t.mesh2sdf("a.obj"), lambda: t.preprocess_mesh("a.obj", "b.obj"),
                 lambda: TSDFfromMesh(1, 0.5, 10, "cpu", debug=True, sdf_dicts=parts),
                 lambda: t.load_sdf("/nonexistent/sdf.npy", "mesh.obj")):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the query itself has no CPU path
        t.query_tsdf(torch.eye(3).repeat(1, 12, 1, 1), torch.zeros(1, 12, 3))


def test_attributes_have_the_reference_values_for_every_origin_form():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    parts = small_parts()
    lst = [-0.25, -0.25, -0.0503]
    a = TSDFfromMesh(3, 0.5, 50, "cpu", sdf_dicts=parts)
    b = TSDFfromMesh(3, 0.5, 50, "cpu", sdf_dicts=parts, vox_origin=lst)
    c = TSDFfromMesh(3, 0.5, 50, "cpu", sdf_dicts=parts, vox_origin=torch.tensor(lst))
    for t in (a, b, c):
        assert torch.equal(t.vox_coords, a.vox_coords) and torch.equal(t.vox_origin, a.vox_origin)
    assert a.resolution == 50 and a.size == 0.5 and a.vox_size == 0.5 / 50 and a.sdf_trunc == 4 * (0.5 / 50)
    assert a.point_num == 125000 and a.part_num == 12 and a.vox_coords.dtype == torch.float32
    # the reference's expression (mesh2sdf.py:29-37), k fastest
    ax = torch.arange(50)
    xv, yv, zv = torch.meshgrid(ax, ax, ax, indexing="ij")
    want = torch.stack([xv.flatten(), yv.flatten(), zv.flatten()], dim=1).long() * (0.5 / 50) + torch.tensor(lst)
    assert torch.equal(a.vox_coords, want)
    assert tuple(a.init_tsdf.shape) == (3, 125000) and torch.equal(a.init_tsdf[2], want[:, 2])
    assert tuple(a.ground_tsdf.shape) == (3, 125000) and torch.equal(a.ground_tsdf[1], want[:, 2])
    pred = torch.from_numpy(P.seeded_pred(5, B=3))
    a.initialize_sdf(pred)
    assert torch.equal(a.init_tsdf, pred * a.sdf_trunc) and torch.equal(a.ground_tsdf[0], want[:, 2])


def test_merge_sdf_field_tables():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    parts = small_parts()
    t = TSDFfromMesh(1, 0.5, 50, "cpu", sdf_dicts=parts)
    shapes = [d["sdf"].shape for d in parts]
    assert len(set(shapes)) > 6                              # un-padded: the grids keep their own shapes
    sizes = [int(np.prod(s)) for s in shapes]
    assert t.sdf_field_off.dtype == torch.int64 and t.sdf_field_off.tolist() == [int(v) for v in np.cumsum([0] + sizes[:-1])]
    assert t.sdf_field_res.dtype == torch.int32 and t.sdf_field_res.tolist() == [list(s) for s in shapes]
    assert t.sdf_field.dtype == torch.float32 and t.sdf_field.numel() == sum(sizes)
    for p in (0, 5, 11):
        o = t.sdf_field_off[p].item()
        np.testing.assert_array_equal(t.sdf_field[o:o + sizes[p]].numpy().reshape(shapes[p]), parts[p]["sdf"])
    np.testing.assert_array_equal(t.sdf_bbox_min.numpy(), np.stack([d["bbox_min"] for d in parts]))
    np.testing.assert_array_equal(t.sdf_voxel_size.numpy(), np.array([d["voxel_size"] for d in parts], dtype=np.float32))
    assert len(set(t.sdf_voxel_size.tolist())) == 2          # one family member has another voxel size
