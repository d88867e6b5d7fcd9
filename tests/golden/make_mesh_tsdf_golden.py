#!/usr/bin/env python3
"""Generate tests/golden/mesh_tsdf_*.npz by RUNNING THE REFERENCE's `utils/mesh2sdf.py: TSDFfromMesh` (dev machine only, like
make_golden.py; only inputs / outputs are written, no reference source travels).

    python -m tests.golden.make_mesh_tsdf_golden --reference <checkout of the reference>       (from the repo root)

The reference module is loaded by path with `trimesh` and `skimage` stubbed in sys.modules (neither is touched by the query
path).  The 11 + 1 synthetic part grids of tests/mesh_tsdf_parts.py are written as .npy dicts at the reference's relative paths
inside a temporary directory, the process changes into it and constructs `TSDFfromMesh(B, 0.5, 50, 'cpu')` unmodified.  Every
case runs twice on the same fp32-rounded inputs: under torch.set_default_dtype(float32) -> ref32 and float64 -> ref64.

A family is stored one environment per file (tests/mesh_tsdf_parts.py: save_family / load_family) so that every committed file
stays below the largest existing fixture.  The grids themselves are not stored (12 parts are ~5 MB): the tests regenerate them from the seed, and the fixture pins every
grid with its SHA-256 (`part_sha`).

  mesh_tsdf_cont_env*.npz       B = 2, 'cont' parts: pose_R, pose_T, scene32 / obj32 / scene64 / obj64 of query_tsdf_seperately
                           (query_tsdf is their minimum bit for bit: asserted here)
  mesh_tsdf_cont_init_env0.npz  B = 1, 'cont' parts, after initialize_sdf(pred): pose_R, pose_T, pred, ref32, ref64 of query_tsdf
  mesh_tsdf_cut_env*.npz        B = 4, 'cut' parts (grids end inside the truncation band, as the reference's bake): ref32, ref64 of
                           query_tsdf.  A sample within round-off of the valid box's border legitimately jumps here; this
                           maker refuses to write the fixture if ref32 and ref64 differ (by more than 4 e_ref of the 'cont'
                           family) on more than 3 voxels -- pick another seed then.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import mesh_tsdf_parts as P  # noqa: E402


def load_reference(root):
    for name in ("trimesh", "skimage", "skimage.measure"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]
    spec = importlib.util.spec_from_file_location("ref_mesh2sdf", os.path.join(root, "utils", "mesh2sdf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_parts(parts, root):
    franka = os.path.join(root, "assets", "franka_description", "sdf", "visual")
    os.makedirs(franka)
    os.makedirs(os.path.join(root, "assets", "objs", "cube"))
    names = [f"link{i}" for i in range(8)] + ["hand", "finger"]
    # 'finger' is loaded twice from one file (mesh2sdf.py:145): parts 9 and 10 must be the same grid
    assert P.parts_digest([parts[9]]) == P.parts_digest([parts[10]])
    for name, d in zip(names, parts[:10]):
        np.save(os.path.join(franka, name + ".npy"), d)
    np.save(os.path.join(root, "assets", "objs", "cube", "sdf.npy"), parts[11])


def run(ref, parts, B, dtype, fn):
    """Construct the reference in a temporary asset tree under the given default dtype and hand it to fn."""
    old, cwd = torch.get_default_dtype(), os.getcwd()
    torch.set_default_dtype(dtype)
    try:
        with tempfile.TemporaryDirectory() as d:
            write_parts(parts, d)
            os.chdir(d)
            origin = torch.tensor([float(np.float32(o)) for o in P.ORIGIN], dtype=dtype)
            obj = ref.TSDFfromMesh(B, P.SIZE, P.RES, 'cpu', vox_origin=origin)
            return fn(obj, lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype))
    finally:
        os.chdir(cwd)
        torch.set_default_dtype(old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PARTMANIP_REFERENCE", ""), help="checkout of the reference project")
    a = ap.parse_args()
    ref = load_reference(a.reference)

    # ---- cont, B = 2
    parts = P.fixture_parts("cont")
    R, T = P.random_poses(3101, 2)
    out = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        def both(obj, t):
            s, o = obj.query_tsdf_seperately(t(R), t(T))
            q = obj.query_tsdf(t(R), t(T))
            assert torch.equal(torch.minimum(s, o), q), "min(scene, obj) != query_tsdf in the reference"
            return s.numpy(), o.numpy()
        out["scene" + tag], out["obj" + tag] = run(ref, parts, 2, dt, both)
    e_ref = max(np.abs(out["scene32"] - out["scene64"]).max(), np.abs(out["obj32"] - out["obj64"]).max())
    q = np.minimum(out["scene64"], out["obj64"])
    print(f"cont: e_ref = {e_ref:.3e}; at 1.0: {np.mean(q == 1.0):.3f}, negative: {np.mean(q < 0):.3f}")
    sha = np.array([P.parts_digest([d]) for d in parts])
    sizes = {"mesh_tsdf_cont": P.save_family("mesh_tsdf_cont", HERE, dict(part_sha=sha, seed=P.CONT_SEED), dict(pose_R=R, pose_T=T, **out))}

    # ---- cont after initialize_sdf, B = 1
    R1, T1 = P.random_poses(3102, 1)
    pred = P.seeded_pred(3103)
    init = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        def after_init(obj, t):
            obj.initialize_sdf(t(pred))
            return obj.query_tsdf(t(R1), t(T1)).numpy()
        init["ref" + tag] = run(ref, parts, 1, dt, after_init)
    print(f"cont_init: max |ref32 - ref64| = {np.abs(init['ref32'] - init['ref64']).max():.3e}")
    sizes["mesh_tsdf_cont_init"] = P.save_family("mesh_tsdf_cont_init", HERE, dict(part_sha=sha, seed=P.CONT_SEED),
                                                 dict(pose_R=R1, pose_T=T1, pred=pred, **init))

    # ---- cut, B = 4
    cparts = P.fixture_parts("cut")
    R4, T4 = P.random_poses(3104, 4)
    cut = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        cut["ref" + tag] = run(ref, cparts, 4, dt, lambda obj, t: obj.query_tsdf(t(R4), t(T4)).numpy())
    differ = int((np.abs(cut["ref32"] - cut["ref64"]) > 4 * e_ref).sum())
    print(f"cut: ref32 vs ref64 differ on {differ} of {cut['ref64'].size} voxels")
    assert differ <= 3, "pick another seed"
    csha = np.array([P.parts_digest([d]) for d in cparts])
    sizes["mesh_tsdf_cut"] = P.save_family("mesh_tsdf_cut", HERE, dict(part_sha=csha, seed=P.CUT_SEED), dict(pose_R=R4, pose_T=T4, **cut))
    for f, sz in sizes.items():
        print(f, sz, "bytes per environment file")
        assert max(sz) < 750 * 1024, "a fixture file above the size of the largest existing fixture"


if __name__ == "__main__":
    main()
