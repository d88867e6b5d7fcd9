"""Dev-machine generator of the posed-point-cloud fixtures (tests/test_mesh_pc_host.py, tests/test_gpu_mesh_pc.py): runs the
REFERENCE's own PCfromMesh.query_pc (utils/mesh2pc.py:56-65) on the CPU, once in float32 and once in float64.

    python tests/golden/make_mesh_pc_golden.py /path/to/reference

The reference module imports trimesh at its top and uses it only in its constructor, so an empty stand-in module is put into
sys.modules and the object is built with object.__new__ (num_envs, num_points and all_pc set by hand); query_pc itself is the
reference's code, including its torch.randperm under torch.manual_seed(seed).  Part clouds: meshio.sample_surface of seeded
boxes (links and the cube), hand.obj and finger.stl (twice, seeds differ).  Poses: tests/mesh_tsdf_parts.random_poses.
Writes mesh_pc_ref_small.npz (b = 3, m = 12, p = 64) and mesh_pc_ref_1024.npz (b = 2, m = 12, p = 1024) with part_pcs, R, T,
seed, perm, out32, out64."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from partmanip_amd import meshio  # noqa: E402
from tests import mesh_bake_ref as MB  # noqa: E402
from tests.mesh_tsdf_parts import random_poses  # noqa: E402

M = 12
CASES = (("mesh_pc_ref_small", 3, 64, 4101), ("mesh_pc_ref_1024", 2, 1024, 4102))


def part_meshes(seed):
    """link0..7 = seeded boxes, hand, finger, finger, cube = a seeded box."""
    rng = np.random.RandomState(seed)
    boxes = [MB.box_mesh(tuple(rng.uniform(0.02, 0.07, size=3)), tuple(rng.uniform(-0.01, 0.01, size=3))) for _ in range(9)]
    finger = meshio.load_mesh(os.path.join(HERE, "finger.stl"))
    return boxes[:8] + [meshio.load_mesh(MB.hand_obj()), finger, finger, boxes[8]]


def main(reference_root):
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    spec = importlib.util.spec_from_file_location("ref_mesh2pc", os.path.join(reference_root, "utils", "mesh2pc.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name, b, p, seed in CASES:
        pcs = np.stack([meshio.sample_surface(v, f, p, torch.Generator().manual_seed(seed + i))[0]
                        for i, (v, f) in enumerate(part_meshes(seed))])
        R, T = random_poses(seed + 50, b, M)
        outs = {}
        for key, dt in (("out32", torch.float32), ("out64", torch.float64)):
            obj = object.__new__(ref.PCfromMesh)
            obj.num_envs, obj.num_points, obj.device = b, p, "cpu"
            obj.all_pc = torch.from_numpy(pcs).to(dt).unsqueeze(0).repeat(b, 1, 1, 1).reshape(-1, p, 3)
            torch.manual_seed(seed)
            outs[key] = obj.query_pc(torch.from_numpy(R).to(dt), torch.from_numpy(T).to(dt)).numpy()
        torch.manual_seed(seed)
        perm = torch.randperm(M * p).numpy().astype(np.int32)
        assert outs["out32"].dtype == np.float32 and outs["out64"].dtype == np.float64 and outs["out64"].shape == (b, p, 3)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, part_pcs=pcs, R=R, T=T, seed=np.int64(seed), perm=perm, **outs)
        e = np.abs(outs["out32"].astype(np.float64) - outs["out64"]).max()
        print(f"{name}: {os.path.getsize(path)} bytes, e_ref = max|out32 - out64| = {e:.3e}")


if __name__ == "__main__":
    main(sys.argv[1])
