"""Bake signed-distance grids from meshes on the GPU (TSDFfromMesh.mesh2sdf -> pm_mesh_sdf_bake_f32), into the files the
'mesh_tsdf' observation loads.

One mesh:            python tools/bake_sdf.py --mesh part.obj --out part.npy
A whole asset root:  python tools/bake_sdf.py --asset-root .
    bakes assets/franka_description/meshes/visual/{link0..7,hand}.obj and finger.stl into assets/franka_description/sdf/visual/*.npy
    and assets/objs/cube/cube.obj into assets/objs/cube/sdf.npy (the reference's layout); existing files are kept.

--size / --resolution give the truncation distance (4 * size / resolution) as the task's configuration does; the grid's voxel is
2 mm.  Each file holds the reference's dict {'sdf': float32 (X, Y, Z), 'bbox_min': float32 (3,), 'voxel_size': 0.002}.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.mesh2sdf import TSDFfromMesh, bake_mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh")
    ap.add_argument("--out")
    ap.add_argument("--asset-root")
    ap.add_argument("--size", type=float, default=0.5)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if bool(a.mesh) == bool(a.asset_root) or (a.mesh and not a.out):
        ap.error("give either --mesh with --out, or --asset-root")
    if a.asset_root:
        t0 = time.time()
        t = TSDFfromMesh(1, a.size, a.resolution, a.device, asset_root=a.asset_root, bake=True)
        print(f"{t.part_num} parts ready under {a.asset_root} in {time.time() - t0:.1f} s: "
              + ", ".join("x".join(str(s) for s in d['sdf'].shape) for d in t.sdf_dict_list))
        return
    t0 = time.time()
    d = bake_mesh(a.device, 4 * (a.size / a.resolution), 0.002, a.mesh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.save(a.out, d)
    print(f"{a.mesh}: grid {d['sdf'].shape}, bbox_min {d['bbox_min'].tolist()}, inside share {float((d['sdf'] < 0).mean()):.4f}, "
          f"{time.time() - t0:.1f} s -> {a.out}")


if __name__ == "__main__":
    main()
