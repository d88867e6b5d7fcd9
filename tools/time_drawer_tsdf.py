"""Time the two mesh observers over a scene whose environments differ (TSDFfromMesh(groups=): pm_mesh_tsdf_query_groups_f32;
PCfromMesh(groups=): pm_mesh_pc_query_f32 with one selection per environment) beside the only alternative the ungrouped TSDF entry
offers, in one process and taken in turn:

  grouped     12 synthetic shared parts plus a library of 8 synthetic cabinets of 2 ... 7 bodies, environment e holding cabinet e % 8:
              an environment tests and samples its own cabinet's grids only;
  all_in_one  the same 12 parts and ALL 8 cabinets (34 bodies) in one scene through pm_mesh_tsdf_query_f32, every body in a slot of its
              own; the cabinets an environment does not hold are posed far outside the workspace by FINITE poses (a NaN pose would
              turn the whole volume NaN there): every environment tests all 46 parts.

The two volumes are equal bit for bit, which is asserted: an absent cabinet's samples are all invalid, i.e. 1 (metre), and the base
field -- the ground plane, the voxel's world z -- is below 1 everywhere in this workspace, so they never win the minimum.
res = 50, 64 and 1024 environments.  Next to it the cloud: query_pc of the grouped library with a group_sel() table, and the ungrouped
query_pc of the 12 parts plus one 7-body cabinet with the reference's one selection for all environments.

No thresholds: the JSON says what was measured.  Prints one JSON line and writes it to profiles/drawer_tsdf_timing.json (--out;
nothing is written with --tiny).  The yardstick -- the existing query_tsdf on tools/time_mesh_tsdf.py's scene, which this change must
not slow down -- is that tool itself run by turns from a checkout of the parent commit and from this one (fresh processes, three
each); its printed lines are handed back with --parent-runs / --new-runs and kept in the JSON with the verdict: the new median within
[min, max] of the parent's runs, per size.

    python tools/time_drawer_tsdf.py [--tiny] [--sizes 64,1024] [--parent-runs a.json ... --new-runs b.json ...]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.mesh2pc import PCfromMesh, random_poses  # noqa: E402
from partmanip_amd.mesh2sdf import TSDFfromMesh  # noqa: E402
from tools.time_mesh_tsdf import DEV, RES, SIZE, synthetic_parts  # noqa: E402
from tools.timing import timed  # noqa: E402

BODIES = (2, 3, 4, 5, 6, 7, 3, 4)                             # the body counts of the 8 cabinets
NUM_POINTS = 1024
FAR = 100.0                                                   # where all_in_one parks an absent cabinet (metres; the workspace is 0.5 m)


def cabinet_library(seed=51):
    """8 cabinets; cabinet k's bodies are the first BODIES[k] parts of tools/time_mesh_tsdf.py's generator under seed + k."""
    return [synthetic_parts(seed + k)[:n] for k, n in enumerate(BODIES)]


def poses(B, M, seed):
    """The pose distribution of tools/time_mesh_tsdf.py (translations inside the workspace) over M slots."""
    R, _ = random_poses(B, M, torch.Generator(device=DEV).manual_seed(seed), DEV)
    u = torch.rand(B, M, 3, generator=torch.Generator(device=DEV).manual_seed(seed + 1), device=DEV)
    T = torch.stack([u[..., 0] * 0.4 - 0.2, u[..., 1] * 0.4 - 0.2, u[..., 2] * 0.35], dim=-1)
    return R.contiguous(), T.contiguous()


def in_turn(fns, calls, rounds=3):
    """ms per call of every entry of `fns`, the entries taken in turn, `rounds` times after one untimed round: {name: [ms, ...]}."""
    out = {k: [] for k in fns}
    for fn in fns.values():
        timed(fn, calls)
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(round(timed(fn, calls), 5))
    return out


def scene_rows(sizes, tiny):
    shared, library = synthetic_parts(), cabinet_library()
    if tiny:
        shared, library = shared[:3], [bodies[:2] for bodies in library[:3]]
    S, G, most = len(shared), len(library), max(len(b) for b in library)
    flat = [d for bodies in library for d in bodies]
    first = S + np.concatenate([[0], np.cumsum([len(b) for b in library])[:-1]])           # all_in_one: cabinet k's body j is slot first[k] + j
    rng = np.random.RandomState(52)
    cloud_shared = rng.uniform(-0.05, 0.05, size=(S, NUM_POINTS, 3)).astype(np.float32)
    cloud_groups = [[rng.uniform(-0.05, 0.05, size=(NUM_POINTS, 3)).astype(np.float32) for _ in bodies] for bodies in library]
    rows, calls = [], 3 if tiny else 20
    for B in sizes:
        group_of = np.arange(B) % G
        grouped = TSDFfromMesh(B, SIZE, RES, DEV, sdf_dicts=shared, groups=library, group_of=group_of)
        whole = TSDFfromMesh(B, SIZE, RES, DEV, sdf_dicts=shared + flat)
        assert bool((grouped._ground < 1.0).all())                                         # the base is below 1 everywhere
        R, T = poses(B, S + most, 53)
        Rw = torch.eye(3, device=DEV).expand(B, S + len(flat), 3, 3).contiguous()
        Tw = torch.full((B, S + len(flat), 3), FAR, device=DEV)
        Rw[:, :S], Tw[:, :S] = R[:, :S], T[:, :S]
        for k, bodies in enumerate(library):
            e = torch.as_tensor(np.flatnonzero(group_of == k), device=DEV)
            n = len(bodies)
            Rw[e, first[k]:first[k] + n], Tw[e, first[k]:first[k] + n] = R[e, S:S + n], T[e, S:S + n]
        n3 = RES ** 3
        out_g, out_w = torch.empty(B, n3, device=DEV), torch.empty(B, n3, device=DEV)
        pc_g = PCfromMesh(B, DEV, num_points=NUM_POINTS, part_pcs=cloud_shared, groups=cloud_groups, group_of=group_of)
        pc_u = PCfromMesh(B, DEV, num_points=NUM_POINTS, part_pcs=np.concatenate([cloud_shared, np.stack(cloud_groups[int(np.argmax(BODIES[:G]))])]))
        sel_g = pc_g.group_sel(generator=torch.Generator().manual_seed(54))
        sel_u = torch.randperm(pc_u.pts.shape[0], generator=torch.Generator().manual_seed(54))[:NUM_POINTS].to(torch.int32).to(DEV)
        Ru, Tu = R[:, :pc_u.part_num].contiguous(), T[:, :pc_u.part_num].contiguous()
        out_pg, out_pu = torch.empty(B, 3 * NUM_POINTS, device=DEV), torch.empty(B, 3 * NUM_POINTS, device=DEV)
        ms = in_turn(dict(grouped=lambda: grouped.query_tsdf(R, T, out=out_g), all_in_one=lambda: whole.query_tsdf(Rw, Tw, out=out_w)), calls)
        ms.update(in_turn(dict(cloud_grouped=lambda: pc_g.query_pc(R, T, out=out_pg, sel=sel_g),
                               cloud_ungrouped=lambda: pc_u.query_pc(Ru, Tu, out=out_pu, sel=sel_u)), 10 * calls))
        torch.cuda.synchronize()
        same = bool(torch.equal(out_g.view(torch.int32), out_w.view(torch.int32)))
        assert same, "the grouped volume differs from the all-in-one volume"
        shared_only = grouped.query_tsdf(R, T, group_of=np.full(B, -1))
        row = dict(B=B, res=RES, shared_parts=S, cabinets=G, cabinet_bodies=[len(b) for b in library], max_group_grids=grouped.max_group_grids,
                   mean_parts_per_env_grouped=round(S + float(np.mean([len(library[k]) for k in group_of])), 2),
                   parts_per_env_all_in_one=S + len(flat), grid_cells=int(grouped.sdf_field.numel()), same_bits=same,
                   finite=bool(torch.isfinite(out_g).all()), valid_lt1_fraction=round(float((out_g < 1).float().mean()), 3),
                   voxels_changed_by_the_cabinets=round(float((shared_only.reshape(B, -1) != out_g).float().mean()), 4),
                   cloud_points=NUM_POINTS, cloud_library_points=int(pc_g.pts.shape[0]), cloud_finite=bool(torch.isfinite(out_pg).all()))
        for k, v in ms.items():
            row[k + "_ms"], row[k + "_ms_rounds"] = round(float(np.mean(v)), 5), v
        row["all_in_one_over_grouped"] = round(row["all_in_one_ms"] / row["grouped_ms"], 3)
        row["cloud_grouped_over_ungrouped"] = round(row["cloud_grouped_ms"] / row["cloud_ungrouped_ms"], 3)
        rows.append(row)
        del grouped, whole, out_g, out_w, Rw, Tw, pc_g, pc_u
        torch.cuda.empty_cache()
    return rows


def regression(parent_files, new_files):
    """The lines tools/time_mesh_tsdf.py printed in fresh processes run by turns on the parent commit and on this one -> per size both
    sets of runs (ms per query_tsdf), the new median and whether it lies within the spread of the parent's runs."""
    def load(files):
        runs = []
        for path in files:
            with open(path) as f:
                runs.append({r["B"]: r["hip_ms"] for r in json.loads(f.read().strip().splitlines()[-1])["sizes"]})
        return runs
    parent, new = load(parent_files), load(new_files)
    rows = []
    for key in parent[0]:
        p, n = [r[key] for r in parent], [r[key] for r in new]
        med = float(np.median(n))
        rows.append(dict(B=key, parent_ms=p, new_ms=n, new_median_ms=med, parent_min_ms=min(p), parent_max_ms=max(p),
                         new_median_within_parent_spread=bool(min(p) <= med <= max(p)), new_median_over_parent_median=round(med / float(np.median(p)), 5)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="B = 4, 3 shared parts, 3 cabinets of 2 bodies, 3 calls; writes nothing")
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--parent-runs", nargs="*", default=[], help="lines of tools/time_mesh_tsdf.py on the parent commit, one file per process")
    ap.add_argument("--new-runs", nargs="*", default=[], help="lines of tools/time_mesh_tsdf.py on this commit, one file per process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    line = dict(tool="time_drawer_tsdf", measured=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0),
                rows=scene_rows(sizes, a.tiny))
    if a.parent_runs or a.new_runs:
        line["existing_query_tsdf_parent_vs_new"] = regression(a.parent_runs, a.new_runs)
    line = json.dumps(line)
    print(line)
    out_path = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "drawer_tsdf_timing.json"))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
