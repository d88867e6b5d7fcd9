"""Time the cameras over a scene whose environments differ (DepthFromMesh(groups=): pm_mesh_depth_render_groups_f32,
pm_mesh_frame_render_groups_f32) beside the only alternative the ungrouped entries offer, in one process and taken in turn:

  grouped     a robot of 11 synthetic parts shared by every environment plus a library of 8 synthetic cabinets of 4 bodies each and
              of different triangle counts, environment e holding cabinet e % 8: an environment sets up its own cabinet's triangles;
  all_in_one  the same robot and ALL 8 cabinets in one scene through the existing entries, every body in a slot of its own and NaN
              poses for the 7 cabinets an environment does not hold: every environment pays the set-up of the whole library.

Both give the same image (checked bit for bit here).  render at 64 and 1024 environments for the image rig (1 x 72 x 128) and the
shipped rig (3 x 288 x 512); render_frame for the image rig at both sizes and the shipped rig at 64 (the keys of 1024 would take 3.6 GB).
In the same process the yardstick: the existing render on the scene of tools/time_mesh_depth.py (12 ellipsoids, 133 200 triangles),
which this change must not slow down.

--yardstick times only that and prints its rows; run by turns from a checkout of the parent commit and from this one (fresh
processes, three each), the printed lines are handed back with --parent-runs / --new-runs and kept in the JSON with the verdict:
the new median within [min, max] of the parent's runs, per row.

Prints one JSON line and writes it to profiles/drawer_scene_timing.json (--out; nothing is written with --tiny or --yardstick).

    python tools/time_drawer_scene.py [--tiny] [--yardstick] [--parent-runs a.json ... --new-runs b.json ...]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd import camera  # noqa: E402
from partmanip_amd.mesh2depth import PALETTE, DepthFromMesh  # noqa: E402
from partmanip_amd.mesh2pc import random_poses  # noqa: E402
from tools.time_mesh_depth import CAM, DEV, M, calls_for, ellipsoid, synthetic_parts  # noqa: E402
from tools.timing import timed  # noqa: E402

ROBOT_PARTS, CABINETS, BODIES = 11, 8, 4
RIGS = (("image", True), ("shipped", False))


def cabinet_library(tiny, seed=41):
    """8 cabinets of 4 ellipsoid bodies; cabinet k's bodies have 2 n (n - 1) triangles with n = 20 + 8 k (3 040 ... 45 600 per cabinet)."""
    rng = np.random.RandomState(seed)
    return [[ellipsoid(rng.uniform(0.05, 0.15, size=3), *((4 + k, 4 + k) if tiny else (20 + 8 * k, 20 + 8 * k))) for _ in range(BODIES)]
            for k in range(CABINETS)]


def rig(image_mode, tiny):
    poses, intr, im_h, im_w = camera.shipped_rig(CAM, image_mode)
    if tiny:
        im_h, im_w, intr = im_h // 16 + 1, im_w // 16 + 1, intr / np.array([[16.0], [16.0], [1.0]])
    return poses, intr, im_h, im_w


def in_turn(fns, rounds=3):
    """ms per call of every entry of `fns`, the entries taken in turn, `rounds` times: {name: [ms, ...]}."""
    calls = {k: calls_for(fn) for k, fn in fns.items()}
    out = {k: [] for k in fns}
    for k, fn in fns.items():                                 # one untimed round: the first timed one is otherwise the slowest
        timed(fn, calls[k])
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(round(timed(fn, calls[k]), 5))
    return out


def yardstick_rows(sizes, tiny):
    """The existing render on tools/time_mesh_depth.py's scene: its meshes, its seed, its rigs."""
    meshes = synthetic_parts(3, 8, 8) if tiny else synthetic_parts(M, 75, 75)
    rows = []
    for name, image_mode in RIGS:
        poses, intr, im_h, im_w = rig(image_mode, tiny)
        for B in sizes:
            cam = DepthFromMesh(B, DEV, poses, intr, im_h, im_w, meshes=meshes)
            R, T = random_poses(B, len(meshes), torch.Generator(device=DEV).manual_seed(32), DEV)
            out = torch.empty(B, cam.num_view * im_h * im_w, device=DEV)
            ms = in_turn(dict(render=lambda: cam.render(R, T, out=out)))["render"]
            rows.append(dict(rig=name, B=B, triangles=int(cam.faces.shape[0]), render_ms=round(float(np.mean(ms)), 5), render_ms_rounds=ms))
            del cam, out
            torch.cuda.empty_cache()
    return rows


def scene_rows(sizes, tiny):
    robot = synthetic_parts(3 if tiny else ROBOT_PARTS, *((8, 8) if tiny else (75, 75)))
    library = cabinet_library(tiny)
    nr, rows = len(robot), []
    flat = [mesh for bodies in library for mesh in bodies]                                 # all_in_one: slot nr + 4 k + j
    # ... coloured like slot nr + j of the grouped scene, so that the two colour images can be compared
    palette = [PALETTE[s % len(PALETTE)] for s in range(nr)] + [PALETTE[(nr + j) % len(PALETTE)] for _ in library for j in range(BODIES)]
    for name, image_mode in RIGS:
        poses, intr, im_h, im_w = rig(image_mode, tiny)
        for B in sizes:
            group_of = np.arange(B) % CABINETS
            grouped = DepthFromMesh(B, DEV, poses, intr, im_h, im_w, meshes=robot, groups=library, group_of=group_of)
            whole = DepthFromMesh(B, DEV, poses, intr, im_h, im_w, meshes=robot + flat, palette=palette)
            R, T = random_poses(B, nr + BODIES, torch.Generator(device=DEV).manual_seed(33), DEV)
            Rw = torch.full((B, nr + CABINETS * BODIES, 3, 3), float("nan"), device=DEV)
            Tw = torch.full((B, nr + CABINETS * BODIES, 3), float("nan"), device=DEV)
            Rw[:, :nr], Tw[:, :nr] = R[:, :nr], T[:, :nr]
            slot = torch.as_tensor(nr + BODIES * group_of, device=DEV)[:, None] + torch.arange(BODIES, device=DEV)[None]
            e = torch.arange(B, device=DEV)[:, None]
            Rw[e, slot], Tw[e, slot] = R[:, nr:], T[:, nr:]
            V = grouped.num_view
            out = torch.empty(B, V * im_h * im_w, device=DEV)
            fns = dict(grouped=lambda: grouped.render(R, T, out=out), all_in_one=lambda: whole.render(Rw, Tw, out=out))
            frames = image_mode or B <= 64
            if frames:
                fns.update(grouped_frame=lambda: grouped.render_frame(R, T), all_in_one_frame=lambda: whole.render_frame(Rw, Tw))
            ms = in_turn(fns)
            a, b = grouped.render(R, T), whole.render(Rw, Tw)
            same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
            if frames:
                fa, fb = grouped.render_frame(R, T), whole.render_frame(Rw, Tw)
                same = same and bool(torch.equal(fa.depth.view(torch.int32), fb.depth.view(torch.int32)) and torch.equal(fa.rgb, fb.rgb))
            own = np.diff(grouped.group_off)[group_of]
            row = dict(rig=name, B=B, views=V, im_h=im_h, im_w=im_w, shared_triangles=grouped.face_shared,
                       library_triangles=int(grouped.group_off[-1]), cabinet_triangles=np.diff(grouped.group_off).tolist(),
                       max_group_faces=grouped.max_group_faces, mean_triangles_per_env_grouped=round(grouped.face_shared + float(own.mean()), 1),
                       triangles_per_env_all_in_one=int(whole.faces.shape[0]), same_bits=same, hit_share=round(float((a < grouped.far).float().mean()), 4))
            for k, v in ms.items():
                row[k + "_ms"], row[k + "_ms_rounds"] = round(float(np.mean(v)), 5), v
            row["all_in_one_over_grouped"] = round(row["all_in_one_ms"] / row["grouped_ms"], 3)
            if frames:
                row["all_in_one_over_grouped_frame"] = round(row["all_in_one_frame_ms"] / row["grouped_frame_ms"], 3)
            rows.append(row)
            del grouped, whole, out, Rw, Tw
            torch.cuda.empty_cache()
    return rows


def regression(parent_files, new_files):
    """The yardstick lines of fresh processes run by turns on the parent commit and on this one -> per (rig, B) both sets of runs, the
    new median and whether it lies within the spread of the parent's runs."""
    def load(files):
        runs = []
        for path in files:
            with open(path) as f:
                runs.append({(r["rig"], r["B"]): r["render_ms"] for r in json.loads(f.read().strip().splitlines()[-1])["rows"]})
        return runs
    parent, new = load(parent_files), load(new_files)
    rows = []
    for key in parent[0]:
        p, n = [r[key] for r in parent], [r[key] for r in new]
        med = float(np.median(n))
        rows.append(dict(rig=key[0], B=key[1], parent_ms=p, new_ms=n, new_median_ms=med, parent_min_ms=min(p), parent_max_ms=max(p),
                         new_median_within_parent_spread=bool(min(p) <= med <= max(p)), new_median_over_parent_median=round(med / float(np.median(p)), 5)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="B = 2, small meshes, a 16th of each image side; writes nothing")
    ap.add_argument("--yardstick", action="store_true", help="only the existing render on time_mesh_depth.py's scene; writes nothing")
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--parent-runs", nargs="*", default=[], help="yardstick lines of the parent commit, one file per process")
    ap.add_argument("--new-runs", nargs="*", default=[], help="yardstick lines of this commit, one file per process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [2] if a.tiny else [int(v) for v in a.sizes.split(",")]
    head = dict(tool="time_drawer_scene", measured=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0))
    if a.yardstick:
        print(json.dumps(dict(head, mode="yardstick", rows=yardstick_rows(sizes, a.tiny))))
        return
    line = dict(head, robot_parts=ROBOT_PARTS, cabinets=CABINETS, bodies_per_cabinet=BODIES, rows=scene_rows(sizes, a.tiny),
                existing_render_same_process=yardstick_rows(sizes, a.tiny))
    if a.parent_runs or a.new_runs:
        line["existing_render_parent_vs_new"] = regression(a.parent_runs, a.new_runs)
    line = json.dumps(line)
    print(line)
    out_path = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "drawer_scene_timing.json"))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
