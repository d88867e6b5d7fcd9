"""Time the part-mask clouds beside what they are built from, in one process, alternating (device events around warmed calls):

  front    ops.depth_cloud (pm_depth_cloud_f32: depth images -> compact cloud + source pixels, one launch) against
           ops.depth_backproject + ops.depth_compact, with the bytes of the buffers either side allocates;
  masked   TSDFVolume.depth2pc_masked against TSDFVolume.depth2pc (K = 1024; the sampler is in both);
  mesh     PCfromMesh.query_pc(mask=True) against query_pc with the same device selection (12 parts x 1024 points)

on the image rig (1 x 72 x 128) and the shipped rig (3 x 288 x 512) at 64 environments and the image rig at 1024.  The headline is
the front end's ratio and the memory it no longer allocates: the sampler dominates depth2pc either way.  No threshold applies.

  --unchanged          only the paths this feature did not mean to change -- the default query_pc, query_pc with a device selection
                       and depth2pc at 64 and 1024 environments -- as one JSON line (what --ab runs in fresh processes);
  --root DIR           time the partmanip_amd package of another built checkout (with --unchanged);
  --ab DIR             run `--unchanged` in three fresh processes of this tree and three of the checkout DIR (the parent commit,
                       built), by turns, and record the medians, their ratio new / parent and the parent's own spread (max / min of
                       its three processes; inside_parent_spread: the new median lies between the parent's fastest and slowest
                       process, ratio_within_parent_spread: 1 / spread <= ratio <= spread).  A child that fails stops the tool:
                       nothing more is started.

Prints one JSON line and writes it to profiles/depth_cloud_timing.json (--out; nothing is written with --tiny or --unchanged).

    python tools/time_depth_cloud.py [--tiny] [--ab DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
RIGS = (("image", True, 64), ("shipped", False, 64), ("image", True, 1024))
K = 1024
PARTS, POINTS = 12, 1024


def timed(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, calls, rounds=2):
    """{name: mean ms per call} of the warmed functions, timed by turns."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, calls))
    return {k: float(np.mean(v)) for k, v in ms.items()}


def rig(image_mode, B, tiny=False):
    """(volume with the rig registered, depth (B, V, h, w) on the device, V, h, w): the shipped cameras around the default workspace,
    seeded depths from 0.3 to 0.9 along every ray, so that part of every image falls inside the box."""
    import torch
    from partmanip_amd import camera
    from partmanip_amd.depth2tsdf import TSDFVolume
    cam_pose, intr, im_h, im_w = camera.shipped_rig({"look_at": [0.0, 0.0, 0.1], "radius": 0.6}, image_mode=image_mode)
    if tiny:
        intr = np.array([[intr[0][0] / 4, 0, im_w // 8], [0, intr[1][1] / 4, im_h // 8], [0, 0, 1]])
        im_h, im_w = im_h // 4, im_w // 4
    vol = TSDFVolume(DEV)
    vol.register_camera(cam_pose, intr, im_h, im_w, B)
    g = torch.Generator(device=DEV).manual_seed(31)
    depth = torch.rand(B, len(cam_pose), im_h, im_w, device=DEV, generator=g) * 0.6 + 0.3
    return vol, depth, len(cam_pose), im_h, im_w


def box_args(vol):
    i = vol.cam_intr
    lo = vol._vol_origin.cpu().numpy().astype(np.float32)
    return float(i[0][0]), float(i[1][1]), float(i[0][2]), float(i[1][2]), lo, (np.float32(vol._size) + lo).astype(np.float32)


def mesh_cloud(B, m=PARTS, p=POINTS):
    import torch
    from partmanip_amd.mesh2pc import PCfromMesh, random_poses
    parts = np.random.RandomState(21).uniform(-0.07, 0.07, size=(m, p, 3)).astype(np.float32)
    pc = PCfromMesh(B, DEV, num_points=p, part_pcs=parts)
    R, T = random_poses(B, m, torch.Generator(device=DEV).manual_seed(22), DEV)
    sel = torch.randperm(m * p, device=DEV)[:p].to(torch.int32)
    return pc, R, T, sel


def unchanged(tiny):
    """ms per call of the paths that exist on both sides of this feature."""
    import torch
    rows = {}
    for B in ((4,) if tiny else (64, 1024)):
        m, p = (3, 64) if tiny else (PARTS, POINTS)
        pc, R, T, sel = mesh_cloud(B, m, p)
        out = torch.empty(B, 3 * p, device=DEV)
        vol, depth, _, _, _ = rig(True, B, tiny)
        k = 64 if tiny else K
        ms = alternate(dict(query_pc=lambda: pc.query_pc(R, T, out=out), query_pc_sel=lambda: pc.query_pc(R, T, out=out, sel=sel),
                            depth2pc=lambda: vol.depth2pc(depth, K=k)), 3 if tiny else 20)
        rows[str(B)] = {n: round(v, 5) for n, v in ms.items()}
        del pc, vol, depth, out
        torch.cuda.empty_cache()
    return rows


def ab(parent, tiny):
    """Three fresh processes per side, by turns; a child that fails ends the run."""
    runs = {"new": [], "parent": []}
    for _ in range(3):
        for side, root in (("new", None), ("parent", parent)):
            cmd = [sys.executable, os.path.abspath(__file__), "--unchanged"] + (["--tiny"] if tiny else []) + (["--root", root] if root else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"{side}: `{' '.join(cmd)}` ended with {p.returncode}; nothing more is started\n{p.stderr[-2000:]}")
            runs[side].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["unchanged"])
    res = {}
    for B in runs["new"][0]:
        res[B] = {}
        for name in runs["new"][0][B]:
            new, old = ([r[B][name] for r in runs[s]] for s in ("new", "parent"))
            ratio, spread = float(np.median(new) / np.median(old)), float(max(old) / min(old))
            res[B][name] = dict(new_ms=new, parent_ms=old, new_median_ms=float(np.median(new)), parent_median_ms=float(np.median(old)),
                                ratio_new_over_parent=round(ratio, 4), parent_spread_max_over_min=round(spread, 4),
                                inside_parent_spread=bool(min(old) <= np.median(new) <= max(old)),
                                ratio_within_parent_spread=bool(1 / spread <= ratio <= spread))
    return res


def feature(tiny):
    import torch
    from partmanip_amd import ops
    rows = []
    for name, image_mode, B in (RIGS[:1] if tiny else RIGS):
        B = 4 if tiny else B
        vol, depth, V, h, w = rig(image_mode, B, tiny)
        P = V * h * w
        args = box_args(vol)
        seg = torch.randint(-1, 12, depth.shape, device=DEV, dtype=torch.int32)
        k = 64 if tiny else K
        big = not tiny and P * B > 10 ** 7                               # the shipped rig: the sampler walks ~10^5 points per pick
        calls = 3 if tiny or big else 20
        front = alternate(dict(fused=lambda: ops.depth_cloud(depth, vol.cam_pose, *args),
                               pair=lambda: ops.depth_compact(ops.depth_backproject(depth, vol.cam_pose, *args))), 3 if tiny else 20)
        lengths = ops.depth_cloud(depth, vol.cam_pose, *args)[2]
        whole = alternate(dict(depth2pc_masked=lambda: vol.depth2pc_masked(depth, seg, K=k), depth2pc=lambda: vol.depth2pc(depth, K=k)), calls)
        a, b = vol.depth2pc_masked(depth, seg, K=k)[..., :3], vol.depth2pc(depth, K=k)
        same = bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
        rows.append(dict(rig=name, B=B, views=V, im_h=h, im_w=w, pixels_per_env=P, K=k, kept_fraction=round(float(lengths.float().mean()) / P, 4),
                         front_ms={n: round(v, 5) for n, v in front.items()}, front_ratio_fused_over_pair=round(front["fused"] / front["pair"], 4),
                         buffer_bytes=dict(pair=2 * B * P * 12, fused=B * P * 16 + 4 * B),
                         whole_ms={n: round(v, 5) for n, v in whole.items()},
                         whole_ratio_masked_over_plain=round(whole["depth2pc_masked"] / whole["depth2pc"], 4), xyz_bits_equal=same,
                         calls=dict(front=2 * (3 if tiny else 20), whole=2 * calls)))
        del vol, depth, seg
        torch.cuda.empty_cache()
    mesh = []
    for B in ((4,) if tiny else (64, 1024)):
        m, p = (3, 64) if tiny else (PARTS, POINTS)
        pc, R, T, sel = mesh_cloud(B, m, p)
        o3, o4 = torch.empty(B, 3 * p, device=DEV), torch.empty(B, 4 * p, device=DEV)
        ms = alternate(dict(mask=lambda: pc.query_pc(R, T, out=o4, sel=sel, mask=True), plain=lambda: pc.query_pc(R, T, out=o3, sel=sel)),
                       3 if tiny else 20)
        mesh.append(dict(B=B, parts=m, points=p, ms={n: round(v, 5) for n, v in ms.items()}, ratio_mask_over_plain=round(ms["mask"] / ms["plain"], 4)))
    return rows, mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="4 environments, a quarter-size image rig, 3 calls (the test suite's smoke run)")
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--ab", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.join(HERE, ".."))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_depth_cloud: needs the GPU (no timing is taken on a CPU)")
    if a.unchanged:
        print(json.dumps(dict(tool="time_depth_cloud", unchanged=unchanged(a.tiny))))
        return
    res = dict(measured=time.strftime("%Y-%m-%d"), tool="time_depth_cloud", device=torch.cuda.get_device_name(0))
    if a.ab:
        res["unchanged_paths_new_vs_parent"] = ab(a.ab, a.tiny)
    res["sizes"], res["mesh_cloud"] = feature(a.tiny)
    line = json.dumps(res)
    print(line)
    out = a.out or (None if a.tiny else os.path.join(HERE, "..", "profiles", "depth_cloud_timing.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
