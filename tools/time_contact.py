"""Time ContactSensor.sense (pm_mesh_sdf_points_f32 / pm_mesh_sdf_points_groups_f32) beside a plain tensor-library evaluation of the
same contract, in one process, alternating, and the whole KinematicEnv.step with and without contact=.

Workload: 3 sensing bodies x 512 points (the hand's and the fingers' slots), N in {64, 1024, 4096} environments, against
  cube      one target grid (a 5 cm box on 2.5 mm cells) among 12 parts, the ungrouped entry;
  cabinets  a grouped library of 8 synthetic cabinets of 2-7 bodies behind 11 shared grids, every environment sensing its own
            cabinet's rows, the grouped entry.
The sensing bodies sit within a few centimetres of their targets, so most points fall inside a valid box (`in_range`): the cull has
little to reject and the gathers are paid for.  No threshold: the lines say what was measured.  A point within float32 round-off of a
validity border may be sampled by one evaluation and called far by the other (the tensor library's bmm rounds in another order);
such points are counted (`border_flips`) and left out of `max_abs_diff`.

    python tools/time_contact.py [--tiny] [--sizes 64,1024,4096] [--out profiles/contact_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from partmanip_amd.contact import ContactSensor  # noqa: E402
from partmanip_amd.mesh2sdf import TSDFfromMesh  # noqa: E402
from tools.time_mesh_tsdf import synthetic_parts  # noqa: E402
from tools.timing import timed  # noqa: E402

DEV = "cuda:0"
SLOTS, PER_BODY = (8, 9, 10), 512
BODIES = (2, 3, 4, 5, 6, 7, 3, 4)                             # bodies of the 8 cabinets
URDF = os.path.join(ROOT, "tests", "golden", "franka_panda_sdf.urdf")
SCENE = os.path.join(ROOT, "tests", "golden", "kinematic_grasp_scene.json")


def box_grid(half=0.025, vs=0.0025, trunc=0.02):
    n = int(np.ceil((2 * half + 2 * trunc) / vs)) + 10
    idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1)
    pts = (idx - n // 2) * vs
    q = np.abs(pts) - half
    d = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    return {'sdf': np.clip(d, -trunc, trunc).astype(np.float32), 'bbox_min': pts.reshape(-1, 3).min(axis=0).astype(np.float32), 'voxel_size': vs}


def rotations(B, M, g):
    q = torch.nn.functional.normalize(torch.randn(B, M, 4, generator=g), dim=-1)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(B, M, 3, 3)


def build(scene, B, per_body=PER_BODY, seed=21):
    """(sensor, pose_R, pose_T, own: per group the list of (row, slot) of the target ordinals, group of every environment)."""
    g = torch.Generator().manual_seed(seed)
    robot = synthetic_parts()[:11]
    if scene == "cube":
        tsdf = TSDFfromMesh(B, 0.5, 50, DEV, sdf_dicts=robot + [box_grid()])
        targets, own, group = (11, 12), [[(11, 11)]], np.zeros(B, dtype=np.int64)
    else:
        cab = [synthetic_parts(seed=31 + k)[:n] for k, n in enumerate(BODIES)]
        tsdf = TSDFfromMesh(B, 0.5, 50, DEV, sdf_dicts=robot, groups=cab)
        targets = (11, 11 + max(BODIES))
        rows, own = 11, []
        for n in BODIES:
            own.append([(rows + j, 11 + j) for j in range(n)])
            rows += n
        group = np.arange(B) % len(BODIES)
    M = tsdf.part_num
    R = rotations(B, M, g)
    centre = torch.stack([torch.rand(B, generator=g) * 0.3 - 0.15, torch.rand(B, generator=g) * 0.3 - 0.15, torch.rand(B, generator=g) * 0.3], dim=-1)
    T = centre[:, None] + (torch.rand(B, M, 3, generator=g) - 0.5) * (0.06 if scene == "cube" else 0.16)
    pts = (torch.rand(len(SLOTS) * per_body, 3, generator=g) - 0.5) * torch.tensor([0.04, 0.02, 0.06])
    sensor = ContactSensor(tsdf, pts.numpy(), np.repeat(SLOTS, per_body), [per_body] * len(SLOTS), targets, names=("hand", "lfinger", "rfinger"))
    return sensor, R.to(DEV).contiguous(), T.to(DEV).contiguous(), own, group


def torch_sense(sensor, R, T, own, group, shapes, offs, chunk=256):
    """The contract with tensor-library calls: pose the points, loop over each group's target rows, minimum, per-body minimum."""
    o = sensor.tsdf
    pts, car = sensor._pts, sensor._carrier.long()
    real = sensor._pt_id >= 0
    pts, car = pts[real], car[real]                           # the layout keeps each body's points together, in order
    B, NB = R.shape[0], sensor.num_bodies
    dist = torch.ones(B, pts.shape[0], device=R.device)
    f = o.sdf_field
    for gid, rows in enumerate(own):
        envs = torch.from_numpy(np.flatnonzero(group == gid)).to(R.device)
        for b0 in range(0, len(envs), chunk):
            e = envs[b0:b0 + chunk]
            Rc, Tc = R[e], T[e]
            w = torch.einsum("bnij,nj->bni", Rc[:, car], pts) + Tc[:, car]
            best = torch.ones(len(e), pts.shape[0], device=R.device)
            for row, slot in rows:
                u = (torch.bmm(w - Tc[:, slot, None, :], Rc[:, slot]) - o.sdf_bbox_min[row]) / o.sdf_voxel_size[row]
                ok = ((u >= 1) & (u - o.sdf_field_res[row] <= -2)).all(dim=-1)
                u = u * ok[..., None]
                l = u.long()
                x, y, z = (u - l).unbind(-1)
                ry, rz = shapes[row][1], shapes[row][2]
                sy, sx = rz, rz * ry
                i0 = offs[row] + (l[..., 0] * ry + l[..., 1]) * rz + l[..., 2]
                val = ((f[i0] * (1 - z) + f[i0 + 1] * z) * (1 - y) + (f[i0 + sy] * (1 - z) + f[i0 + sy + 1] * z) * y) * (1 - x) \
                    + ((f[i0 + sx] * (1 - z) + f[i0 + sx + 1] * z) * (1 - y) + (f[i0 + sx + sy] * (1 - z) + f[i0 + sx + sy + 1] * z) * y) * x
                best = torch.minimum(best, torch.where(ok, val, torch.ones_like(val)))
            dist[e] = best
    return dist, dist.view(B, NB, -1).min(dim=2)[0]


def sense_rows(sizes, tiny=False):
    rows = []
    hip_calls = 3 if tiny else 50
    for B in sizes:
        for scene in ("cube", "cabinets"):
            sensor, R, T, own, group = build(scene, B, per_body=64 if tiny else PER_BODY)
            o = sensor.tsdf
            shapes, offs = o.sdf_field_res.cpu().tolist(), o.sdf_field_off.cpu().tolist()
            hip = lambda: sensor.sense(R, T, per_point=False)                            # noqa: E731
            full = lambda: sensor.sense(R, T)                                            # noqa: E731
            ref = lambda: torch_sense(sensor, R, T, own, group, shapes, offs)            # noqa: E731
            hip(), full(), ref()
            torch.cuda.synchronize()
            t_one = timed(ref, 1)
            torch_calls = 2 if tiny else int(max(2, min(20, 1000.0 / max(t_one, 1e-3))))
            hip_ms, full_ms, torch_ms = [], [], []
            for _ in range(2):                                                           # alternate in one process
                hip_ms.append(timed(hip, hip_calls))
                full_ms.append(timed(full, hip_calls))
                torch_ms.append(timed(ref, torch_calls))
            r = full()
            d_t, body_t = ref()
            assert r.dist.shape == d_t.shape                   # the sensor's bodies are one carrier each: the caller's order is kept
            diff = (r.dist - d_t).abs()
            flips = diff > 0.5 * (1 - 0.1)                      # far (1) on one side, a value inside the truncation band on the other
            same_cull = all(torch.equal(a, b) for a, b in zip(sensor.sense(R, T, cull=False), r))
            rows.append(dict(scene=scene, N=B, points=sensor.num_points, hip_ms=round(float(np.mean(hip_ms)), 5),
                             hip_with_per_point_ms=round(float(np.mean(full_ms)), 5), torch_ms=round(float(np.mean(torch_ms)), 4),
                             speedup=round(float(np.mean(torch_ms) / np.mean(hip_ms)), 1), hip_calls=2 * hip_calls, torch_calls=2 * torch_calls,
                             hip_ms_rounds=[round(v, 5) for v in hip_ms], max_abs_diff=float(diff[~flips].max()), border_flips=int(flips.sum()),
                             body_max_abs_diff=float((r.body_dist - body_t).abs().max()), in_range=round(float((r.dist < 1).float().mean()), 3),
                             cull_on_equals_off=bool(same_cull)))
            assert same_cull
            del sensor, R, T
            torch.cuda.empty_cache()
    return rows


def step_rows(sizes, steps=50):
    """ms per KinematicEnv.step of grasp_cube (golden Franka URDF, no observers) without contact=, with it, and with grasp='contact'."""
    from partmanip_amd.envs import make_grasp_cube_env
    from partmanip_amd.urdf import load_urdf
    with open(SCENE) as f:
        s = json.load(f)
    cfg = {"robot": {"driveMode": "ik", "mobile": False}, "explore_step": 40, "maxEpisodeLength": 200}
    tree = load_urdf(URDF)
    rows = []
    for N in sizes:
        g = torch.Generator().manual_seed(3)
        pts = (torch.rand(len(SLOTS) * PER_BODY, 3, generator=g) - 0.5) * torch.tensor([0.04, 0.02, 0.06])
        tsdf = TSDFfromMesh(N, 0.5, 50, DEV, sdf_dicts=synthetic_parts()[:11] + [box_grid()])
        sensor = ContactSensor(tsdf, pts.numpy(), np.repeat(SLOTS, PER_BODY), [PER_BODY] * 3, (11, 12), names=("hand", "lfinger", "rfinger"))
        a = torch.rand(N, 7, generator=g).to(DEV) * 2 - 1
        ms = {}
        envs = {"plain": {}, "contact": dict(contact=sensor), "contact_grasp": dict(contact=sensor, grasp="contact")}
        built = {k: make_grasp_cube_env(cfg, N, DEV, tree, 1.0 / 60.0, base_pose=s["root"], dof=s["dof"], **kw) for k, kw in envs.items()}
        for env in built.values():
            env.reset()
            for _ in range(5):
                env.step(a)
        torch.cuda.synchronize()
        for rnd in range(2):                                                             # alternate
            for k, env in built.items():
                ms.setdefault(k, []).append(timed(lambda: env.step(a), steps))
        rows.append(dict(N=N, steps=2 * steps, **{f"{k}_step_ms": round(float(np.mean(v)), 4) for k, v in ms.items()},
                         contact_adds_ms=round(float(np.mean(ms["contact"]) - np.mean(ms["plain"])), 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="N = 4, 64 points per body, 3 calls (the test suite's smoke run)")
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None, help="also write the JSON there (profiles/contact_timing.json)")
    a = ap.parse_args()
    sizes = [4] if a.tiny else [int(v) for v in a.sizes.split(",")]
    res = dict(tool="time_contact", device=torch.cuda.get_device_name(0), bodies=len(SLOTS), points_per_body=64 if a.tiny else PER_BODY,
               cabinets=list(BODIES), sense=sense_rows(sizes, a.tiny), step=step_rows(sizes, 3 if a.tiny else 50))
    line = json.dumps(res)
    print(line)
    if a.out and not a.tiny:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
