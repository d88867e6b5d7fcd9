"""Time DepthFromMesh.render (pm_mesh_depth_render_f32) for the shipped rig (3 views x 288 x 512) and the image rig (view 0 at 72 x
128) of partmanip_amd.camera.shipped_rig, at B in {64, 1024}, with synthetic parts of about the Franka's triangle count (12
ellipsoids of 11 100 triangles each; the Franka's visual meshes, hand, fingers and cube hold 134 936).  Device events around warmed
calls.  Beside it, in the same process and alternating with it, a tensor-library ray caster of the same contract (every pixel
against every triangle, chunked over triangles) at the largest size at which it fits a sitting: the image rig at B = 1.
(It poses the vertices with einsum, so its last bits and a few edge pixels differ from the kernel's stated association; the JSON
records how many.)  Prints one JSON line and writes it to profiles/mesh_depth_timing.json (--out; nothing is written with --tiny).

Per row: hip_ms per render; pixel_triangle_tests = the pixels of all triangle boxes (counted by tensor ops that restate the box
rule, so it is the work the rasteriser does, not B V H W F) and tests_per_s; floor_ms = 4 B V H W output bytes / 6.29 TB/s (the
measured HBM copy rate of the MI355X) and share_of_output_bandwidth_floor = floor_ms / hip_ms.  The kernel is bound by its
pixel-triangle tests and the triangle set-up, not by the output stream; the share says how far from a pure fill it is.

    python tools/time_mesh_depth.py [--tiny] [--sizes 64,1024]
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
from partmanip_amd.mesh2depth import DepthFromMesh  # noqa: E402
from partmanip_amd.mesh2pc import random_poses  # noqa: E402
from tools.timing import HBM_BYTES_PER_S, timed  # noqa: E402

DEV = "cuda:0"
M = 12
CAM = dict(look_at=[0.0, 0.0, 0.0], radius=0.8)                               # the grasp_cube task's `cam` block


def ellipsoid(half, nu, nv):
    """Closed mesh of 2 nu (nv - 1) triangles on an ellipsoid with the given half-extents."""
    th = np.pi * np.arange(1, nv) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nu))], axis=-1)
    verts = np.concatenate([ring.reshape(-1, 3), [[0, 0, 1], [0, 0, -1]]]) * np.asarray(half)
    top, bottom = (nv - 1) * nu, (nv - 1) * nu + 1
    faces = []
    for j in range(nu):
        k = (j + 1) % nu
        faces.append((top, j, k))
        faces.append((bottom, (nv - 2) * nu + k, (nv - 2) * nu + j))
        for i in range(nv - 2):
            a, b, c, d = i * nu + j, i * nu + k, (i + 1) * nu + k, (i + 1) * nu + j
            faces += [(a, d, c), (a, c, b)]
    return verts.astype(np.float32), np.asarray(faces, dtype=np.int64)


def synthetic_parts(m, nu, nv, seed=31):
    rng = np.random.RandomState(seed)
    return [ellipsoid(rng.uniform(0.03, 0.10, size=3), nu, nv) for _ in range(m)]


def camera_vertices(cam, R, T):
    """(B, V, NV, 3) camera-space vertices by tensor ops."""
    part = cam.vert_part.long()
    world = torch.einsum("bnji,ni->bnj", R[:, part], cam.verts) + T[:, part]
    C = cam.cam_pose
    return torch.einsum("bvnj,vjk->bvnk", world[:, None] - C[None, :, None, :3, 3], C[:, :3, :3])


def count_tests(cam, R, T, env_chunk=16):
    """Pixels in the boxes of all triangles: the rule of csrc/mesh_depth.hip restated with tensor ops."""
    H, W, total = cam.im_h, cam.im_w, 0
    faces = cam.faces.long()
    for lo in range(0, R.shape[0], env_chunk):
        p = camera_vertices(cam, R[lo:lo + env_chunk], T[lo:lo + env_chunk])[:, :, faces]          # (b, V, F, 3, 3)
        z = p[..., 2]
        u, v = p[..., 0] / z * cam.fx + cam.cx, p[..., 1] / z * cam.fy + cam.cy
        front = (z > cam.near).all(-1)
        ulo = torch.where(front, (u.min(-1).values.floor() - 1).clamp(min=0), torch.zeros_like(u[..., 0]))
        uhi = torch.where(front, (u.max(-1).values.ceil() + 1).clamp(max=W - 1), torch.full_like(u[..., 0], W - 1))
        vlo = torch.where(front, (v.min(-1).values.floor() - 1).clamp(min=0), torch.zeros_like(u[..., 0]))
        vhi = torch.where(front, (v.max(-1).values.ceil() + 1).clamp(max=H - 1), torch.full_like(u[..., 0], H - 1))
        n = (uhi - ulo + 1).clamp(min=0) * (vhi - vlo + 1).clamp(min=0)
        total += int(n.double().sum().item())
    return total


def torch_cast(cam, R, T, face_chunk=4096):
    """The contract with tensor-library calls: every pixel of every view against every triangle, (B, V, H, W)."""
    H, W, dev = cam.im_h, cam.im_w, R.device
    p = camera_vertices(cam, R, T)
    dx = ((torch.arange(W, device=dev, dtype=torch.float32) - cam.cx) / cam.fx).view(1, 1, 1, W, 1)
    dy = ((torch.arange(H, device=dev, dtype=torch.float32) - cam.cy) / cam.fy).view(1, 1, H, 1, 1)
    out = torch.full((R.shape[0], cam.num_view, H, W), cam.far, device=dev)
    faces = cam.faces.long()
    for lo in range(0, faces.shape[0], face_chunk):
        tri = p[:, :, faces[lo:lo + face_chunk]]                                                    # (B, V, f, 3, 3)
        p0, p1, p2 = (tri[:, :, None, None, :, i] for i in range(3))                                # (B, V, 1, 1, f, 3)
        w = [(dx * n[..., 0] + dy * n[..., 1]) + n[..., 2] for n in (torch.linalg.cross(p1, p2), torch.linalg.cross(p2, p0),
                                                                     torch.linalg.cross(p0, p1))]
        s = (w[0] + w[1]) + w[2]
        z = ((w[0] * p0[..., 2] + w[1] * p1[..., 2]) + w[2] * p2[..., 2]) / s
        same = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
        hit = same & (s != 0) & (z > cam.near) & (z < cam.far)
        out = torch.minimum(out, torch.where(hit, z, torch.full_like(z, cam.far)).amin(dim=-1))
    return out


def calls_for(fn, window_ms=400.0, most=20):
    """Warm `fn` and choose how many calls fill the timing window."""
    fn()
    torch.cuda.synchronize()
    one = timed(fn, 1)
    return max(2, min(most, int(window_ms / max(one, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="B = 2, 3 parts of 112 triangles, a 16th of each image side")
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--out", default=None, help="file the JSON line is also written to (default: profiles/mesh_depth_timing.json; "
                                                "none with --tiny)")
    a = ap.parse_args()
    sizes = [2] if a.tiny else [int(v) for v in a.sizes.split(",")]
    meshes = synthetic_parts(3, 8, 8) if a.tiny else synthetic_parts(M, 75, 75)
    m = len(meshes)
    rows, torch_row = [], None
    for rig, image_mode in (("shipped", False), ("image", True)):
        poses, intr, im_h, im_w = camera.shipped_rig(CAM, image_mode)
        if a.tiny:
            im_h, im_w, intr = im_h // 16 + 1, im_w // 16 + 1, intr / np.array([[16.0], [16.0], [1.0]])
        for B in sizes:
            cam = DepthFromMesh(B, DEV, poses, intr, im_h, im_w, meshes=meshes)
            R, T = random_poses(B, m, torch.Generator(device=DEV).manual_seed(32), DEV)
            V = cam.num_view
            out = torch.empty(B, V * im_h * im_w, device=DEV)
            fn = lambda: cam.render(R, T, out=out)                                                  # noqa: E731
            calls = calls_for(fn)
            rounds = [timed(fn, calls) for _ in range(3)]
            ms = float(np.mean(rounds))
            tests = count_tests(cam, R, T)
            floor = 4.0 * B * V * im_h * im_w / HBM_BYTES_PER_S * 1e3
            hit_share = float((out < cam.far).float().mean())
            rows.append(dict(rig=rig, B=B, views=V, im_h=im_h, im_w=im_w, triangles=int(cam.faces.shape[0]), hip_ms=round(ms, 5),
                             hip_ms_rounds=[round(x, 5) for x in rounds], calls=3 * calls, pixel_triangle_tests=tests,
                             tests_per_s=round(tests / (ms * 1e-3), 1), brute_force_pairs=B * V * im_h * im_w * int(cam.faces.shape[0]),
                             floor_ms=round(floor, 6), share_of_output_bandwidth_floor=round(floor / ms, 5), hit_share=round(hit_share, 4)))
            if image_mode and B == sizes[0]:
                # the tensor-library ray caster at B = 1, alternating with the kernel on the same single environment
                R1, T1 = R[:1].contiguous(), T[:1].contiguous()
                ref = lambda: torch_cast(cam, R1, T1)                                               # noqa: E731
                hip1 = lambda: cam.render(R1, T1)                                                   # noqa: E731
                c_ref, c_hip = calls_for(ref, most=5), calls_for(hip1)
                t_ms, h_ms = [], []
                for _ in range(2):
                    h_ms.append(timed(hip1, c_hip))
                    t_ms.append(timed(ref, c_ref))
                got, want = hip1(), ref()
                pairs = V * im_h * im_w * int(cam.faces.shape[0])
                torch_row = dict(rig=rig, B=1, torch_ms=round(float(np.mean(t_ms)), 4), hip_ms=round(float(np.mean(h_ms)), 5),
                                 speedup=round(float(np.mean(t_ms)) / float(np.mean(h_ms)), 1), torch_ms_rounds=[round(x, 4) for x in t_ms],
                                 hip_ms_rounds=[round(x, 5) for x in h_ms], torch_pairs_per_s=round(pairs / (float(np.mean(t_ms)) * 1e-3), 1),
                                 hit_or_miss_disagreements=int(((got < cam.far) != (want < cam.far)).sum()),
                                 max_abs_diff_where_both_hit=float(((got - want).abs() * ((got < cam.far) & (want < cam.far))).max()))
            del cam, out
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="time_mesh_depth", measured=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0),
                           parts=m, bound="pixel-triangle tests and triangle set-up (VALU), not bandwidth",
                           hbm_bytes_per_s=HBM_BYTES_PER_S, near=0.01, far=100.0, rows=rows, tensor_library_ray_caster=torch_row))
    print(line)
    out_path = a.out or (None if a.tiny else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mesh_depth_timing.json"))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
