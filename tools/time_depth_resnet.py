#!/usr/bin/env python3
"""Time the image students (network.name: depthResNet / ResNet) on the GPU -> profiles/depth_resnet_timing.json, or with
--student ResNet / both -> profiles/rgb_resnet_timing.json.

    python tools/time_depth_resnet.py [--student depthResNet|ResNet|both] [--batches 16 100] [--reps 10] [--out FILE]

--student both times the two students beside each other in one process (they differ by the stem only: a 160-column patch matrix
of three planes instead of a 64-column one) and, per step at 64 and 1024 environments on the image rig (1 x 72 x 128, the scene
of tools/time_mesh_depth.py), rgb_img_observer beside depth_img_observer.

Per batch size (16, and 100 = the shipped ring's mini-batch: 1600 rows / 16 mini-batches): ms per training forward + backward and
per eval forward (device events around `reps` passes after a warm-up), split into
  conv     the gathered-GEMM launches (ops.sparse_conv_fwd / _bwd_data / _bwd_data_scatter / _bwd_weight),
  bn_pool  the launches of csrc/bn_pool2d.hip (ops.bn2d_* and ops.pool2d_*),
  rest     everything else of the pass: the stem's patch matrix and GEMM, the head, the weight-layout copies, allocations and the
           gaps between launches,
the split being taken in a SECOND set of passes with an event pair around every such call (the brackets slow the host, so the
split is scaled to the un-bracketed total).  Beside it the same network as torch.nn modules (tests/depth_resnet_ref.py) on the
same device in the same process, and the batch-norm kernels alone on the largest activation of the pass against the HBM floor
(bytes the algorithm must move over the measured copy bandwidth of the chip).  No threshold is attached to any of these numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12          # MI355X: measured float4 copy rate (8.0 TB/s on the data sheet)
CONV = ("sparse_conv_fwd", "sparse_conv_bwd_data", "sparse_conv_bwd_data_scatter", "sparse_conv_bwd_weight")
BN_POOL = ("bn2d_stats", "bn2d_invstd", "bn2d_apply", "bn2d_bwd", "pool2d_max_fwd", "pool2d_max_bwd", "pool2d_avg_fwd", "pool2d_avg_bwd")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


class Brackets:
    """An event pair around every call of the named ops, while active."""

    def __init__(self, ops):
        self.ops, self.events, self.saved = ops, {"conv": [], "bn_pool": []}, {}

    def __enter__(self):
        for kind, names in (("conv", CONV), ("bn_pool", BN_POOL)):
            for n in names:
                self.saved[n] = getattr(self.ops, n)
                setattr(self.ops, n, self._wrap(self.saved[n], kind))
        return self

    def _wrap(self, fn, kind):
        def call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.events[kind].append((e0, e1))
            return out
        return call

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.ops, n, fn)

    def ms(self, kind):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events[kind]), len(self.events[kind])


def depth_obs(n, width, device):
    g = torch.Generator().manual_seed(1)
    x = 0.3 + 1.5 * torch.rand(n, width, generator=g)
    x[:, :72 * 128][torch.rand(n, 72 * 128, generator=g) < 0.2] = 100.0
    return x.to(device)


def rgb_obs(n, width, device):
    """Raw 0..255 planes, a fifth of the pixels white; the tail as depth_obs has it."""
    g = torch.Generator().manual_seed(1)
    x = 0.3 + 1.5 * torch.rand(n, width, generator=g)
    img = torch.randint(0, 256, (n, 3, 72 * 128), generator=g).float()
    img[(torch.rand(n, 72 * 128, generator=g) < 0.2)[:, None].expand(n, 3, 72 * 128)] = 255.0
    x[:, :3 * 72 * 128] = img.reshape(n, -1)
    return x.to(device)


STUDENTS = dict(depthResNet=(1, depth_obs, dict(name="depthResNet", activation="tanh")),
                ResNet=(3, rgb_obs, dict(name="ResNet", activation="tanh", pretrained=False)))


def time_observers(sizes, reps):
    """ms per write of depth_img_observer and rgb_img_observer into an observation row, taken in turn (three rounds)."""
    import numpy as np
    from partmanip_amd import camera
    from partmanip_amd.envs import depth_img_observer, rgb_img_observer
    from partmanip_amd.mesh2depth import DepthFromMesh
    from partmanip_amd.mesh2pc import random_poses
    from tools.time_mesh_depth import CAM, DEV, M, calls_for, synthetic_parts
    from tools.timing import timed as timed_calls
    meshes = synthetic_parts(M, 75, 75)
    rows = []
    for B in sizes:
        poses, intr, im_h, im_w = camera.shipped_rig(CAM, True)
        cam = DepthFromMesh(B, DEV, poses, intr, im_h, im_w, meshes=meshes)
        R, T = random_poses(B, len(meshes), torch.Generator(device=DEV).manual_seed(32), DEV)
        obs = dict(depth_img=depth_img_observer(cam), rgb_img=rgb_img_observer(cam))
        out = {k: torch.empty(B, ob.width + 22, device=DEV) for k, ob in obs.items()}
        fns = {k: (lambda k=k: obs[k].write(R, T, out[k])) for k in obs}
        calls = {k: calls_for(fn, most=max(reps, 2)) for k, fn in fns.items()}
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed_calls(fn, calls[k]))
        ms = {k: float(np.median(v)) for k, v in rounds.items()}
        rows.append(dict(envs=B, im_h=im_h, im_w=im_w, triangles=int(cam.faces.shape[0]), depth_img_ms=ms["depth_img"],
                         rgb_img_ms=ms["rgb_img"], ratio_rgb_over_depth=ms["rgb_img"] / ms["depth_img"], rounds_ms=rounds, calls=calls))
        print(f"envs={B}: depth_img_observer {ms['depth_img']:.4f} ms, rgb_img_observer {ms['rgb_img']:.4f} ms per step")
        del cam, out
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--proprio", type=int, default=22)
    ap.add_argument("--actions", type=int, default=10)
    ap.add_argument("--student", choices=("depthResNet", "ResNet", "both"), default="depthResNet")
    ap.add_argument("--observer-envs", type=int, nargs="*", default=[64, 1024], help="environments of the observer timing (--student both)")
    ap.add_argument("--out", default=None, help="default: profiles/depth_resnet_timing.json, or profiles/rgb_resnet_timing.json with "
                                                "--student ResNet / both")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn evaluation of the same network")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_depth_resnet.py measures on the GPU: none found (there is no CPU timing to fall back to)")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "depth_resnet_timing.json" if args.student == "depthResNet" else "rgb_resnet_timing.json")
    if args.student == "depthResNet":
        res = time_student("depthResNet", args, args.out)
    else:
        import datetime
        res = dict(tool="time_depth_resnet", measured=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0),
                   note="no threshold is attached to these numbers; the two students differ by the stem only", students={})

        def flush():
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        for name in (("depthResNet", "ResNet") if args.student == "both" else ("ResNet",)):
            res["students"][name] = time_student(name, args, None, bn_kernels=False)
            flush()
        if args.student == "both":
            for B in args.batches:
                d, r = (res["students"][n]["batches"][str(B)] for n in ("depthResNet", "ResNet"))
                res.setdefault("ResNet_over_depthResNet", {})[str(B)] = {k: r[k]["ms"] / d[k]["ms"] for k in ("train_fwd_bwd", "eval_fwd")}
            res["observers"] = time_observers(args.observer_envs, args.reps)
            flush()
    print("->", args.out)


def time_student(student, args, out_path, bn_kernels=True):
    """The timing record of one student; written to out_path after every batch size when one is given."""
    from partmanip_amd import ops
    from partmanip_amd.algo_utils import network
    in_ch, make_obs, cfg = STUDENTS[student]
    dev = torch.device("cuda:0")
    width = in_ch * 72 * 128 + args.proprio
    torch.manual_seed(0)
    net = getattr(network, student)(width, args.actions, cfg, args.proprio).to(dev)
    net.set_grad_views({k: torch.zeros_like(p) for k, p in net.named_parameters()})
    res = dict(device=torch.cuda.get_device_name(0), student=student, reps=args.reps, proprio=args.proprio, actions=args.actions,
               hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S, note="no threshold is attached to these numbers",
               bn_kernels_note="bytes = what the algorithm must move (stats 1, apply 3, backward 8 passes over the activation); the activation "
                               "(9 MB at B = 16, 59 MB at B = 100) fits the 256 MiB Infinity Cache, so a share of the HBM floor above 1 is "
                               "cache residency between the repeated calls, not HBM bandwidth", batches={})

    def flush():
        if out_path is None:
            return
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for B in args.batches:
        x = make_obs(B, width, dev)
        dy = torch.full((B, args.actions), 1.0 / (B * args.actions), device=dev)

        def train_pass():
            net.hip_forward(x)
            net.hip_backward(dy)

        def eval_pass():
            net.hip_forward(x)
        entry = {}
        for name, fn, training in (("train_fwd_bwd", train_pass, True), ("eval_fwd", eval_pass, False)):
            net.train(training)
            for _ in range(3):
                fn()
            total = timed(fn, args.reps)
            with Brackets(ops) as br:
                whole = timed(fn, args.reps)
            conv, n_conv = br.ms("conv")
            bnp, n_bnp = br.ms("bn_pool")
            conv, bnp = conv / args.reps, bnp / args.reps
            scale = total / whole
            entry[name] = dict(ms=total, ms_with_brackets=whole, conv_ms=conv * scale, bn_pool_ms=bnp * scale,
                               rest_ms=total - (conv + bnp) * scale, conv_launches=n_conv // args.reps, bn_pool_calls=n_bnp // args.reps)
            print(f"{student} B={B} {name}: {total:.3f} ms (conv {conv * scale:.3f}, bn+pool {bnp * scale:.3f}, rest {total - (conv + bnp) * scale:.3f})")
        if not bn_kernels:
            res["batches"][str(B)] = entry
            flush()
            continue
        # the batch-norm kernels alone on the pass's largest activation (the stem's: B*36*64 rows of 64 channels)
        rows, C = B * 36 * 64, 64
        z, r, y, d = (torch.randn(rows, C, device=dev) for _ in range(4))
        dx, dm = torch.empty_like(z), torch.empty_like(z)
        mean, invstd, gamma, beta, dg, db = (torch.ones(C, device=dev) for _ in range(6))
        ws = ops.Workspace(dev)
        nbytes = rows * C * 4
        kernels = dict(
            stats=(lambda: ops.bn2d_stats(z, 1e-5, mean, invstd, ws), 1 * nbytes),
            apply_residual_relu=(lambda: ops.bn2d_apply(z, mean, invstd, gamma, beta, y, r, True), 3 * nbytes),
            backward_relu_masked_out=(lambda: ops.bn2d_bwd(d, z, y, mean, invstd, gamma, dg, db, dx, ws, relu=True, dy_masked=dm), 8 * nbytes))
        entry["bn_kernels"] = {}
        for k, (fn, moved) in kernels.items():
            for _ in range(3):
                fn()
            ms = timed(fn, 50)
            entry["bn_kernels"][k] = dict(rows=rows, C=C, ms=ms, bytes=moved, bytes_per_s=moved / (ms * 1e-3),
                                          floor_ms=moved / HBM_COPY_BYTES_PER_S * 1e3, share_of_hbm_floor=moved / HBM_COPY_BYTES_PER_S * 1e3 / ms)
            print(f"B={B} bn {k}: {ms * 1e3:.1f} us, {moved / (ms * 1e-3) / 1e12:.2f} TB/s")
        res["batches"][str(B)] = entry
        flush()
    if not args.no_torch:
        from tests.depth_resnet_ref import DepthResNetRef
        from tests.rgb_resnet_ref import RGBResNetRef
        tl = (DepthResNetRef if in_ch == 1 else RGBResNetRef)(width, args.actions, "tanh", args.proprio).to(dev)
        tl.load_state_dict(net.state_dict())
        for B in args.batches:
            x = make_obs(B, width, dev)
            dy = torch.full((B, args.actions), 1.0 / (B * args.actions), device=dev)

            def t_train():
                for p in tl.parameters():
                    p.grad = None
                tl(x).backward(dy)

            def t_eval():
                with torch.no_grad():
                    tl(x)
            out = {}
            for name, fn, training in (("train_fwd_bwd", t_train, True), ("eval_fwd", t_eval, False)):
                tl.train(training)
                for _ in range(3):
                    fn()
                out[name] = dict(ms=timed(fn, args.reps))
                print(f"B={B} torch.nn {name}: {out[name]['ms']:.3f} ms")
            res["batches"][str(B)]["torch_nn_same_process"] = out
            flush()
    return res


if __name__ == "__main__":
    main()
