#!/usr/bin/env python3
"""Time the depthResNet student (network.name: depthResNet) on the GPU -> profiles/depth_resnet_timing.json.

    python tools/time_depth_resnet.py [--batches 16 100] [--reps 10] [--out profiles/depth_resnet_timing.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--proprio", type=int, default=22)
    ap.add_argument("--actions", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_resnet_timing.json"))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn evaluation of the same network")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_depth_resnet.py measures on the GPU: none found (there is no CPU timing to fall back to)")
    from partmanip_amd import ops
    from partmanip_amd.algo_utils.network import depthResNet
    dev = torch.device("cuda:0")
    width = 72 * 128 + args.proprio
    torch.manual_seed(0)
    net = depthResNet(width, args.actions, dict(name="depthResNet", activation="tanh"), args.proprio).to(dev)
    net.set_grad_views({k: torch.zeros_like(p) for k, p in net.named_parameters()})
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, proprio=args.proprio, actions=args.actions,
               hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S, note="no threshold is attached to these numbers",
               bn_kernels_note="bytes = what the algorithm must move (stats 1, apply 3, backward 8 passes over the activation); the activation "
                               "(9 MB at B = 16, 59 MB at B = 100) fits the 256 MiB Infinity Cache, so a share of the HBM floor above 1 is "
                               "cache residency between the repeated calls, not HBM bandwidth", batches={})

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for B in args.batches:
        x = depth_obs(B, width, dev)
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
            print(f"B={B} {name}: {total:.3f} ms (conv {conv * scale:.3f}, bn+pool {bnp * scale:.3f}, rest {total - (conv + bnp) * scale:.3f})")
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
        tl = DepthResNetRef(width, args.actions, "tanh", args.proprio).to(dev)
        tl.load_state_dict(net.state_dict())
        for B in args.batches:
            x = depth_obs(B, width, dev)
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
    print("->", args.out)


if __name__ == "__main__":
    main()
