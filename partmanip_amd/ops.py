"""Tensor-level wrappers over the C ABI (include/partmanip_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every op below passes
raw device pointers to libpartmanip_hip.so.  Ops refuse CPU tensors -- there is no CPU path.
"""
import ctypes as C
import os

import numpy as np

import torch

from ._lib import lib, check

ACT_NONE, ACT_TANH, ACT_RELU, ACT_LRELU, ACT_ELU, ACT_SELU, ACT_SIGMOID = range(7)      # PM_ACT_* of the header


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class KernelTimer:
    """HIP-event bracket around named launches (bench.py's live roofline measurement).
    Events are recorded on torch's current stream, which is the stream every op launches on."""

    def __init__(self):
        self.enabled = set()
        self.events = {}

    def enable(self, *names):
        self.enabled = set(names)
        self.events = {n: [] for n in names}

    def add(self, *names):
        """Enable more names without dropping the events collected so far."""
        self.enabled |= set(names)
        for n in names:
            self.events.setdefault(n, [])

    def disable(self):
        self.enabled = set()

    def bracket(self, name):
        return _Bracket(self, name) if name in self.enabled else _NULL

    def mean_ms(self, name):
        ev = self.events.get(name, [])
        if not ev:
            return None
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev), len(ev)


class _Bracket:
    def __init__(self, timer, name):
        self.t, self.n = timer, name

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.t.events[self.n].append((self.a, self.b))


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL = _Null()
TIMER = KernelTimer()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_NO_CPU = "partmanip_amd ops run on MI355X only: got a CPU tensor (no CPU fallback exists)"


def _req(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _one_device(fn, *ts):
    """_req, and all the tensors (None entries skipped) of the wrapper `fn` on the same device; one pass, it runs on every call."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{fn}: all tensors must live on one device")


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")


def _rows(t, name):
    """(ptr-able 2-D view, row stride in elements); last dim must be contiguous."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] != 1 and t.stride(1) != 1):   # a size-1 inner dim may carry any stride
        raise ValueError(f"{name}: expected a 2-D float32 tensor with unit inner stride, got {tuple(t.shape)} {t.stride()}")
    return t.stride(0)


def check_poses(pose_R, pose_T, M=None):
    """The pose inputs of an observer: float32 pose_R (B > 0, M > 0, 3, 3) and pose_T (B, M, 3), with M parts when M is given.
    Returns (B, M)."""
    s = pose_R.shape
    if len(s) != 4 or s[2] != 3 or s[3] != 3 or s[0] == 0 or (s[1] == 0 if M is None else s[1] != M):
        raise ValueError(f"pose_R: expected (B, {'M' if M is None else M}, 3, 3), got {tuple(s)}")
    if pose_T.shape != (s[0], s[1], 3):
        raise ValueError(f"pose_T: expected ({s[0]}, {s[1]}, 3), got {tuple(pose_T.shape)}")
    if pose_R.dtype != torch.float32 or pose_T.dtype != torch.float32:
        raise ValueError(f"pose_R / pose_T: expected float32, got {pose_R.dtype} and {pose_T.dtype}")
    return s[0], s[1]


def _out_rows(out, B, n, device=None, dtype=torch.float32, name="out"):
    """The `out=` rule of the observers: None gives a fresh (B, n) on `device`; otherwise a 2-D view (B, >= n) of `dtype` (float32;
    the frame camera's seg and rgb images are int32 and uint8) with unit inner stride and row stride >= n.  Returns (out, the row
    stride in elements to hand to C); a one-row view may carry any row stride, which counts as n.  The check reads no memory, so the
    observer classes run it on a given `out` before they ask for the device."""
    if out is None:
        return torch.empty(B, n, dtype=dtype, device=device), n
    s, st = out.shape, out.stride()
    if len(s) != 2 or s[0] != B or s[1] < n or out.dtype != dtype or (s[1] != 1 and st[1] != 1) or (B > 1 and st[0] < n):
        raise ValueError(f"{name}: expected a {str(dtype).replace('torch.', '')} view ({B}, >= {n}) with unit inner stride and row "
                         f"stride >= {n}, got {out.dtype} {tuple(s)} {st}")
    return out, max(st[0], n)


class Workspace:
    """Grow-only device scratch buffer handed to the C ABI (the library never allocates)."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.buf


# ----------------------------------------------------------------------------- K1-K3
def gae_scan(rewards, values, dones, succs, last_values, returns, advantages, gamma, lam, succ_value):
    _req(rewards, values, dones, succs, last_values, returns, advantages)
    T, N = rewards.shape[0], rewards.shape[1]
    for t, n in ((rewards, "rewards"), (values, "values"), (returns, "returns"), (advantages, "advantages"),
                 (last_values, "last_values")):
        _f32c(t, n)
    d8 = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
    s8 = succs.view(torch.uint8) if succs.dtype == torch.bool else succs
    use = succ_value is not None
    with TIMER.bracket("gae_scan"):
        check(lib.pm_gae_scan_f32(_ptr(rewards), _ptr(values), _ptr(d8), _ptr(s8), _ptr(last_values), _ptr(returns),
                                  _ptr(advantages), T, N, float(gamma), float(gamma * lam), int(use),
                                  float(succ_value) if use else 0.0, _stream()), "pm_gae_scan_f32")


def moments(x, out2, ws):
    _req(x, out2)
    _f32c(x, "x")
    n = x.numel()
    w = ws.get(lib.pm_moments_workspace_bytes(n))
    check(lib.pm_moments_f64(_ptr(x), n, _ptr(out2), _ptr(w), w.numel(), _stream()), "pm_moments_f64")


def normalize_apply(x, mom2, count, eps=1e-8):
    _req(x, mom2)
    _f32c(x, "x")
    check(lib.pm_normalize_apply_f32(_ptr(x), x.numel(), _ptr(mom2), float(count), float(eps), _stream()),
          "pm_normalize_apply_f32")


def gather_rows(src2d, idx, dst2d):
    _req(src2d, idx, dst2d)
    ls, ld = _rows(src2d, "src"), _rows(dst2d, "dst")
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64")
    check(lib.pm_gather_rows_f32(_ptr(src2d), _ptr(idx), _ptr(dst2d), idx.numel(), src2d.shape[1], ls, ld, _stream()),
          "pm_gather_rows_f32")


# ----------------------------------------------------------------------------- K4/K5
def linear_fwd(x, w, b, y, act):
    _req(x, w, b, y)
    M, K = x.shape
    N = w.shape[0]
    with (TIMER.bracket(f"linear_fwd_{M}x{K}x{N}") if TIMER.enabled else _NULL):     # (bench.py names the glue GEMMs it wants timed by shape)
        check(lib.pm_linear_fwd_f32(_ptr(x), _rows(x, "x"), _ptr(w), _rows(w, "w"), _ptr(b), _ptr(y), _rows(y, "y"),
                                    M, N, K, act, _stream()), "pm_linear_fwd_f32")


def linear_bwd_data(dy, w, h, dx, act):
    _req(dy, w, h, dx)
    M, N = dy.shape
    K = w.shape[1]
    with (TIMER.bracket(f"linear_bwd_data_{M}x{N}x{K}") if TIMER.enabled else _NULL):
        check(lib.pm_linear_bwd_data_f32(_ptr(dy), _rows(dy, "dy"), _ptr(w), _rows(w, "w"), _ptr(h),
                                         _rows(h, "h") if h is not None else 0, _ptr(dx), _rows(dx, "dx"), M, N, K, act,
                                         _stream()), "pm_linear_bwd_data_f32")
    return dx


def linear_bwd_weight(dy, x, dw, db, ws):
    _req(dy, x, dw, db)
    M, N = dy.shape
    K = x.shape[1]
    w = ws.get(lib.pm_linear_bwd_weight_workspace_bytes(M, N, K))
    with (TIMER.bracket(f"linear_bwd_weight_{M}x{N}x{K}") if TIMER.enabled else _NULL):
        check(lib.pm_linear_bwd_weight_f32(_ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(dw), _rows(dw, "dw"),
                                           _ptr(db), M, N, K, _ptr(w), w.numel(), _stream()), "pm_linear_bwd_weight_f32")


# ---- grouped forms: several independent problems of one kind in ONE launch (the actor's and the critic's layer l; all
# weight gradients of a backward pass).  Each item is the argument tuple of the single-problem op.
def linear_fwd_group(items):
    """items: [(x, w, b, y, act), ...]"""
    from ._lib import LinearFwdDesc
    arr = (LinearFwdDesc * len(items))()
    for d, (x, w, b, y, act) in zip(arr, items):
        _req(x, w, b, y)
        d.X, d.ldx, d.W, d.ldw, d.b, d.Y, d.ldy = _ptr(x), _rows(x, "x"), _ptr(w), _rows(w, "w"), _ptr(b), _ptr(y), _rows(y, "y")
        d.M, d.K, d.N, d.act = x.shape[0], x.shape[1], w.shape[0], act
    check(lib.pm_linear_fwd_group_f32(len(items), arr, _stream()), "pm_linear_fwd_group_f32")


def linear_bwd_data_group(items):
    """items: [(dy, w, h, dx, act), ...]"""
    from ._lib import LinearBwdDataDesc
    arr = (LinearBwdDataDesc * len(items))()
    for d, (dy, w, h, dx, act) in zip(arr, items):
        _req(dy, w, h, dx)
        d.dY, d.lddy, d.W, d.ldw, d.dX, d.lddx = _ptr(dy), _rows(dy, "dy"), _ptr(w), _rows(w, "w"), _ptr(dx), _rows(dx, "dx")
        d.H, d.ldh = _ptr(h), (_rows(h, "h") if h is not None else 0)
        d.M, d.N, d.K, d.act = dy.shape[0], dy.shape[1], w.shape[1], act
    check(lib.pm_linear_bwd_data_group_f32(len(items), arr, _stream()), "pm_linear_bwd_data_group_f32")


PM_EUNSUPPORTED = -4


def _chain_ws(ws, kind, M, N, n_layers):
    """The monotonic stripe counters + error word of one chain shape (zeroed once, never shared between shapes / directions)."""
    n = int(lib.pm_linear_chain_workspace_bytes(M)) // 8
    tab = getattr(ws, "chain_ctr", None)
    if tab is None:
        tab = ws.chain_ctr = {}
    key = (kind, M, N, n_layers)
    if key not in tab:
        tab[key] = torch.zeros(n, dtype=torch.int64, device=ws.device)
    return tab[key], n


def linear_fwd_chain(items, ws):
    """items: [(x, w, b, y, act), ...] with items[i + 1].x is items[i].y: consecutive layers in ONE launch (pm_linear_fwd_chain_f32).
    Returns False when the shapes do not fit the scheme (nothing was launched: issue the layers one by one)."""
    from ._lib import LinearFwdDesc
    arr = (LinearFwdDesc * len(items))()
    for d, (x, w, b, y, act) in zip(arr, items):
        _req(x, w, b, y)
        d.X, d.ldx, d.W, d.ldw, d.b, d.Y, d.ldy = _ptr(x), _rows(x, "x"), _ptr(w), _rows(w, "w"), _ptr(b), _ptr(y), _rows(y, "y")
        d.M, d.K, d.N, d.act = x.shape[0], x.shape[1], w.shape[0], act
    ctr, n = _chain_ws(ws, "fwd", items[0][0].shape[0], items[0][1].shape[0], len(items))
    rc = lib.pm_linear_fwd_chain_f32(len(items), arr, _ptr(ctr), n * 8, _stream())
    if rc == PM_EUNSUPPORTED:
        return False
    check(rc, "pm_linear_fwd_chain_f32")
    return True


def linear_bwd_data_chain(items, ws):
    """items: [(dy, w, h, dx, act), ...] top layer first, items[i + 1].dy is items[i].dx (pm_linear_bwd_data_chain_f32)."""
    from ._lib import LinearBwdDataDesc
    arr = (LinearBwdDataDesc * len(items))()
    for d, (dy, w, h, dx, act) in zip(arr, items):
        _req(dy, w, h, dx)
        d.dY, d.lddy, d.W, d.ldw, d.dX, d.lddx = _ptr(dy), _rows(dy, "dy"), _ptr(w), _rows(w, "w"), _ptr(dx), _rows(dx, "dx")
        d.H, d.ldh = _ptr(h), (_rows(h, "h") if h is not None else 0)
        d.M, d.N, d.K, d.act = dy.shape[0], dy.shape[1], w.shape[1], act
    ctr, n = _chain_ws(ws, "bwd", items[0][0].shape[0], items[0][1].shape[1], len(items))
    rc = lib.pm_linear_bwd_data_chain_f32(len(items), arr, _ptr(ctr), n * 8, _stream())
    if rc == PM_EUNSUPPORTED:
        return False
    check(rc, "pm_linear_bwd_data_chain_f32")
    return True


def chain_gave_up(ws):
    """True when a stripe barrier of the last chain launch on this workspace ran into its spin limit (host sync)."""
    tab = getattr(ws, "chain_ctr", None) or {}
    bad = [t for t in tab.values() if int(t[-1].item()) != 0]
    for t in bad:                # counters are monotonic across launches: after a failed launch they are off a launch boundary --
        t.zero_()                # start over (error word included), so that the NEXT launch is valid again
    return bool(bad)


def padded_cols(rows, cols, device, zero=False):
    """(rows, cols) fp32 view of a buffer whose rows are padded to a multiple of 4 floats; the view carries `_pm_cols` (the
    readable row width), which `linear_bwd_weight_group` hands to the kernels so that a 10- or 53-column operand takes the
    16-byte loaders."""
    w = (cols + 3) // 4 * 4
    buf = (torch.zeros if zero else torch.empty)(rows, w, device=device)
    v = buf[:, :cols]
    v._pm_cols = w
    return v


def linear_bwd_weight_group(items, splits=1):
    """items: [(dy, x, dw, db, slab_stride), ...]; splits > 1: slab z of dw / db lands at + z * slab_stride elements and the
    caller sums the slabs (clip_adam_group does)."""
    from ._lib import LinearBwdWeightDesc
    arr = (LinearBwdWeightDesc * len(items))()
    for d, (dy, x, dw, db, stride) in zip(arr, items):
        _req(dy, x, dw, db)
        # tensors whose allocator marked their rows as readable past the last column (`padded_cols`): 16-byte loaders
        d.dy_cols, d.x_cols = int(getattr(dy, "_pm_cols", 0)), int(getattr(x, "_pm_cols", 0))
        d.dY, d.lddy, d.X, d.ldx, d.dW, d.lddw, d.db = _ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(dw), _rows(dw, "dw"), _ptr(db)
        d.slab_stride, d.M, d.N, d.K = int(stride), dy.shape[0], dy.shape[1], x.shape[1]
    check(lib.pm_linear_bwd_weight_group_f32(len(items), arr, int(splits), _stream()), "pm_linear_bwd_weight_group_f32")


def linear_variant(kind, problems, splits=1, workspace=0):
    """Which kernel `kind` would run on (pm_linear_*_variant_f32: host only, no launch, no device needed).
    kind: "fwd", "bwd_data", "bwd_weight" with ONE problem, or "fwd_group", "bwd_data_group", "bwd_weight_group" with a list.
    A problem is a dict of the header's descriptor fields (fwd: X ldx W ldw b Y ldy M N K act; bwd_data: dY lddy W ldw H ldh dX
    lddx M N K act; bwd_weight: dY lddy X ldx dW lddw db M N K, grouped also slab_stride dy_cols x_cols); a pointer field is an
    address (only its alignment matters, 0 = NULL) or a tensor.  Returns the record as a dict: path ("skinny" / "reg" / "dma"),
    tm, tn, lay, stages, vec, big, grid, and per-problem lists vecC, splits, kchunk."""
    from ._lib import LinearFwdDesc, LinearBwdDataDesc, LinearBwdWeightDesc, LinearVariant, LINEAR_PATHS
    group = kind.endswith("_group")
    base = kind[:-6] if group else kind
    cls = {"fwd": LinearFwdDesc, "bwd_data": LinearBwdDataDesc, "bwd_weight": LinearBwdWeightDesc}[base]
    probs = list(problems) if group else [problems]
    arr = (cls * len(probs))()
    for d, q in zip(arr, probs):
        for k, v in q.items():
            setattr(d, k, _ptr(v) if isinstance(v, torch.Tensor) else (v or 0))
    out = LinearVariant()
    if group:
        args = (len(probs), arr) + ((int(splits),) if base == "bwd_weight" else ()) + (C.byref(out),)
    else:
        d = arr[0]
        if base == "fwd":
            args = (d.X, d.ldx, d.W, d.ldw, d.b, d.Y, d.ldy, d.M, d.N, d.K, d.act, C.byref(out))
        elif base == "bwd_data":
            args = (d.dY, d.lddy, d.W, d.ldw, d.H, d.ldh, d.dX, d.lddx, d.M, d.N, d.K, d.act, C.byref(out))
        else:
            args = (d.dY, d.lddy, d.X, d.ldx, d.dW, d.lddw, d.db, d.M, d.N, d.K,
                    _ptr(workspace) if isinstance(workspace, torch.Tensor) else workspace, C.byref(out))
    name = f"pm_linear_{kind}_variant_f32"
    check(getattr(lib, name)(*args), name)
    n = out.n
    return {"path": LINEAR_PATHS[out.path], "tm": out.tm, "tn": out.tn, "lay": out.lay, "stages": out.stages, "vec": out.vec,
            "big": out.big, "grid": out.grid, "vecC": list(out.vecC[:n]), "splits": list(out.splits[:n]),
            "kchunk": list(out.kchunk[:n])}


_SPARSE_VARIANT_FIELDS = {
    "fwd": ("src", "lds", "idx", "rows", "J", "C", "W", "ldw", "b", "Y", "ldy", "N", "act", "zero"),
    "bwd_data": ("dY", "lddy", "idxT", "rows", "J", "Cout", "Wt", "ldwt", "H", "ldh", "dX", "lddx", "Cin", "act", "zero"),
    "bwd_scatter": ("dY", "lddy", "W", "ldw", "idx", "rows", "J", "C", "Cout", "H", "dX", "act"),
    "bwd_weight": ("dY", "lddy", "src", "lds", "idx", "rows", "J", "C", "dW", "lddw", "db", "N", "zero", "workspace"),
}


def sparse_conv_variant(kind, problem):
    """Which kernel a sparse-convolution call would run on (pm_sparse_conv_*_variant_f32: host only, no launch, no device needed).
    kind: "fwd", "bwd_data", "bwd_scatter" (pm_sparse_conv_bwd_data_scatter_f32) or "bwd_weight".  `problem` is a dict of the launch's
    arguments by their header names, without the stream and workspace_bytes (a missing field is 0 / NULL); a pointer field is an
    address (only its alignment matters, 0 = NULL) or a tensor.  Returns the same dict as linear_variant."""
    from ._lib import LinearVariant, LINEAR_PATHS
    fields = _SPARSE_VARIANT_FIELDS[kind]
    unknown = set(problem) - set(fields)
    if unknown:
        raise ValueError(f"sparse_conv_variant({kind!r}): unknown fields {sorted(unknown)}")
    vals = [problem.get(k) for k in fields]
    out = LinearVariant()
    name = {"fwd": "pm_sparse_conv_fwd_variant_f32", "bwd_data": "pm_sparse_conv_bwd_data_variant_f32",
            "bwd_scatter": "pm_sparse_conv_bwd_data_scatter_variant_f32", "bwd_weight": "pm_sparse_conv_bwd_weight_variant_f32"}[kind]
    check(getattr(lib, name)(*[_ptr(v) if isinstance(v, torch.Tensor) else (v or 0) for v in vals], C.byref(out)), name)
    n = out.n
    return {"path": LINEAR_PATHS[out.path], "tm": out.tm, "tn": out.tn, "lay": out.lay, "stages": out.stages, "vec": out.vec,
            "big": out.big, "grid": out.grid, "vecC": list(out.vecC[:n]), "splits": list(out.splits[:n]),
            "kchunk": list(out.kchunk[:n])}


def clip_adam_group(items):
    """items: [dict(p, g, m, v, n_clip, max_norm, lr, b1, b2, eps, state, skip_flag, gnorm, ws, extra, extra_stride, n_sum,
    n_extra)]: pm_clip_adam_step_f32 for several optimisers in two launches; `extra` = split-K slabs 1.. of g[:n_sum]."""
    from ._lib import ClipAdamDesc
    arr = (ClipAdamDesc * len(items))()
    for d, it in zip(arr, items):
        p, g = it["p"], it["g"]
        _req(p, g, it["m"], it["v"], it["state"], it.get("skip_flag"), it.get("gnorm"), it.get("extra"))
        n = p.numel()
        w = it["ws"].get(lib.pm_clip_adam_workspace_bytes(n) + 8)
        base = w.data_ptr()
        d.params, d.grads, d.exp_avg, d.exp_avg_sq, d.n, d.n_clip = _ptr(p), _ptr(g), _ptr(it["m"]), _ptr(it["v"]), n, int(it["n_clip"])
        d.extra, d.extra_stride, d.n_sum, d.n_extra = _ptr(it.get("extra")), int(it.get("extra_stride", 0)), int(it.get("n_sum", 0)), int(it.get("n_extra", 0))
        d.max_norm, d.lr, d.b1, d.b2, d.eps = float(it["max_norm"]), float(it["lr"]), float(it["b1"]), float(it["b2"]), float(it["eps"])
        d.state, d.skip_flag, d.gnorm_out, d.workspace = _ptr(it["state"]), _ptr(it.get("skip_flag")), _ptr(it.get("gnorm")), base + (-base) % 8
        dp = it.get("dp")                                  # (1/W, scal or None, desired_kl or 0): data-parallel step, see the header
        if dp is not None:
            _req(dp[1])
            d.grad_scale, d.dp_scal, d.dp_kl_desired = float(dp[0]), _ptr(dp[1]), float(dp[2])
        st = it.get("stats")                               # (acc, scal, which): ppo_accumulate_stats inside the norm pass
        if st is not None:
            _req(st[0], st[1])
            d.stats_acc, d.stats_scal, d.stats_which = _ptr(st[0]), _ptr(st[1]), int(st[2])
    check(lib.pm_clip_adam_group_f32(len(items), arr, _stream()), "pm_clip_adam_group_f32")


def grad_slab_sum(g, extra, extra_stride, n_sum, n_extra):
    """g[:n_sum] += the n_extra split-K slabs (pm_grad_slab_sum_f32): before a gradient all-reduce."""
    _req(g, extra)
    check(lib.pm_grad_slab_sum_f32(_ptr(g), _ptr(extra), int(extra_stride), int(n_sum), int(n_extra), _stream()), "pm_grad_slab_sum_f32")


# ----------------------------------------------------------------------------- K6/K7
def pointnet_packed_elems():
    return int(lib.pm_pointnet_packed_elems())


def pointnet_pack(w2, w3, packed):
    _req(w2, w3, packed)
    check(lib.pm_pointnet_pack_weights_f32(_ptr(w2), _ptr(w3), _ptr(packed), _stream()), "pm_pointnet_pack_weights_f32")


def pointnet_enc_fwd(x, P, Cc, sub_mean, w1, b1, b2, b3, packed, max_mean, feat, argmax, h2_save=None, act=None):
    """h2_save: optional (B, P, 256) buffer the training forward fills with the layer-2 activations; act: ACT_* of the
    two hidden layers (default tanh)."""
    _req(x, w1, b1, b2, b3, packed, feat, argmax, h2_save)
    B = x.shape[0]
    with TIMER.bracket("pointnet_enc_fwd"):
        check(lib.pm_pointnet_enc_fwd_f32(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2),
                                          _ptr(b3), _ptr(packed), int(max_mean), _ptr(feat), _rows(feat, "feat"),
                                          _ptr(argmax), _ptr(h2_save), int(ACT_TANH if act is None else act), _stream()),
              "pm_pointnet_enc_fwd_f32")


def pointnet_packed_screen_bytes():
    return int(lib.pm_pointnet_packed_screen_bytes())


def pointnet_pack_screen(w3, b3, packed):
    _req(w3, b3, packed)
    check(lib.pm_pointnet_pack_weights_screen(_ptr(w3), _ptr(b3), _ptr(packed), _stream()), "pm_pointnet_pack_weights_screen")


def pointnet_enc_fwd_screen(x, P, Cc, sub_mean, w1, b1, b2, b3, packed, packed_screen, max_mean, feat, argmax, h2_save=None,
                            counters=None, schedule=None):
    """The screened tanh forward (csrc/pointnet_enc_screen.h).  counters: optional 3 x int64 device tensor the kernel adds
    [survivors, dense-fallback (wave, tile) pairs, (tile, channel) pairs with a survivor] to.  schedule: None = the library's
    default, 0 = lock-step, 1 = waves 4-7 staggered (same results bit for bit; anything else is refused)."""
    _req(x, w1, b1, b2, b3, packed, packed_screen, feat, argmax, h2_save, counters)
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() < 3 or not counters.is_contiguous()):
        raise ValueError("counters: expected a contiguous int64 tensor of 3 elements")
    B = x.shape[0]
    if schedule is not None:
        with TIMER.bracket("pointnet_enc_fwd"):
            check(lib.pm_pointnet_enc_fwd_screen_sched_f32(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1),
                                                           _ptr(b2), _ptr(b3), _ptr(packed), _ptr(packed_screen), int(max_mean),
                                                           _ptr(feat), _rows(feat, "feat"), _ptr(argmax), _ptr(h2_save),
                                                           _ptr(counters), int(schedule), _stream()),
                  "pm_pointnet_enc_fwd_screen_sched_f32")
        return
    with TIMER.bracket("pointnet_enc_fwd"):
        check(lib.pm_pointnet_enc_fwd_screen_f32(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2),
                                                 _ptr(b3), _ptr(packed), _ptr(packed_screen), int(max_mean), _ptr(feat),
                                                 _rows(feat, "feat"), _ptr(argmax), _ptr(h2_save), _ptr(counters), _stream()),
              "pm_pointnet_enc_fwd_screen_f32")


def pointnet_pack_bf3(w2, w3, packed):
    _req(w2, w3, packed)
    check(lib.pm_pointnet_pack_weights_bf3(_ptr(w2), _ptr(w3), _ptr(packed), _stream()), "pm_pointnet_pack_weights_bf3")


def pointnet_enc_fwd_bf3(x, P, Cc, sub_mean, w1, b1, b2, b3, packed, max_mean, feat, argmax, h2_save=None):
    _req(x, w1, b1, b2, b3, packed, feat, argmax)
    B = x.shape[0]
    with TIMER.bracket("pointnet_enc_fwd"):
        check(lib.pm_pointnet_enc_fwd_bf3(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2),
                                          _ptr(b3), _ptr(packed), int(max_mean), _ptr(feat), _rows(feat, "feat"),
                                          _ptr(argmax), _ptr(h2_save), _stream()), "pm_pointnet_enc_fwd_bf3")


def pointnet_pack_bf6(w2, w3, packed):
    _req(w2, w3, packed)
    check(lib.pm_pointnet_pack_weights_bf6(_ptr(w2), _ptr(w3), _ptr(packed), _stream()), "pm_pointnet_pack_weights_bf6")


def pointnet_enc_fwd_bf6(x, P, Cc, sub_mean, w1, b1, b2, b3, packed, max_mean, feat, argmax, h2_save=None):
    _req(x, w1, b1, b2, b3, packed, feat, argmax)
    B = x.shape[0]
    with TIMER.bracket("pointnet_enc_fwd"):
        check(lib.pm_pointnet_enc_fwd_bf6(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2),
                                          _ptr(b3), _ptr(packed), int(max_mean), _ptr(feat), _rows(feat, "feat"),
                                          _ptr(argmax), _ptr(h2_save), _stream()), "pm_pointnet_enc_fwd_bf6")


def pointnet_enc_bwd(x, P, Cc, sub_mean, w1, b1, b2, w3, packed, max_mean, dfeat, argmax, dw1, db1, dw2, db2, dw3, db3,
                     ws, h2_saved=None, act=None, four_wave=False):
    """four_wave: run the 4-wave kernel also when h2_saved is given (pm_pointnet_enc_bwd_w4_f32; the default entry sends a saved
    layer 2 to the 16-wave kernel)."""
    _req(x, w1, b1, b2, w3, packed, dfeat, argmax, dw1, db1, dw2, db2, dw3, db3, h2_saved)
    fn, name = (lib.pm_pointnet_enc_bwd_w4_f32, "pm_pointnet_enc_bwd_w4_f32") if four_wave else (lib.pm_pointnet_enc_bwd_f32, "pm_pointnet_enc_bwd_f32")
    B = x.shape[0]
    w = ws.get(lib.pm_pointnet_enc_bwd_workspace_bytes(B, P, Cc) + 256)
    base = w.data_ptr()
    al = (-base) % 256
    with TIMER.bracket("pointnet_enc_bwd"):
        check(fn(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2), _ptr(w3), _ptr(packed), int(max_mean),
                 _ptr(dfeat), _rows(dfeat, "dfeat"), _ptr(argmax), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(dw3), _ptr(db3),
                 _ptr(h2_saved), int(ACT_TANH if act is None else act), base + al, w.numel() - al, _stream()), name)


def pointnet_pack_bwd_bf6(w2, packed):
    _req(w2, packed)
    check(lib.pm_pointnet_pack_weights_bwd_bf6(_ptr(w2), _ptr(packed), _stream()), "pm_pointnet_pack_weights_bwd_bf6")


def pointnet_enc_bwd_bf6(x, P, Cc, sub_mean, w1, b1, b2, w3, packed, packed_w2, max_mean, dfeat, argmax, dw1, db1, dw2, db2, dw3,
                         db3, ws, h2_saved):
    """pointnet_enc_bwd with dW2 / dh1 on split-bf16 MFMAs (three planes, six products); tanh, saved layer 2."""
    _req(x, w1, b1, b2, w3, packed, packed_w2, dfeat, argmax, dw1, db1, dw2, db2, dw3, db3, h2_saved)
    B = x.shape[0]
    w = ws.get(lib.pm_pointnet_enc_bwd_workspace_bytes(B, P, Cc) + 256)
    base = w.data_ptr()
    al = (-base) % 256
    with TIMER.bracket("pointnet_enc_bwd"):
        check(lib.pm_pointnet_enc_bwd_bf6(_ptr(x), _rows(x, "x"), B, P, Cc, int(sub_mean), _ptr(w1), _ptr(b1), _ptr(b2),
                                          _ptr(w3), _ptr(packed), _ptr(packed_w2), int(max_mean), _ptr(dfeat),
                                          _rows(dfeat, "dfeat"), _ptr(argmax), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2),
                                          _ptr(dw3), _ptr(db3), _ptr(h2_saved), base + al, w.numel() - al, _stream()),
              "pm_pointnet_enc_bwd_bf6")


# ----------------------------------------------------------------------------- K8-K11
def ppo_actor_loss(mu, log_std, actions, old_logp, adv, old_mu, old_sigma, max_action, act_tanh, eps_clip, desired_kl,
                   adv_moments, adv_count, scal, dmu, dlog_std, ws):
    _req(mu, log_std, actions, old_logp, adv, old_mu, old_sigma, scal, dmu, dlog_std)
    B, A = mu.shape
    w = ws.get(lib.pm_ppo_actor_loss_workspace_bytes(B))
    check(lib.pm_ppo_actor_loss_fwd_bwd_f32(_ptr(mu), _rows(mu, "mu"), _ptr(log_std), _ptr(actions),
                                            _rows(actions, "actions"), _ptr(old_logp), _ptr(adv), _ptr(old_mu),
                                            _rows(old_mu, "old_mu"), _ptr(old_sigma), _rows(old_sigma, "old_sigma"),
                                            B, A, float(max_action), int(act_tanh), float(eps_clip), float(desired_kl),
                                            _ptr(adv_moments), float(adv_count), _ptr(scal), _ptr(dmu),
                                            _rows(dmu, "dmu"), _ptr(dlog_std), _ptr(w), w.numel(), _stream()),
          "pm_ppo_actor_loss_fwd_bwd_f32")


def ppo_actor_head_supported(h, w, dh):
    return bool(lib.pm_ppo_actor_head_supported(_ptr(h), _rows(h, "h"), _ptr(w), _rows(w, "w"), w.shape[0], w.shape[1], _ptr(dh),
                                                _rows(dh, "dh")))


def ppo_actor_head(h, w, b, hidden_act, log_std, actions, old_logp, adv, old_mu, old_sigma, max_action, act_tanh, eps_clip,
                   desired_kl, adv_moments, adv_count, scal, dmu, dh, dlog_std, ws, mu_out=None):
    """Policy head forward + PPO actor loss + dmu + head data gradient in one launch (pm_ppo_actor_head_f32); `ws` also keeps
    the launch's self-resetting work-group counter."""
    _req(h, w, b, log_std, actions, old_logp, adv, old_mu, old_sigma, scal, dmu, dh, dlog_std, mu_out)
    B, K = h.shape
    A = w.shape[0]
    buf = ws.get(lib.pm_ppo_actor_loss_workspace_bytes(B))
    ctr = getattr(ws, "counter", None)
    if ctr is None:
        ctr = ws.counter = torch.zeros(4, dtype=torch.int32, device=h.device)
    check(lib.pm_ppo_actor_head_f32(_ptr(h), _rows(h, "h"), _ptr(w), _rows(w, "w"), _ptr(b), K, int(hidden_act), _ptr(log_std),
                                    _ptr(actions), _rows(actions, "actions"), _ptr(old_logp), _ptr(adv), _ptr(old_mu),
                                    _rows(old_mu, "old_mu"), _ptr(old_sigma), _rows(old_sigma, "old_sigma"), B, A,
                                    float(max_action), int(act_tanh), float(eps_clip), float(desired_kl), _ptr(adv_moments),
                                    float(adv_count), _ptr(scal), _ptr(mu_out), _rows(mu_out, "mu_out") if mu_out is not None else 0,
                                    _ptr(dmu), _rows(dmu, "dmu"), _ptr(dh), _rows(dh, "dh"), _ptr(dlog_std), _ptr(buf), buf.numel(),
                                    _ptr(ctr), _stream()), "pm_ppo_actor_head_f32")


def gaussian_logp(mu, log_std, actions, max_action, act_tanh, logp, entropy):
    _req(mu, log_std, actions, logp, entropy)
    B, A = mu.shape
    check(lib.pm_gaussian_logp_f32(_ptr(mu), _rows(mu, "mu"), _ptr(log_std), _ptr(actions), _rows(actions, "actions"),
                                   B, A, float(max_action), int(act_tanh), _ptr(logp), _ptr(entropy), _stream()),
          "pm_gaussian_logp_f32")


def gaussian_logp_bwd(mu, log_std, actions, max_action, act_tanh, dlogp, dent, dmu, dlog_std):
    _req(mu, log_std, actions, dlogp, dent, dmu, dlog_std)
    B, A = mu.shape
    check(lib.pm_gaussian_logp_bwd_f32(_ptr(mu), _rows(mu, "mu"), _ptr(log_std), _ptr(actions), _rows(actions, "actions"), B, A,
                                       float(max_action), int(act_tanh), _ptr(dlogp), _ptr(dent), _ptr(dmu),
                                       _rows(dmu, "dmu") if dmu is not None else 0, _ptr(dlog_std), _stream()),
          "pm_gaussian_logp_bwd_f32")


def action_activation_bwd(out, dout, dmu, max_action, act_tanh):
    _req(out, dout, dmu)
    for t_, n_ in ((out, "out"), (dout, "dout"), (dmu, "dmu")):
        _f32c(t_, n_)
    check(lib.pm_action_activation_bwd_f32(_ptr(out), _ptr(dout), _ptr(dmu), out.numel(), float(max_action), int(act_tanh),
                                           _stream()), "pm_action_activation_bwd_f32")


def value_loss(v, returns, old_values, clipped, eps_clip, clip_mean_extern, grad_scale, scal, dv):
    _req(v, returns, old_values, clip_mean_extern, scal, dv)
    check(lib.pm_value_loss_fwd_bwd_f32(_ptr(v), _ptr(returns), _ptr(old_values), v.numel(), int(clipped),
                                        float(eps_clip), _ptr(clip_mean_extern), float(grad_scale), _ptr(scal), _ptr(dv),
                                        dv.stride(0) if dv.dim() == 2 else 1, _stream()), "pm_value_loss_fwd_bwd_f32")


def value_head_supported(h, w, dh):
    return w.shape[0] == 1 and w.is_contiguous() and bool(lib.pm_value_head_supported(_ptr(h), _rows(h, "h"), _ptr(w), w.shape[1], _ptr(dh),
                                                                                      _rows(dh, "dh")))


def value_head(h, w, b, hidden_act, returns, old_values, clipped, eps_clip, clip_mean_extern, grad_scale, scal, dv, dh, ws, v_out=None):
    """Value head forward + value loss + dV + head data gradient in one launch (pm_value_head_f32)."""
    _req(h, w, b, returns, old_values, clip_mean_extern, scal, dv, dh, v_out)
    B, K = h.shape
    buf = ws.get(lib.pm_value_head_workspace_bytes())
    ctr = getattr(ws, "counter", None)
    if ctr is None:
        ctr = ws.counter = torch.zeros(4, dtype=torch.int32, device=h.device)
    check(lib.pm_value_head_f32(_ptr(h), _rows(h, "h"), _ptr(w), _ptr(b), K, int(hidden_act), _ptr(returns), _ptr(old_values), B,
                                int(clipped), float(eps_clip), _ptr(clip_mean_extern), float(grad_scale), _ptr(scal), _ptr(v_out),
                                _ptr(dv), dv.stride(0) if dv.dim() == 2 else 1, _ptr(dh), _rows(dh, "dh"), _ptr(buf), buf.numel(),
                                _ptr(ctr), _stream()), "pm_value_head_f32")


def mse_tanh_loss(stu_mu, tea_mu, max_action, act_tanh, grad_scale, scal, dstu):
    _req(stu_mu, tea_mu, scal, dstu)
    B, A = stu_mu.shape
    check(lib.pm_mse_tanh_loss_fwd_bwd_f32(_ptr(stu_mu), _rows(stu_mu, "stu_mu"), _ptr(tea_mu), _rows(tea_mu, "tea_mu"),
                                           B, A, float(max_action), int(act_tanh), float(grad_scale), _ptr(scal),
                                           _ptr(dstu), _rows(dstu, "dstu"), _stream()), "pm_mse_tanh_loss_fwd_bwd_f32")


def action_activation(mu, out, max_action, act_tanh):
    _req(mu, out)
    _f32c(mu, "mu")
    _f32c(out, "out")
    check(lib.pm_action_activation_f32(_ptr(mu), _ptr(out), mu.numel(), float(max_action), int(act_tanh), _stream()),
          "pm_action_activation_f32")


def clip_adam_step(p, g, m, v, n_clip, max_norm, lr, b1, b2, eps, state, skip_flag, gnorm_out, ws):
    _req(p, g, m, v, state, skip_flag, gnorm_out)
    n = p.numel()
    w = ws.get(lib.pm_clip_adam_workspace_bytes(n))
    check(lib.pm_clip_adam_step_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, int(n_clip), float(max_norm), float(lr),
                                    float(b1), float(b2), float(eps), _ptr(state), _ptr(skip_flag), _ptr(gnorm_out),
                                    _ptr(w), w.numel(), _stream()), "pm_clip_adam_step_f32")


def ppo_accumulate_stats(acc, scal, which):
    _req(acc, scal)
    check(lib.pm_ppo_accumulate_stats_f32(_ptr(acc), _ptr(scal), int(which), _stream()), "pm_ppo_accumulate_stats_f32")


# ----------------------------------------------------------------------------- K12-K14
def fps(xyz, K, ws):
    """xyz (B,P,D) -> idx (B,K) int32 (pytorch3d sample_farthest_points defaults)."""
    _req(xyz)
    _f32c(xyz, "xyz")
    B, P, Dd = xyz.shape
    idx = torch.empty(B, K, dtype=torch.int32, device=xyz.device)
    nb = lib.pm_fps_workspace_bytes(B, P)
    w = ws.get(nb) if nb else None
    check(lib.pm_fps_f32(_ptr(xyz), B, P, Dd, K, _ptr(idx), _ptr(w), w.numel() if w is not None else 0, _stream()),
          "pm_fps_f32")
    return idx


def ball_query(xyz, centers, radius, nsample):
    _req(xyz, centers)
    _f32c(xyz, "xyz")
    _f32c(centers, "centers")
    B, P, _ = xyz.shape
    S = centers.shape[1]
    idx = torch.empty(B, S, nsample, dtype=torch.int32, device=xyz.device)
    check(lib.pm_ball_query_f32(_ptr(xyz), _ptr(centers), B, P, S, float(radius), nsample, _ptr(idx), _stream()),
          "pm_ball_query_f32")
    return idx


def group_points(feat, idx):
    _req(feat, idx)
    _f32c(feat, "feat")
    B, P, Cc = feat.shape
    S, ns = idx.shape[1], idx.shape[2]
    out = torch.empty(B, S, ns, Cc, dtype=torch.float32, device=feat.device)
    check(lib.pm_group_points_f32(_ptr(feat), _ptr(idx), B, P, Cc, S, ns, _ptr(out), _stream()), "pm_group_points_f32")
    return out


def group_points_bwd(dout, idx, P):
    _req(dout, idx)
    _f32c(dout, "dout")
    B, S, ns, Cc = dout.shape
    dfeat = torch.zeros(B, P, Cc, dtype=torch.float32, device=dout.device)
    check(lib.pm_group_points_bwd_f32(_ptr(dout), _ptr(idx), B, P, Cc, S, ns, _ptr(dfeat), _stream()),
          "pm_group_points_bwd_f32")
    return dfeat


# ----------------------------------------------------------------------------- K15 (PointNet++ glue)
def group_concat(xyz, feat, centers, idx, ldo):
    """-> (B*S*ns, ldo) rows [xyz[idx]-center | feat[idx] | 0-pad]."""
    _req(xyz, feat, centers, idx)
    B, P, _ = xyz.shape
    S, ns = idx.shape[1], idx.shape[2]
    Cf = 0 if feat is None else feat.shape[2]
    out = torch.empty(B * S * ns, ldo, dtype=torch.float32, device=xyz.device)
    check(lib.pm_group_concat_f32(_ptr(xyz), _ptr(feat), _ptr(centers), _ptr(idx), B, P, Cf, S, ns, ldo, _ptr(out),
                                  _stream()), "pm_group_concat_f32")
    return out


def group_concat_bwd(dout, idx, B, P, Cf, ldo):
    _req(dout, idx)
    S, ns = idx.shape[1], idx.shape[2]
    dfeat = torch.zeros(B, P, Cf, dtype=torch.float32, device=dout.device)
    check(lib.pm_group_concat_bwd_f32(_ptr(dout), _ptr(idx), B, P, Cf, S, ns, ldo, _ptr(dfeat), _stream()),
          "pm_group_concat_bwd_f32")
    return dfeat


def maxpool_rows(x, G, ns, out):
    """x (G*ns, C) -> out (G, C) view (any row stride), arg (G, C) int32."""
    _req(x, out)
    _f32c(x, "x")
    Cc = x.shape[1]
    arg = torch.empty(G, Cc, dtype=torch.int32, device=x.device)
    check(lib.pm_maxpool_rows_f32(_ptr(x), G, ns, Cc, _ptr(out), _rows(out, "out"), _ptr(arg), _stream()),
          "pm_maxpool_rows_f32")
    return arg


def maxpool_rows_bwd(dout, arg, ns, y_tanh=None):
    """dx (G*ns, C); `y_tanh` = the pooled (G*ns, C) tanh outputs -> the activation derivative is fused in."""
    _req(dout, arg, y_tanh)
    G, Cc = arg.shape
    dx = torch.empty(G * ns, Cc, dtype=torch.float32, device=dout.device)
    check(lib.pm_maxpool_rows_bwd_f32(_ptr(dout), _rows(dout, "dout"), _ptr(arg), G, ns, Cc, _ptr(y_tanh), _ptr(dx),
                                      _stream()), "pm_maxpool_rows_bwd_f32")
    return dx


# ----------------------------------------------------------------------------- SURVEY 8(b) names: one-call forms
def adv_normalize(x, ws, eps=1e-8):
    """In place x <- (x - mean) / (std_unbiased + eps) over all elements (storage.py:114, single process): pm_adv_normalize_f32."""
    _req(x)
    _f32c(x, "x")
    n = x.numel()
    w = ws.get(int(lib.pm_adv_normalize_workspace_bytes(n)) + 8)
    base = w.data_ptr()
    al = (-base) % 8
    check(lib.pm_adv_normalize_f32(_ptr(x), n, float(eps), base + al, w.numel() - al, _stream()), "pm_adv_normalize_f32")
    return x


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


def mlp_fwd(x, weights, biases, act):
    """network.py:27-54 `MLP` forward through pm_mlp_fwd_f32 -> list of the layer outputs (the last one is the network output)."""
    _req(x, *weights, *biases)
    M = x.shape[0]
    dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    hs = [torch.empty(M, d, dtype=torch.float32, device=x.device) for d in dims[1:]]
    check(lib.pm_mlp_fwd_f32(_ptr(x), _rows(x, "x"), M, len(weights), (C.c_int * len(dims))(*dims), _ptr_array(weights),
                             _ptr_array(biases), act, _ptr_array(hs), _stream()), "pm_mlp_fwd_f32")
    return hs


def mlp_bwd(x, weights, hs, act, dy, ws, need_dx=False):
    """-> (dW list, db list, dX or None) through pm_mlp_bwd_f32."""
    _req(x, dy, *weights, *hs)
    M = x.shape[0]
    dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    cd = (C.c_int * len(dims))(*dims)
    dws = [torch.empty_like(w) for w in weights]
    dbs = [torch.empty(w.shape[0], dtype=torch.float32, device=x.device) for w in weights]
    dx = torch.empty(M, dims[0], dtype=torch.float32, device=x.device) if need_dx else None
    w = ws.get(int(lib.pm_mlp_bwd_workspace_bytes(M, len(weights), cd)) + 16)
    base = w.data_ptr()
    al = (-base) % 16
    check(lib.pm_mlp_bwd_f32(_ptr(x), _rows(x, "x"), M, len(weights), cd, _ptr_array(weights), _ptr_array(hs), act, _ptr(dy),
                             _ptr_array(dws), _ptr_array(dbs), _ptr(dx), base + al, w.numel() - al, _stream()), "pm_mlp_bwd_f32")
    return dws, dbs, dx


# ----------------------------------------------------------------------------- K15 fused SA level
def sa_supported(C1, C2, C3, ns):
    return bool(lib.pm_sa_supported(C1, C2, C3, ns))


def sa_pack(w2, w3, packed):
    _req(w2, w3, packed)
    C2, C1 = w2.shape
    C3 = w3.shape[0]
    _f32c(w2, "w2")
    _f32c(w3, "w3")
    check(lib.pm_sa_pack_weights_f32(_ptr(w2), _ptr(w3), C1, C2, C3, _ptr(packed), _stream()),
          "pm_sa_pack_weights_f32")


def sa_fwd(xyz, centers, idx, Y, w1, b1, b2, b3, packed, dims, pooled, h2_save=None):
    """xyz (B,P,3), centers (B,S,3), idx (B,S,32) int32, Y (B*P,C1) or None -> pooled (B*S, C3) view, arg int32."""
    _req(xyz, centers, idx, Y, w1, packed, pooled)
    B, P, _ = xyz.shape
    S, ns = idx.shape[1], idx.shape[2]
    C1, C2, C3 = dims
    _f32c(xyz, "xyz")
    _f32c(centers, "centers")
    arg = torch.empty(B * S, C3, dtype=torch.int32, device=xyz.device)
    with TIMER.bracket(f"sa_fwd_{C1}x{C2}x{C3}"):
        check(lib.pm_sa_fwd_f32(_ptr(xyz), _ptr(centers), _ptr(idx), _ptr(Y), B, P, S, ns,
                                _ptr(w1), _rows(w1, "w1"), _ptr(b1), _ptr(b2), _ptr(b3), _ptr(packed), C1, C2, C3,
                                _ptr(pooled), _rows(pooled, "pooled"), _ptr(arg), _ptr(h2_save), _stream()), "pm_sa_fwd_f32")
    return arg


def sa_bwd(xyz, centers, idx, Y, w1, b1, b2, w3, packed, dims, pooled, arg, dpooled, dw1, db1, dw2, db2, dw3, db3, dY, ws,
           h2_saved=None):
    _req(xyz, centers, idx, Y, w1, w3, packed, pooled, arg, dpooled, dw1, dw2, dw3, dY)
    B, P, _ = xyz.shape
    S, ns = idx.shape[1], idx.shape[2]
    C1, C2, C3 = dims
    _f32c(w3, "w3")
    w = ws.get(lib.pm_sa_bwd_workspace_bytes(C1, C2, C3))
    with TIMER.bracket(f"sa_bwd_{C1}x{C2}x{C3}"):
        check(lib.pm_sa_bwd_f32(_ptr(xyz), _ptr(centers), _ptr(idx), _ptr(Y), B, P, S, ns, _ptr(w1), _rows(w1, "w1"),
                                _ptr(b1), _ptr(b2), _ptr(w3), _ptr(packed), C1, C2, C3, _ptr(pooled),
                                _rows(pooled, "pooled"), _ptr(arg), _ptr(dpooled), _rows(dpooled, "dpooled"), _ptr(dw1),
                                _rows(dw1, "dw1"), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(dw3), _ptr(db3), _ptr(dY),
                                _ptr(h2_saved), _ptr(w), w.numel(), _stream()), "pm_sa_bwd_f32")


# ---- group-all level: last layer + max over the cloud in one kernel, structured backward (csrc/sa_groupall.hip)
def sa_groupall_supported(ck, co, rows):
    return bool(lib.pm_sa_groupall_supported(int(ck), int(co), int(rows)))


def sa_groupall_pack(w, packed):
    _req(w, packed)
    _f32c(w, "w")
    check(lib.pm_sa_groupall_pack_f32(_ptr(w), w.shape[1], w.shape[0], _ptr(packed), _stream()), "pm_sa_groupall_pack_f32")


def sa_groupall_fwd(h, B, R, bias, packed, feat):
    """h (B*R, CK) -> feat (B, CO) view (any row stride) = max over the cloud's rows of tanh(h W^T + bias); arg (B, CO) int32."""
    _req(h, bias, packed, feat)
    _f32c(h, "h")
    ck, co = h.shape[1], feat.shape[1]
    arg = torch.empty(B, co, dtype=torch.int32, device=h.device)
    with TIMER.bracket("sa_groupall_fwd"):
        check(lib.pm_sa_groupall_fwd_f32(_ptr(h), B, R, ck, co, _ptr(bias), _ptr(packed), _ptr(feat), _rows(feat, "feat"), _ptr(arg),
                                         _stream()), "pm_sa_groupall_fwd_f32")
    return arg


def sa_groupall_bwd(dfeat, feat, arg, w, h, B, R, dh, dw, db, ws):
    """dh (B*R, CK) = d loss / d (pre-activation of h), every row written; dw (CO, CK), db (CO) overwritten."""
    _req(dfeat, feat, arg, w, h, dh, dw, db)
    _f32c(w, "w")
    _f32c(h, "h")
    _f32c(dh, "dh")
    _f32c(dw, "dw")
    co, ck = w.shape
    wsb = ws.get(int(lib.pm_sa_groupall_bwd_workspace_bytes(B, ck, co)) + 16)
    base = wsb.data_ptr()
    al = (-base) % 16
    with TIMER.bracket("sa_groupall_bwd"):
        check(lib.pm_sa_groupall_bwd_f32(_ptr(dfeat), _rows(dfeat, "dfeat"), _ptr(feat), _rows(feat, "feat"), _ptr(arg), _ptr(w), _ptr(h),
                                         B, R, ck, co, _ptr(dh), _ptr(dw), _ptr(db), base + al, wsb.numel() - al, _stream()),
              "pm_sa_groupall_bwd_f32")


# ---- duplicate-free ("packed") form: the level over each group's DISTINCT rows (ball query pads with copies of the first hit)
class SaPlan:
    """Packed-row tables of one neighbourhood table (pm_sa_plan_i32): nothing here is read by the host."""
    __slots__ = ("grow", "rowmap", "relxyz", "tiles", "totals", "B", "P", "S", "ns", "dims", "ready", "inv_start", "inv_rows")

    def counts(self):
        """(packed rows, tiles) -- a host read; diagnostics / buffer sizing only."""
        t = self.totals.cpu()
        return int(t[0]), int(t[1])

    def trim(self, counts=None):
        """Drop the worst-case capacity of the tables: for plans that are kept, e.g. per mini-batch slice.  counts: the (packed rows,
        tiles) a caller has already read (several plans, one host read); None: read here."""
        R, T = counts if counts is not None else self.counts()
        self.rowmap = self.rowmap[:max(R, 1)].clone()
        self.relxyz = self.relxyz[:max(R, 1)].clone()
        self.tiles = self.tiles[:max(T, 1)].clone()
        if self.inv_rows is not None:
            self.inv_rows = self.inv_rows[:max(R, 1)].clone()
        return self


def sa_packed_tile(dims):
    r, g = C.c_int(0), C.c_int(0)
    check(lib.pm_sa_packed_tile(dims[0], dims[1], dims[2], C.byref(r), C.byref(g)), "pm_sa_packed_tile")
    return r.value, g.value


def sa_plan(idx, xyz, centers, dims, ws, inverse=False):
    """idx (B, S, 32) int32 ball-query table of centres (B, S, 3) over xyz (B, P, 3) -> SaPlan for the fused level `dims`.
    inverse: also list every source point's packed rows in ascending order (pm_sa_plan_inverse_i32) -- what the deterministic
    gradient of a level with input features sums over (sa_dy_segsum)."""
    _req(idx, xyz, centers)
    _f32c(xyz, "xyz")
    _f32c(centers, "centers")
    B, S, ns = idx.shape
    P = xyz.shape[1]
    if idx.dtype != torch.int32 or not idx.is_contiguous():
        raise TypeError("sa_plan: idx must be a contiguous int32 tensor")
    tr, tg = sa_packed_tile(dims)
    G = B * S
    pl = SaPlan()
    pl.ready = None                       # set by a caller that shares the plan between streams (an event recorded after the build)
    pl.B, pl.P, pl.S, pl.ns, pl.dims = B, P, S, ns, tuple(dims)
    dev = idx.device
    pl.grow = torch.empty(G + 1, dtype=torch.int32, device=dev)
    pl.rowmap = torch.empty(G * ns, 2, dtype=torch.int32, device=dev)
    pl.relxyz = torch.empty(G * ns, 4, dtype=torch.float32, device=dev)
    pl.tiles = torch.empty(G, 4, dtype=torch.int32, device=dev)
    pl.totals = torch.zeros(4, dtype=torch.int32, device=dev)
    nb = int(lib.pm_sa_plan_workspace_bytes(B, S))
    w = ws.get(nb + 16)
    base = w.data_ptr()
    al = (-base) % 16
    with TIMER.bracket("sa_plan"):
        check(lib.pm_sa_plan_i32(_ptr(idx), _ptr(xyz), _ptr(centers), B, P, S, ns, tr, tg, _ptr(pl.grow), _ptr(pl.rowmap),
                                 _ptr(pl.relxyz), _ptr(pl.tiles), _ptr(pl.totals), base + al, w.numel() - al, _stream()), "pm_sa_plan_i32")
        pl.inv_start = pl.inv_rows = None
        if inverse:
            pl.inv_start = torch.empty(B * P + 1, dtype=torch.int32, device=dev)
            pl.inv_rows = torch.empty(G * ns, dtype=torch.int32, device=dev)
            check(lib.pm_sa_plan_inverse_i32(_ptr(pl.rowmap), _ptr(pl.grow), B, P, S, _ptr(pl.inv_start), _ptr(pl.inv_rows), _stream()),
                  "pm_sa_plan_inverse_i32")
    return pl


def sa_dy_segsum(plan, dz1, dY):
    """dY (B*P, C1) = per source point the sum of its packed rows of dz1 (R, C1) in ascending row order (no atomics, no zero-fill)."""
    _req(dz1, dY)
    _f32c(dz1, "dz1")
    if plan.inv_start is None:
        raise ValueError("sa_dy_segsum: the plan was built without its inverse (sa_plan(..., inverse=True))")
    if dY.shape[0] != plan.B * plan.P or dz1.shape[1] != dY.shape[1]:
        raise ValueError("sa_dy_segsum: shapes do not match the plan")
    with TIMER.bracket("sa_dy_segsum"):
        check(lib.pm_sa_dy_segsum_f32(_ptr(dz1), _ptr(plan.inv_start), _ptr(plan.inv_rows), plan.B * plan.P, dz1.shape[1], _ptr(dY),
                                      _rows(dY, "dY"), _stream()), "pm_sa_dy_segsum_f32")
    return dY


def gather_copy(dst, src, table):
    """dst[q] = src[table[q]] (0 where table[q] < 0): all weight-derived operand copies of a network in one launch."""
    _req(dst, src, table)
    _f32c(dst, "dst")
    _f32c(src, "src")
    _i32c(table, "table")
    if table.numel() != dst.numel():
        raise ValueError("gather_copy: one table entry per destination element")
    check(lib.pm_gather_copy_f32(_ptr(dst), _ptr(src), _ptr(table), dst.numel(), _stream()), "pm_gather_copy_f32")
    return dst


def sa_fwd_packed(plan, Y, w1, b1, b2, b3, packed, dims, pooled, h2_save=None, tail_xyz=None):
    """tail_xyz (B*S, 3): the columns of `pooled`'s rows behind the C3 features become (x, y, z, 0 ...) -- pooled is then a view of
    a group-all level's input rows and needs no tail copy."""
    _req(Y, w1, packed, pooled, tail_xyz)
    if tail_xyz is not None:
        _f32c(tail_xyz, "tail_xyz")
        if tuple(tail_xyz.shape) != (plan.B * plan.S, 3):
            raise ValueError("sa_fwd_packed: tail_xyz must be (B*S, 3)")
    B, P, S = plan.B, plan.P, plan.S
    C1, C2, C3 = dims
    if tuple(dims) != plan.dims or pooled.shape[0] != B * S or (Y is not None and Y.shape[0] != B * P):
        raise ValueError("sa_fwd_packed: the plan was built for another batch / level shape")
    arg = torch.empty(B * S, C3, dtype=torch.int32, device=pooled.device)
    with TIMER.bracket(f"sa_fwd_{C1}x{C2}x{C3}"):
        check(lib.pm_sa_fwd_packed_f32(_ptr(Y), B, P, S, _ptr(plan.grow), _ptr(plan.rowmap), _ptr(plan.relxyz),
                                       _ptr(plan.tiles), _ptr(plan.totals), _ptr(w1), _rows(w1, "w1"), _ptr(b1), _ptr(b2),
                                       _ptr(b3), _ptr(packed), C1, C2, C3, _ptr(pooled), _rows(pooled, "pooled"), _ptr(arg),
                                       _ptr(h2_save), _ptr(tail_xyz), (_rows(pooled, "pooled") - C3) if tail_xyz is not None else 0,
                                       _stream()), "pm_sa_fwd_packed_f32")
    return arg


def sa_dy_consume_supported(C1, cf):
    return bool(lib.pm_sa_dy_consume_supported(int(C1), int(cf)))


def sa_dy_consume_pack(w1, cf, packed):
    """w1 (C1, >= 3 + cf): its feature columns in MFMA operand order (after every update)."""
    _req(w1, packed)
    check(lib.pm_sa_dy_consume_pack_f32(_ptr(w1), _rows(w1, "w1"), w1.shape[0], cf, _ptr(packed), _stream()), "pm_sa_dy_consume_pack_f32")
    return packed


def sa_dy_consume(plan, dz1, feat, packed_w1f, dfeat, dw1, ws, dY=None):
    """dz1 (R, C1) per packed row -> dfeat (B*P, cf) = dY W1f, dw1[:, 3:3+cf] = dY^T feat (pad columns zeroed), with dY = the fixed-order
    per-source-point sums of dz1 formed in LDS (never written, unless the optional dY copy is asked for)."""
    _req(dz1, feat, packed_w1f, dfeat, dw1, dY)
    _f32c(dz1, "dz1")
    C1, cf = dz1.shape[1], feat.shape[1]
    npts = plan.B * plan.P
    if plan.inv_start is None or feat.shape[0] != npts or (dfeat is not None and tuple(dfeat.shape) != (npts, cf)) or dw1.shape[0] != C1:
        raise ValueError("sa_dy_consume: shapes do not match the plan (built with inverse=True?)")
    w = ws.get(lib.pm_sa_dy_consume_workspace_bytes(C1, cf))
    with TIMER.bracket("sa_dy_consume"):
        check(lib.pm_sa_dy_consume_f32(_ptr(dz1), _ptr(plan.inv_start), _ptr(plan.inv_rows), npts, C1, cf, _ptr(feat), _rows(feat, "feat"),
                                       _ptr(packed_w1f), _ptr(dfeat), _rows(dfeat, "dfeat") if dfeat is not None else 0, _ptr(dw1),
                                       _rows(dw1, "dw1"), dw1.shape[1], _ptr(dY), _rows(dY, "dY") if dY is not None else 0, _ptr(w),
                                       w.numel(), _stream()), "pm_sa_dy_consume_f32")
    return dfeat


def sa_bwd_packed(plan, Y, w1, b1, b2, w3, packed, dims, pooled, arg, dpooled, dw1, db1, dw2, db2, dw3, db3, dY, ws, h2_saved=None,
                  dz1=None, zero_pad_cols=False):
    """dz1 (R, C1): the layer-1 gradient per packed row (plain stores; sum it per source point with sa_dy_segsum) -- the
    deterministic path; dY (B*P, C1) zero-filled: the same sums by fp32 atomics (run-dependent last bits; kept for A/B).
    zero_pad_cols: a level without input features -- columns 3.. of dw1 are padding and are zeroed by the reduction launch."""
    _req(Y, w1, w3, packed, pooled, arg, dpooled, dw1, dw2, dw3, dY, dz1)
    if dz1 is not None:
        _f32c(dz1, "dz1")
        if dz1.shape[1] != dims[0]:
            raise ValueError("sa_bwd_packed: dz1 must be (R, C1)")
    B, P, S = plan.B, plan.P, plan.S
    C1, C2, C3 = dims
    if tuple(dims) != plan.dims or pooled.shape[0] != B * S:
        raise ValueError("sa_bwd_packed: the plan was built for another batch / level shape")
    _f32c(w3, "w3")
    w = ws.get(lib.pm_sa_bwd_workspace_bytes(C1, C2, C3))
    with TIMER.bracket(f"sa_bwd_{C1}x{C2}x{C3}"):
        check(lib.pm_sa_bwd_packed_f32(_ptr(Y), B, P, S, _ptr(plan.grow), _ptr(plan.rowmap), _ptr(plan.relxyz),
                                       _ptr(plan.tiles), _ptr(plan.totals), _ptr(w1), _rows(w1, "w1"), _ptr(b1), _ptr(b2),
                                       _ptr(w3), _ptr(packed), C1, C2, C3, _ptr(pooled), _rows(pooled, "pooled"), _ptr(arg),
                                       _ptr(dpooled), _rows(dpooled, "dpooled"), _ptr(dw1), _rows(dw1, "dw1"), _ptr(db1),
                                       _ptr(dw2), _ptr(db2), _ptr(dw3), _ptr(db3), _ptr(dY), _ptr(dz1), dw1.shape[1] if zero_pad_cols else 0,
                                       _ptr(h2_saved), _ptr(w), w.numel(), _stream()), "pm_sa_bwd_packed_f32")


# ----------------------------------------------------------------------------- sparse-voxel U-Net blocks
def voxel_grid0(x, P, C, R):
    """x (B, >= P*C) rows of P points (x, y, z, f...) -> (grid (B*R^3) i32, coords (B*P, 4) i32, feat (B*P, 4) f32)."""
    _req(x)
    B = x.shape[0]
    grid = torch.empty(B * R ** 3, dtype=torch.int32, device=x.device)
    coords = torch.empty(B * P, 4, dtype=torch.int32, device=x.device)
    feat = torch.empty(B * P, 4, dtype=torch.float32, device=x.device)
    check(lib.pm_voxel_grid0_f32(_ptr(x), _rows(x, "x"), B, P, C, R, _ptr(grid), _ptr(coords), _ptr(feat), _stream()),
          "pm_voxel_grid0_f32")
    return grid, coords, feat


def voxel_nbr27(coords, grid, R, taps=27):
    """(rows, 27) neighbour table; taps > 27: the rows are `taps` wide and the extra columns hold -1 (absent taps), returned
    as the (rows, taps) table -- its [:, :27] view is the plain table."""
    _req(coords, grid)
    rows = coords.shape[0]
    nbr = torch.empty(rows, taps, dtype=torch.int32, device=coords.device)
    check(lib.pm_voxel_nbr27_i32(_ptr(coords), rows, _ptr(grid), R, _ptr(nbr), int(taps), _stream()), "pm_voxel_nbr27_i32")
    return nbr


def voxel_mirror27(nbr):
    """The mirrored 27-neighbour table of the data gradient (pm_voxel_mirror27_i32)."""
    _req(nbr)
    out = torch.empty_like(nbr)
    check(lib.pm_voxel_mirror27_i32(_ptr(nbr), nbr.shape[0], _ptr(out), _stream()), "pm_voxel_mirror27_i32")
    return out


def voxel_down(coords_f, grid_f, Rf, B):
    """The 2x strided level of a fine level: dict(R, rows, grid, coords, child (rows, 8), parent / parent_canon / slot (rows_f)).
    One host read (the level's row count sizes its buffers and GEMMs)."""
    _req(coords_f, grid_f)
    dev = coords_f.device
    Rc = (Rf + 1) // 2
    rows_f = coords_f.shape[0]
    grid_c = torch.empty(B * Rc ** 3, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.pm_voxel_down_count_i32(_ptr(coords_f), rows_f, B, Rc, _ptr(grid_c), _ptr(counts), _stream()),
          "pm_voxel_down_count_i32")
    base = torch.empty(B + 1, dtype=torch.int32, device=dev)            # base[B] = the level's row count
    check(lib.pm_exclusive_scan_i32(_ptr(counts), B, _ptr(base), base.data_ptr() + 4 * B, _stream()), "pm_exclusive_scan_i32")
    rows_c = int(base[B].item())
    coords_c = torch.empty(rows_c, 4, dtype=torch.int32, device=dev)
    child = torch.empty(rows_c, 8, dtype=torch.int32, device=dev)
    parent = torch.empty(rows_f, dtype=torch.int32, device=dev)
    parent_canon = torch.empty(rows_f, dtype=torch.int32, device=dev)
    slot = torch.empty(rows_f, dtype=torch.int32, device=dev)
    check(lib.pm_voxel_down_build_i32(_ptr(coords_f), rows_f, _ptr(grid_f), Rf, B, Rc, _ptr(base), _ptr(grid_c), rows_c,
                                      _ptr(coords_c), _ptr(child), _ptr(parent), _ptr(parent_canon), _ptr(slot), _stream()),
          "pm_voxel_down_build_i32")
    return dict(R=Rc, rows=rows_c, grid=grid_c, coords=coords_c, child=child, parent=parent, parent_canon=parent_canon, slot=slot)


def rows_gather(src, idx, C, dst):
    """dst[r][j*C:(j+1)*C] = src[idx[r][j]][:C] (zeros where idx < 0); src / dst are 2-D views with unit inner stride."""
    _req(src, idx, dst)
    rows = idx.shape[0]
    J = idx.shape[1] if idx.dim() == 2 else 1
    check(lib.pm_rows_gather_f32(_ptr(src), _rows(src, "src"), _ptr(idx), rows, J, C, _ptr(dst), _rows(dst, "dst"), _stream()),
          "pm_rows_gather_f32")
    return dst


# How a gathered layer (a (rows, J) table over rows of C channels) feeds its GEMM: ONE decision, for the forward, the weight gradient
# and the tests.  FUSED: the GEMM's LDS-DMA loader gathers, the (rows x J*C) operand never reaches HBM (J*C is whole K-steps of 32).
# PADDED: the same on a table widened by absent taps (index -1 -> zero rows) against zero weight columns, where the missing columns
# are whole taps (27 taps x 4 channels = 108 columns -> 32 taps).  MATERIALISED: rows_gather writes the operand for the Linear kernels.
FUSED, PADDED, MATERIALISED = "fused", "padded", "materialised"


def sparse_operand_form(fused_gather, J, C):
    if not fused_gather or ((-J * C) % 32) % C != 0:
        return MATERIALISED
    return FUSED if (J * C) % 32 == 0 else PADDED


def sparse_dgrad_fused(fused_gather, cout):   # the data gradient of a 3^3 convolution is another GEMM shape: K = 27 * C_out
    return fused_gather and (27 * cout) % 32 == 0


def sparse_conv_fwd(src, idx, C, w, b, y, act, zero):
    """y = act(gather(src, idx) @ w.T + b) with the gather inside the GEMM loader (J*C % 32 == 0)."""
    _req(src, idx, w, b, y, zero)
    rows, J = idx.shape
    check(lib.pm_sparse_conv_fwd_f32(_ptr(src), _rows(src, "src"), _ptr(idx), rows, J, C, _ptr(w), _rows(w, "w"), _ptr(b), _ptr(y),
                                     _rows(y, "y"), w.shape[0], int(act), _ptr(zero), _stream()), "pm_sparse_conv_fwd_f32")
    return y


def sparse_conv_bwd_data(dy, idx_t, wt, h, dx, act, zero):
    """dx = (gather(dy, idx_t) @ wt.T) * act'(h): the data gradient of a submanifold convolution through the mirrored table
    `idx_t` and the transposed weight view `wt` (C_in, J*C_out), wt[ci, j*C_out + co] = w[co, j*C_in + ci] -- see pm_sparse_conv_bwd_data_f32."""
    _req(dy, idx_t, wt, h, dx, zero)
    rows, J = idx_t.shape
    Cout = dy.shape[1]
    check(lib.pm_sparse_conv_bwd_data_f32(_ptr(dy), _rows(dy, "dy"), _ptr(idx_t), rows, J, Cout, _ptr(wt), _rows(wt, "wt"), _ptr(h),
                                          _rows(h, "h") if h is not None else 0, _ptr(dx), _rows(dx, "dx"), wt.shape[0], int(act),
                                          _ptr(zero), _stream()), "pm_sparse_conv_bwd_data_f32")
    return dx


def sparse_conv_bwd_data_scatter(dy, w, idx, C, h, dx, act):
    """dx[idx[r, j]] = (dy[r] @ w[:, j*C:(j+1)*C]) * act'(h[idx[r, j]]) for convolutions with non-overlapping patches
    (pm_sparse_conv_bwd_data_scatter_f32); w = the forward's tap-major weight (Cout, J*C)."""
    _req(dy, w, idx, h, dx)
    _f32c(dx, "dx")
    rows, J = idx.shape
    check(lib.pm_sparse_conv_bwd_data_scatter_f32(_ptr(dy), _rows(dy, "dy"), _ptr(w), _rows(w, "w"), _ptr(idx), rows, J, C,
                                                  dy.shape[1], _ptr(h), _ptr(dx), int(act), _stream()),
          "pm_sparse_conv_bwd_data_scatter_f32")
    return dx


def sparse_conv_bwd_weight(dy, src, idx, C, dw, db, zero, ws):
    _req(dy, src, idx, dw, db, zero)
    rows, J = idx.shape
    N = dy.shape[1]
    w = ws.get(lib.pm_sparse_conv_bwd_weight_workspace_bytes(rows, N, J, C) + 256)
    base = w.data_ptr()
    al = (-base) % 256
    check(lib.pm_sparse_conv_bwd_weight_f32(_ptr(dy), _rows(dy, "dy"), _ptr(src), _rows(src, "src"), _ptr(idx), rows, J, C, _ptr(dw),
                                            _rows(dw, "dw"), _ptr(db), N, _ptr(zero), base + al, w.numel() - al, _stream()),
          "pm_sparse_conv_bwd_weight_f32")


# ----------------------------------------------------------------------------- 2-D residual network layers (csrc/bn_pool2d.hip)
def _cl_rows(t, name, C=None):
    """A channels-last activation: 2-D float32 (rows, C) with unit inner stride, C % 4 == 0, 16-byte rows.  Returns its row stride."""
    ld = _rows(t, name)
    if t.shape[1] % 4 or ld % 4 or t.data_ptr() % 16 or (C is not None and t.shape[1] != C):
        raise ValueError(f"{name}: expected (rows, {'C' if C is None else C}) with C % 4 == 0, a row stride that is a multiple of 4 and "
                         f"16-byte alignment, got {tuple(t.shape)} {t.stride()}")
    return ld


def _chan(t, name, C):
    if t.dtype != torch.float32 or t.shape != (C,) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 ({C},), got {t.dtype} {tuple(t.shape)}")


def bn2d_stats(x, eps, mean, invstd, ws, var=None, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1):
    """Batch statistics of x (rows, C) per channel into mean / invstd (/ var, biased); running_* and num_batches_tracked (int64, one
    element) are updated in place when given (pm_bn2d_stats_f32).  rows < 2 is refused, as torch's training batch norm refuses it."""
    _one_device("bn2d_stats", x, mean, invstd, var, running_mean, running_var, num_batches_tracked)
    ld = _cl_rows(x, "x")
    rows, C = x.shape
    for t, n in ((mean, "mean"), (invstd, "invstd"), (var, "var"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _chan(t, n, C)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise ValueError("num_batches_tracked: expected one int64")
    w = ws.get(lib.pm_bn2d_workspace_bytes(rows, C))
    check(lib.pm_bn2d_stats_f32(_ptr(x), ld, rows, C, float(eps), _ptr(mean), _ptr(var), _ptr(invstd), _ptr(running_mean),
                                _ptr(running_var), _ptr(num_batches_tracked), float(momentum), _ptr(w), w.numel(), _stream()),
          "pm_bn2d_stats_f32")


def bn2d_invstd(var, eps, invstd):
    """invstd = 1 / sqrt(var + eps) per channel: what bn2d_apply takes beside running_mean at inference."""
    _one_device("bn2d_invstd", var, invstd)
    C = var.numel()
    _chan(var, "var", C)
    _chan(invstd, "invstd", C)
    check(lib.pm_bn2d_invstd_f32(_ptr(var), C, float(eps), _ptr(invstd), _stream()), "pm_bn2d_invstd_f32")
    return invstd


def bn2d_apply(x, mean, invstd, gamma, beta, y, residual=None, relu=False):
    """y = gamma (x - mean) invstd + beta [+ residual] [relu] (pm_bn2d_apply_f32); y may be x."""
    _one_device("bn2d_apply", x, mean, invstd, gamma, beta, y, residual)
    rows, C = x.shape
    ldx, ldy = _cl_rows(x, "x"), _cl_rows(y, "y", C)
    ldr = _cl_rows(residual, "residual", C) if residual is not None else 0
    if y.shape[0] != rows or (residual is not None and residual.shape[0] != rows):
        raise ValueError("bn2d_apply: x, y and residual must have the same rows")
    for t, n in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (beta, "beta")):
        _chan(t, n, C)
    check(lib.pm_bn2d_apply_f32(_ptr(x), ldx, rows, C, _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(residual), ldr, int(relu),
                                _ptr(y), ldy, _stream()), "pm_bn2d_apply_f32")
    return y


def bn2d_bwd(dy, x, y, mean, invstd, gamma, dgamma, dbeta, dx, ws, relu=False, dy2=None, dy_masked=None):
    """Backward of bn2d_stats + bn2d_apply (pm_bn2d_bwd_f32): dgamma, dbeta, dx, and dy_masked = (dy [+ dy2]) [* (y > 0)] for the
    residual branch when wanted.  y (the layer's output) is read only with relu."""
    _one_device("bn2d_bwd", dy, x, y, mean, invstd, gamma, dgamma, dbeta, dx, dy2, dy_masked)
    rows, C = x.shape
    ldx, lddy, lddx = _cl_rows(x, "x"), _cl_rows(dy, "dy", C), _cl_rows(dx, "dx", C)
    if relu and y is None:
        raise ValueError("bn2d_bwd: relu=True needs the layer's output y")
    ldy = _cl_rows(y, "y", C) if relu else 0
    lddy2 = _cl_rows(dy2, "dy2", C) if dy2 is not None else 0
    lddym = _cl_rows(dy_masked, "dy_masked", C) if dy_masked is not None else 0
    for t in (dy, dx, y if relu else None, dy2, dy_masked):
        if t is not None and t.shape[0] != rows:
            raise ValueError("bn2d_bwd: all activations must have the same rows")
    for t, n in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _chan(t, n, C)
    w = ws.get(lib.pm_bn2d_workspace_bytes(rows, C))
    check(lib.pm_bn2d_bwd_f32(_ptr(dy), lddy, _ptr(dy2), lddy2, _ptr(x), ldx, _ptr(y) if relu else 0, ldy, int(relu), rows, C, _ptr(mean),
                              _ptr(invstd), _ptr(gamma), _ptr(dgamma), _ptr(dbeta), _ptr(dx), lddx, _ptr(dy_masked), lddym, _ptr(w),
                              w.numel(), _stream()), "pm_bn2d_bwd_f32")
    return dx


def pool2d_out(n):
    """Output extent of the 3 x 3 / stride 2 / padding 1 pool (and of a 3 x 3 or 1 x 1 stride-2 convolution with padding k // 2)."""
    return lib.pm_pool2d_out(int(n))


def pool2d_max_fwd(x, B, H, W, y, idx):
    """3 x 3 / 2 / 1 max pool of channels-last x (B*H*W, C) into y (B*Ho*Wo, C) and idx (same shape, int32: ih*W + iw of the winner)."""
    _one_device("pool2d_max_fwd", x, y, idx)
    C = x.shape[1]
    ldx, ldy = _cl_rows(x, "x"), _cl_rows(y, "y", C)
    n_out = B * pool2d_out(H) * pool2d_out(W)
    if x.shape[0] != B * H * W or y.shape[0] != n_out or idx.shape != (n_out, C) or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError(f"pool2d_max_fwd: x ({B * H * W}, C), y ({n_out}, C) and a contiguous int32 idx ({n_out}, C) expected, got "
                         f"{tuple(x.shape)}, {tuple(y.shape)}, {idx.dtype} {tuple(idx.shape)}")
    check(lib.pm_pool2d_max3s2_fwd_f32(_ptr(x), ldx, B, H, W, C, _ptr(y), ldy, _ptr(idx), _stream()), "pm_pool2d_max3s2_fwd_f32")
    return y, idx


def pool2d_max_bwd(dy, idx, B, H, W, dx, dy2=None):
    """dx (B*H*W, C) = the gather of dy [+ dy2] (B*Ho*Wo, C) through the winners idx of pool2d_max_fwd."""
    _one_device("pool2d_max_bwd", dy, idx, dx, dy2)
    C = dx.shape[1]
    lddx, lddy = _cl_rows(dx, "dx"), _cl_rows(dy, "dy", C)
    lddy2 = _cl_rows(dy2, "dy2", C) if dy2 is not None else 0
    n_out = B * pool2d_out(H) * pool2d_out(W)
    if dx.shape[0] != B * H * W or dy.shape[0] != n_out or idx.shape != (n_out, C) or idx.dtype != torch.int32 or not idx.is_contiguous() \
            or (dy2 is not None and dy2.shape[0] != n_out):
        raise ValueError(f"pool2d_max_bwd: dx ({B * H * W}, C), dy ({n_out}, C) and a contiguous int32 idx ({n_out}, C) expected")
    check(lib.pm_pool2d_max3s2_bwd_f32(_ptr(dy), lddy, _ptr(dy2), lddy2, _ptr(idx), B, H, W, C, _ptr(dx), lddx, _stream()),
          "pm_pool2d_max3s2_bwd_f32")
    return dx


def pool2d_avg_fwd(x, B, HW, y):
    """y[:, :C] (B rows, any stride) = the mean over the HW rows of each sample of x (B*HW, C)."""
    _one_device("pool2d_avg_fwd", x, y)
    C = x.shape[1]
    ldx = _cl_rows(x, "x")
    if x.shape[0] != B * HW or y.shape[0] != B or y.shape[1] < C:
        raise ValueError(f"pool2d_avg_fwd: x ({B * HW}, C) and y ({B}, >= C) expected, got {tuple(x.shape)}, {tuple(y.shape)}")
    check(lib.pm_pool2d_avg_fwd_f32(_ptr(x), ldx, B, HW, C, _ptr(y), _rows(y, "y"), _stream()), "pm_pool2d_avg_fwd_f32")
    return y


def pool2d_avg_bwd(dy, B, HW, dx):
    """dx (B*HW, C) rows of sample b = dy[b, :C] / HW."""
    _one_device("pool2d_avg_bwd", dy, dx)
    C = dx.shape[1]
    lddx = _cl_rows(dx, "dx")
    if dx.shape[0] != B * HW or dy.shape[0] != B or dy.shape[1] < C:
        raise ValueError(f"pool2d_avg_bwd: dx ({B * HW}, C) and dy ({B}, >= C) expected, got {tuple(dx.shape)}, {tuple(dy.shape)}")
    check(lib.pm_pool2d_avg_bwd_f32(_ptr(dy), _rows(dy, "dy"), B, HW, C, _ptr(dx), lddx, _stream()), "pm_pool2d_avg_bwd_f32")
    return dx


def im2col2d_c1(x, H, W, k, stride, pad, dst):
    """Patch matrix of single-channel images: x (B, >= H*W) rows (the leading H*W columns are the image) -> dst (B*Ho*Wo, ldd >= k*k),
    zero in the padding and in the columns past k*k."""
    _one_device("im2col2d_c1", x, dst)
    ldx = _rows(x, "x")
    _f32c(dst, "dst")
    B = x.shape[0]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if x.shape[1] < H * W or dst.dim() != 2 or dst.shape[0] != B * Ho * Wo or dst.shape[1] < k * k:
        raise ValueError(f"im2col2d_c1: x ({B}, >= {H * W}) and dst ({B * Ho * Wo}, >= {k * k}) expected, got {tuple(x.shape)}, {tuple(dst.shape)}")
    check(lib.pm_im2col2d_c1_f32(_ptr(x), ldx, B, H, W, k, stride, pad, _ptr(dst), dst.shape[1], _stream()), "pm_im2col2d_c1_f32")
    return dst


def im2col2d(x, C, H, W, k, stride, pad, dst):
    """Patch matrix of planar C-channel images: x (B, >= C*H*W) rows (the leading C*H*W columns are the C planes) -> dst (B*Ho*Wo,
    ldd >= C*k*k) with columns (c, kh, kw) -- conv.weight.view(Cout, C*k*k)'s order -- zero in the padding and in the columns past
    C*k*k."""
    _one_device("im2col2d", x, dst)
    ldx = _rows(x, "x")
    _f32c(dst, "dst")
    B = x.shape[0]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if C < 1 or x.shape[1] < C * H * W or dst.dim() != 2 or dst.shape[0] != B * Ho * Wo or dst.shape[1] < C * k * k:
        raise ValueError(f"im2col2d: x ({B}, >= {C * H * W}) and dst ({B * Ho * Wo}, >= {C * k * k}) expected, got {tuple(x.shape)}, "
                         f"{tuple(dst.shape)}")
    check(lib.pm_im2col2d_f32(_ptr(x), ldx, B, C, H, W, k, stride, pad, _ptr(dst), dst.shape[1], _stream()), "pm_im2col2d_f32")
    return dst


def rgb_planes(rgb, view, out):
    """View `view` of a colour frame, rgb uint8 (B, V, h, w, 3) contiguous, as float planes at the head of the rows of out (B, >= 3*h*w):
    out[b, c*h*w + y*w + x] = float(rgb[b, view, y, x, c]), raw 0..255; the columns past 3*h*w are not touched (pm_rgb_planes_f32)."""
    _one_device("rgb_planes", rgb, out)
    if rgb.dim() != 5 or rgb.shape[4] != 3 or rgb.dtype != torch.uint8 or not rgb.is_contiguous():
        raise ValueError(f"rgb_planes: rgb: expected a contiguous uint8 (B, V, h, w, 3), got {rgb.dtype} {tuple(rgb.shape)}")
    B, V, h, w = rgb.shape[:4]
    out, ldo = _out_rows(out, B, 3 * h * w, rgb.device)
    check(lib.pm_rgb_planes_f32(_ptr(rgb), B, V, h, w, int(view), _ptr(out), ldo, _stream()), "pm_rgb_planes_f32")
    return out


# `accumulate` of rows_gather_bwd (pm_rows_gather_bwd_f32): what dsrc holds when the call starts
ACC_OVERWRITE = 0         # nothing: dsrc is overwritten
ACC_ADD = 1               # a finished gradient: the (already multiplied) result is added to it
ACC_RAW_SKIP = 2          # a RAW contribution, added to the gathered sum BEFORE the activation derivative: (skip + strided) * act'


def rows_gather_bwd(dcols, tidx, C, dsrc, tslot=None, mode=0, reverse=False, self_col=-1, y_tanh=None, accumulate=ACC_OVERWRITE, rowmap=None,
                    skip=None):
    """accumulate: ACC_OVERWRITE, ACC_ADD or ACC_RAW_SKIP (above).
    rowmap (int32, one entry per row the table can name): dcols holds a subset of those rows -- rowmap[row] = its row in dcols or -1.
    skip = (values (N, C), skipmap (rows) int32): a sparse raw contribution added before the activation derivative (dsrc is overwritten)."""
    _req(dcols, tidx, dsrc, tslot, y_tanh, rowmap)
    rows = tidx.shape[0]
    J = tidx.shape[1] if tidx.dim() == 2 else 1
    if skip is not None:
        sv, sm = skip
        _req(sv, sm)
        if rowmap is not None or accumulate:
            raise ValueError("rows_gather_bwd: skip= takes neither rowmap nor accumulate")
        if sm.dtype != torch.int32 or sm.numel() < rows:
            raise TypeError("rows_gather_bwd: skipmap must be int32 with one entry per row")
        check(lib.pm_rows_gather_bwd_skip_f32(_ptr(dcols), _rows(dcols, "dcols"), _ptr(tidx), _ptr(tslot), int(mode), int(reverse),
                                              int(self_col), rows, J, C, _ptr(y_tanh), _rows(y_tanh, "y") if y_tanh is not None else 0,
                                              _ptr(dsrc), _rows(dsrc, "dsrc"), _ptr(sv), _rows(sv, "skip"), _ptr(sm), _stream()),
              "pm_rows_gather_bwd_skip_f32")
        return dsrc
    check(lib.pm_rows_gather_bwd_mapped_f32(_ptr(dcols), _rows(dcols, "dcols"), _ptr(tidx), _ptr(tslot), int(mode), int(reverse),
                                            int(self_col), rows, J, C, _ptr(y_tanh), _rows(y_tanh, "y") if y_tanh is not None else 0,
                                            int(accumulate), _ptr(dsrc), _rows(dsrc, "dsrc"), _ptr(rowmap), _stream()),
          "pm_rows_gather_bwd_mapped_f32")
    return dsrc


def col_blocks(dst, src, blocks, zero_other=True, col0=0, dst_cols=None):
    """dst[:, d : d + e - s] = src[:, s:e] for the (s, e, d) in `blocks` (at most two); the other columns of dst in [col0, dst_cols)
    are zeroed if zero_other (pm_col_blocks_f32).  dst / src: 2-D float32 views with unit inner stride; src=None with no block: zero-only.
    Blocks must land inside [col0, dst_cols) and must not overlap (the library refuses otherwise)."""
    _req(dst, src)
    if dst.dim() != 2 or dst.stride(1) != 1 or (src is not None and (src.dim() != 2 or src.stride(1) != 1 or dst.shape[0] != src.shape[0])):
        raise ValueError("col_blocks: 2-D views with unit inner stride and equal row counts")
    if src is None and blocks:
        raise ValueError("col_blocks: blocks need a source")
    b = list(blocks) + [(0, 0, 0)] * (2 - len(blocks))
    (s0, e0, d0), (s1, e1, d1) = b
    check(lib.pm_col_blocks_f32(_ptr(dst), dst.stride(0), _ptr(src), src.stride(0) if src is not None else 0, dst.shape[0],
                                dst.shape[1] if dst_cols is None else dst_cols,
                                int(col0), s0, e0, d0, s1, e1, d1, int(zero_other), _stream()), "pm_col_blocks_f32")
    return dst


def _i32c(t, name):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous int32 tensor")


def rows_uniq(src, S, pad_out, row_base=0, table=None, pad_in=-1):
    """src (B, >= S) int32 ids per cloud -> (u, um, rank), each (B, S) int32: the cloud's distinct ids ascending (through `table` if
    given; src == pad_in -> pad_out), padded with pad_out / -1, and every id's slot (pm_rows_uniq_i32; S <= 64)."""
    _req(src, table)
    if src.dtype != torch.int32 or src.stride(-1) != 1 or src.dim() != 2:
        raise TypeError("rows_uniq: src must be a 2-D int32 tensor with unit inner stride")
    if table is not None:
        _i32c(table, "table")
    B = src.shape[0]
    u, um, rank = (torch.empty(B, S, dtype=torch.int32, device=src.device) for _ in range(3))
    check(lib.pm_rows_uniq_i32(_ptr(src), src.stride(0), B, S, int(row_base), _ptr(table), int(pad_in), int(pad_out), _ptr(u), _ptr(um),
                               _ptr(rank), _stream()), "pm_rows_uniq_i32")
    return u, um, rank


def child_sum(x, rank, out):
    """out[b*S + j] = sum over i (ascending) with rank[b, i] == j of x[b*S + i]   (pm_child_sum_f32)."""
    _req(x, rank, out)
    _i32c(rank, "rank")
    B, S = rank.shape
    check(lib.pm_child_sum_f32(_ptr(x), _rows(x, "x"), _ptr(rank), B, S, x.shape[1], _ptr(out), _rows(out, "out"), _stream()),
          "pm_child_sum_f32")
    return out


def rowmap_scatter(n, ids, pad):
    """(n,) int32 map: -1 everywhere, map[ids[k]] = k for ids[k] != pad   (pm_rowmap_scatter_i32)."""
    _req(ids)
    _i32c(ids, "ids")
    m = torch.empty(n, dtype=torch.int32, device=ids.device)
    check(lib.pm_rowmap_scatter_i32(_ptr(m), n, _ptr(ids), ids.numel(), int(pad), _stream()), "pm_rowmap_scatter_i32")
    return m


def table_rows(table, sel):
    """Rows sel (N,) of an int32 index table (rows, J) (unit inner stride; -1 in sel -> a row of -1)   (pm_table_rows_i32)."""
    _req(table, sel)
    _i32c(sel, "sel")
    if table.dtype != torch.int32 or table.stride(1) != 1:
        raise TypeError("table_rows: table must be int32 with unit inner stride")
    out = torch.empty(sel.numel(), table.shape[1], dtype=torch.int32, device=table.device)
    check(lib.pm_table_rows_i32(_ptr(table), table.stride(0), table.shape[1], _ptr(sel), sel.numel(), _ptr(out), _stream()),
          "pm_table_rows_i32")
    return out


def voxel_vcat_table(parent, m, rows_hi):
    """(rows, m + 1) int32 gather table of a virtual [unpool | skip] operand   (pm_voxel_vcat_table_i32)."""
    _req(parent)
    _i32c(parent, "parent")
    rows = parent.numel()
    out = torch.empty(rows, m + 1, dtype=torch.int32, device=parent.device)
    check(lib.pm_voxel_vcat_table_i32(_ptr(parent), rows, int(m), int(rows_hi), _ptr(out), _stream()), "pm_voxel_vcat_table_i32")
    return out


# ----------------------------------------------------------------------------- depth -> cloud
def depth_backproject(depth, cam_pose, fx, fy, cx, cy, lo, hi):
    """depth (B,M,H,W), cam_pose (M,4,4) device -> world cloud (B, M*H*W, 3), out-of-box points zeroed."""
    import ctypes
    _req(depth, cam_pose)
    _f32c(depth, "depth")
    _f32c(cam_pose, "cam_pose")
    B, M, H, W = depth.shape
    out = torch.empty(B, M * H * W, 3, dtype=torch.float32, device=depth.device)
    lo3 = (ctypes.c_float * 3)(*[float(v) for v in lo])
    hi3 = (ctypes.c_float * 3)(*[float(v) for v in hi])
    check(lib.pm_depth_backproject_f32(_ptr(depth), B, M, H, W, _ptr(cam_pose), float(fx), float(fy), float(cx),
                                       float(cy), ctypes.cast(lo3, ctypes.c_void_p), ctypes.cast(hi3, ctypes.c_void_p),
                                       _ptr(out), _stream()), "pm_depth_backproject_f32")
    return out


def depth_cloud(depth, cam_pose, fx, fy, cx, cy, lo, hi, cap=None, want_src=True):
    """depth_compact(depth_backproject(...)) in one launch that never writes the (B, P, 3) world cloud (pm_depth_cloud_f32):
    depth (B, M, H, W), cam_pose (M, 4, 4) -> (xyz (B, cap, 3), src (B, cap) int32 or None, lengths (B) int32).  xyz[b, :lengths[b]]
    are the non-zero world points plus the first zero one, in pixel order, src their pixels r = view * H W + row * W + col; rows at
    and past lengths[b] are not written.  cap (default P = M H W): the rows kept per environment; fewer than an environment's count
    truncates its cloud to the first cap points.  want_src=False: no src buffer."""
    import ctypes
    for t_, name, nd in ((depth, "depth", 4), (cam_pose, "cam_pose", 3)):
        if not torch.is_tensor(t_) or t_.dim() != nd or 0 in t_.shape:
            raise ValueError(f"{name}: expected a non-empty {nd}-D tensor, got {tuple(t_.shape) if torch.is_tensor(t_) else type(t_)}")
        _f32c(t_, name)
    B, M, H, W = depth.shape
    if tuple(cam_pose.shape) != (M, 4, 4):
        raise ValueError(f"cam_pose: expected ({M}, 4, 4), got {tuple(cam_pose.shape)}")
    P = M * H * W
    if P > 2 ** 31 - 1:
        raise ValueError(f"depth: {P} pixels per environment, more than 2^31 - 1")
    cap = P if cap is None else int(cap)
    if cap < 1:
        raise ValueError(f"cap: expected a positive row count, got {cap}")
    box = [np.asarray(v, dtype=np.float32).reshape(-1) for v in (lo, hi)]
    if box[0].size != 3 or box[1].size != 3:
        raise ValueError("lo, hi: expected three numbers each")
    _one_device("depth_cloud", depth, cam_pose)
    xyz = torch.empty(B, cap, 3, dtype=torch.float32, device=depth.device)
    src = torch.empty(B, cap, dtype=torch.int32, device=depth.device) if want_src else None
    lengths = torch.empty(B, dtype=torch.int32, device=depth.device)
    lo3, hi3 = ((ctypes.c_float * 3)(*[float(v) for v in a]) for a in box)
    with TIMER.bracket("depth_cloud"):
        check(lib.pm_depth_cloud_f32(_ptr(depth), B, M, H, W, _ptr(cam_pose), float(fx), float(fy), float(cx), float(cy),
                                     ctypes.cast(lo3, ctypes.c_void_p), ctypes.cast(hi3, ctypes.c_void_p), cap, _ptr(xyz), _ptr(src),
                                     _ptr(lengths), _stream()), "pm_depth_cloud_f32")
    return xyz, src, lengths


def cloud_gather_labeled(xyz, src, idx, seg, zero_label=0.0, out=None):
    """Rows (x, y, z, label) of the sampled points of a depth_cloud (pm_cloud_gather_labeled_f32): xyz (B, ld, 3), src (B, ld) int32,
    idx (B, K) int32 into them, seg: int32 labels per pixel, (B, ...) contiguous or a 2-D view (B, P) with unit inner stride.  The
    label of point i is seg[b, src[b, i]], or zero_label for the point (0, 0, 0); an idx outside [0, ld) gives four NaN, a src
    outside [0, P) a NaN label.  out: None (a fresh (B, 4K)) or a 2-D float32 view (B, >= 4K) with unit inner stride -- columns past
    4K are left alone.  Returns out."""
    for t_, name in ((xyz, "xyz"), (src, "src"), (idx, "idx"), (seg, "seg")):
        if not torch.is_tensor(t_):
            raise ValueError(f"{name}: expected a tensor, got {type(t_)}")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or 0 in xyz.shape:
        raise ValueError(f"xyz: expected (B, ld > 0, 3), got {tuple(xyz.shape)}")
    _f32c(xyz, "xyz")
    B, ld, _ = xyz.shape
    if src.dtype != torch.int32 or not src.is_contiguous() or tuple(src.shape) != (B, ld):
        raise ValueError(f"src: expected a contiguous int32 tensor ({B}, {ld}), got {src.dtype} {tuple(src.shape)}")
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.dim() != 2 or idx.shape[0] != B or idx.shape[1] == 0:
        raise ValueError(f"idx: expected a contiguous int32 tensor ({B}, K > 0), got {idx.dtype} {tuple(idx.shape)}")
    K = idx.shape[1]
    if seg.dtype != torch.int32 or seg.dim() < 2 or seg.shape[0] != B or 0 in seg.shape:
        raise ValueError(f"seg: expected an int32 tensor ({B}, ...), got {seg.dtype} {tuple(seg.shape)}")
    if seg.dim() == 2 and (seg.shape[1] == 1 or seg.stride(1) == 1) and (B == 1 or seg.stride(0) >= seg.shape[1]):
        P, seg_stride = seg.shape[1], (seg.stride(0) if B > 1 else seg.shape[1])
    elif seg.is_contiguous():
        P = seg_stride = seg[0].numel()
    else:
        raise ValueError(f"seg: expected a contiguous tensor or a 2-D view with unit inner stride, got {tuple(seg.shape)} {seg.stride()}")
    if P > 2 ** 31 - 1:
        raise ValueError(f"seg: {P} pixels per environment, more than 2^31 - 1")
    if out is not None:
        _out_rows(out, B, 4 * K)
    _one_device("cloud_gather_labeled", xyz, src, idx, seg, out)
    out, ldo = _out_rows(out, B, 4 * K, xyz.device)
    with TIMER.bracket("cloud_gather_labeled"):
        check(lib.pm_cloud_gather_labeled_f32(_ptr(xyz), _ptr(src), B, ld, _ptr(idx), K, _ptr(seg), seg_stride, P, float(zero_label),
                                              _ptr(out), ldo, _stream()), "pm_cloud_gather_labeled_f32")
    return out


# ----------------------------------------------------------------------------- Conv3D students
def conv3d_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def im2col3d(x5, k, stride, pad, ldc):
    """x5: a 5-D VIEW (B, C, D, H, W) with arbitrary strides -> cols (B*Do*Ho*Wo, ldc)."""
    _req(x5)
    B, Cc, D, H, W = x5.shape
    Do, Ho, Wo = (conv3d_out(n, k, stride, pad) for n in (D, H, W))
    cols = torch.empty(B * Do * Ho * Wo, ldc, dtype=torch.float32, device=x5.device)
    check(lib.pm_im2col3d_f32(_ptr(x5), B, Cc, D, H, W, k, stride, pad, *x5.stride(), _ptr(cols), ldc, _stream()),
          "pm_im2col3d_f32")
    return cols


def conv3d_c1_supported(k, cout):
    return bool(lib.pm_conv3d_c1_supported(int(k), int(cout)))


def conv3d_c1_fwd(x5, k, stride, pad, wt, bias, act, rows=None):
    """Direct conv of a single-channel 5-D VIEW (B, 1, D, H, W) with wt (k^3, Cout) -> y (B*Do*Ho*Wo, Cout) = act(conv + b).
    rows (int64, optional): the batch is rows[b] of x5's first dimension (no gathered copy)."""
    _req(x5, wt, bias, rows)
    B, Cc, D, H, W = x5.shape
    if rows is not None:
        B = rows.numel()
    if Cc != 1:
        raise ValueError("conv3d_c1_fwd: one input channel")
    _f32c(wt, "wt")
    Do, Ho, Wo = (conv3d_out(n, k, stride, pad) for n in (D, H, W))
    cout = wt.shape[1]
    y = torch.empty(B * Do * Ho * Wo, cout, dtype=torch.float32, device=x5.device)
    sb, _, sd, sh, sw = x5.stride()
    with TIMER.bracket("conv3d_c1_fwd"):
        check(lib.pm_conv3d_c1_fwd_f32(_ptr(x5), B, D, H, W, k, stride, pad, sb, sd, sh, sw, _ptr(wt), _ptr(bias), cout, int(act),
                                       _ptr(y), cout, _ptr(rows), _stream()), "pm_conv3d_c1_fwd_f32")
    return y


def conv3d_c1_wgrad(dz, x5, k, stride, pad, dw, db, ws, rows=None):
    """dw (Cout, k^3) / db (Cout) of the direct input-layer conv from dz (rows, Cout); `rows` as in conv3d_c1_fwd."""
    _req(dz, x5, dw, db, rows)
    B, Cc, D, H, W = x5.shape
    if rows is not None:
        B = rows.numel()
    cout = dw.shape[0]
    w = ws.get(lib.pm_conv3d_c1_wgrad_workspace_bytes(cout))
    sb, _, sd, sh, sw = x5.stride()
    with TIMER.bracket("conv3d_c1_wgrad"):
        check(lib.pm_conv3d_c1_wgrad_f32(_ptr(dz), _rows(dz, "dz"), _ptr(x5), B, D, H, W, k, stride, pad, sb, sd, sh, sw, cout,
                                         _ptr(dw), _rows(dw, "dw"), _ptr(db), _ptr(rows), _ptr(w), w.numel(), _stream()),
              "pm_conv3d_c1_wgrad_f32")


def col2im3d(dcols, dx5, k, stride, pad, y_tanh5=None, act=None):
    """dcols (B*Do*Ho*Wo, ldc) -> every element of the 5-D view dx5 (B, C, D, H, W); y_tanh5 = the layer input
    (an activation output -- tanh unless `act` says otherwise -- of the same shape AND strides as dx5): its derivative is folded in."""
    _req(dcols, dx5, y_tanh5)
    B, Cc, D, H, W = dx5.shape
    if y_tanh5 is not None and (y_tanh5.shape != dx5.shape or y_tanh5.stride() != dx5.stride()):
        raise ValueError("col2im3d: y_tanh5 must be laid out like dx5")
    check(lib.pm_col2im3d_f32(_ptr(dcols), B, Cc, D, H, W, k, stride, pad, *dx5.stride(), _ptr(y_tanh5), ACT_TANH if act is None else int(act), _ptr(dx5),
                              _rows(dcols, "dcols"), _stream()), "pm_col2im3d_f32")


def tsdf_integrate(depth, pix_idx, pix_z, trunc, default_tsdf):
    """depth (B,M,H,W), pix_idx (M,V) int32, pix_z (M,V) -> (B,V)."""
    _req(depth, pix_idx, pix_z)
    _f32c(depth, "depth")
    _f32c(pix_z, "pix_z")
    B, M, H, W = depth.shape
    V = pix_idx.shape[1]
    out = torch.empty(B, V, dtype=torch.float32, device=depth.device)
    check(lib.pm_tsdf_integrate_f32(_ptr(depth), _ptr(pix_idx), _ptr(pix_z), B, M, H * W, V, float(trunc),
                                    float(default_tsdf), _ptr(out), _stream()), "pm_tsdf_integrate_f32")
    return out


def _mesh_tsdf_tables(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, base, grouped):
    """The table checks mesh_tsdf_query and mesh_tsdf_query_groups share.  The tables have one row per pose slot (M parts), or when
    `grouped` one per grid of a library (NG >= 1 grids, any M).  Returns (the tables' rows, B, M)."""
    _f32c(fields, "fields"), _f32c(part_bbox_min, "part_bbox_min"), _f32c(part_voxel_size, "part_voxel_size")
    _f32c(pose_R, "pose_R"), _f32c(pose_T, "pose_T")
    if base is not None:                                      # the point query has no base field
        _f32c(base, "base")
    n = part_off.numel()
    if part_off.dtype != torch.int64 or not part_off.is_contiguous() or (grouped and n == 0):
        raise ValueError("part_off: expected a contiguous int64 tensor" + (" of at least one row" if grouped else ""))
    _i32c(part_shape, "part_shape")
    B, M = check_poses(pose_R, pose_T, None if grouped else n)
    if tuple(part_shape.shape) != (n, 3) or tuple(part_bbox_min.shape) != (n, 3) or part_voxel_size.numel() != n:
        what, r = ("grid", "NG") if grouped else ("part", "M")
        raise ValueError(f"{what} tables: expected part_shape ({r},3), part_bbox_min ({r},3), part_voxel_size ({r})")
    return n, B, M


def _mesh_tsdf_volume(res, origin, base, B, out, device):
    """The volume arguments the two queries share, checked once their tables are: base (res^3) or (B, res^3), the `out=` rule and
    the origin's three floats.  Returns (per_env, out, its row stride, ox, oy, oz)."""
    n = int(res) ** 3
    if tuple(base.shape) == (n,):
        per_env = 0
    elif tuple(base.shape) == (B, n):
        per_env = 1
    else:
        raise ValueError(f"base: expected ({n},) or ({B}, {n}), got {tuple(base.shape)}")
    out, ldo = _out_rows(out, B, n, device)
    ox, oy, oz = (float(v) for v in origin)
    return per_env, out, ldo, ox, oy, oz


def mesh_tsdf_query(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, res, vox_size, origin,
                    sdf_trunc, base, p0=0, p1=None, out=None, brick_skip=True):
    """The mesh-TSDF observation of parts [p0, p1) (pm_mesh_tsdf_query_f32): fields (flat float32), part_off (M) int64,
    part_shape (M,3) int32, part_bbox_min (M,3), part_voxel_size (M), pose_R (B,M,3,3), pose_T (B,M,3), origin = 3 floats,
    base (res^3) or (B, res^3).  out: None (a fresh (B, res^3)) or a 2-D float32 view (B, >= res^3) with unit inner stride --
    columns past res^3 are left alone.  Returns out."""
    _one_device("mesh_tsdf_query", fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, base, out)
    _, B, M = _mesh_tsdf_tables(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, base, grouped=False)
    per_env, out, ldo, ox, oy, oz = _mesh_tsdf_volume(res, origin, base, B, out, pose_R.device)
    with TIMER.bracket("mesh_tsdf_query"):
        check(lib.pm_mesh_tsdf_query_f32(_ptr(fields), _ptr(part_off), _ptr(part_shape), _ptr(part_bbox_min), _ptr(part_voxel_size),
                                         _ptr(pose_R), _ptr(pose_T), B, M, int(p0), M if p1 is None else int(p1), int(res),
                                         float(vox_size), ox, oy, oz, float(sdf_trunc), _ptr(base), per_env, _ptr(out),
                                         ldo, 1 if brick_skip else 0, _stream()), "pm_mesh_tsdf_query_f32")
    return out


def mesh_tsdf_query_groups(fields, part_off, part_shape, part_bbox_min, part_voxel_size, grid_slot, NG_shared, group_off, env_group,
                           pose_R, pose_T, res, vox_size, origin, sdf_trunc, base, t0=0, t1=None, out=None, brick_skip=True,
                           max_group_grids=None):
    """mesh_tsdf_query over a scene whose environments differ (pm_mesh_tsdf_query_groups_f32): the part tables are a library of NG
    grids; environment b samples rows [0, NG_shared) and the rows of group env_group[b] (-1: none), group g being rows NG_shared +
    [group_off[g], group_off[g + 1]); row r is placed by pose slot grid_slot[r] of pose_R (B, M, 3, 3), pose_T (B, M, 3).  [t0, t1):
    the ordinals of an environment's own rows that are sampled (default: all, t1 = NG_shared + max_group_grids).  grid_slot: (NG) host
    integers (checked against [0, M) and copied) or an int32 device tensor (type and length only; the kernel leaves a row with a
    slot outside [0, M) unsampled).  group_off / env_group / max_group_grids as face_groups takes them; everything else, and the
    result, as mesh_tsdf_query."""
    NG, B, M = _mesh_tsdf_tables(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, base, grouped=True)
    if torch.is_tensor(grid_slot) and grid_slot.is_cuda:
        _i32c(grid_slot, "grid_slot")
        if tuple(grid_slot.shape) != (NG,):
            raise ValueError(f"grid_slot: expected ({NG},), got {tuple(grid_slot.shape)}")
    else:
        gs = np.asarray(grid_slot.numpy() if torch.is_tensor(grid_slot) else grid_slot)
        if gs.dtype.kind not in "iu" or gs.shape != (NG,) or gs.min() < 0 or gs.max() >= M:
            raise ValueError(f"grid_slot: expected {NG} integers in [0, {M}), got {gs.dtype} {gs.shape}")
        grid_slot = torch.from_numpy(np.ascontiguousarray(gs, dtype=np.int32)).to(pose_R.device)
    group_off, env_group, G, most = face_groups(group_off, env_group, NG, NG_shared, B, pose_R.device, max_group_grids,
                                                names=("NG", "NG_shared", "max_group_grids"))
    _one_device("mesh_tsdf_query_groups", fields, part_off, part_shape, part_bbox_min, part_voxel_size, grid_slot, group_off, env_group,
                pose_R, pose_T, base, out)
    t0, t1 = int(t0), int(NG_shared) + most if t1 is None else int(t1)
    if not 0 <= t0 < t1 <= int(NG_shared) + most:
        raise ValueError(f"t0, t1: expected 0 <= t0 < t1 <= NG_shared + max_group_grids = {int(NG_shared) + most}, got {t0}, {t1}")
    per_env, out, ldo, ox, oy, oz = _mesh_tsdf_volume(res, origin, base, B, out, pose_R.device)
    with TIMER.bracket("mesh_tsdf_query_groups"):
        check(lib.pm_mesh_tsdf_query_groups_f32(_ptr(fields), _ptr(part_off), _ptr(part_shape), _ptr(part_bbox_min),
                                                _ptr(part_voxel_size), _ptr(grid_slot), NG, int(NG_shared), _ptr(group_off), G,
                                                _ptr(env_group), most, _ptr(pose_R), _ptr(pose_T), B, M, t0, t1, int(res),
                                                float(vox_size), ox, oy, oz, float(sdf_trunc), _ptr(base), per_env, _ptr(out), ldo,
                                                1 if brick_skip else 0, _stream()), "pm_mesh_tsdf_query_groups_f32")
    return out


def _host_i32(a, name, n, lo, hi, device):
    """A host table (list, numpy, CPU tensor) of n integers in [lo, hi) -> int32 on `device`; a device tensor is checked for type and
    length only (reading it would synchronise; the kernel cuts whatever it holds)."""
    if torch.is_tensor(a) and a.is_cuda:
        _i32c(a, name)
        if tuple(a.shape) != (n,):
            raise ValueError(f"{name}: expected ({n},), got {tuple(a.shape)}")
        return a
    v = np.asarray(a.numpy() if torch.is_tensor(a) else a)
    if v.dtype.kind not in "iu" or v.shape != (n,) or (n and (v.min() < lo or v.max() >= hi)):
        raise ValueError(f"{name}: expected {n} integers in [{lo}, {hi}), got {v.dtype} {v.shape}")
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(device)


def _sdf_point_args(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier, p0, p1, pt_id,
                     chunk_sphere, seg_off, grid_slot, NG_shared, group_off, env_group, max_group_grids, point_output=True):
    """The argument checks mesh_sdf_points and articulation_sweep share (the tables, the points and their side tables, the ordinal
    range, the group tables).  Returns (grouped, NG, B, M, dev, NP, stride, carrier, pt_id, seg_off, NS, grid_slot, group_off,
    env_group, G, most, p0, p1) with the host tables copied to the device."""
    grouped = grid_slot is not None
    NG, B, M = _mesh_tsdf_tables(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, None, grouped=grouped)
    dev = pose_R.device
    if not torch.is_tensor(pts) or pts.dtype != torch.float32 or not pts.is_contiguous() or pts.dim() not in (2, 3) or \
            pts.shape[-1] != 3 or pts.shape[-2] == 0 or (pts.dim() == 3 and pts.shape[0] != B):
        raise ValueError(f"pts: expected a contiguous float32 (NP > 0, 3) or ({B}, NP, 3), got "
                         f"{tuple(pts.shape) if torch.is_tensor(pts) else type(pts).__name__}")
    NP = int(pts.shape[-2])
    if NP > 2 ** 30:
        raise ValueError(f"pts: at most 2^30 points, got {NP}")
    stride = 3 * NP if pts.dim() == 3 else 0
    carrier = torch.full((NP,), -1, dtype=torch.int32, device=dev) if carrier is None else _host_i32(carrier, "carrier", NP, -1, M, dev)
    if pt_id is not None:
        pt_id = _host_i32(pt_id, "pt_id", NP, -2 ** 31, 2 ** 31, dev)
    NS = 0
    if seg_off is not None:
        if torch.is_tensor(seg_off) and seg_off.is_cuda:
            _i32c(seg_off, "seg_off")
            if seg_off.dim() != 1 or seg_off.numel() < 2:
                raise ValueError(f"seg_off: expected (NS + 1 >= 2,), got {tuple(seg_off.shape)}")
        else:
            so = np.asarray(seg_off.numpy() if torch.is_tensor(seg_off) else seg_off)
            if so.dtype.kind not in "iu" or so.ndim != 1 or so.size < 2 or so[0] != 0 or so[-1] != NP or (np.diff(so) < 0).any():
                raise ValueError(f"seg_off: expected NS + 1 >= 2 non-decreasing integers from 0 to NP = {NP}, got {so.tolist() if so.ndim == 1 else so.shape}")
            seg_off = torch.from_numpy(np.ascontiguousarray(so, dtype=np.int32)).to(dev)
        NS = seg_off.numel() - 1
    if chunk_sphere is not None:
        _f32c(chunk_sphere, "chunk_sphere")
        if tuple(chunk_sphere.shape) != ((NP + 63) // 64, 4):
            raise ValueError(f"chunk_sphere: expected ({(NP + 63) // 64}, 4), got {tuple(chunk_sphere.shape)}")
    if not point_output and NS == 0:
        raise ValueError("want_dist=False: needs seg_off (nothing would be computed)")
    if grouped:
        grid_slot = _host_i32(grid_slot, "grid_slot", NG, 0, M, dev)
        group_off, env_group, G, most = face_groups(group_off, env_group, NG, NG_shared, B, dev, max_group_grids,
                                                    names=("NG", "NG_shared", "max_group_grids"))
        top = int(NG_shared) + most
    else:
        if any(a is not None for a in (NG_shared, group_off, env_group, max_group_grids)):
            raise ValueError("NG_shared / group_off / env_group / max_group_grids: need grid_slot=")
        top, G, most = M, 0, 0
    p0, p1 = int(p0), top if p1 is None else int(p1)
    if not 0 <= p0 < p1 <= top:
        raise ValueError(f"p0, p1: expected 0 <= p0 < p1 <= {top}, got {p0}, {p1}")
    return grouped, NG, B, M, dev, NP, stride, carrier, pt_id, seg_off, NS, grid_slot, group_off, env_group, G, most, p0, p1


def mesh_sdf_points(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier=None, p0=0, p1=None,
                    pt_id=None, chunk_sphere=None, seg_off=None, want_dist=True, want_arg=False, dist=None, cull=True, grid_slot=None,
                    NG_shared=None, group_off=None, env_group=None, max_group_grids=None):
    """Signed distance, in metres, of posed points to the part grids (pm_mesh_sdf_points_f32; with grid_slot= the grouped entry
    pm_mesh_sdf_points_groups_f32, whose tables are those of mesh_tsdf_query_groups).  Part tables and poses as mesh_tsdf_query.
    pts (NP, 3) shared by all environments or (B, NP, 3); carrier: None (world points) or NP integers in [-1, M), the pose slot that
    carries each point (-1: world); [p0, p1): the ordinals sampled.  pt_id: None or NP integers, the id a point is reported under in
    seg_arg (negative: a padding point, in no segment result); chunk_sphere: None or (ceil(NP / 64), 4) float32, what the cull
    reads (include/partmanip_hip.h); seg_off: None or NS + 1 non-decreasing integers from 0 to NP.  carrier / pt_id / seg_off on the
    host are validated and copied; on the device they are checked for type and length only.  dist: None or a float32 view (B, >= NP)
    with unit inner stride to write into.  Returns (dist (B, NP) or None, arg (B, NP) int32 or None, seg_min (B, NS) or None, seg_arg
    (B, NS) int32 or None): dist unless want_dist is False, arg with want_arg, the segment pair with seg_off."""
    (grouped, NG, B, M, dev, NP, stride, carrier, pt_id, seg_off, NS, grid_slot, group_off, env_group, G, most, p0, p1) = _sdf_point_args(
        fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier, p0, p1, pt_id, chunk_sphere, seg_off,
        grid_slot, NG_shared, group_off, env_group, max_group_grids, point_output=want_dist or dist is not None or want_arg)
    ld = NP
    if dist is not None:
        _out_rows(dist, B, NP, name="dist")
    _one_device("mesh_sdf_points", fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier, pt_id,
                chunk_sphere, seg_off, dist, grid_slot, group_off, env_group)
    arg = seg_min = seg_arg = None
    if want_dist or dist is not None:
        dist, ld = _out_rows(dist, B, NP, dev, name="dist")
    if want_arg:
        arg = torch.empty(B, ld, dtype=torch.int32, device=dev)
    if NS:
        seg_min = torch.empty(B, NS, dtype=torch.float32, device=dev)
        seg_arg = torch.empty(B, NS, dtype=torch.int32, device=dev)
    head = (_ptr(fields), _ptr(part_off), _ptr(part_shape), _ptr(part_bbox_min), _ptr(part_voxel_size))
    tail = (_ptr(pts), stride, _ptr(carrier), _ptr(pt_id), _ptr(chunk_sphere), NP, _ptr(seg_off), NS, _ptr(dist), ld, _ptr(arg),
            _ptr(seg_min), _ptr(seg_arg), 1 if cull else 0, _stream())
    with TIMER.bracket("mesh_sdf_points"):
        if grouped:
            check(lib.pm_mesh_sdf_points_groups_f32(*head, _ptr(grid_slot), NG, int(NG_shared), _ptr(group_off), G, _ptr(env_group), most,
                                                    _ptr(pose_R), _ptr(pose_T), B, M, p0, p1, *tail), "pm_mesh_sdf_points_groups_f32")
        else:
            check(lib.pm_mesh_sdf_points_f32(*head, _ptr(pose_R), _ptr(pose_T), B, M, p0, p1, *tail), "pm_mesh_sdf_points_f32")
    return dist, None if arg is None else arg[:, :NP], seg_min, seg_arg


def mesh_pc_query(pts, part_of, pose_R, pose_T, sel=None, out=None, labels=None):
    """The posed mesh point cloud (pm_mesh_pc_query_f32): pts (Q, 3) canonical surface points, part_of (Q) int32, pose_R (B, M, 3, 3),
    pose_T (B, M, 3); sel: None (every point, K = Q), (K) int32 shared by all environments or (B, K) int32 with unit inner stride.
    out: None (a fresh (B, 3K)) or a 2-D float32 view (B, >= 3K) with unit inner stride -- columns past 3K are left alone.
    Returns out; out[b, 3k + j] = coordinate j of point pts[sel[.., k]] under the pose of its part in environment b.
    labels: None, or (M) float32, one number per pose slot: the rows are then 4K wide (pm_mesh_pc_query_labeled_f32), out[b, 4k + j]
    the coordinates as above and out[b, 4k + 3] = labels[part_of[sel[.., k]]]."""
    _one_device("mesh_pc_query", pts, part_of, pose_R, pose_T, sel, out, labels)
    for t_, name in ((pts, "pts"), (pose_R, "pose_R"), (pose_T, "pose_T")):
        _f32c(t_, name)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError(f"pts: expected (Q > 0, 3), got {tuple(pts.shape)}")
    Q = pts.shape[0]
    if part_of.dtype != torch.int32 or not part_of.is_contiguous() or tuple(part_of.shape) != (Q,):
        raise ValueError(f"part_of: expected a contiguous int32 tensor ({Q},), got {part_of.dtype} {tuple(part_of.shape)}")
    B, M = check_poses(pose_R, pose_T)
    if sel is None:
        K, sel_stride = Q, 0
    else:
        if sel.dtype != torch.int32 or sel.dim() not in (1, 2) or sel.shape[-1] == 0 or sel.stride(-1) != 1:
            raise ValueError(f"sel: expected an int32 tensor (K,) or (B, K) with unit inner stride, got {sel.dtype} {tuple(sel.shape)}")
        K = sel.shape[-1]
        if sel.dim() == 1:
            sel_stride = 0
        else:
            sel_stride = sel.stride(0) if B > 1 else K
            if sel.shape[0] != B or sel_stride < K:
                raise ValueError(f"sel: expected ({B}, K) with row stride >= K, got {tuple(sel.shape)} {sel.stride()}")
    if labels is not None:
        _f32c(labels, "labels")
        if tuple(labels.shape) != (M,):
            raise ValueError(f"labels: expected ({M},), one number per pose slot, got {tuple(labels.shape)}")
        out, ldo = _out_rows(out, B, 4 * K, pose_R.device)
        with TIMER.bracket("mesh_pc_query_labeled"):
            check(lib.pm_mesh_pc_query_labeled_f32(_ptr(pts), _ptr(part_of), Q, _ptr(pose_R), _ptr(pose_T), B, M, _ptr(sel), sel_stride,
                                                   K, _ptr(out), ldo, _ptr(labels), _stream()), "pm_mesh_pc_query_labeled_f32")
        return out
    out, ldo = _out_rows(out, B, 3 * K, pose_R.device)
    with TIMER.bracket("mesh_pc_query"):
        check(lib.pm_mesh_pc_query_f32(_ptr(pts), _ptr(part_of), Q, _ptr(pose_R), _ptr(pose_T), B, M, _ptr(sel), sel_stride, K,
                                       _ptr(out), ldo, _stream()), "pm_mesh_pc_query_f32")
    return out


def _mesh_camera_args(verts, vert_part, faces, pose_R, pose_T, cam_pose, im_h, im_w, near, far):
    """The geometry, pose and camera checks the depth and the frame camera share.  Returns (NV, B, M, V, im_h, im_w)."""
    for t_, name in ((verts, "verts"), (pose_R, "pose_R"), (pose_T, "pose_T"), (cam_pose, "cam_pose")):
        _f32c(t_, name)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise ValueError(f"verts: expected (NV > 0, 3), got {tuple(verts.shape)}")
    NV = verts.shape[0]
    if vert_part.dtype != torch.int32 or not vert_part.is_contiguous() or tuple(vert_part.shape) != (NV,):
        raise ValueError(f"vert_part: expected a contiguous int32 tensor ({NV},), got {vert_part.dtype} {tuple(vert_part.shape)}")
    if faces.dtype != torch.int32 or not faces.is_contiguous() or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError(f"faces: expected a contiguous int32 tensor (F > 0, 3), got {faces.dtype} {tuple(faces.shape)}")
    B, M = check_poses(pose_R, pose_T)
    if cam_pose.dim() != 3 or tuple(cam_pose.shape[1:]) != (4, 4) or cam_pose.shape[0] == 0:
        raise ValueError(f"cam_pose: expected (V > 0, 4, 4), got {tuple(cam_pose.shape)}")
    V, im_h, im_w = cam_pose.shape[0], int(im_h), int(im_w)
    if im_h < 1 or im_w < 1:
        raise ValueError(f"image size: expected positive im_h and im_w, got {im_h} x {im_w}")
    if not (near > 0 and far > near):
        raise ValueError(f"clip planes: expected 0 < near < far, got near = {near}, far = {far}")
    return NV, B, M, V, im_h, im_w


def mesh_depth_render(verts, vert_part, faces, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h, im_w, near=0.01, far=100.0, out=None,
                      groups=None):
    """Depth images of the posed part meshes (pm_mesh_depth_render_f32): verts (NV, 3) canonical vertices of all parts, vert_part (NV)
    int32, faces (F, 3) int32 into verts, pose_R (B, M, 3, 3), pose_T (B, M, 3), cam_pose (V, 4, 4) camera->world (camera looks along
    +z, x right, y down).  out: None (a fresh (B, V h w)) or a 2-D float32 view (B, >= V h w) with unit inner stride -- columns past
    V h w are left alone.  Returns out; out[b, (v h + r) w + c] = z-depth of the nearest surface through pixel (r, c) of view v, `far`
    where nothing is hit; the fp32 arithmetic is fixed (include/partmanip_hip.h), so the bits repeat.
    groups: None, or mesh_depth_render_groups' (F_shared, group_off, env_group, max_group_faces)."""
    if groups is None:                                       # each entry keeps its own order of refusals: devices first here, tables first below
        _one_device("mesh_depth_render", verts, vert_part, faces, pose_R, pose_T, cam_pose, out)
    NV, B, M, V, im_h, im_w = _mesh_camera_args(verts, vert_part, faces, pose_R, pose_T, cam_pose, im_h, im_w, near, far)
    if groups is not None:
        F_shared, group_off, env_group, most = groups
        group_off, env_group, G, most = face_groups(group_off, env_group, faces.shape[0], F_shared, B, pose_R.device, most)
        _one_device("mesh_depth_render_groups", verts, vert_part, faces, group_off, env_group, pose_R, pose_T, cam_pose, out)
    out, ldo = _out_rows(out, B, V * im_h * im_w, pose_R.device)
    # the arguments after F, which both entries share; the grouped entry takes five more before them
    rest = (_ptr(pose_R), _ptr(pose_T), B, M, _ptr(cam_pose), V, float(fx), float(fy), float(cx), float(cy), im_h, im_w, float(near),
            float(far), _ptr(out), ldo, _stream())
    if groups is None:
        with TIMER.bracket("mesh_depth_render"):
            check(lib.pm_mesh_depth_render_f32(_ptr(verts), _ptr(vert_part), NV, _ptr(faces), faces.shape[0], *rest),
                  "pm_mesh_depth_render_f32")
        return out
    with TIMER.bracket("mesh_depth_render_groups"):
        check(lib.pm_mesh_depth_render_groups_f32(_ptr(verts), _ptr(vert_part), NV, _ptr(faces), faces.shape[0], int(F_shared),
                                                  _ptr(group_off), G, _ptr(env_group), most, *rest), "pm_mesh_depth_render_groups_f32")
    return out


def face_groups(group_off, env_group, F, F_shared, B, device, max_group_faces=None, names=("F", "F_shared", "max_group_faces")):
    """The group arguments of mesh_depth_render_groups / mesh_frame_render_groups -> (group_off (G + 1) int32 on `device`, env_group
    (B) int32 on `device`, G, max_group_faces).  Host arrays (numpy, lists, CPU tensors) are validated here -- group_off starts at 0,
    never decreases and ends at F - F_shared; env_group holds B values in [-1, G) -- and copied to the device, and max_group_faces
    is computed from them.  Device tensors are only checked for type and length (reading them would synchronise; the kernel clamps
    whatever they hold) and need max_group_faces from the caller.  names: what the messages call F, F_shared and max_group_faces
    (mesh_tsdf_query_groups partitions the rows of a grid library the same way)."""
    nF, nS, nM = names
    F, F_shared, B = int(F), int(F_shared), int(B)
    if not 0 <= F_shared <= F:
        raise ValueError(f"{nS}: expected a value in [0, {F}], got {F_shared}")
    on_device = [torch.is_tensor(a) and a.is_cuda for a in (group_off, env_group)]
    if on_device[0] != on_device[1]:
        raise ValueError("group_off and env_group: expected both on the host or both on the device")
    if on_device[0]:
        if max_group_faces is None:
            raise ValueError(f"{nM}: needed with device tables (the host arrays give it for free)")
        _i32c(group_off, "group_off"), _i32c(env_group, "env_group")
        if group_off.dim() != 1 or group_off.numel() < 1 or tuple(env_group.shape) != (B,):
            raise ValueError(f"group_off / env_group: expected (G + 1,) and ({B},), got {tuple(group_off.shape)} and {tuple(env_group.shape)}")
        if int(max_group_faces) < 0:
            raise ValueError(f"{nM}: expected a non-negative count, got {max_group_faces}")
        return group_off, env_group, group_off.numel() - 1, int(max_group_faces)
    off, eg = (np.asarray(a.numpy() if torch.is_tensor(a) else a) for a in (group_off, env_group))
    if off.dtype.kind not in "iu" or eg.dtype.kind not in "iu" or off.ndim != 1 or off.size < 1 or eg.shape != (B,):
        raise ValueError(f"group_off / env_group: expected integers (G + 1,) and ({B},), got {off.dtype} {off.shape} and {eg.dtype} {eg.shape}")
    off, eg = off.astype(np.int64), eg.astype(np.int64)
    G = off.size - 1
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != F - F_shared:
        raise ValueError(f"group_off: expected a non-decreasing table from 0 to {nF} - {nS} = {F - F_shared}, got {off.tolist()}")
    if eg.min() < -1 or eg.max() >= G:
        raise ValueError(f"env_group: values must lie in [-1, {G}), got [{eg.min()}, {eg.max()}]")
    most = int(np.diff(off).max()) if G else 0
    if max_group_faces is not None and int(max_group_faces) < most:
        raise ValueError(f"{nM}: {max_group_faces} is below the largest group's {most} rows")
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)       # noqa: E731
    return i32(off), i32(eg), G, most if max_group_faces is None else int(max_group_faces)


def mesh_depth_render_groups(verts, vert_part, faces, F_shared, group_off, env_group, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h,
                             im_w, near=0.01, far=100.0, out=None, max_group_faces=None):
    """mesh_depth_render over a scene whose environments differ (pm_mesh_depth_render_groups_f32): environment b draws rows
    [0, F_shared) of faces and the rows of group env_group[b] (-1: none), group g being rows F_shared + [group_off[g], group_off[g + 1]).
    group_off / env_group / max_group_faces as face_groups takes them; everything else, and the result, as mesh_depth_render."""
    return mesh_depth_render(verts, vert_part, faces, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h, im_w, near, far, out,
                             groups=(F_shared, group_off, env_group, max_group_faces))


def mesh_frame_render(verts, vert_part, faces, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h, im_w, near, far, workspace,
                      part_label=None, miss_label=-1, palette=None, ambient=0.25, one_minus_ambient=None, background=(255, 255, 255),
                      depth=True, seg=True, rgb=True, groups=None):
    """Depth, part-label and shaded colour images of the posed part meshes from one rasterisation (pm_mesh_frame_render_f32); the
    geometry, pose and camera arguments are mesh_depth_render's.  part_label (M) int32 or None (the part index itself), miss_label
    for pixels nothing hits; palette (M, 3) float32 in [0, 255], ambient and one_minus_ambient (default 1 - ambient) the headlight's
    two weights, background three ints in 0..255.  depth / seg / rgb: False (not wanted), True (a fresh (B, V h w) float32 / (B, V h w)
    int32 / (B, 3 V h w) uint8) or a 2-D view of that type with at least that many columns and unit inner stride; columns past
    them are left alone.  workspace: a device tensor of at least pm_mesh_frame_workspace_bytes(B, V, h, w) bytes, 8-byte aligned
    (the library checks both).  Returns (depth, seg, rgb) with None for the ones switched off.  The winner of a pixel is the nearest
    triangle, the smaller row of `faces` on a tie; all three images are defined bit for bit (include/partmanip_hip.h).
    groups: None, or mesh_frame_render_groups' (F_shared, group_off, env_group, max_group_faces)."""
    outs = [o if torch.is_tensor(o) else None for o in (depth, seg, rgb)]
    _one_device("mesh_frame_render", verts, vert_part, faces, pose_R, pose_T, cam_pose, workspace, part_label, palette, *outs)
    NV, B, M, V, im_h, im_w = _mesh_camera_args(verts, vert_part, faces, pose_R, pose_T, cam_pose, im_h, im_w, near, far)
    if depth is False and seg is False and rgb is False:
        raise ValueError("mesh_frame_render: depth, seg and rgb are all switched off")
    if part_label is not None and (part_label.dtype != torch.int32 or not part_label.is_contiguous() or tuple(part_label.shape) != (M,)):
        raise ValueError(f"part_label: expected a contiguous int32 tensor ({M},), got {part_label.dtype} {tuple(part_label.shape)}")
    if rgb is not False:
        if palette is None:
            raise ValueError("palette: needed for the rgb image")
        _f32c(palette, "palette")
        if tuple(palette.shape) != (M, 3):
            raise ValueError(f"palette: expected ({M}, 3), got {tuple(palette.shape)}")
    one_minus_ambient = 1.0 - float(ambient) if one_minus_ambient is None else float(one_minus_ambient)
    if not (0.0 <= ambient <= 1.0 and 0.0 <= one_minus_ambient <= 1.0):
        raise ValueError(f"ambient, one_minus_ambient: expected both in [0, 1], got {ambient}, {one_minus_ambient}")
    bg = [int(c) for c in background]
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError(f"background: expected three values in 0..255, got {background}")
    n, dev = V * im_h * im_w, pose_R.device
    ldd = lds = ldc = 0
    if depth is not False:
        depth, ldd = _out_rows(None if depth is True else depth, B, n, dev)
    if seg is not False:
        seg, lds = _out_rows(None if seg is True else seg, B, n, dev, torch.int32, "seg")
    if rgb is not False:
        rgb, ldc = _out_rows(None if rgb is True else rgb, B, 3 * n, dev, torch.uint8, "rgb")
    d_, s_, c_ = (None if o is False else o for o in (depth, seg, rgb))
    # the arguments after F, which both entries share; the grouped entry takes five more before them
    rest = (_ptr(pose_R), _ptr(pose_T), B, M, _ptr(cam_pose), V, float(fx), float(fy), float(cx), float(cy), im_h, im_w, float(near),
            float(far), _ptr(part_label), int(miss_label), _ptr(palette), float(ambient), one_minus_ambient, bg[0], bg[1], bg[2], _ptr(d_),
            ldd, _ptr(s_), lds, _ptr(c_), ldc, _ptr(workspace), workspace.numel() * workspace.element_size(), _stream())
    if groups is None:
        with TIMER.bracket("mesh_frame_render"):
            check(lib.pm_mesh_frame_render_f32(_ptr(verts), _ptr(vert_part), NV, _ptr(faces), faces.shape[0], *rest),
                  "pm_mesh_frame_render_f32")
        return d_, s_, c_
    F_shared, group_off, env_group, most = groups
    group_off, env_group, G, most = face_groups(group_off, env_group, faces.shape[0], F_shared, B, dev, most)
    _one_device("mesh_frame_render_groups", verts, group_off, env_group)
    with TIMER.bracket("mesh_frame_render_groups"):
        check(lib.pm_mesh_frame_render_groups_f32(_ptr(verts), _ptr(vert_part), NV, _ptr(faces), faces.shape[0], int(F_shared),
                                                  _ptr(group_off), G, _ptr(env_group), most, *rest), "pm_mesh_frame_render_groups_f32")
    return d_, s_, c_


def mesh_frame_render_groups(verts, vert_part, faces, F_shared, group_off, env_group, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h,
                             im_w, near, far, workspace, max_group_faces=None, **kw):
    """mesh_frame_render over a scene whose environments differ (pm_mesh_frame_render_groups_f32): the face subset of an environment
    as in mesh_depth_render_groups, the winner the nearest triangle of the subset (the smaller row of `faces` on a tie); the
    keywords and the result are mesh_frame_render's."""
    return mesh_frame_render(verts, vert_part, faces, pose_R, pose_T, cam_pose, fx, fy, cx, cy, im_h, im_w, near, far, workspace,
                             groups=(F_shared, group_off, env_group, max_group_faces), **kw)


def body_pose_gather(rigid_body, rows, part_C=None, pose_R=None, pose_T=None):
    """Body poses of a whole scene in one launch (pm_body_pose_gather_f32): rigid_body (..., 13) float32 contiguous, read as flat rows;
    rows (B, M) int32, slot m of environment b is flat row rows[b, m] (outside [0, rows): a NaN pose); part_C (MC <= M, 3, 3) or None:
    the mesh-frame matrices of the first MC slots.  pose_R (B, M, 3, 3) / pose_T (B, M, 3): None (fresh) or contiguous float32
    tensors to write.  Returns (pose_R, pose_T): the position, and quat_to_mat(q) (times C_m for m < MC) exactly as the task kernels
    compute them."""
    _one_device("body_pose_gather", rigid_body, rows, part_C, pose_R, pose_T)
    _f32c(rigid_body, "rigid_body")
    if rigid_body.dim() < 2 or rigid_body.shape[-1] != 13 or rigid_body.numel() == 0:
        raise ValueError(f"rigid_body: expected (..., 13) with at least one row, got {tuple(rigid_body.shape)}")
    _i32c(rows, "rows")
    if rows.dim() != 2 or rows.numel() == 0:
        raise ValueError(f"rows: expected (B > 0, M > 0), got {tuple(rows.shape)}")
    B, M = rows.shape
    MC = 0
    if part_C is not None:
        _f32c(part_C, "part_C")
        if part_C.dim() != 3 or tuple(part_C.shape[1:]) != (3, 3) or part_C.shape[0] > M:
            raise ValueError(f"part_C: expected (MC <= {M}, 3, 3), got {tuple(part_C.shape)}")
        MC = part_C.shape[0]
    f = dict(dtype=torch.float32, device=rigid_body.device)
    pose_R = torch.empty(B, M, 3, 3, **f) if pose_R is None else pose_R
    pose_T = torch.empty(B, M, 3, **f) if pose_T is None else pose_T
    _f32c(pose_R, "pose_R"), _f32c(pose_T, "pose_T")
    if tuple(pose_R.shape) != (B, M, 3, 3) or tuple(pose_T.shape) != (B, M, 3):
        raise ValueError(f"pose_R / pose_T: expected ({B}, {M}, 3, 3) and ({B}, {M}, 3), got {tuple(pose_R.shape)} and {tuple(pose_T.shape)}")
    with TIMER.bracket("body_pose_gather"):
        check(lib.pm_body_pose_gather_f32(_ptr(rigid_body), rigid_body.numel() // 13, _ptr(rows), B, M, _ptr(part_C if MC else None), MC,
                                          _ptr(pose_R), _ptr(pose_T), _stream()), "pm_body_pose_gather_f32")
    return pose_R, pose_T


def _vec(t_, name, n, dtype=torch.float32):
    if t_.dtype != dtype or not t_.is_contiguous() or t_.numel() != n:
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of {n} elements, got {t_.dtype} {tuple(t_.shape)}")


def _flags(t_, name, n):
    if t_.dtype not in (torch.bool, torch.uint8) or not t_.is_contiguous() or t_.numel() != n:
        raise ValueError(f"{name}: expected a contiguous bool / uint8 tensor of {n} elements, got {t_.dtype} {tuple(t_.shape)}")


def _shape_f32c(t_, name, shape):
    _f32c(t_, name)
    if tuple(t_.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)}, got {tuple(t_.shape)}")


def _root_dims(root, N=None):
    """(N, na) of the simulator's root tensor (N, na, 13); with N given, the batch it must have."""
    if root.dim() != 3 or root.shape[2] != 13 or root.shape[1] == 0 or (root.shape[0] == 0 if N is None else root.shape[0] != N):
        raise ValueError(f"root: expected ({'N' if N is None else N}, na, 13), got {tuple(root.shape)}")
    return root.shape[0], root.shape[1]


def _pose_outputs(N, part, arg, part_C, pose_R, pose_T):
    """The part-pose arguments of a post wrapper: the part list `part` (M) int32 (the argument called `arg`), part_C (M, 3, 3) or
    None, pose_R (N, M, 3, 3) and pose_T (N, M, 3), either or both None.  Returns M, 0 where no pose is asked for."""
    if pose_R is None and pose_T is None:
        return 0
    if part is None or part.dim() != 1 or part.numel() == 0:
        raise ValueError(f"pose_R / pose_T need {arg} (M) int32")
    M = part.numel()
    _vec(part, arg, M, torch.int32)
    if part_C is not None:
        _shape_f32c(part_C, "part_C", (M, 3, 3))
    for t_, name, shape in ((pose_R, "pose_R", (N, M, 3, 3)), (pose_T, "pose_T", (N, M, 3))):
        if t_ is not None:
            _shape_f32c(t_, name, shape)
    return M


def _row_view(t_, name, N, width):
    """Row stride (in elements) of a 2-D float32 output view (N, width) with unit inner stride."""
    if t_.dtype != torch.float32 or t_.dim() != 2 or tuple(t_.shape) != (N, width) or t_.stride(1) != 1:
        raise ValueError(f"{name}: expected a float32 view ({N}, {width}) with unit inner stride, got {t_.dtype} {tuple(t_.shape)} "
                         f"{t_.stride()}")
    ld = t_.stride(0) if N > 1 else width
    if ld < width:
        raise ValueError(f"{name}: row stride {ld} below the row width {width}")
    return ld


def grasp_cube_post(rigid_body, dof_state, root, obj_actor, ltip, rtip, dof_lo, dof_hi, pose_lo, pose_hi, goal, goal_thresh,
                    obj_default_pos, part_body=None, part_C=None, normal_state=None, proprio=None, rew=None, success=None,
                    is_reached=None, extras=None, pose_R=None, pose_T=None):
    """Everything after physics of the grasp_cube task in one launch (pm_grasp_cube_post_f32, include/partmanip_hip.h): rigid_body
    (N, nb, 13), dof_state (N, nd, 2), root (N, na, 13), all contiguous float32.  Outputs are written in place and every one may be
    None (skipped): normal_state (N, 19 + 2 nd), proprio (N, 7 + 2 nd) and extras (N, 8) may be column views of a wider buffer;
    rew (N) float32; success, is_reached (N) bool or uint8; pose_R (N, M, 3, 3), pose_T (N, M, 3) with part_body (M) int32 and
    part_C (M, 3, 3) or None."""
    _one_device("grasp_cube_post", rigid_body, dof_state, root, dof_lo, dof_hi, pose_lo, pose_hi, goal, obj_default_pos, part_body,
                part_C, normal_state, proprio, rew, success, is_reached, extras, pose_R, pose_T)
    for t_, name in ((rigid_body, "rigid_body"), (dof_state, "dof_state"), (root, "root")):
        _f32c(t_, name)
    if rigid_body.dim() != 3 or rigid_body.shape[2] != 13 or rigid_body.shape[0] == 0 or rigid_body.shape[1] == 0:
        raise ValueError(f"rigid_body: expected (N, nb, 13), got {tuple(rigid_body.shape)}")
    N, nb = rigid_body.shape[0], rigid_body.shape[1]
    if dof_state.dim() != 3 or dof_state.shape[0] != N or dof_state.shape[2] != 2 or dof_state.shape[1] == 0:
        raise ValueError(f"dof_state: expected ({N}, nd, 2), got {tuple(dof_state.shape)}")
    nd = dof_state.shape[1]
    na = _root_dims(root, N)[1]
    if not (0 <= obj_actor < na and 0 <= ltip < nb and 0 <= rtip < nb):
        raise ValueError(f"obj_actor {obj_actor} / ltip {ltip} / rtip {rtip} outside ({na} actors, {nb} bodies)")
    for t_, name, n in ((dof_lo, "dof_lo", nd), (dof_hi, "dof_hi", nd), (pose_lo, "pose_lo", 7), (pose_hi, "pose_hi", 7),
                        (goal, "goal", 3), (obj_default_pos, "obj_default_pos", 3)):
        _vec(t_, name, n)
    M = _pose_outputs(N, part_body, "part_body", part_C, pose_R, pose_T)
    lns = _row_view(normal_state, "normal_state", N, 19 + 2 * nd) if normal_state is not None else 0
    lpr = _row_view(proprio, "proprio", N, 7 + 2 * nd) if proprio is not None else 0
    lex = _row_view(extras, "extras", N, 8) if extras is not None else 0
    if rew is not None:
        _vec(rew, "rew", N)
    for t_, name in ((success, "success"), (is_reached, "is_reached")):
        if t_ is not None:
            _flags(t_, name, N)
    with TIMER.bracket("grasp_cube_post"):
        check(lib.pm_grasp_cube_post_f32(_ptr(rigid_body), _ptr(dof_state), _ptr(root), N, nb, nd, na, int(obj_actor), int(ltip),
                                         int(rtip), _ptr(dof_lo), _ptr(dof_hi), _ptr(pose_lo), _ptr(pose_hi), _ptr(goal),
                                         float(goal_thresh), _ptr(obj_default_pos), _ptr(part_body), _ptr(part_C), M,
                                         _ptr(normal_state), lns, _ptr(proprio), lpr, _ptr(rew), _ptr(success), _ptr(is_reached),
                                         _ptr(extras), lex, _ptr(pose_R), _ptr(pose_T), _stream()), "pm_grasp_cube_post_f32")


DRIVE_MODES = {"ik": 0, "pos": 1}                            # drive_mode of pm_franka_control_f32


def franka_control(actions, dof_state, jac, jl, jr, dof_lo, dof_hi, default_dof_pos, dt, drive_mode, rew, success, progress,
                   explore_step, max_episode_length, train, pos_act, epis_max_rew, epis_max_step, reset, reset_succ, counters, slot,
                   num_base_dofs=0, base_R=None):
    """Everything before physics in one launch (pm_franka_control_f32): joint targets from the actions ('ik': damped least squares
    over jac (N, nl, 6, nd), link rows jl and jr; 'pos': scaled actions; jac may be None there) and the reference's episode
    bookkeeping, in place: success (N) bool / uint8, progress and epis_max_step (N) int64, epis_max_rew (N), pos_act (N, nd), reset
    and reset_succ (N) bool / uint8, counters (4) int32 (this call adds to pair `slot` and zeroes the other).  Returns pos_act.

    num_base_dofs = 3 with base_R (3, 3) float32 (quat_to_mat of the robot's default root quaternion) drives the mobile Franka
    (pm_franka_control_mobile_f32, still one launch): actions are then (N, 10) for 'ik' = [base 3 | pose 6 | gripper] and (N, nd - 1)
    for 'pos', the base targets are qpos + base_R^T (0.005 a[:3]) and the arm is DOFs [3, nd - 2)."""
    nbase = int(num_base_dofs)
    if nbase not in (0, 3):
        raise ValueError(f"num_base_dofs: expected 0 (fixed base) or 3 (mobile base), got {num_base_dofs}")
    tensors = (actions, dof_state, jac, dof_lo, dof_hi, default_dof_pos, rew, success, progress, pos_act, epis_max_rew, epis_max_step,
               reset, reset_succ, counters, base_R)
    if not nbase:                                             # the mobile path checks its shapes first, the device before the launch
        _one_device("franka_control", *tensors)
    if drive_mode not in DRIVE_MODES:
        raise ValueError(f"drive_mode: expected one of {tuple(DRIVE_MODES)}, got {drive_mode!r}")
    _f32c(dof_state, "dof_state")
    if nbase:
        if base_R is None or base_R.dtype != torch.float32 or tuple(base_R.shape) != (3, 3) or not base_R.is_contiguous():
            raise ValueError("base_R: expected a contiguous float32 (3, 3) tensor for a mobile base, got "
                             + ("None" if base_R is None else f"{base_R.dtype} {tuple(base_R.shape)}"))
    elif base_R is not None:
        raise ValueError("base_R is given but num_base_dofs is 0")
    if dof_state.dim() != 3 or dof_state.shape[2] != 2 or dof_state.shape[0] == 0 or dof_state.shape[1] < nbase + 3:
        raise ValueError(f"dof_state: expected (N, nd >= {nbase + 3}, 2), got {tuple(dof_state.shape)}")
    N, nd = dof_state.shape[0], dof_state.shape[1]
    A = 7 + nbase if drive_mode == "ik" else nd - 1
    if actions.dtype != torch.float32 or actions.dim() != 2 or tuple(actions.shape) != (N, A) or actions.stride(1) != 1:
        raise ValueError(f"actions: expected a float32 ({N}, {A}) tensor with unit inner stride for drive mode {drive_mode!r}, got "
                         f"{actions.dtype} {tuple(actions.shape)}")
    lda = actions.stride(0) if N > 1 else A
    if lda < A:
        raise ValueError(f"actions: row stride {lda} below {A}")
    nl = 0
    if drive_mode == "ik":
        if jac is None:
            raise ValueError("drive mode 'ik' needs the Jacobian")
        _f32c(jac, "jac")
        if jac.dim() != 4 or jac.shape[0] != N or tuple(jac.shape[2:]) != (6, nd) or jac.shape[1] == 0:
            raise ValueError(f"jac: expected ({N}, nl, 6, {nd}), got {tuple(jac.shape)}")
        nl = jac.shape[1]
        if not (0 <= jl < nl and 0 <= jr < nl):
            raise ValueError(f"link rows {jl}, {jr} outside the {nl} links of the Jacobian")
    else:
        jac = None
    for t_, name, n in ((dof_lo, "dof_lo", nd), (dof_hi, "dof_hi", nd), (default_dof_pos, "default_dof_pos", nd), (rew, "rew", N),
                        (epis_max_rew, "epis_max_rew", N), (pos_act, "pos_act", N * nd)):
        _vec(t_, name, n)
    _vec(progress, "progress", N, torch.int64)
    _vec(epis_max_step, "epis_max_step", N, torch.int64)
    _vec(counters, "counters", 4, torch.int32)
    for t_, name in ((success, "success"), (reset, "reset"), (reset_succ, "reset_succ")):
        _flags(t_, name, N)
    if slot not in (0, 1):
        raise ValueError(f"slot: expected 0 or 1, got {slot}")
    head = [_ptr(actions), lda, A, _ptr(dof_state), _ptr(jac), N, nd, nl, int(jl), int(jr), _ptr(dof_lo), _ptr(dof_hi),
            _ptr(default_dof_pos), float(dt), DRIVE_MODES[drive_mode]]
    tail = [_ptr(rew), _ptr(success), _ptr(progress), int(explore_step), int(max_episode_length), 1 if train else 0, _ptr(pos_act),
            _ptr(epis_max_rew), _ptr(epis_max_step), _ptr(reset), _ptr(reset_succ), _ptr(counters), int(slot)]
    entry = "pm_franka_control_f32"
    if nbase:                                                 # the mobile entry point takes (nbase, base_R) between the two
        _one_device("franka_control", *tensors)
        head += [nbase, _ptr(base_R)]
        entry = "pm_franka_control_mobile_f32"
    with TIMER.bracket("franka_control"):
        check(getattr(lib, entry)(*head, *tail, _stream()), entry)
    return pos_act


def _rows_of(t_, name, width, N, n, row0):
    """(rows in all, rows per environment) of a simulator tensor that holds n rows of `width` per environment: dense (N, >= n, width)
    with row0 None, flat (rows, width) with the (N) int32 row table row0."""
    _f32c(t_, name)
    if row0 is None:
        if t_.dim() != 3 or t_.shape[0] != N or t_.shape[1] < n or t_.shape[2] != width:
            raise ValueError(f"{name}: expected ({N}, >= {n}, {width}), got {tuple(t_.shape)}")
        return N * t_.shape[1], t_.shape[1]
    if t_.dim() != 2 or t_.shape[1] != width or t_.shape[0] < n:
        raise ValueError(f"{name}: expected (rows >= {n}, {width}) with a row table, got {tuple(t_.shape)}")
    _vec(row0, f"{name}'s row table", N, torch.int32)
    return t_.shape[0], 0


def _articulation_args(who, parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, vmax, base_pose, dof_state, dof_row0):
    """The tree, limit, base-pose and DOF-row checks articulation_step and articulation_sweep share.  Returns (nb, nd, N, the base
    pose's stride, the rows of dof_state, its rows per environment)."""
    nb, nd = parent.numel(), dof_lo.numel()
    if not (1 <= nb <= 64 and 1 <= nd <= 64):
        raise ValueError(f"{who}: {nb} bodies / {nd} DOFs outside [1, 64]")
    for t_, name in ((parent, "parent"), (jtype, "jtype"), (dof, "dof")):
        _vec(t_, name, nb, torch.int32)
    _vec(anc_mask, "anc_mask", nb, torch.int64)
    _shape_f32c(origin_q, "origin_q", (nb, 4))
    _shape_f32c(origin_t, "origin_t", (nb, 3))
    _shape_f32c(axis, "axis", (nb, 3))
    _vec(dof_hi, "dof_hi", nd)
    _vec(dof_lo, "dof_lo", nd)
    if vmax is not None:
        _vec(vmax, "vmax", nd)
    _f32c(base_pose, "base_pose")
    if base_pose.dim() == 1 and base_pose.numel() == 7:
        N, lbase = None, 0
    elif base_pose.dim() == 2 and base_pose.shape[1] == 7 and base_pose.shape[0] > 0:
        N, lbase = base_pose.shape[0], 7
    else:
        raise ValueError(f"base_pose: expected (7) or (N, 7), got {tuple(base_pose.shape)}")
    if dof_row0 is not None:
        N = dof_row0.numel() if N is None else N
    elif dof_state.dim() == 3:
        N = dof_state.shape[0] if N is None else N
    if not N:
        raise ValueError(f"dof_state: expected (N, >= {nd}, 2) or flat (D, 2) with dof_row0, got {tuple(dof_state.shape)}")
    dof_rows, ldd = _rows_of(dof_state, "dof_state", 2, N, nd, dof_row0)
    return nb, nd, N, lbase, dof_rows, ldd


def articulation_step(parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, base_pose, dof_state, targets=None,
                      reset=None, vmax=None, dt=0.0, rigid_body=None, jac=None, rb_row0=None, dof_row0=None):
    """One step of the kinematic articulation in one launch (pm_articulation_step_f32, include/partmanip_hip.h).  The tree tables
    (nb) / (nb, 4) / (nb, 3) and anc_mask (nb) int64 come from kinematics.Articulation, which validates them; dof_lo, dof_hi, vmax
    (nd); base_pose (7) or (N, 7); dof_state (N, >= nd, 2), or flat (D, 2) with dof_row0 (N) int32, updated in place when targets
    (N, nd) is given (reset (N) bool / uint8 then snaps an environment to its clamped target); rigid_body (N, >= nb, 13) or flat
    (B, 13) with rb_row0; jac (N, nb - 1, 6, nd).  rigid_body and jac may be None (skipped)."""
    _one_device("articulation_step", parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, base_pose, dof_state,
                targets, reset, vmax, rigid_body, jac, rb_row0, dof_row0)
    nb, nd, N, lbase, dof_rows, ldd = _articulation_args("articulation_step", parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo,
                                                         dof_hi, vmax, base_pose, dof_state, dof_row0)
    rb_rows, ldr = _rows_of(rigid_body, "rigid_body", 13, N, nb, rb_row0) if rigid_body is not None else (0, 0)
    if jac is not None:
        _shape_f32c(jac, "jac", (N, nb - 1, 6, nd))
    ldt = 0
    if targets is not None:
        ldt = _row_view(targets, "targets", N, nd)
        if not float(dt) > 0:
            raise ValueError(f"dt: expected a positive step with targets, got {dt}")
    elif reset is not None:
        raise ValueError("reset is given without targets")
    if reset is not None:
        _flags(reset, "reset", N)
    with TIMER.bracket("articulation_step"):
        check(lib.pm_articulation_step_f32(_ptr(parent), _ptr(jtype), _ptr(dof), _ptr(origin_q), _ptr(origin_t), _ptr(axis),
                                           _ptr(anc_mask), _ptr(dof_lo), _ptr(dof_hi), _ptr(vmax), float(dt), _ptr(base_pose), lbase,
                                           _ptr(dof_state), dof_rows, _ptr(targets), ldt, _ptr(reset), _ptr(rb_row0), ldr, rb_rows,
                                           _ptr(dof_row0), ldd, N, nb, nd, _ptr(rigid_body), _ptr(jac), _stream()),
              "pm_articulation_step_f32")


def articulation_sweep(parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, base_pose, dof_state, targets, dt, fields,
                       part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier, seg_off, slot_body, substeps,
                       margin=0.0, reset=None, free=None, vmax=None, dof_row0=None, slot_C=None, p0=0, p1=None, pt_id=None,
                       chunk_sphere=None, cull=True, grid_slot=None, NG_shared=None, group_off=None, env_group=None,
                       max_group_grids=None, sweep_dist=None, steps=None, targets_out=None):
    """The swept contact test of one kinematic step in one launch (pm_articulation_sweep_f32; with grid_slot= the grouped entry;
    include/partmanip_hip.h states the rule): how many of `substeps` parts of the step from dof_state towards targets the robot can
    take before a sensing point comes within `margin` of a target grid, or deeper into one.  The tree tables, limits, vmax, base_pose,
    dof_state (only read), targets (N, nd), reset and dof_row0 as articulation_step; the part tables, pose_R / pose_T (N, M, ...: the
    scene pose as it stands), pts, carrier, pt_id, chunk_sphere, seg_off (required), [p0, p1), cull and the group tables as
    mesh_sdf_points.  slot_body: M integers, the robot body in [0, nb) that places pose slot m or -1 for a slot the table places (on
    the host: validated and copied; on the device: type and length only); slot_C (MC <= M, 3, 3) or None: body_pose_gather's part_C;
    free (N) bool / uint8 or None: environments that are not guarded.  sweep_dist (N, substeps + 1) float32, steps (N) int32,
    targets_out (N, nd) float32: None (fresh) or contiguous tensors to write.  Returns (sweep_dist, steps, targets_out); nothing
    else is written."""
    nb, nd, N, lbase, dof_rows, ldd = _articulation_args("articulation_sweep", parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo,
                                                         dof_hi, vmax, base_pose, dof_state, dof_row0)
    if targets is None:
        raise ValueError("targets: the sweep needs the step's targets (N, nd)")
    ldt = _row_view(targets, "targets", N, nd)
    if not float(dt) > 0:
        raise ValueError(f"dt: expected a positive step, got {dt}")
    for t_, name in ((reset, "reset"), (free, "free")):
        if t_ is not None:
            _flags(t_, name, N)
    S = int(substeps)
    if not 1 <= S <= 63:
        raise ValueError(f"substeps: expected 1 .. 63 parts of a step, got {substeps}")
    margin = float(margin)
    if margin != margin:
        raise ValueError("margin: expected a number, got NaN")
    if seg_off is None:
        raise ValueError("seg_off: the sweep needs the sensing bodies' segments")
    (grouped, NG, B, M, dev, NP, stride, carrier, pt_id, seg_off, NS, grid_slot, group_off, env_group, G, most, p0, p1) = _sdf_point_args(
        fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts, carrier, p0, p1, pt_id, chunk_sphere, seg_off,
        grid_slot, NG_shared, group_off, env_group, max_group_grids)
    if B != N:
        raise ValueError(f"pose_R / pose_T: expected the {N} environments of the articulation, got {B}")
    slot_body = _host_i32(slot_body, "slot_body", M, -1, nb, dev)
    MC = 0
    if slot_C is not None:
        _f32c(slot_C, "slot_C")
        if slot_C.dim() != 3 or tuple(slot_C.shape[1:]) != (3, 3) or slot_C.shape[0] > M:
            raise ValueError(f"slot_C: expected (MC <= {M}, 3, 3), got {tuple(slot_C.shape)}")
        MC = slot_C.shape[0]
    lds = (S + 1) * (((7 * nb) | 1) * 8 + 4 * nd)
    if lds > 57344:
        raise ValueError(f"substeps: {S} parts of a {nb}-body chain need {lds} bytes of LDS, above 57344")
    f = dict(dtype=torch.float32, device=dev)
    sweep_dist = torch.empty(N, S + 1, **f) if sweep_dist is None else sweep_dist
    steps = torch.empty(N, dtype=torch.int32, device=dev) if steps is None else steps
    targets_out = torch.empty(N, nd, **f) if targets_out is None else targets_out
    _shape_f32c(sweep_dist, "sweep_dist", (N, S + 1))
    _vec(steps, "steps", N, torch.int32)
    _shape_f32c(targets_out, "targets_out", (N, nd))
    _one_device("articulation_sweep", parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, base_pose, dof_state,
                targets, reset, free, vmax, dof_row0, fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, pts,
                carrier, pt_id, seg_off, chunk_sphere, slot_body, slot_C, grid_slot, group_off, env_group, sweep_dist, steps, targets_out)
    head = (_ptr(parent), _ptr(jtype), _ptr(dof), _ptr(origin_q), _ptr(origin_t), _ptr(axis), _ptr(dof_lo), _ptr(dof_hi), _ptr(vmax),
            float(dt), _ptr(base_pose), lbase, _ptr(dof_state), dof_rows, _ptr(targets), ldt, _ptr(reset), _ptr(dof_row0), ldd, N, nb, nd,
            _ptr(fields), _ptr(part_off), _ptr(part_shape), _ptr(part_bbox_min), _ptr(part_voxel_size))
    tail = (_ptr(pose_R), _ptr(pose_T), M, p0, p1, _ptr(pts), stride, _ptr(carrier), _ptr(pt_id), _ptr(chunk_sphere), NP, _ptr(seg_off), NS,
            1 if cull else 0, _ptr(slot_body), _ptr(slot_C if MC else None), MC, S, margin, _ptr(free), _ptr(sweep_dist), _ptr(steps),
            _ptr(targets_out), _stream())
    with TIMER.bracket("articulation_sweep"):
        if grouped:
            check(lib.pm_articulation_sweep_groups_f32(*head, _ptr(grid_slot), NG, int(NG_shared), _ptr(group_off), G, _ptr(env_group), most,
                                                       *tail), "pm_articulation_sweep_groups_f32")
        else:
            check(lib.pm_articulation_sweep_f32(*head, *tail), "pm_articulation_sweep_f32")
    return sweep_dist, steps, targets_out


def articulation_objects_step(body_off, dof_off, parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi, max_nb, max_nd,
                              obj_type, obj_pose, obj_rb_row0, obj_dof_row0, dof_state, rigid_body, order=None, hold=None, reset=None,
                              target_dof=None, tip_rows=None, dt=0.0):
    """One object tree per environment, posed into the flat tensors in one launch (pm_articulation_objects_step_f32,
    include/partmanip_hip.h).  The library tables come from kinematics.ObjectLibrary, which validates them: body_off, dof_off
    (K + 1) int32, the per-body tables over all the trees' bodies, dof_lo / dof_hi over all their DOFs, max_nb / max_nd the largest
    tree.  obj_type (N) int32; obj_pose (7), or an (N, 7) view with unit inner stride (root[:, obj_actor, :7]); obj_rb_row0,
    obj_dof_row0 (N) int32; dof_state (D, 2) and rigid_body (B, 13) flat; order (N) int32 or None.  The hold group hold, reset (N)
    bool / uint8, target_dof (N) int32, tip_rows (N, 2) int32 and dt > 0 comes together or not at all; without it dof_state is only
    read."""
    _one_device("articulation_objects_step", body_off, dof_off, parent, jtype, dof, origin_q, origin_t, axis, anc_mask, dof_lo, dof_hi,
                obj_type, obj_pose, obj_rb_row0, obj_dof_row0, dof_state, rigid_body, order, hold, reset, target_dof, tip_rows)
    K, TB, TD, N = body_off.numel() - 1, parent.numel(), dof_lo.numel(), obj_type.numel()
    if K < 1 or TB < 1 or TD < 1 or N < 1:
        raise ValueError(f"articulation_objects_step: {K} trees, {TB} bodies, {TD} DOFs, {N} environments: expected at least one of each")
    if not (1 <= int(max_nb) <= 64 and 1 <= int(max_nd) <= 64):
        raise ValueError(f"articulation_objects_step: max_nb {max_nb} / max_nd {max_nd} outside [1, 64]")
    _vec(body_off, "body_off", K + 1, torch.int32)
    _vec(dof_off, "dof_off", K + 1, torch.int32)
    for t_, name in ((parent, "parent"), (jtype, "jtype"), (dof, "dof")):
        _vec(t_, name, TB, torch.int32)
    _vec(anc_mask, "anc_mask", TB, torch.int64)
    _shape_f32c(origin_q, "origin_q", (TB, 4))
    _shape_f32c(origin_t, "origin_t", (TB, 3))
    _shape_f32c(axis, "axis", (TB, 3))
    _vec(dof_lo, "dof_lo", TD)
    _vec(dof_hi, "dof_hi", TD)
    for t_, name in ((obj_type, "obj_type"), (obj_rb_row0, "obj_rb_row0"), (obj_dof_row0, "obj_dof_row0")):
        _vec(t_, name, N, torch.int32)
    if order is not None:
        _vec(order, "order", N, torch.int32)
    if obj_pose.dim() == 1:
        _shape_f32c(obj_pose, "obj_pose", (7,))
        lpose = 0
    else:
        lpose = _row_view(obj_pose, "obj_pose", N, 7)
    _shape_f32c(dof_state, "dof_state", (dof_state.shape[0], 2))
    _shape_f32c(rigid_body, "rigid_body", (rigid_body.shape[0], 13))
    if dof_state.shape[0] < 1 or rigid_body.shape[0] < 1:
        raise ValueError("dof_state / rigid_body: expected at least one row")
    group = (hold, reset, target_dof, tip_rows)
    if any(g is not None for g in group):
        if any(g is None for g in group):
            raise ValueError("hold, reset, target_dof and tip_rows come together or not at all")
        _flags(hold, "hold", N)
        _flags(reset, "reset", N)
        _vec(target_dof, "target_dof", N, torch.int32)
        _vec(tip_rows, "tip_rows", 2 * N, torch.int32)
        if not float(dt) > 0:
            raise ValueError(f"dt: expected a positive step with the hold group, got {dt}")
    with TIMER.bracket("articulation_objects_step"):
        check(lib.pm_articulation_objects_step_f32(_ptr(body_off), _ptr(dof_off), K, TB, TD, int(max_nb), int(max_nd), _ptr(parent),
                                                   _ptr(jtype), _ptr(dof), _ptr(origin_q), _ptr(origin_t), _ptr(axis), _ptr(anc_mask),
                                                   _ptr(dof_lo), _ptr(dof_hi), _ptr(obj_type), _ptr(order), _ptr(obj_pose), lpose,
                                                   _ptr(obj_rb_row0), _ptr(obj_dof_row0), _ptr(dof_state), dof_state.shape[0],
                                                   _ptr(rigid_body), rigid_body.shape[0], _ptr(hold), _ptr(reset), _ptr(target_dof),
                                                   _ptr(tip_rows), float(dt), N, _stream()),
              "pm_articulation_objects_step_f32")


def free_body_step(rigid_body, tip_rows, body_row, root, obj_actor, hold, reset, grip, default_pose, dt, u=None, reset_range=0.15,
                   rest_z=0.025, fall_speed=0.0):
    """One free rigid body per environment, moved by the stated rule in one launch (pm_free_body_step_f32, include/partmanip_hip.h),
    after the robot's launch on the same stream.  rigid_body (N, nb, 13) or flat (B, 13), contiguous; tip_rows (N, 2) and body_row (N)
    int32 are FLAT rows of it either way; root (N, na, 13); hold, reset (N) bool / uint8; grip (N, 8) float32, read and written;
    default_pose (7); u (N, 3) in [0, 1) or None.  Written in place: root[:, obj_actor], the body rows, grip."""
    _one_device("free_body_step", rigid_body, tip_rows, body_row, root, hold, reset, grip, default_pose, u)
    _f32c(rigid_body, "rigid_body")
    if rigid_body.dim() not in (2, 3) or rigid_body.shape[-1] != 13 or rigid_body.numel() == 0:
        raise ValueError(f"rigid_body: expected (N, nb, 13) or (B, 13), got {tuple(rigid_body.shape)}")
    _f32c(root, "root")
    N, na = _root_dims(root)
    if not 0 <= int(obj_actor) < na:
        raise ValueError(f"obj_actor {obj_actor} outside the {na} actors of root")
    _vec(tip_rows, "tip_rows", 2 * N, torch.int32)
    _vec(body_row, "body_row", N, torch.int32)
    _flags(hold, "hold", N)
    _flags(reset, "reset", N)
    _shape_f32c(grip, "grip", (N, 8))
    _vec(default_pose, "default_pose", 7)
    if u is not None:
        _shape_f32c(u, "u", (N, 3))
    if not float(dt) > 0:
        raise ValueError(f"dt: expected a positive step, got {dt}")
    if not float(fall_speed) >= 0 or not float(reset_range) >= 0 or float(rest_z) != float(rest_z):
        raise ValueError(f"fall_speed {fall_speed} and reset_range {reset_range}: expected non-negative numbers, rest_z {rest_z} a number")
    with TIMER.bracket("free_body_step"):
        check(lib.pm_free_body_step_f32(_ptr(rigid_body), rigid_body.numel() // 13, _ptr(tip_rows), _ptr(body_row), _ptr(root), na,
                                        int(obj_actor), _ptr(hold), _ptr(reset), _ptr(grip), _ptr(default_pose), _ptr(u),
                                        float(reset_range), float(dt), float(rest_z), float(fall_speed), N, _stream()),
              "pm_free_body_step_f32")


def _index_table(t_, name, N):
    if t_.dtype != torch.int32 or t_.dim() != 2 or t_.shape[0] != N or not t_.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 tensor ({N}, width), got {t_.dtype} {tuple(t_.shape)}")
    return t_.shape[1]


def open_drawer_post(rigid_body_all, dof_state_all, root, rigid_body_mask, dof_state_mask, obj_actor, ltip, rtip, part_bbox_init,
                     part_axis_dir_init, joint_lo, joint_hi, dof_lo, dof_hi, suc_prop=0.5, obj_id=None, part_slot=None, part_C=None,
                     normal_state=None, rew=None, success=None, is_reached=None, part_bbox=None, extras=None, succ_objid=None,
                     robot_dof_state=None, part_dof_state=None, pose_R=None, pose_T=None):
    """Everything after physics of the open_drawer task in one launch (pm_open_drawer_post_f32, include/partmanip_hip.h): flat
    rigid_body_all (B, 13) and dof_state_all (D, 2), root (N, na, 13), all contiguous float32, reached through rigid_body_mask
    (N, nrb + 2) and dof_state_mask (N, nd + 1) int32 (the caller guarantees their range: OpenDrawerTensors checks it once).
    Outputs are written in place and every one may be None (skipped): normal_state (N, 29 + 2 nd) and extras (N, 8) may be column
    views of a wider buffer; rew (N); success, is_reached (N) and succ_objid (num_objs, with obj_id (N) int32) bool or uint8;
    part_bbox (N, 8, 3); robot_dof_state (N, nd, 2); part_dof_state (N, 2); pose_R (N, M, 3, 3), pose_T (N, M, 3) with part_slot
    (M) int32 and part_C (M, 3, 3) or None."""
    for t_, name, w in ((rigid_body_all, "rigid_body_all", 13), (dof_state_all, "dof_state_all", 2)):
        _f32c(t_, name)
        if t_.dim() != 2 or t_.shape[1] != w or t_.shape[0] == 0:
            raise ValueError(f"{name}: expected (rows, {w}), got {tuple(t_.shape)}")
    _f32c(root, "root")
    N, na = _root_dims(root)
    B, D = rigid_body_all.shape[0], dof_state_all.shape[0]
    nrb = _index_table(rigid_body_mask, "rigid_body_mask", N) - 2
    nd = _index_table(dof_state_mask, "dof_state_mask", N) - 1
    if nrb < 1 or nd < 1:
        raise ValueError(f"masks: expected widths nrb + 2 >= 3 and nd + 1 >= 2, got {nrb + 2} and {nd + 1}")
    if not (0 <= obj_actor < na and 0 <= ltip < nrb and 0 <= rtip < nrb):
        raise ValueError(f"obj_actor {obj_actor} / ltip {ltip} / rtip {rtip} outside ({na} actors, {nrb} robot bodies)")
    _shape_f32c(part_bbox_init, "part_bbox_init", (N, 8, 3))
    _shape_f32c(part_axis_dir_init, "part_axis_dir_init", (N, 3))
    for t_, name, n in ((joint_lo, "joint_lo", N), (joint_hi, "joint_hi", N), (dof_lo, "dof_lo", nd), (dof_hi, "dof_hi", nd)):
        _vec(t_, name, n)
    num_objs = 0
    if succ_objid is not None:
        if obj_id is None:
            raise ValueError("succ_objid needs obj_id (N) int32")
        num_objs = succ_objid.numel()
        if num_objs == 0:
            raise ValueError("succ_objid: expected at least one object")
        _flags(succ_objid, "succ_objid", num_objs)
    if obj_id is not None:
        _vec(obj_id, "obj_id", N, torch.int32)
    M = _pose_outputs(N, part_slot, "part_slot", part_C, pose_R, pose_T)
    lns = _row_view(normal_state, "normal_state", N, 29 + 2 * nd) if normal_state is not None else 0
    lex = _row_view(extras, "extras", N, 8) if extras is not None else 0
    if rew is not None:
        _vec(rew, "rew", N)
    for t_, name in ((success, "success"), (is_reached, "is_reached")):
        if t_ is not None:
            _flags(t_, name, N)
    for t_, name, shape in ((part_bbox, "part_bbox", (N, 8, 3)), (robot_dof_state, "robot_dof_state", (N, nd, 2)),
                            (part_dof_state, "part_dof_state", (N, 2))):
        if t_ is not None:
            _shape_f32c(t_, name, shape)
    _one_device("open_drawer_post", rigid_body_all, dof_state_all, root, rigid_body_mask, dof_state_mask, part_bbox_init,
                part_axis_dir_init, joint_lo, joint_hi, dof_lo, dof_hi, obj_id, part_slot, part_C, normal_state, rew, success,
                is_reached, part_bbox, extras, succ_objid, robot_dof_state, part_dof_state, pose_R, pose_T)
    with TIMER.bracket("open_drawer_post"):
        check(lib.pm_open_drawer_post_f32(_ptr(rigid_body_all), B, _ptr(dof_state_all), D, _ptr(root), N, nrb, nd, na, int(obj_actor),
                                          int(ltip), int(rtip), _ptr(rigid_body_mask), _ptr(dof_state_mask), _ptr(obj_id), num_objs,
                                          _ptr(part_bbox_init), _ptr(part_axis_dir_init), _ptr(joint_lo), _ptr(joint_hi),
                                          _ptr(dof_lo), _ptr(dof_hi), float(suc_prop), _ptr(part_slot), _ptr(part_C), M,
                                          _ptr(normal_state), lns, _ptr(rew), _ptr(success), _ptr(is_reached), _ptr(part_bbox),
                                          _ptr(extras), lex, _ptr(succ_objid), _ptr(robot_dof_state), _ptr(part_dof_state),
                                          _ptr(pose_R), _ptr(pose_T), _stream()), "pm_open_drawer_post_f32")


def open_drawer_reset(reset, pos_act, dof_state_mask, root, dof_state_all, pos_act_all, robot_actor, obj_actor, robot_default_root,
                      obj_default_root, default_dof_pos, joint_lo, u=None, t_range=0.05, r_range=0.2617993877991494,
                      robot_dof_state=None, part_dof_state=None):
    """The state half of open_drawer.reset_idx in one launch (pm_open_drawer_reset_f32), in place: pos_act (N, nd) is scattered into
    pos_act_all (D) through dof_state_mask (N, nd + 1) int32 for every environment; environments with reset (N) bool / uint8 set get
    their default root rows in root (N, na, 13) (u (N, 4) in [0, 1), when given, perturbs the object's position and yaw), default DOF
    rows in dof_state_all (D, 2) and the same values in robot_dof_state (N, nd, 2) / part_dof_state (N, 2).  dof_state_mask must
    not name a row twice."""
    _f32c(root, "root")
    N, na = _root_dims(root)
    nd = _index_table(dof_state_mask, "dof_state_mask", N) - 1
    if nd < 1:
        raise ValueError(f"dof_state_mask: expected a width nd + 1 >= 2, got {nd + 1}")
    _f32c(dof_state_all, "dof_state_all")
    if dof_state_all.dim() != 2 or dof_state_all.shape[1] != 2 or dof_state_all.shape[0] == 0:
        raise ValueError(f"dof_state_all: expected (D, 2), got {tuple(dof_state_all.shape)}")
    D = dof_state_all.shape[0]
    _flags(reset, "reset", N)
    for t_, name, n in ((pos_act, "pos_act", N * nd), (pos_act_all, "pos_act_all", D), (robot_default_root, "robot_default_root", 7),
                        (obj_default_root, "obj_default_root", 7), (default_dof_pos, "default_dof_pos", nd), (joint_lo, "joint_lo", N)):
        _vec(t_, name, n)
    if not (0 <= robot_actor < na and 0 <= obj_actor < na) or robot_actor == obj_actor:
        raise ValueError(f"robot_actor {robot_actor} / obj_actor {obj_actor}: expected two different actors of {na}")
    if u is not None:
        _shape_f32c(u, "u", (N, 4))
    for t_, name, shape in ((robot_dof_state, "robot_dof_state", (N, nd, 2)), (part_dof_state, "part_dof_state", (N, 2))):
        if t_ is not None:
            _shape_f32c(t_, name, shape)
    _one_device("open_drawer_reset", reset, pos_act, dof_state_mask, root, dof_state_all, pos_act_all, robot_default_root,
                obj_default_root, default_dof_pos, joint_lo, u, robot_dof_state, part_dof_state)
    with TIMER.bracket("open_drawer_reset"):
        check(lib.pm_open_drawer_reset_f32(_ptr(reset), _ptr(pos_act), _ptr(dof_state_mask), N, nd, na, int(robot_actor),
                                           int(obj_actor), _ptr(robot_default_root), _ptr(obj_default_root), 0 if u is None else 1,
                                           _ptr(u), float(t_range), float(r_range), _ptr(default_dof_pos), _ptr(joint_lo), _ptr(root),
                                           _ptr(dof_state_all), D, _ptr(pos_act_all), _ptr(robot_dof_state), _ptr(part_dof_state),
                                           _stream()), "pm_open_drawer_reset_f32")


def mesh_sdf_bake(tri, shape, voxel_size, centre, trunc, tri_cull=True):
    """Signed-distance grid of a triangle mesh (pm_mesh_sdf_bake_f32): tri (F, 3, 3) float32 corner positions, shape = (X, Y, Z),
    voxel (i, j, k) at (idx - shape // 2) * voxel_size + centre (3 floats; fp32, two roundings).  Returns (X, Y, Z) float32:
    clamp(+-distance, -trunc, trunc), negative where |generalised winding number| >= 0.5.  tri_cull=False turns the per-brick
    triangle rejection off (same bits, slower; for tests)."""
    _req(tri)
    _f32c(tri, "tri")
    if tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3) or tri.shape[0] == 0:
        raise ValueError(f"tri: expected (F > 0, 3, 3), got {tuple(tri.shape)}")
    X, Y, Z = (int(v) for v in shape)
    if min(X, Y, Z) <= 0 or X * Y * Z >= 2 ** 31:
        raise ValueError(f"shape: expected three positive sizes with fewer than 2^31 cells, got {(X, Y, Z)}")
    if not (float(voxel_size) > 0 and float(trunc) > 0):
        raise ValueError("voxel_size and trunc must be positive")
    F_ = tri.shape[0]
    cx, cy, cz = (float(v) for v in centre)
    nbytes = lib.pm_mesh_sdf_bake_workspace_bytes(F_)
    with torch.cuda.device(tri.device):
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=tri.device)
        out = torch.empty(X, Y, Z, dtype=torch.float32, device=tri.device)
        with TIMER.bracket("mesh_sdf_bake"):
            check(lib.pm_mesh_sdf_bake_f32(_ptr(tri), F_, X, Y, Z, float(voxel_size), cx, cy, cz, float(trunc), 1 if tri_cull else 0,
                                           _ptr(out), _ptr(ws), nbytes, _stream()), "pm_mesh_sdf_bake_f32")
    return out


def depth_compact(world):
    """world (B,P,3) cropped cloud -> (compact (B,P,3): non-zero points + the first zero point, order kept; lengths (B) i32)."""
    _req(world)
    _f32c(world, "world")
    B, P, _ = world.shape
    out = torch.empty_like(world)
    lengths = torch.empty(B, dtype=torch.int32, device=world.device)
    check(lib.pm_depth_compact_f32(_ptr(world), B, P, _ptr(out), _ptr(lengths), _stream()), "pm_depth_compact_f32")
    return out, lengths


_HIP_RT = [None]


def cu_masked_stream(first, count, total=256):
    """A HIP stream whose kernels may only occupy CU-mask bits [first, first + count) (hipExtStreamCreateWithCUMask), as a
    torch.cuda.ExternalStream.  On the MI355X mask bit i is CU i // 8 of XCD i % 8 -- work-groups are still dealt round-robin over
    ALL eight XCDs, and a mask that leaves an XCD without a CU is ignored (tools/ubench/cu_mask_probe.hip,
    profiles/round6_cu_mask_probe.txt): a mask can split every XCD's CUs between two streams, it cannot give a stream its own
    XCDs / L2s.  hipGraphs replayed into the stream keep the mask.  Never destroyed (process lifetime)."""
    if _HIP_RT[0] is None:
        _HIP_RT[0] = C.CDLL("libamdhip64.so")
        _HIP_RT[0].hipExtStreamCreateWithCUMask.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32)]
        _HIP_RT[0].hipExtStreamCreateWithCUMask.restype = C.c_int
    words = (C.c_uint32 * ((total + 31) // 32))()
    for i in range(first, first + count):
        words[i // 32] |= 1 << (i % 32)
    h = C.c_void_p()
    rc = _HIP_RT[0].hipExtStreamCreateWithCUMask(C.byref(h), len(words), words)
    if rc != 0 or not h.value:
        raise RuntimeError(f"hipExtStreamCreateWithCUMask failed ({rc})")
    return torch.cuda.ExternalStream(h.value)


class FpsConfig(C.Structure):
    """pm_fps_config (include/partmanip_hip.h): the launch policy of the multi-work-group sampler, passed with every call."""
    _fields_ = [("max_groups", C.c_int), ("resident_cus", C.c_int), ("spin_limit", C.c_uint), ("spin_limit_set", C.c_int),
                ("legacy_shape", C.c_int)]


class _FpsPolicy:
    """Process-local policy behind fps_varlen's default (the LIBRARY has no state: this object is turned into a pm_fps_config
    for every call).  max_groups: cap on the work-groups per cloud (None: the library's own; 1: one work-group per cloud);
    resident_cus: the CUs a launch may occupy when the caller masks / shares the device (None: all); spin_limit: the hand-off
    poll budget (None: ~1 s; tests force give-ups with 0); legacy_shape: the round-2 launch shape (A/B).  The PM_FPS_MAXG /
    PM_FPS_SPIN_LIMIT / PM_FM_CFG environment variables of earlier rounds are read ONCE here, at import."""

    def __init__(self):
        e = os.environ
        self.max_groups = int(e["PM_FPS_MAXG"]) if "PM_FPS_MAXG" in e else None
        self.spin_limit = int(e["PM_FPS_SPIN_LIMIT"]) if "PM_FPS_SPIN_LIMIT" in e else None
        self.legacy_shape = e.get("PM_FM_CFG", "1") == "0"
        self.resident_cus = None
        self.gave_up_cap = False                              # set by the watch below: a give-up capped the group count

    def struct(self, max_groups=None, spin_limit=None, resident_cus=None):
        mg = self.max_groups if max_groups is None else max_groups
        sl = self.spin_limit if spin_limit is None else spin_limit
        rc = self.resident_cus if resident_cus is None else resident_cus
        return FpsConfig(-1 if mg is None else int(mg), 0 if rc is None else int(rc), 0 if sl is None else int(sl),
                         0 if sl is None else 1, int(self.legacy_shape))


FPS_POLICY = _FpsPolicy()


def fps_varlen(xyz, lengths, K, ws, pad=False, max_groups=None, spin_limit=None, resident_cus=None):
    """FPS over the first lengths[b] rows of each cloud of xyz (B, ld, D) -> idx (B, K) int32; pad=True: pytorch3d's
    -1 once a cloud is exhausted, pad=False: keep sampling (index 0 repeats), as the full depth cloud would.
    max_groups / spin_limit / resident_cus override FPS_POLICY for this call (see _FpsPolicy)."""
    _req(xyz, lengths)
    _f32c(xyz, "xyz")
    B, ld, Dd = xyz.shape
    idx = torch.empty(B, K, dtype=torch.int32, device=xyz.device)
    nb = int(lib.pm_fps_varlen_workspace_bytes(B, ld))
    w, base, al = None, 0, 0
    if nb:
        w = ws.get(nb + 8)
        base = w.data_ptr()
        al = (-base) % 8
    _fps_watch_poll(ws)
    cfg = FPS_POLICY.struct(max_groups, spin_limit, resident_cus)
    check(lib.pm_fps_varlen_cfg_f32(_ptr(xyz), B, ld, Dd, K, _ptr(lengths), int(pad), _ptr(idx), C.byref(cfg),
                                    (base + al) if w is not None else None, (w.numel() - al) if w is not None else 0, _stream()),
          "pm_fps_varlen_cfg_f32")
    # a multi-work-group launch that gives up degrades on the device (a launch queued behind it re-samples the big clouds when
    # the reservation's last word is set): nothing to check here, no host sync.  fps_varlen_gave_up(ws) reads the word; the
    # watch below copies it to pinned host memory behind the launch and the NEXT call looks at it (no sync either).  Only a call
    # that finds no earlier watch pending arms one (give-ups of the calls in between are seen by fps_varlen_gave_up only), and
    # none is armed inside a stream capture (the pinned copy and the event are not capturable work).
    multi = nb and int(lib.pm_fps_varlen_groups_cfg(B, ld, Dd, C.byref(cfg))) >= 2
    ws.fps_err = w[al + nb - 8: al + nb].view(torch.int64) if multi else None
    if ws.fps_err is not None and getattr(ws, "_fps_watch", None) is None and not torch.cuda.is_current_stream_capturing():
        host = torch.empty(1, dtype=torch.int64, pin_memory=True)
        host.copy_(ws.fps_err, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ws._fps_watch = (host, ev, cfg.spin_limit_set != 0)                        # (a forced budget -- a test: report, do not act)
    return idx


_FPS_GIVE_UPS = [0]


def _fps_watch_poll(ws):
    """A multi-work-group FPS launch that gave up costs its whole spin budget (~1 s) before the one-work-group sampler redoes the
    clouds -- correct, but silent.  The give-up word of an earlier call on this workspace, copied to the host behind that call:
    once it has arrived and is set, say so and cap FPS_POLICY.max_groups at 1 for the rest of the process (a module-level flag
    that every later call PASSES to the library -- nothing in the environment or the library changes; not when that call ran
    with a forced spin budget: the tests' way to provoke give-ups)."""
    watch = getattr(ws, "_fps_watch", None)
    if watch is None or not watch[1].query():
        return
    ws._fps_watch = None
    if int(watch[0][0]) != 0:
        _FPS_GIVE_UPS[0] += 1
        if not watch[2] and FPS_POLICY.max_groups != 1:
            import warnings
            warnings.warn("pm_fps_varlen_cfg_f32: a multi-work-group sampling launch gave up waiting for its partner work-groups (the "
                          "device is shared or CU-masked?) and fell back to one work-group per cloud; ops.FPS_POLICY.max_groups = 1 "
                          "from now on (pass resident_cus to keep the multi-work-group path on a masked device)")
            FPS_POLICY.max_groups = 1
            FPS_POLICY.gave_up_cap = True


def fps_varlen_gave_up(ws):
    """Diagnostics (a host read): did the last multi-work-group fps_varlen call on this workspace fall back to the
    one-work-group sampler because a work-group's partners were not resident?"""
    e = getattr(ws, "fps_err", None)
    return bool(e is not None and int(e.item()) != 0)


def tsdf_sparse_voxel(vol, K, lo, hi, ws):
    """vol (B, res, res, res) -> (B, K, 4) rows (x, y, z, tsdf) of FPS-sampled voxels with lo < tsdf < hi."""
    _req(vol)
    _f32c(vol, "vol")
    B, res = vol.shape[0], vol.shape[1]
    V = res ** 3
    coords = torch.empty(B, V, 3, dtype=torch.float32, device=vol.device)
    lengths = torch.empty(B, dtype=torch.int32, device=vol.device)
    check(lib.pm_tsdf_select_f32(_ptr(vol), B, res, float(lo), float(hi), _ptr(coords), _ptr(lengths), _stream()),
          "pm_tsdf_select_f32")
    idx = fps_varlen(coords, lengths, K, ws, pad=True)
    out = torch.empty(B, K, 4, dtype=torch.float32, device=vol.device)
    check(lib.pm_tsdf_sparse_gather_f32(_ptr(coords), _ptr(idx), _ptr(vol), B, res, K, _ptr(out), _stream()),
          "pm_tsdf_sparse_gather_f32")
    return out


def gaussian_sample(mu, log_std, eps, max_action, act_tanh, want_log_std_rows=True):
    """actor_critic.py:36-47 after the forwards: -> (squashed actions (B, A), logp (B,), log_std rows (B, A))."""
    _req(mu, log_std, eps)
    _f32c(eps, "eps")
    B, A = mu.shape
    actions = torch.empty(B, A, dtype=torch.float32, device=mu.device)
    logp = torch.empty(B, dtype=torch.float32, device=mu.device)
    rows = torch.empty(B, A, dtype=torch.float32, device=mu.device) if want_log_std_rows else None
    check(lib.pm_gaussian_sample_f32(_ptr(mu), _rows(mu, "mu"), _ptr(log_std), _ptr(eps), B, A, float(max_action),
                                     int(act_tanh), _ptr(actions), _ptr(logp), _ptr(rows), _stream()),
          "pm_gaussian_sample_f32")
    return actions, logp, rows


def rms_update(x, n_new, mean, S, std, ws):
    """RMS.py:10-18 for one (N, D) batch; mean / S / std ((1, D) fp32, contiguous) are updated in place."""
    _req(x, mean, S, std)
    N, D = x.shape
    w = ws.get(lib.pm_rms_update_workspace_bytes(D))
    check(lib.pm_rms_update_f32(_ptr(x), _rows(x, "x"), N, D, int(n_new), _ptr(mean), _ptr(S), _ptr(std), _ptr(w),
                                w.numel(), _stream()), "pm_rms_update_f32")


def rms_update_dp(x, n_new, mean, S, std, ws, mom, sum_over_ranks, world):
    """The same update when the batch is sharded over `world` ranks: local column moments -> `sum_over_ranks(mom)`
    (one all-reduce of 2*D doubles) -> RMS.py:10-18 from the global moments over N * world rows."""
    _req(x, mean, S, std, mom)
    N, D = x.shape
    w = ws.get(lib.pm_rms_update_workspace_bytes(D))
    check(lib.pm_rms_moments_f64(_ptr(x), _rows(x, "x"), N, D, _ptr(mom), _ptr(w), w.numel(), _stream()), "pm_rms_moments_f64")
    sum_over_ranks(mom)
    check(lib.pm_rms_apply_moments_f32(_ptr(mom), N * world, D, int(n_new), _ptr(mean), _ptr(S), _ptr(std), _stream()),
          "pm_rms_apply_moments_f32")


def rms_normalize(x, mean, std):
    _req(x, mean, std)
    N, D = x.shape
    out = torch.empty(N, D, dtype=torch.float32, device=x.device)
    check(lib.pm_rms_normalize_f32(_ptr(x), _rows(x, "x"), N, D, _ptr(mean), _ptr(std), _ptr(out), D, _stream()),
          "pm_rms_normalize_f32")
    return out
