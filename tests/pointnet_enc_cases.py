"""What the op-level PointNet encoder tests share (tests/test_pointnet_enc_cases_host.py, tests/test_gpu_pointnet_enc_variants.py):
the list of kernel instantiations the host code can launch, the cases and which of them each one runs, a float64 restatement
of the forward and of the backward with the pooling index GIVEN, integer data on which every float32 summation order is exact,
the arg-max tables handed to the backward, and the int32 sentinel buffer of `argmax`.  Nothing here touches the GPU at import."""
import functools

import numpy as np
import torch

from tests.exact_gemm import SENT, GUARD, TANH, RELU, ELU, DEV       # noqa: F401  (the poisoned float buffers are exact_gemm's)

C1, C2, C3 = 128, 256, 512
BWD_MAXG = 512                               # PN_BWD_MAXG: pn_bwd_kernel's grid limit
AM_SENT = -777                               # what an untouched int32 of an argmax buffer holds
ACT_NAME = {TANH: "tanh", RELU: "relu", ELU: "elu"}


# ------------------------------------------------------------------------------------------------ kernel coverage list
# Written by hand from the launch macros of the host code, one key per instantiation they can name:
#   pointnet_enc.hip       PN_FWD_LAUNCH(CT)    pn_fwd_kernel<CT, PN_FWD_NW, TANH>           CT in 3, 4, 0 (any other C); TANH = act == tanh
#   pointnet_enc_screen.h  PS_LAUNCH(CT, S)     pn_fwd_screen_kernel<CT, S>                  S = schedule 0, 1 (tanh only)
#   pointnet_enc_bf3.hip   B3_LAUNCH(CT)        pn_fwd_bf3_kernel<CT>                        (tanh only)
#   pointnet_enc_bf6.hip   B6_LAUNCH(CT)        pn_fwd_bf6_kernel<CT>                        (tanh only)
#   pointnet_enc.hip       PN_BWD_LAUNCH(CT)    pn_bwd_kernel<CT, SAVED, TANH>               SAVED = h2_saved given; with PN_BWD16 == 1 a saved
#                                                                                            layer 2 reaches it through pm_pointnet_enc_bwd_w4_f32 only
#                          PN_BWD16_LAUNCH(CT)  pn_bwd16_kernel<CT, TANH>                    h2_saved given, pm_pointnet_enc_bwd_f32
#                          PN_BF6_LAUNCH(CT)    pn_bwd_bf6_kernel<CT>                        (tanh, h2_saved given)
CTS = (3, 4, 0)
FWD_KERNELS = ([f"pn_fwd_kernel<{ct},{th}>" for ct in CTS for th in ("tanh", "generic")]
               + [f"pn_fwd_screen_kernel<{ct},{s}>" for ct in CTS for s in (0, 1)]
               + [f"pn_fwd_bf3_kernel<{ct}>" for ct in CTS] + [f"pn_fwd_bf6_kernel<{ct}>" for ct in CTS])
BWD_KERNELS = ([f"pn_bwd_kernel<{ct},{sv},{th}>" for ct in CTS for sv in ("saved", "recompute") for th in ("tanh", "generic")]
               + [f"pn_bwd16_kernel<{ct},{th}>" for ct in CTS for th in ("tanh", "generic")]
               + [f"pn_bwd_bf6_kernel<{ct}>" for ct in CTS])


def ct_of(C):
    return C if C in (3, 4) else 0


def fwd_entries(c):
    """The forward entry points a case runs: (name, kernel key)."""
    ct, th = ct_of(c["C"]), "tanh" if c["act"] == TANH else "generic"
    out = [("f32", f"pn_fwd_kernel<{ct},{th}>")]
    if c["act"] == TANH:
        out += [("screen0", f"pn_fwd_screen_kernel<{ct},0>"), ("screen1", f"pn_fwd_screen_kernel<{ct},1>"), ("bf6", f"pn_fwd_bf6_kernel<{ct}>")]
        if c["P"] % 128 == 0:
            out.append(("bf3", f"pn_fwd_bf3_kernel<{ct}>"))
    return out


def bwd_entries(c):
    """The backward entry points a case runs: (name, kernel key).  saved16: pm_pointnet_enc_bwd_f32 with h2_saved; recompute: without;
    saved4: pm_pointnet_enc_bwd_w4_f32 with h2_saved; bf6: pm_pointnet_enc_bwd_bf6."""
    ct, th = ct_of(c["C"]), "tanh" if c["act"] == TANH else "generic"
    out = [("saved16", f"pn_bwd16_kernel<{ct},{th}>"), ("recompute", f"pn_bwd_kernel<{ct},recompute,{th}>"),
           ("saved4", f"pn_bwd_kernel<{ct},saved,{th}>")]
    if c["act"] == TANH:
        out.append(("bf6", f"pn_bwd_bf6_kernel<{ct}>"))
    return out


# ------------------------------------------------------------------------------------------------ the cases
# Arg-max tables of the backward, one letter per cloud (cloud b of a case gets TABLES[(rot + b) % 7]):
#   a  all 512 channels at point 0                     b  all at point P - 1
#   c  channel c at point c % P                        d  channels alternating between points 6 and 7 (one row block, a run of 512)
#   e  the first-index arg-max of the case's own forward
#   f  e, and the cloud's dfeat row all zero           g  e, with dmax == 0 and only dmean set
TABLES = "abcdefg"


def tables_of(c, B):
    return [TABLES[(c["rot"] + b) % len(TABLES)] for b in range(B)]


def _case(tier, P, B, C, sub_mean, max_mean, ldf, seed, rot=None, **kw):
    act = RELU if tier == "exact" else TANH
    d = dict(tier=tier, P=P, B=B, C=C, act=act, sub_mean=sub_mean, max_mean=max_mean, ldf=ldf, seed=seed, rot=rot, tail=kw.pop("tail", 5), **kw)
    d["id"] = f"{tier}-P{P}-B{B}-C{C}-sub{int(sub_mean)}-mm{int(max_mean)}-ldf{ldf}" + ("" if rot is None else f"-rot{rot}")
    return d


# B: a number, or "cu+3" (the device's CU count + 3: a work-group of the one-group-per-CU kernels walks two clouds, most walk one)
# ldx = P * C + tail in every case (the tail is NaN); ldf is 1024 or larger.
EXACT_FWD = [_case("exact", 64, 3, C, True, True, 1024, 100 + C) for C in (3, 4, 6)] \
    + [_case("exact", 128, 3, C, False, False, 1536, 110 + C) for C in (3, 4, 6)] \
    + [_case("exact", 512, 1, C, True, True, 1100, 120 + C, tail=1) for C in (3, 4, 6)] \
    + [_case("exact", 4096, 1, C, False, True, 1024, 130 + C) for C in (3, 4, 6)]
EXACT_BWD = [_case("exact", 64, 3, 3, True, True, 1024, 200, rot) for rot in (0, 3, 6)] \
    + [_case("exact", 128, 3, 4, False, True, 1536, 210, rot) for rot in (0, 3, 6)] \
    + [_case("exact", 512, 3, 6, True, True, 1100, 220, rot) for rot in (0, 3, 6)] \
    + [_case("exact", 128, 1, 3, False, False, 1024, 230, 4)] \
    + [_case("exact", 4096, 1, 3, False, True, 1024, 240, rot) for rot in range(7)] \
    + [_case("exact", 64, "cu+3", 4, True, True, 1024, 250, 0), _case("exact", 64, BWD_MAXG + 3, 6, False, True, 1024, 260, 0)]
F64_FWD = [_case("fp64", 64, 3, 3, True, True, 1024, 300), _case("fp64", 128, 3, 4, False, True, 1536, 311),
           _case("fp64", 128, 3, 6, True, True, 1024, 312), _case("fp64", 320, 3, 6, True, False, 1024, 320),
           _case("fp64", 512, 1, 3, False, True, 1100, 330), _case("fp64", 4096, 1, 4, True, True, 1024, 340)]
F64_BWD = [_case("fp64", 64, 3, 3, True, True, 1024, 400, rot) for rot in (0, 3, 6)] \
    + [_case("fp64", 128, 3, 4, False, True, 1536, 410, rot) for rot in (0, 3, 6)] \
    + [_case("fp64", 320, 3, 6, True, False, 1024, 420, 2)] \
    + [_case("fp64", 512, 3, 6, True, True, 1100, 430, rot) for rot in (0, 3, 6)] \
    + [_case("fp64", 4096, 1, 3, False, True, 1024, 440, rot) for rot in range(7)] \
    + [_case("fp64", 64, "cu+3", 4, True, True, 1024, 450, 0), _case("fp64", 64, BWD_MAXG + 3, 6, False, True, 1024, 460, 0)]
NONFINITE = _case("exact", 512, 3, 3, False, True, 1024, 500)      # the clean base of the NaN / inf tests (ReLU and ELU)


def batch(c, cu=256):
    return cu + 3 if c["B"] == "cu+3" else c["B"]


# ------------------------------------------------------------------------------------------------ float64 restatement
def _act(z, act):
    if act == TANH:
        return torch.tanh(z)
    if act == RELU:
        return torch.relu(z)
    if act == ELU:
        return torch.nn.functional.elu(z)
    raise ValueError(act)


def _dact(h, act):
    """The derivative through the OUTPUT h (common.h pm_dact)."""
    if act == TANH:
        return 1.0 - h * h
    if act == RELU:
        return (h > 0).to(h.dtype)
    if act == ELU:
        return torch.where(h > 0, torch.ones_like(h), h + 1.0)
    raise ValueError(act)


def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def centre(x, sub_mean):
    """network.py:172-173: the first three coordinates minus their mean over the cloud."""
    if not sub_mean:
        return x
    return torch.cat([x[..., :3] - x[..., :3].mean(dim=1, keepdim=True), x[..., 3:]], dim=-1)


def forward64(x, W1, b1, W2, b2, W3, b3, act, sub_mean, max_mean, dtype=torch.float64):
    """x (B, P, C) -> dict of numpy arrays: h2 (B, P, 256), z3 (B, P, 512), max (B, 512), argmax (B, 512; the first index of the
    maximum, a NaN counting as the maximum: numpy's argmax), mean (B, 512) or None."""
    x, W1, b1, W2, b2, W3, b3 = (_t(a, dtype) for a in (x, W1, b1, W2, b2, W3, b3))
    h1 = _act(centre(x, sub_mean) @ W1.t() + b1, act)
    h2 = _act(h1 @ W2.t() + b2, act)
    z3 = (h2 @ W3.t() + b3).numpy()
    am = np.argmax(z3, axis=1)
    return dict(h2=h2.numpy(), z3=z3, max=np.take_along_axis(z3, am[:, None, :], 1)[:, 0], argmax=am,
                mean=z3.mean(axis=1) if max_mean else None)


def backward64(x, weights, act, sub_mean, max_mean, argmax, dfeat, h2=None, dtype=torch.float64, parts=False):
    """The six gradients of sum(dfeat * feat), feat = [z3[b, argmax[b, c], c] | mean_p z3[b, p, c]], with the pooling index GIVEN.
    The comment above the backward in pointnet_enc.hip as matrix algebra:
        G[b, p, c] = dmean[b, c] / P + dmax[b, c] [p == argmax[b, c]]
        dW3 = G^T h2   db3 = sum G   dh2 = G W3   dz2 = dh2 .* act'(h2)   dW2 = dz2^T h1   db2 = sum dz2
        dh1 = dz2 W2   dz1 = dh1 .* act'(h1)      dW1 = dz1^T xc          db1 = sum dz1      (sums over all B * P points)
    h2: use these layer-2 activations instead of recomputing them.  weights: (W1, b1, W2, b2, W3, b3).  dtype float32 gives the
    yardstick: the same algebra evaluated by torch on the CPU in float32.  parts: also return G, h1, h2, dz2, dz1, xc."""
    W1, b1, W2, b2, W3, b3 = (_t(a, dtype) for a in weights)
    x, dfeat = _t(x, dtype), _t(dfeat, dtype)
    B, P, _ = x.shape
    xc = centre(x, sub_mean)
    h1 = _act(xc @ W1.t() + b1, act)
    h2 = _act(h1 @ W2.t() + b2, act) if h2 is None else _t(h2, dtype).reshape(B, P, C2)
    G = (dfeat[:, None, C3:2 * C3] / P).expand(B, P, C3).clone() if max_mean else torch.zeros(B, P, C3, dtype=dtype)
    am = _t(argmax, torch.int64)
    G.scatter_add_(1, am[:, None, :], dfeat[:, None, :C3].contiguous())
    G2, h1f, h2f, xf = G.reshape(-1, C3), h1.reshape(-1, C1), h2.reshape(-1, C2), xc.reshape(B * P, -1)
    dz2 = (G2 @ W3) * _dact(h2f, act)
    dz1 = (dz2 @ W2) * _dact(h1f, act)
    out = dict(dW1=dz1.t() @ xf, db1=dz1.sum(0), dW2=dz2.t() @ h1f, db2=dz2.sum(0), dW3=G2.t() @ h2f, db3=G2.sum(0))
    out = {k: v.numpy() for k, v in out.items()}
    if parts:
        out.update(G=G2.numpy(), h1=h1f.numpy(), h2=h2f.numpy(), dz2=dz2.numpy(), dz1=dz1.numpy(), xc=xf.numpy())
    return out


GRADS = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


# ------------------------------------------------------------------------------------------------ data
def _sparse(rng, shape, density):
    return (rng.integers(0, 2, size=shape) * 2 - 1) * (rng.random(shape) < density)


def exact_data(c, cu=256):
    """Integer data for the ReLU kernels: points in [-2, 2], W1 dense in {-1, 0, 1}, W2 / W3 in {-1, 0, 1} at densities 1/8 and
    1/16, biases in {-1, 0, 1}, dmax in [-2, 2], dmean = P x an integer in [-1, 1]; P a power of two.  Duplicated points give
    the forward exact ties of every kind (beside those the small integers give anyway): 5 == 37 (one 64-point tile, 32 apart: the lane-half exchange), 5 == 69 (two tiles,
    where P > 64) and 0 == P - 1; with sub_mean every coordinate sum of a cloud is a multiple of P (an integer centre)."""
    B, P, C = batch(c, cu), c["P"], c["C"]
    assert P & (P - 1) == 0
    rng = np.random.default_rng(c["seed"])
    x = rng.integers(-2, 3, size=(B, P, C))
    x[:, 0] = 2 * (-1) ** np.arange(C)                               # an extreme point: it wins channels, and ties point P - 1
    x[:, 37] = x[:, 5]
    x[:, P - 1] = x[:, 0]
    fixed = np.zeros(P, dtype=bool)
    fixed[[0, 5, 37, P - 1]] = True
    if P > 64:
        x[:, 69] = x[:, 5]
        fixed[69] = True
    if c["sub_mean"]:
        for b in range(B):
            for d in range(3):
                r = int(x[b, :, d].sum()) % P
                r = r - P if r > P // 2 else r                       # remove r: |r| <= P / 2 steps of one
                step = -1 if r > 0 else 1
                ok = np.flatnonzero(~fixed & (x[b, :, d] + step >= -2) & (x[b, :, d] + step <= 2))[:abs(r)]
                assert len(ok) == abs(r), (c["id"], b, d, r)
                x[b, ok, d] += step
                assert int(x[b, :, d].sum()) % P == 0
    w = (rng.integers(-1, 2, size=(C1, C)), rng.integers(-1, 2, size=C1), _sparse(rng, (C2, C1), 1 / 8), rng.integers(-1, 2, size=C2),
         _sparse(rng, (C3, C2), 1 / 16), rng.integers(-1, 2, size=C3))
    w[4][7] = 0                                                      # a constant channel: all P points tie, point 0 must win
    dfeat = np.concatenate([rng.integers(-2, 3, size=(B, C3)), P * rng.integers(-1, 2, size=(B, C3))], axis=1)
    if not c["max_mean"]:
        dfeat = dfeat[:, :C3]
    return dict(x=x.astype(np.float64), w=tuple(a.astype(np.float64) for a in w), dfeat=dfeat.astype(np.float64))


def float_data(c, cu=256):
    """Default-initialised shared MLP, clouds from the distribution of test_pointnet_forward_backward, random float dfeat."""
    B, P, C = batch(c, cu), c["P"], c["C"]
    torch.manual_seed(c["seed"])
    lin = [torch.nn.Linear(C, C1), torch.nn.Linear(C1, C2), torch.nn.Linear(C2, C3)]
    w = tuple(getattr(m, a).detach().numpy().copy() for m in lin for a in ("weight", "bias"))
    g = torch.Generator().manual_seed(c["seed"] + 1)
    x = torch.rand(B, P, C, generator=g) * 2 - 1 + (torch.rand(B, 1, C, generator=g) - 0.5)
    dfeat = torch.randn(B, C3 * (2 if c["max_mean"] else 1), generator=g)
    return dict(x=x.numpy(), w=w, dfeat=dfeat.numpy())


def apply_tables(c, dfeat, own_argmax):
    """(argmax (B, 512) int32 with every value in [0, P), dfeat with the rows of tables f / g edited) of a backward case."""
    B, P = own_argmax.shape[0], c["P"]
    ch = np.arange(C3)
    am, df = np.empty((B, C3), dtype=np.int32), dfeat.copy()
    for b, t in enumerate(tables_of(c, B)):
        am[b] = {"a": np.zeros(C3), "b": np.full(C3, P - 1), "c": ch % P, "d": 6 + (ch & 1)}.get(t, own_argmax[b])
        if t == "f":
            df[b] = 0
        if t == "g":
            df[b, :C3] = 0
    assert am.min() >= 0 and am.max() < P
    return am, df


@functools.lru_cache(maxsize=4)
def reference(cid, cu=256):
    """Data, float64 forward, tables and float64 backward of a case, computed once (the arrays are shared: leave them unchanged).
    The backward of an fp64 case is NOT here: it takes the float32 h2 the device forward saved."""
    c = BY_ID[cid]
    d = exact_data(c, cu) if c["tier"] == "exact" else float_data(c, cu)
    d["fwd"] = forward64(d["x"], *d["w"], c["act"], c["sub_mean"], c["max_mean"])
    if c["rot"] is not None:
        d["argmax"], d["dfeat_t"] = apply_tables(c, d["dfeat"], d["fwd"]["argmax"])
        if c["tier"] == "exact":
            d["bwd"] = backward64(d["x"], d["w"], c["act"], c["sub_mean"], c["max_mean"], d["argmax"], d["dfeat_t"], parts=True)
    for v in list(d.values()) + list(d["fwd"].values()) + list(d.get("bwd", {}).values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


ALL = EXACT_FWD + EXACT_BWD + F64_FWD + F64_BWD + [NONFINITE]
BY_ID = {c["id"]: c for c in ALL}
assert len(BY_ID) == len(ALL)


# The NaN-row Linear checks: cases of tests/linear_variant_cases.py by id -> the path they select
LINEAR_NAN_SHAPES = {"fwd-skinny-M256-N16": "skinny", "fwd-reg64-vec-M65-N63-K36": "reg", "fwd-dma64-M65-N63-K64": "dma"}


# ------------------------------------------------------------------------------------------------ the int32 argmax buffer
def argmax_buffer(B):
    """(buffer, view): a contiguous (B, 512) int32 view inside a buffer of AM_SENT, GUARD words before it and two rows + GUARD after."""
    buf = torch.full((GUARD + (B + 2) * C3 + GUARD,), AM_SENT, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + B * C3].view(B, C3)


def argmax_outside_intact(buf, B):
    a = buf.cpu().numpy()
    return bool((a[:GUARD] == AM_SENT).all() and (a[GUARD + B * C3:] == AM_SENT).all())
