"""Every dispatched kernel of the Linear GEMM family against answers known to the bit.

The kernels multiply with v_mfma_f32_32x32x2_f32 or fp32 FMA chains; with integer operands in [-3, 3] every product and every
partial sum is an integer below 2^24, exact in any order, so forward pre-activations, data gradients and weight / bias gradients
are compared with a float64 matmul on the CPU with NO tolerance.  Each case of tests/linear_variant_cases.py names the variant
it selects, and the test first asks the selector (with the real tensors) that this is what runs.

Every operand is a view inside a larger buffer that is NaN everywhere else (a guard band before and after, the columns between the
width and the row stride, two rows after the last); every result is a view inside a buffer of the sentinel -777.25, which must
survive everywhere outside the view (the gaps between rows and between the slabs of a grouped weight gradient included).
"""
import zlib

import numpy as np
import pytest
import torch

from tests import linear_variant_cases as LV
from tests.exact_gemm import (ACT_NAMES, DEV, DOCUMENTED_ULP, ELU, GUARD, LRELU, NONE, RELU, SELU, SELU_A, SELU_L, SENT, SIGMOID, TANH, _act64,
                              _act_torch32, _dact64, _input, _ints, _mm, _outside_intact, _ulps, _view)
from tests.helpers import record_margin, same_bits

pytestmark = pytest.mark.gpu


def _cases(*kinds):
    sel = [c for c in LV.CASES if c["kind"] in kinds]
    return pytest.mark.parametrize("c", sel, ids=[c["id"] for c in sel])


@pytest.fixture(scope="module")
def o():
    from partmanip_amd import ops
    return ops


def _rng(c):
    return np.random.default_rng(zlib.crc32(c["id"].encode()))


def _ld(kind, p, name):
    return p["ld"].get(name, LV.operand_shape(kind, name, p)[-1])


def _check_selected(o, c, tensors, act, slab_strides=None):
    """The selector, asked with the tensors the launch gets, names the variant the case is meant to run."""
    kind = c["kind"]
    descs = [LV.query_problem(kind, p, lambda n, t=t: t[n], act, (slab_strides or [0] * len(tensors))[i])
             for i, (p, t) in enumerate(zip(c["probs"], tensors))]
    got = o.linear_variant(kind, descs, splits=c["splits"]) if kind.endswith("_group") else o.linear_variant(kind, descs[0])
    want = c["expect" if act else "expect_noact"]
    assert {k: got[k] for k in want} == want, (c["id"], act, got)
    return got


# ------------------------------------------------------------------------------------------------ forward
@_cases("fwd", "fwd_group")
def test_forward(o, c):
    """act NONE and RELU: the bits of the float64 reference.  TANH: the bound test_fast_tanh_accuracy pins (< 6 ulp, < 3e-7) against
    float64 tanh of the exact pre-activation.  LRELU / ELU / SELU / SIGMOID: within max(4 e_ref, the documented libm figure), e_ref
    being the worst ulp error of torch's float32 CPU evaluation on the same z; observed / allowed of every case are recorded.
    (Measured in units of 2^-23 max(|ref|, 1e-30) like test_fast_tanh_accuracy: a sigmoid below 1e-38, where the kernel's 1 / (1 + inf)
    is 0 and torch returns a denormal, counts as exact.)"""
    rng, group = _rng(c), c["kind"].endswith("_group")
    data, tens = [], []
    for p in c["probs"]:
        M, N, K = p["M"], p["N"], p["K"]
        X, W, b = _ints(rng, (M, K)), _ints(rng, (N, K)), _ints(rng, (N,), -5, 5)
        assert (np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T).max() + np.abs(b).max() < 2 ** 24
        z = (_mm(X, W.T) + b.astype(np.float64)).astype(np.float32)
        data.append(z)
        tens.append(dict(X=_input(X, _ld("fwd", p, "X"), p["off"].get("X", 0)), W=_input(W, _ld("fwd", p, "W"), p["off"].get("W", 0)),
                         b=_input(b, N, p["off"].get("b", 0))))
    worst = {}                                   # activation -> (observed ulp error, allowed) of the problem nearest to its bound
    for act in (NONE, RELU, TANH, LRELU, ELU, SELU, SIGMOID):
        outs = [_view((p["M"], p["N"]), _ld("fwd", p, "Y"), p["off"].get("Y", 0), SENT) for p in c["probs"]]
        for t, (_, y) in zip(tens, outs):
            t["Y"] = y
        if act == NONE:
            _check_selected(o, c, tens, 1)
        items = [(t["X"], t["W"], t["b"], t["Y"], act) for t in tens]
        if group:
            o.linear_fwd_group(items)
        else:
            o.linear_fwd(*items[0])
        for i, (p, z, (buf, y)) in enumerate(zip(c["probs"], data, outs)):
            got = y.cpu().numpy()
            assert _outside_intact(buf, [(GUARD + p["off"].get("Y", 0), p["M"], p["N"], _ld("fwd", p, "Y"))]), (c["id"], i, act)
            if act == NONE:
                assert same_bits(got, z), (c["id"], i, "none")
            elif act == RELU:
                assert same_bits(got, np.maximum(z, np.float32(0))), (c["id"], i, "relu")
            else:
                assert np.isfinite(got).all(), (c["id"], i, ACT_NAMES[act])
                ref = _act64(z, act)
                u = float(_ulps(got, ref).max())
                if act == TANH:
                    allowed = 6.0
                    assert float(np.abs(got.astype(np.float64) - ref).max()) < 3e-7
                else:
                    allowed = max(4.0 * float(_ulps(_act_torch32(z, act), ref).max()), DOCUMENTED_ULP[act])
                if act not in worst or u * worst[act][1] > worst[act][0] * allowed:
                    worst[act] = (u, allowed)
                print(f"{c['id']} problem {i} {ACT_NAMES[act]}: {u:.3f} ulp, allowed {allowed:.3f}")
                assert u < allowed if act == TANH else u <= allowed, (c["id"], i, ACT_NAMES[act], u, allowed)
    for act, (u, allowed) in worst.items():
        if allowed > 0:
            record_margin(f"linear variants: forward {ACT_NAMES[act]} ulp error against float64 of the exact z", u, allowed,
                          unit="ulp; allowed = 6 (tanh) or max(4 e_ref, libm's documented 1 ulp)")


# ------------------------------------------------------------------------------------------------ data gradient
@_cases("bwd_data", "bwd_data_group")
def test_data_gradient(o, c):
    """dX = (dY W) .* act'(H) with H dyadic (multiples of 1/8 in [-1, 1]; in [0, 1] for sigmoid): 1 - h^2, h + 1 and h (1 - h) are
    multiples of 1/64 and their products with the integer dY W exact, so NONE / RELU / TANH / ELU / SIGMOID must give the reference's
    bits.  LRELU and SELU multiply the exact integer by a rounded constant (SELU's negative branch rounds h + lambda alpha first): the
    same one or two float32 operations in numpy, within 2 ulp (at most two roundings apart)."""
    rng, group = _rng(c), c["kind"].endswith("_group")
    data, tens = [], []
    for p in c["probs"]:
        M, N, K = p["M"], p["N"], p["K"]
        dY, W = _ints(rng, (M, N)), _ints(rng, (N, K))
        H = _ints(rng, (M, K), -8, 8) / np.float32(8)
        assert 9 * N * 64 < 2 ** 24
        s = _mm(dY, W)
        data.append((s, H))
        tens.append(dict(dY=_input(dY, _ld("bwd_data", p, "dY"), p["off"].get("dY", 0)), W=_input(W, _ld("bwd_data", p, "W"), p["off"].get("W", 0)),
                         H=_input(H, _ld("bwd_data", p, "H"), p["off"].get("H", 0)),
                         Hs=_input(np.abs(H), _ld("bwd_data", p, "H"), p["off"].get("H", 0))))
    for act in (NONE, RELU, TANH, ELU, SIGMOID, LRELU, SELU):
        outs = [_view((p["M"], p["K"]), _ld("bwd_data", p, "dX"), p["off"].get("dX", 0), SENT) for p in c["probs"]]
        hk = "Hs" if act == SIGMOID else "H"
        for t, (_, dx) in zip(tens, outs):
            t["dX"] = dx
        if act in (NONE, TANH):
            _check_selected(o, c, [dict(t, H=t[hk]) for t in tens], act)
        items = [(t["dY"], t["W"], t[hk] if act else None, t["dX"], act) for t in tens]
        if group:
            o.linear_bwd_data_group(items)
        else:
            o.linear_bwd_data(*items[0])
        for i, (p, (s, H), (buf, dx)) in enumerate(zip(c["probs"], data, outs)):
            got = dx.cpu().numpy()
            h = np.abs(H) if act == SIGMOID else H
            assert _outside_intact(buf, [(GUARD + p["off"].get("dX", 0), p["M"], p["K"], _ld("bwd_data", p, "dX"))]), (c["id"], i, act)
            if act in (LRELU, SELU):
                s32 = s.astype(np.float32)
                if act == LRELU:
                    d = np.where(h > 0, np.float32(1), np.float32(0.01)).astype(np.float32)
                else:
                    d = np.where(h > 0, SELU_L, h + SELU_L * SELU_A).astype(np.float32)
                ref = s32 * d
                assert ref.dtype == np.float32
                err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
                assert (err <= 2 * np.spacing(np.abs(ref)).astype(np.float64)).all(), (c["id"], i, ACT_NAMES[act], float(err.max()))
            else:
                ref = (s * _dact64(h, act)).astype(np.float32)
                assert same_bits(got, ref), (c["id"], i, ACT_NAMES[act], int((got != ref).sum()))


# ------------------------------------------------------------------------------------------------ weight gradient
@_cases("bwd_weight")
def test_weight_gradient(o, c):
    """dW = dY^T X and db = column sums of dY from the single call (which reduces its own slabs): the reference's bits."""
    rng, p = _rng(c), c["probs"][0]
    M, N, K = p["M"], p["N"], p["K"]
    dY, X = _ints(rng, (M, N)), _ints(rng, (M, K))
    assert (np.abs(dY).astype(np.float64).T @ np.abs(X).astype(np.float64)).max() < 2 ** 24 and 3 * M < 2 ** 24
    t = dict(dY=_input(dY, _ld("bwd_weight", p, "dY"), p["off"].get("dY", 0)), X=_input(X, _ld("bwd_weight", p, "X"), p["off"].get("X", 0)))
    (wbuf, t["dW"]), (bbuf, t["db"]) = _view((N, K), _ld("bwd_weight", p, "dW"), p["off"].get("dW", 0), SENT), _view((N,), N, p["off"].get("db", 0), SENT)
    ws = o.Workspace(torch.device(DEV))
    _check_selected(o, c, [t], 1)
    o.linear_bwd_weight(t["dY"], t["X"], t["dW"], t["db"], ws)
    assert same_bits(t["dW"].cpu().numpy(), _mm(dY.T, X).astype(np.float32)), c["id"]
    assert same_bits(t["db"].cpu().numpy(), (dY.astype(np.float64).sum(0) + 0.0).astype(np.float32)), c["id"]
    assert _outside_intact(wbuf, [(GUARD + p["off"].get("dW", 0), N, K, _ld("bwd_weight", p, "dW"))]), c["id"]
    assert _outside_intact(bbuf, [(GUARD + p["off"].get("db", 0), 1, N, N)]), c["id"]


@_cases("bwd_weight_group")
def test_weight_gradient_group(o, c):
    """The grouped call leaves slab z of dW / db at + z * slab_stride: every slab is the exact gradient of its own range of
    kchunk batch rows, their sum in slab order (float32) the whole gradient, and the gaps between the slabs keep the sentinel.
    With dy_cols / x_cols the readable padding of the rows is NaN: it must not reach dW or db."""
    rng, S = _rng(c), c["splits"]
    data, tens, strides, bufs = [], [], [], []
    for p in c["probs"]:
        M, N, K = p["M"], p["N"], p["K"]
        dY, X = _ints(rng, (M, N)), _ints(rng, (M, K))
        assert (np.abs(dY).astype(np.float64).T @ np.abs(X).astype(np.float64)).max() < 2 ** 24 and 3 * M < 2 ** 24
        data.append((dY, X))
        t = dict(dY=_input(dY, _ld("bwd_weight", p, "dY"), p["off"].get("dY", 0)), X=_input(X, _ld("bwd_weight", p, "X"), p["off"].get("X", 0)))
        for n in ("dY", "X"):
            if p["cols"].get(n):
                t[n]._pm_cols = p["cols"][n]
        st = LV.slab_stride(p, S)
        (wbuf, t["dW"]), (bbuf, t["db"]) = (_view((N, K), _ld("bwd_weight", p, "dW"), p["off"].get("dW", 0), SENT, extra=(S - 1) * st),
                                            _view((N,), N, p["off"].get("db", 0), SENT, extra=(S - 1) * st))
        tens.append(t)
        strides.append(st)
        bufs.append((wbuf, bbuf))
    rec = _check_selected(o, c, tens, 1, strides)
    o.linear_bwd_weight_group([(t["dY"], t["X"], t["dW"], t["db"], st) for t, st in zip(tens, strides)], splits=S)
    for i, (p, (dY, X), st, (wbuf, bbuf)) in enumerate(zip(c["probs"], data, strides, bufs)):
        N, K, ldw = p["N"], p["K"], _ld("bwd_weight", p, "dW")
        kc = (-(-p["M"] // S) + 31) // 32 * 32       # the header's rule: equal ranges of whole 32-row steps
        assert rec["kchunk"][i] == kc and rec["splits"][i] == S
        w0, b0 = GUARD + p["off"].get("dW", 0), GUARD + p["off"].get("db", 0)
        wall, ball = wbuf.cpu().numpy(), bbuf.cpu().numpy()
        sum_w, sum_b = np.zeros((N, K), np.float32), np.zeros(N, np.float32)
        for z in range(S):
            gw = np.lib.stride_tricks.as_strided(wall[w0 + z * st:], (N, K), (4 * ldw, 4))
            gb = ball[b0 + z * st:b0 + z * st + N]
            a, x = dY[z * kc:(z + 1) * kc].astype(np.float64), X[z * kc:(z + 1) * kc].astype(np.float64)
            assert same_bits(gw, _mm(a.T, x).astype(np.float32)), (c["id"], i, "dW slab", z)
            assert same_bits(gb, (a.sum(0) + 0.0).astype(np.float32)), (c["id"], i, "db slab", z)
            sum_w, sum_b = sum_w + gw, sum_b + gb
        assert same_bits(sum_w, _mm(dY.T, X).astype(np.float32)), (c["id"], i)
        assert same_bits(sum_b, (dY.astype(np.float64).sum(0) + 0.0).astype(np.float32)), (c["id"], i)
        assert _outside_intact(wbuf, [(w0 + z * st, N, K, ldw) for z in range(S)]), (c["id"], i, "dW surroundings")
        assert _outside_intact(bbuf, [(b0 + z * st, 1, N, N) for z in range(S)]), (c["id"], i, "db surroundings")
