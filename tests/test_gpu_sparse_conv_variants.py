"""Every kernel the sparse-convolution entry points (pm_sparse_conv_*) dispatch to, against answers known to the bit.

As tests/test_gpu_linear_variants.py: integer operands in [-3, 3], so every product and partial sum is an integer below 2^24 and a
float64 reference holds with NO tolerance.  Each case of tests/sparse_conv_variant_cases.py names the variant it selects, and the
test first asks the selector (with the real tensors) that this is what runs.

Poisoning: every float operand is a view inside a NaN buffer (guard band before and after, NaN between the width and the row
stride, NaN rows after the last).  The gathered source also holds trap rows no index names, filled with NaN; the index table is a
view inside an int32 buffer whose surroundings name such a trap row (in bounds: a wrong read shows as NaN, never as a fault); `zero`
is exactly C zeros at a 16-byte boundary between NaN.  Every result is a view inside a buffer of the sentinel -777.25, which must
survive everywhere outside the view; for the scatter form the index table's surroundings name sentinel rows behind the dX view, and
those, the destination rows nobody maps to and the targets of absent taps must survive as well.
"""
import zlib

import numpy as np
import pytest
import torch

from tests import sparse_conv_variant_cases as SV
from tests.exact_gemm import (ACT_NAMES, DEV, DOCUMENTED_ULP, ELU, GUARD, LRELU, NONE, RELU, SELU, SELU_A, SELU_L, SENT, SIGMOID, TANH, _act64,
                              _act_torch32, _dact64, _input, _ints, _mm, _outside_intact, _ulps, _view)
from tests.helpers import record_margin, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _cases(kind):
    sel = [c for c in SV.CASES if c["kind"] == kind]
    return pytest.mark.parametrize("c", sel, ids=[c["id"] for c in sel])


def _one_per_tile(kind=None):
    """The first case of every (kind, path, tile, lay, big, C a power of two or not): the which-element probes and the run-to-run test."""
    seen, sel = set(), []
    for c in SV.CASES:
        e = c["expect"]
        key = (c["kind"], e["path"], e["tm"], e["tn"], e["lay"], e["big"], c["C"] & (c["C"] - 1) == 0)
        if key not in seen and kind in (None, c["kind"]) and c["absent"] < 1.0 and c["mode"] == "random":
            seen.add(key)
            sel.append(c)
    return pytest.mark.parametrize("c", sel, ids=[c["id"] for c in sel])


@pytest.fixture(scope="module")
def o():
    from partmanip_amd import ops
    return ops


def _rng(c, salt=""):
    return np.random.default_rng(zlib.crc32((c["id"] + salt).encode()))


def _off(c, name):
    return c["off"].get(name, 0)


# ------------------------------------------------------------------------------------------------ poisoned operands
def _source(c, a, name):
    """The gathered source: `a` has a row for every row of the tensor (live ones and traps); the traps become NaN."""
    total, _, traps = SV.live_rows(c)
    assert a.shape[0] == total
    a = a.copy()
    a[traps] = NAN
    return _input(a, SV.ld_of(c, name), 0)


def _index(idx, trap):
    """The index table as a view inside an int32 buffer that names the trap row everywhere else."""
    buf = torch.full((GUARD + idx.size + GUARD,), int(trap), dtype=torch.int32, device=DEV)
    v = buf[GUARD:GUARD + idx.size].view(idx.shape)
    v.copy_(torch.from_numpy(idx))
    return v


def _zero(c):
    """Exactly C zeros at a 16-byte boundary; NaN before them and for a whole virtual row (J * C floats) behind them."""
    Cc = c["C"]
    buf = torch.full((GUARD + Cc + max(GUARD, c["J"] * Cc),), NAN, device=DEV)
    z = buf[GUARD:GUARD + Cc]
    z.zero_()
    assert z.data_ptr() % 16 == 0
    return z


def _gathered(a, idx):
    """The virtual (rows, J*C) operand in float64: row idx[r][j] of `a` per tap, zeros for absent taps."""
    rows, J = idx.shape
    g = a.astype(np.float64)[np.maximum(idx, 0)]                         # (rows, J, C)
    g[idx < 0] = 0.0
    return g.reshape(rows, J * a.shape[1])


def _check_selected(o, c, t, act):
    got = o.sparse_conv_variant(c["kind"], SV.query_problem(c, lambda n: t[n], act))
    want = c["expect" if act else "expect_noact"]
    assert {k: got[k] for k in want} == want, (c["id"], act, got)
    return got


def _result(c, name):
    """(buffer, view, the view's (start, rows, cols, ld) for _outside_intact) of a result operand."""
    shape = SV.operand_shape(c, name)
    ld = SV.ld_of(c, name)
    buf, v = _view(shape, ld, _off(c, name), SENT)
    rows, cols = shape if len(shape) == 2 else (1, shape[0])
    return buf, v, (GUARD + _off(c, name), rows, cols, max(ld, cols))


def _gather_setup(c, rng, src_name, w_name):
    """Source, weight, index table and zero of a gathered forward / data gradient; arrays and device views."""
    total, _, traps = SV.live_rows(c)
    J, Cc, N = c["J"], c["C"], c["N"]
    a, W = _ints(rng, (total, Cc)), _ints(rng, (N, J * Cc))
    idx = SV.make_index(c, rng)
    t = {src_name: _source(c, a, src_name), w_name: _input(W, SV.ld_of(c, w_name), 0), "idx": _index(idx, traps[-1]), "zero": _zero(c)}
    return a, W, idx, t


# ------------------------------------------------------------------------------------------------ forward
@_cases("fwd")
def test_forward(o, c):
    """act NONE and RELU: the bits of the float64 reference.  TANH: the bound test_fast_tanh_accuracy pins (< 6 ulp, < 3e-7).  LRELU /
    ELU / SELU / SIGMOID: within max(4 e_ref, the documented libm figure), as test_forward of the Linear file computes it; observed /
    allowed are recorded.  A row whose taps are all absent comes out as act(b) by the same comparison."""
    rng = _rng(c)
    a, W, idx, t = _gather_setup(c, rng, "src", "W")
    b = _ints(rng, (c["N"],), -5, 5)
    assert 9 * c["J"] * c["C"] + 5 < 2 ** 24
    t["b"] = _input(b, c["N"], _off(c, "b"))
    z = (_mm(_gathered(a, idx), W.T) + b.astype(np.float64)).astype(np.float32)
    absent_rows = np.flatnonzero((idx < 0).all(1))
    worst = {}
    for act in (NONE, RELU, TANH, LRELU, ELU, SELU, SIGMOID):
        buf, t["Y"], where = _result(c, "Y")
        if act == NONE:
            _check_selected(o, c, t, 1)
        o.sparse_conv_fwd(t["src"], t["idx"], c["C"], t["W"], t["b"], t["Y"], act, t["zero"])
        got = t["Y"].cpu().numpy()
        assert _outside_intact(buf, [where]), (c["id"], act)
        if act == NONE:
            assert same_bits(got, z), (c["id"], "none", int((got != z).sum()))
            assert same_bits(got[absent_rows], np.broadcast_to(b, (len(absent_rows), c["N"]))), (c["id"], "absent rows")
        elif act == RELU:
            assert same_bits(got, np.maximum(z, np.float32(0))), (c["id"], "relu")
        else:
            assert np.isfinite(got).all(), (c["id"], ACT_NAMES[act])
            ref = _act64(z, act)
            u = float(_ulps(got, ref).max())
            if act == TANH:
                allowed = 6.0
                assert float(np.abs(got.astype(np.float64) - ref).max()) < 3e-7
            else:
                allowed = max(4.0 * float(_ulps(_act_torch32(z, act), ref).max()), DOCUMENTED_ULP[act])
            worst[act] = (u, allowed)
            print(f"{c['id']} {ACT_NAMES[act]}: {u:.3f} ulp, allowed {allowed:.3f}")
            assert u < allowed if act == TANH else u <= allowed, (c["id"], ACT_NAMES[act], u, allowed)
    for act, (u, allowed) in worst.items():
        if allowed > 0:
            record_margin(f"sparse conv variants: forward {ACT_NAMES[act]} ulp error against float64 of the exact z", u, allowed,
                          unit="ulp; allowed = 6 (tanh) or max(4 e_ref, libm's documented 1 ulp)")


# ------------------------------------------------------------------------------------------------ gathered data gradient
def _dact_check(c, got, s, h, act):
    """got against (s .* act'(h)): bits for NONE / RELU / TANH / ELU / SIGMOID, within 2 ulp of the float32 restatement for LRELU /
    SELU (test_data_gradient of the Linear file)."""
    if act in (LRELU, SELU):
        s32 = s.astype(np.float32)
        if act == LRELU:
            d = np.where(h > 0, np.float32(1), np.float32(0.01)).astype(np.float32)
        else:
            d = np.where(h > 0, SELU_L, h + SELU_L * SELU_A).astype(np.float32)
        ref = s32 * d
        assert ref.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        assert (err <= 2 * np.spacing(np.abs(ref)).astype(np.float64)).all(), (c["id"], ACT_NAMES[act], float(err.max()))
    else:
        ref = (s * _dact64(h, act)).astype(np.float32)
        assert same_bits(got, ref), (c["id"], ACT_NAMES[act], int((got != ref).sum()))


@_cases("bwd_data")
def test_data_gradient(o, c):
    """dX = (gather(dY) Wt^T) .* act'(H) with H dyadic (multiples of 1/8 in [-1, 1]; in [0, 1] for sigmoid), as test_data_gradient of
    the Linear file.  A row whose taps are all absent is exactly +0."""
    rng = _rng(c)
    a, Wt, idx, t = _gather_setup(c, rng, "dY", "Wt")
    rows, N = c["rows"], c["N"]
    H = _ints(rng, (rows, N), -8, 8) / np.float32(8)
    assert 9 * c["J"] * c["C"] * 64 < 2 ** 24
    s = _mm(_gathered(a, idx), Wt.T)
    hv = {k: _input(v, SV.ld_of(c, "H"), _off(c, "H")) for k, v in (("H", H), ("Hs", np.abs(H)))}
    absent_rows = np.flatnonzero((idx < 0).all(1))
    for act in (NONE, RELU, TANH, ELU, SIGMOID, LRELU, SELU):
        buf, t["dX"], where = _result(c, "dX")
        t["H"] = hv["Hs" if act == SIGMOID else "H"]
        if act in (NONE, TANH):
            _check_selected(o, c, t, act)
        o.sparse_conv_bwd_data(t["dY"], t["idx"], t["Wt"], t["H"] if act else None, t["dX"], act, t["zero"])
        got = t["dX"].cpu().numpy()
        assert _outside_intact(buf, [where]), (c["id"], act)
        assert same_bits(got[absent_rows], np.zeros((len(absent_rows), N), np.float32)), (c["id"], ACT_NAMES[act], "absent rows")
        _dact_check(c, got, s, np.abs(H) if act == SIGMOID else H, act)


# ------------------------------------------------------------------------------------------------ scattered data gradient
def _front(c):
    """Floats of sentinel (dX) or NaN (H) in front of a scattered operand: two destination rows at the least, so that a row index of
    -1 taken at its word still lands inside the buffer."""
    return max(GUARD, 2 * c["C"])


def _scatter_rows(c, fill):
    """(buffer, contiguous (nsrc, C) view) of a scattered operand: _front(c) floats of `fill` before it, two rows and GUARD after."""
    nsrc, Cc = c["nsrc"], c["C"]
    buf = torch.full((_front(c) + (nsrc + 2) * Cc + GUARD,), fill, device=DEV)
    v = buf[_front(c):_front(c) + nsrc * Cc].view(nsrc, Cc)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return buf, v


def _scatter_h(c, H):
    _, v = _scatter_rows(c, NAN)
    v.copy_(torch.from_numpy(H))
    return v


def _scatter_setup(c, idx):
    """The sentinel dX and the index view of the scatter form: the table's surroundings name the sentinel row behind the dX view."""
    buf, dx = _scatter_rows(c, SENT)
    return buf, dx, _index(idx, c["nsrc"])


def _scatter_view(c, full):
    return full[_front(c):_front(c) + c["nsrc"] * c["C"]].reshape(c["nsrc"], c["C"])


def _scatter_expected(c, idx, vals):
    """The whole dX buffer: `vals` (rows, J, C) at the mapped rows, the sentinel everywhere else."""
    full = np.full(_front(c) + (c["nsrc"] + 2) * c["C"] + GUARD, SENT, np.float32)
    _scatter_view(c, full)[idx[idx >= 0]] = vals[idx >= 0]
    return full


@_cases("bwd_scatter")
def test_data_gradient_scatter(o, c):
    """dX[idx[r][j]] = (dY W)[r][j] .* act'(H[idx[r][j]]): the mapped rows as in test_data_gradient; the whole rest of the dX buffer
    -- rows nobody maps to, the trap rows the index table's surroundings name, the guard bands -- keeps the sentinel.  H is NaN at
    the rows nobody maps to."""
    rng = _rng(c)
    rows, J, Cc, N, nsrc = c["rows"], c["J"], c["C"], c["N"], c["nsrc"]
    dY, W = _ints(rng, (rows, N)), _ints(rng, (N, J * Cc))
    idx = SV.make_index(c, rng)
    live = idx >= 0
    assert len(np.unique(idx[live])) == int(live.sum()) and 9 * N * 64 < 2 ** 24
    H = np.full((nsrc, Cc), NAN, np.float32)
    H[idx[live]] = _ints(rng, (int(live.sum()), Cc), -8, 8) / np.float32(8)
    s = _mm(dY, W).reshape(rows, J, Cc)
    t = dict(dY=_input(dY, SV.ld_of(c, "dY"), 0), W=_input(W, SV.ld_of(c, "W"), 0))
    hv = {k: _scatter_h(c, v) for k, v in (("H", H), ("Hs", np.abs(H)))}
    for act in (NONE, RELU, TANH, ELU, SIGMOID, LRELU, SELU):
        buf, t["dX"], t["idx"] = _scatter_setup(c, idx)
        t["H"] = hv["Hs" if act == SIGMOID else "H"]
        if act in (NONE, TANH):
            _check_selected(o, c, t, act)
        o.sparse_conv_bwd_data_scatter(t["dY"], t["W"], t["idx"], Cc, t["H"] if act else None, t["dX"], act)
        full = buf.cpu().numpy()
        h = (np.abs(H) if act == SIGMOID else H)[np.maximum(idx, 0)]    # (rows, J, C); the absent taps' rows are not compared
        outside = _scatter_expected(c, idx, np.zeros_like(s)) == np.float32(SENT)
        assert same_bits(full[outside], np.full(int(outside.sum()), SENT, np.float32)), (c["id"], ACT_NAMES[act], "surroundings")
        got = _scatter_view(c, full)[idx[live]]
        _dact_check(c, got, s[live], h[live], act)


# ------------------------------------------------------------------------------------------------ weight gradient
@_cases("bwd_weight")
def test_weight_gradient(o, c):
    """dW = dY^T gather(src) and db = column sums of dY from the single call (which reduces its own slabs): the reference's bits,
    the surroundings of dW and db intact after the slab reduction; once more without db."""
    rng = _rng(c)
    total, _, traps = SV.live_rows(c)
    rows, J, Cc, N = c["rows"], c["J"], c["C"], c["N"]
    dY, a = _ints(rng, (rows, N)), _ints(rng, (total, Cc))
    idx = SV.make_index(c, rng)
    assert 9 * rows < 2 ** 24
    t = dict(dY=_input(dY, SV.ld_of(c, "dY"), 0), src=_source(c, a, "src"), idx=_index(idx, traps[-1]), zero=_zero(c))
    ws = o.Workspace(torch.device(DEV))
    ref_w, ref_b = _mm(dY.T, _gathered(a, idx)).astype(np.float32), (dY.astype(np.float64).sum(0) + 0.0).astype(np.float32)
    for with_db in (True, False):
        wbuf, t["dW"], wwhere = _result(c, "dW")
        bbuf, t["db"], bwhere = _result(c, "db")
        if with_db:
            _check_selected(o, c, t, 1)
        o.sparse_conv_bwd_weight(t["dY"], t["src"], t["idx"], Cc, t["dW"], t["db"] if with_db else None, t["zero"], ws)
        got = t["dW"].cpu().numpy()
        assert same_bits(got, ref_w), (c["id"], with_db, int((got != ref_w).sum()))
        assert _outside_intact(wbuf, [wwhere]), (c["id"], with_db)
        if with_db:
            assert same_bits(t["db"].cpu().numpy(), ref_b), c["id"]
            assert _outside_intact(bbuf, [bwhere]), c["id"]
        else:
            assert _outside_intact(bbuf, []), (c["id"], "db written without being asked for")


# ------------------------------------------------------------------------------------------------ which element was read
def _numbered(c):
    """A source whose element (s, ch) is s * C + ch: the value names the row and the channel it was read from."""
    total, _, _ = SV.live_rows(c)
    assert total * c["C"] < 2 ** 24
    return np.arange(total * c["C"], dtype=np.float32).reshape(total, c["C"])


def _picked(a, idx, q):
    """Element q (a column of the virtual operand, per output) of every gathered row: a[idx[r][q // C]][q % C], or 0 for an absent tap."""
    Cc = a.shape[1]
    rows_ = idx[:, q // Cc]                                              # (rows, len(q))
    v = a[np.maximum(rows_, 0), (q % Cc)[None, :]]
    return np.where(rows_ >= 0, v, np.float32(0)).astype(np.float32)


@_one_per_tile("fwd")
def test_forward_reads_the_element_it_should(o, c):
    """Every weight row one-hot at a column q = j * C + ch of its own: the output IS the gathered element (tap j, channel ch of row
    idx[r][j]), or 0 for an absent tap -- small random integers can agree by coincidence, this cannot."""
    rng = _rng(c, "probe")
    J, Cc, N = c["J"], c["C"], c["N"]
    a, idx = _numbered(c), SV.make_index(c, rng)
    q = (J * Cc - 1 - np.arange(N) * 5) % (J * Cc)                       # the last column, then every fifth before it
    W = np.zeros((N, J * Cc), np.float32)
    W[np.arange(N), q] = 1
    t = dict(src=_source(c, a, "src"), W=_input(W, SV.ld_of(c, "W"), 0), idx=_index(idx, SV.live_rows(c)[2][-1]), zero=_zero(c), b=None)
    buf, t["Y"], where = _result(c, "Y")
    o.sparse_conv_fwd(t["src"], t["idx"], Cc, t["W"], None, t["Y"], NONE, t["zero"])
    assert same_bits(t["Y"].cpu().numpy(), _picked(a, idx, q)), c["id"]
    assert _outside_intact(buf, [where]), c["id"]


@_one_per_tile("bwd_data")
def test_data_gradient_reads_the_element_it_should(o, c):
    rng = _rng(c, "probe")
    J, Cc, N = c["J"], c["C"], c["N"]
    a, idx = _numbered(c), SV.make_index(c, rng)
    q = (J * Cc - 1 - np.arange(N) * 5) % (J * Cc)
    Wt = np.zeros((N, J * Cc), np.float32)
    Wt[np.arange(N), q] = 1
    t = dict(dY=_source(c, a, "dY"), Wt=_input(Wt, SV.ld_of(c, "Wt"), 0), idx=_index(idx, SV.live_rows(c)[2][-1]), zero=_zero(c))
    buf, t["dX"], where = _result(c, "dX")
    o.sparse_conv_bwd_data(t["dY"], t["idx"], t["Wt"], None, t["dX"], NONE, t["zero"])
    assert same_bits(t["dX"].cpu().numpy(), _picked(a, idx, q)), c["id"]
    assert _outside_intact(buf, [where]), c["id"]


@_one_per_tile("bwd_weight")
def test_weight_gradient_reads_the_element_it_should(o, c):
    """The mirror image: column n of dY is one-hot at a row r_n of its own, so dW[n] IS the gathered row r_n and db is all ones."""
    rng = _rng(c, "probe")
    rows, J, Cc, N = c["rows"], c["J"], c["C"], c["N"]
    a, idx = _numbered(c), SV.make_index(c, rng)
    r_n = (rows - 1 - np.arange(N) * 5) % rows                           # the last row of the reduction, then every fifth before it
    dY = np.zeros((rows, N), np.float32)
    dY[r_n, np.arange(N)] = 1
    t = dict(dY=_input(dY, SV.ld_of(c, "dY"), 0), src=_source(c, a, "src"), idx=_index(idx, SV.live_rows(c)[2][-1]), zero=_zero(c))
    wbuf, t["dW"], wwhere = _result(c, "dW")
    bbuf, t["db"], bwhere = _result(c, "db")
    o.sparse_conv_bwd_weight(t["dY"], t["src"], t["idx"], Cc, t["dW"], t["db"], t["zero"], o.Workspace(torch.device(DEV)))
    want = _picked(a, idx[r_n], np.arange(J * Cc))
    assert same_bits(t["dW"].cpu().numpy(), want), c["id"]
    assert same_bits(t["db"].cpu().numpy(), np.ones(N, np.float32)), c["id"]
    assert _outside_intact(wbuf, [wwhere]) and _outside_intact(bbuf, [bwhere]), c["id"]


@_one_per_tile("bwd_scatter")
def test_scatter_writes_the_element_it_should(o, c):
    """Row r of dY one-hot at column k_r, every weight entry a number of its own: destination row idx[r][j] IS W[k_r][j*C : (j+1)*C]."""
    rng = _rng(c, "probe")
    rows, J, Cc, N = c["rows"], c["J"], c["C"], c["N"]
    assert N * J * Cc < 2 ** 24
    idx = SV.make_index(c, rng)
    k_r = (N - 1 - np.arange(rows) * 5) % N
    dY = np.zeros((rows, N), np.float32)
    dY[np.arange(rows), k_r] = 1
    W = np.arange(1, N * J * Cc + 1, dtype=np.float32).reshape(N, J * Cc)
    t = dict(dY=_input(dY, SV.ld_of(c, "dY"), 0), W=_input(W, SV.ld_of(c, "W"), 0))
    buf, t["dX"], t["idx"] = _scatter_setup(c, idx)
    o.sparse_conv_bwd_data_scatter(t["dY"], t["W"], t["idx"], Cc, None, t["dX"], NONE)
    assert same_bits(buf.cpu().numpy(), _scatter_expected(c, idx, W[k_r].reshape(rows, J, Cc))), c["id"]


# ------------------------------------------------------------------------------------------------ run to run
@_one_per_tile()
def test_two_launches_give_the_same_bits(o, c):
    """The fixed summation order is a documented property: two launches of one problem on random floats (where the order of the
    additions shows) agree to the bit."""
    rng = _rng(c, "again")
    k, rows, J, Cc, N, nsrc = c["kind"], c["rows"], c["J"], c["C"], c["N"], c["nsrc"]
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)                         # noqa: E731
    idx = SV.make_index(c, rng)
    total, _, traps = SV.live_rows(c)
    ws = o.Workspace(torch.device(DEV))
    if k == "bwd_scatter":
        t = dict(dY=_input(f(rows, N), SV.ld_of(c, "dY"), 0), W=_input(f(N, J * Cc), SV.ld_of(c, "W"), 0), H=_scatter_h(c, f(nsrc, Cc)))
    else:
        g, w = {"fwd": ("src", "W"), "bwd_data": ("dY", "Wt"), "bwd_weight": ("src", None)}[k]
        t = {g: _source(c, f(total, Cc), g), "idx": _index(idx, traps[-1]), "zero": _zero(c)}
        if w:
            t[w] = _input(f(N, J * Cc), SV.ld_of(c, w), 0)
        if k == "fwd":
            t["b"] = _input(f(N), N, _off(c, "b"))
        elif k == "bwd_data":
            t["H"] = _input(f(rows, N), SV.ld_of(c, "H"), _off(c, "H"))
        else:
            t["dY"] = _input(f(rows, N), SV.ld_of(c, "dY"), 0)
    outs = []
    for _ in range(2):
        if k == "fwd":
            _, t["Y"], _ = _result(c, "Y")
            o.sparse_conv_fwd(t["src"], t["idx"], Cc, t["W"], t["b"], t["Y"], TANH, t["zero"])
            outs.append([t["Y"].cpu().numpy()])
        elif k == "bwd_data":
            _, t["dX"], _ = _result(c, "dX")
            o.sparse_conv_bwd_data(t["dY"], t["idx"], t["Wt"], t["H"], t["dX"], TANH, t["zero"])
            outs.append([t["dX"].cpu().numpy()])
        elif k == "bwd_scatter":
            buf, t["dX"], t["idx"] = _scatter_setup(c, idx)
            o.sparse_conv_bwd_data_scatter(t["dY"], t["W"], t["idx"], Cc, t["H"], t["dX"], TANH)
            outs.append([buf.cpu().numpy()])
        else:
            (_, t["dW"], _), (_, t["db"], _) = _result(c, "dW"), _result(c, "db")
            o.sparse_conv_bwd_weight(t["dY"], t["src"], t["idx"], Cc, t["dW"], t["db"], t["zero"], ws)
            outs.append([t["dW"].cpu().numpy(), t["db"].cpu().numpy()])
    for x, y in zip(*outs):
        assert np.isfinite(x[x != np.float32(SENT)]).all() and same_bits(x, y), c["id"]
