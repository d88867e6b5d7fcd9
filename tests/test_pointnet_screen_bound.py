"""Host test of the screen's error bound (csrc/pointnet_enc_screen.h, "eps_c"): no GPU.

The documented formula
    s_c   = min(15 - e, 126), the row's largest finite magnitude being m 2^e with m in [0.5, 1);  w' = 2^s_c w, w16 = fp16(w')
    R     = sum_k (|w' - w16| where w16 is normal, max(|w'|, |w' - w16|) where it is subnormal or zero),  S16 = sum_k |w16|
    eps_c = ((R + 2^-12 S16) 2^-s_c + 1024 * 2^-24 (L + |b3_c|)) (1 + 2^-10) + 2^-116,   L = ||W3[c]||_1
is held against an emulation of the screen's z~ = fmaf(sum_k w16 h16, 2^-s_c, b3): operands rounded to fp16 (numpy: round to
nearest even) with subnormals once kept and once flushed to zero, products exact (float64 holds 11 x 11 bits), the 256 products
accumulated in float32 from zero in a random order and in a worst-sign order (all positive terms first, largest first, then the
negative ones: the partial sums are as large as they can get).  z^ is the exact finish in its documented order: lane j of eight
takes k = 4 j + 32 i + e as one fmaf chain, the xor-4 / -2 / -1 butterfly, + b3 last.  fmaf is emulated as float32(float64
product + float64 sum); that can differ from a true fused operation by a double rounding on a float32 midpoint, which moves a
value by less than 2^-52 of it and is no part of what is asserted.  Asserted everywhere: |z~ - z^| <= eps_c (the float64
formula; the kernel's float is that rounded UP).  Operands: default-initialised weights and tanh activations, the same scaled
by 2^-40 and 2^24, rows of mixed magnitudes (entries 2^-20 and 2^-31 of the row maximum: small normals, subnormals or flushed
after scaling), activations below fp16's smallest normal, and the adversarial case: every w' and every h on an fp16 rounding
midpoint that rounds towards zero, all signs equal, so that every dropped product has the same sign.

Largest |z~ - z^| / eps_c is printed per case."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def row_scale(W):
    a = np.abs(W.astype(F64))
    a[~np.isfinite(a)] = 0.0
    mx = a.max(axis=1)
    e = np.frexp(mx)[1]                                   # mx = m 2^e, m in [0.5, 1); frexp(0) gives e = 0: clamped below by hand
    s = np.where(mx > 0, np.minimum(15 - e, 126), 126)
    return s.astype(np.int64)


def eps_formula(W, b3, s):
    with np.errstate(invalid="ignore", over="ignore"):
        L = np.abs(W.astype(F64)).sum(axis=1)
        ws = np.ldexp(W.astype(F64), s[:, None].astype(np.int32)).astype(F32).astype(F64)
        w16 = ws.astype(np.float16).astype(F64)
        d = np.abs(ws - w16)
        R = np.where(np.abs(w16) < 2.0 ** -14, np.maximum(np.abs(ws), d), d).sum(axis=1)
        S16 = np.abs(w16).sum(axis=1)
        inv = np.ldexp(1.0, (-s).astype(np.int32))
        return ((R + 2.0 ** -12 * S16) * inv + 1024 * 2.0 ** -24 * (L + np.abs(b3.astype(F64)))) * (1 + 2.0 ** -10) + 2.0 ** -116


def to_f16(x, flush):
    """fp16 operand of the matrix unit as float64: RNE, subnormals kept or flushed to zero."""
    with np.errstate(over="ignore"):
        h = x.astype(np.float16).astype(F64)
    if flush:
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    return h


def accumulate(prod, order):
    """prod (N, M, 256) exact products; float32 accumulation from zero along the last axis in `order` (N, M, 256 indices)."""
    p = np.take_along_axis(prod, order, axis=2)
    acc = np.zeros(prod.shape[:2], F32)
    for k in range(p.shape[2]):
        acc = (acc.astype(F64) + p[:, :, k]).astype(F32)      # two-operand sum: float64 then float32 (see the docstring)
    return acc


def worst_sign_order(prod):
    key = np.where(prod >= 0, -prod, 1e300 + prod)            # positives first, largest first; then negatives, largest magnitude last
    return np.argsort(key, axis=2, kind="stable")


def screen_value(W, b3, h, s, flush, order_kind, rng):
    Ws = np.ldexp(W.astype(F64), s[:, None].astype(np.int32)).astype(F32)      # 2^s w: exact in float32 (or an fp32 underflow: in the bound)
    w16, h16 = to_f16(Ws, flush), to_f16(h, flush)
    prod = w16[:, None, :] * h16[None, :, :]                  # exact
    if order_kind == "random":
        order = np.argsort(rng.random(prod.shape), axis=2)
    else:
        order = worst_sign_order(prod)
    acc = accumulate(prod, order)
    inv = np.ldexp(1.0, (-s).astype(np.int32))
    return (acc.astype(F64) * inv[:, None] + b3.astype(F64)[:, None]).astype(F32)


def finish_value(W, b3, h):
    """The exact finish in its documented order, (N, M) float32."""
    W64, h64 = W.astype(F64), h.astype(F64)
    part = []
    for j in range(8):
        sj = np.zeros((W.shape[0], h.shape[0]), F32)
        for i in range(8):
            for e in range(4):
                k = 4 * j + 32 * i + e
                sj = (W64[:, None, k] * h64[None, :, k] + sj.astype(F64)).astype(F32)
        part.append(sj)
    t = [part[j] + part[j ^ 4] for j in range(8)]             # float32 adds
    u = [t[j] + t[j ^ 2] for j in range(8)]
    v = u[0] + u[1]
    return v + b3.astype(F32)[:, None]


def worst_ratio(W, b3, h, label):
    s = row_scale(W)
    eps = eps_formula(W, b3, s)
    zh = finish_value(W, b3, h).astype(F64)
    rng = np.random.default_rng(7)
    worst = 0.0
    for flush in (False, True):
        for kind in ("random", "worst-sign"):
            zt = screen_value(W, b3, h, s, flush, kind, rng).astype(F64)
            err = np.abs(zt - zh)
            assert np.isfinite(err).all(), label
            ratio = float((err / eps[:, None]).max())
            assert (err <= eps[:, None]).all(), (label, flush, kind, ratio)
            worst = max(worst, ratio)
    print(f"{label}: largest |z~ - z^| / eps = {worst:.3f}")
    return worst


def default_operands(seed, N=48, M=48):
    rng = np.random.default_rng(seed)
    bound = 1.0 / 16.0                                        # torch.nn.Linear(256, 512): U(-1 / sqrt(256), 1 / sqrt(256))
    W = rng.uniform(-bound, bound, (N, 256)).astype(F32)
    b3 = rng.uniform(-bound, bound, N).astype(F32)
    h = np.tanh(rng.normal(0, 1, (M, 256))).astype(F32)
    return W, b3, h


def test_random_operands():
    r = worst_ratio(*default_operands(1), "default weights, tanh activations")
    assert r < 0.2                                            # far inside: the bound prices the worst case, not the typical one


def test_weight_range():
    W, b3, h = default_operands(2)
    for k in (-40, 24):
        worst_ratio(np.ldexp(W, k).astype(F32), np.ldexp(b3, k).astype(F32), h, f"weights x 2^{k}")


def test_mixed_magnitudes_in_a_row():
    W, b3, h = default_operands(3)
    W[:16, ::2] = W[:16, ::2] * F32(2.0 ** -20)               # small normals after scaling
    W[16:32, ::2] = W[16:32, ::2] * F32(2.0 ** -31)           # subnormal or flushed after scaling
    W[32:, 5] = W[32:, 5] * F32(2.0 ** 10)                    # one entry 2^10 x the rest
    worst_ratio(W, b3, h, "mixed magnitudes")


def test_small_activations():
    W, b3, _ = default_operands(4)
    rng = np.random.default_rng(5)
    h = (rng.uniform(0.5, 1.0, (48, 256)) * 2.0 ** -14).astype(F32)          # all below fp16's smallest normal
    r = worst_ratio(np.abs(W), b3, h, "activations below 2^-14, weights of one sign")
    assert r > 0.05                                           # flushing really drops them: |r_h| = |h| there, inside the 2^-12 S16 term


def test_zero_row_and_single_entry_row():
    W, b3, h = default_operands(6)
    W[0] = 0
    W[1] = 0
    W[1, 77] = 0.03
    s = row_scale(W)
    assert s[0] == 126
    zt = screen_value(W, b3, h, s, True, "random", np.random.default_rng(0))
    assert (zt[0] == b3[0]).all()                             # the zero row's z~ is b3 exactly
    worst_ratio(W, b3, h, "zero row, single-entry row")


def test_midpoints_with_aligned_signs():
    """w' = 2^14 (1 + 2 j 2^-10) + 2^3 and h = 2^-1 (1 + 2 j' 2^-10) + 2^-12 (0.98 <= h < 1): both sit half an fp16 ulp above a value with an even
    mantissa, so round-to-nearest-even rounds both DOWN; with every weight and activation positive every dropped product has the
    same sign.  The row is written in the real domain at 2^-19 of that (s_c = 19)."""
    rng = np.random.default_rng(8)
    N, M = 32, 32
    jw = rng.integers(0, 8, (N, 256))
    jh = rng.integers(496, 512, (M, 256))                     # h just below 1: |r_h| = 2^-12 is the whole of what the bound allows
    Ws = 2.0 ** 14 * (1 + 2 * jw * 2.0 ** -10) + 2.0 ** 3
    h = (0.5 * (1 + 2 * jh * 2.0 ** -10) + 2.0 ** -12).astype(F32)
    W = np.ldexp(Ws, -19).astype(F32)
    assert (np.ldexp(W.astype(F64), 19) == Ws).all() and (row_scale(W) == 19).all()
    assert (to_f16(Ws, False) < Ws).all() and (to_f16(h, False) < h).all()
    b3 = np.zeros(N, F32)
    r = worst_ratio(W, b3, h, "fp16 midpoints, signs aligned")
    assert 0.9 < r <= 1.0                                     # the case the operand terms R and 2^-12 S16 are there for: nearly all of the bound


def test_scale_keeps_finite_weights_finite_in_fp16():
    rng = np.random.default_rng(9)
    W = (rng.uniform(-1, 1, (64, 256)) * np.exp2(rng.integers(-140, 127, (64, 1)))).astype(F32)
    W[3, 10] = np.inf
    W[4, 11] = np.nan
    s = row_scale(W)
    assert s.max() <= 126 and s.min() >= -126
    Ws = np.ldexp(W.astype(F64), s[:, None].astype(np.int32))
    fin = np.isfinite(W)
    assert np.abs(Ws[fin]).max() < 2.0 ** 15
    big = fin & (np.abs(W) >= 2.0 ** -111)                          # rows the clamp at 126 does not touch reach the top of the range
    rows = big.any(axis=1)
    assert (np.abs(np.where(fin, Ws, 0)).max(axis=1)[rows] >= 2.0 ** 14).all()
    e = eps_formula(W, np.zeros(64, F32), s)
    assert not math.isfinite(e[3]) and not math.isfinite(e[4])    # a row holding inf / NaN keeps a non-finite bound
