"""The survivor finish of the screened PointNet forward (csrc/pointnet_enc_screen.h) evaluates every max feature in ONE documented
fp32 order, whatever the other survivors are.  This file replays that order on the host from the kernel's own outputs and asks
for the same bits.  GPU box only.

The order, as the kernel header states it, for channel c at the winning point p (h = h2_save[b, p, :], w = W3[c, :]):
  eight partial sums s_j, j = 0..7: one fmaf chain from 0 over k = 4 j + 32 i + e, i = 0..7 outer, e = 0..3 inner;
  u_j = s_j + s_{j ^ 4};  t_j = u_j + u_{j ^ 2};  v = t_j + t_{j ^ 1}  (every lane ends with the same v: fp32 adds commute);
  feature = v + b3[c], added last.
fmaf is emulated exactly: the product of two floats is exact in float64, the float64 sum with the accumulator is rounded once,
and rounding that to float32 is the single correct rounding unless the float64 sum sits on a float32 rounding midpoint (or in
the subnormal range); those elements are redone in exact rational arithmetic.

Bounds: bit equality (there is no tolerance to choose); the arg-max equals the dense kernel's wherever the fp64 top-2 gap of
the dense layer 3 exceeds 1e-5, as in test_gpu_pointnet_screen.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.test_gpu_pointnet_screen import GAP, clouds, forward, weights

pytestmark = pytest.mark.gpu


def round_to_f32(fr):
    """Fraction -> nearest float32, ties to even (Python's round() of a Fraction is ties-to-even)."""
    if fr == 0:
        return np.float32(0.0)
    a, e = abs(fr), 0
    while a >= 2:
        a, e = a / 2, e + 1
    while a < 1:
        a, e = a * 2, e - 1
    q = Fraction(2) ** (max(e, -126) - 23)
    return np.float32(float(round(fr / q) * q))


def fmaf(a, b, c):
    """float32 arrays -> fmaf(a, b, c), one rounding."""
    t = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = t.astype(np.float32)
    low = t.view(np.uint64) & np.uint64((1 << 29) - 1)
    redo = (low == np.uint64(1 << 28)) | ((np.abs(t) < 2.0 ** -120) & (t != 0))
    for i in np.flatnonzero(redo):
        out[i] = round_to_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out, int(redo.sum())


def replay(h, w, b3):
    """h, w: (N, 256) float32 rows, b3: (N,) -> the finish's value, (N,) float32."""
    N = h.shape[0]
    s = np.zeros((N, 8), np.float32)
    redone = 0
    j = np.arange(8)
    for i in range(8):
        for e in range(4):
            k = 4 * j + 32 * i + e
            r, n = fmaf(w[:, k].reshape(-1), h[:, k].reshape(-1), s.reshape(-1))
            s, redone = r.reshape(N, 8), redone + n
    u = s + s[:, j ^ 4]
    t = u + u[:, j ^ 2]
    v = t + t[:, j ^ 1]
    assert all(np.array_equal(v[:, 0].view(np.uint32), v[:, q].view(np.uint32)) for q in range(8))
    return v[:, 0] + b3, redone


def test_fmaf_emulation_rounds_once():
    """2^36 + 1 = 4097 * 16773121, both exact in float32: 4097 * (16773121 * 2^-60) + 1 = 1 + 2^-24 + 2^-60, just above the
    float32 midpoint of [1, 1 + 2^-23].  float64 rounds that sum TO the midpoint, and a second rounding would go down to even.
    (No GPU work, but it checks the GPU test's own reference, so it stays beside it.)"""
    one = np.array([1.0], np.float32)
    out, n = fmaf(np.array([4097.0], np.float32), np.array([16773121.0 * 2.0 ** -60], np.float32), one)
    assert n == 1 and out[0] == np.float32(1.0 + 2.0 ** -23)
    out, n = fmaf(one, np.array([2.0 ** -24], np.float32), one)          # 1 + 2^-24 exactly: a true tie, to even
    assert n == 1 and out[0] == np.float32(1.0)
    out, n = fmaf(one, np.array([3 * 2.0 ** -24], np.float32), one)      # 1 + 3 * 2^-24: a true tie, to even (up)
    assert n == 1 and out[0] == np.float32(1.0 + 2.0 ** -22)


@pytest.mark.parametrize("P,C", [(64, 3), (128, 3), (64, 4)])
def test_max_features_follow_the_documented_order(P, C):
    B = 3
    w = weights(C, 10 * C + 1)
    pts = clouds(B, P, C, P + C)
    fs, ams, h2s, cnt = forward(w, pts, True, count=True)
    assert cnt[1] == 0, cnt                                   # no dense fallback: every max feature comes from the finish
    fd, amd, h2d, _ = forward(w, pts, False)
    h = h2s.gather(1, ams[:, :, None].expand(-1, -1, 256)).reshape(B * 512, 256).cpu().numpy()
    W3 = w["W3"].cpu().numpy()
    want, redone = replay(h, np.tile(W3, (B, 1)), np.tile(w["b3"].cpu().numpy(), B))
    got = fs[:, :512].reshape(-1).cpu().numpy()
    same = got.view(np.uint32) == want.view(np.uint32)
    print(f"P={P} C={C}: bit-equal {same.mean():.4f}, worst difference {np.abs(got.astype(np.float64) - want).max():.2e}, "
          f"fmaf steps redone in exact arithmetic {redone}, counters {cnt}")
    assert same.all()
    z = h2d.double() @ w["W3"].double().t() + w["b3"].double()
    top2 = z.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > GAP
    assert torch.equal(ams[clear], amd[clear])
