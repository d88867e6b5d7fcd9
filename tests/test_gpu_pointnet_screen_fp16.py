"""The one-product fp16 screen of the screened PointNet forward (csrc/pointnet_enc_screen.h) where its number format can go
wrong: W3 rows far outside fp16's range (the pack step scales every row by an exact power of two), rows of mixed magnitudes
(entries that become subnormal or are flushed after scaling), the clamped scale of an all-zero row, and a tile with more
survivors per wave than the previous cap of 128.  GPU box only.

Shapes: B = 3, P = 128 (two tiles, so the running-maximum test runs), C = 3.  Tolerances are test_gpu_pointnet_screen's
(check_against_dense): h2_save bit-equal, max / mean features within 3e-6 of the feature scale, arg-max equal wherever the fp64
top-2 gap exceeds 1e-5, the returned max equal to fp64 at the returned arg-max.  For weights scaled by 2^k the gap is 1e-5 * 2^k
(every layer-3 value scales by exactly 2^k), so check_scaled below repeats that function's checks with the scaled gap."""
import pytest
import torch

from tests.test_gpu_pointnet_screen import FEAT_TOL, GAP, check_against_dense, clouds, forward, repack, weights

pytestmark = pytest.mark.gpu
B, P, C = 3, 128, 3


@pytest.fixture(scope="module")
def base():
    w = weights(C, 31)
    pts = clouds(B, P, C, 32)
    fs, ams, _, cnt = forward(w, pts, True, count=True)
    return w, pts, fs.clone(), ams.clone(), cnt


def with_w3(w, W3, b3=None):
    w2 = dict(w, W3=W3.contiguous(), b3=(w["b3"] if b3 is None else b3.contiguous()))
    return repack(w2)


def check_scaled(w, pts, gap, label):
    """check_against_dense's checks with the arg-max gap given by the caller."""
    fs, ams, h2s, cnt = forward(w, pts, True, count=True)
    fd, amd, h2d, _ = forward(w, pts, False)
    assert torch.equal(h2s, h2d), "h2_save differs from the dense kernel's"
    z = h2d.double() @ w["W3"].double().t() + w["b3"].double()
    scale, mscale = float(fd[:, :512].abs().max()), float(fd[:, 512:].abs().max())
    e_max = float((fs[:, :512] - fd[:, :512]).abs().max()) / scale
    top2 = z.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > gap
    e_own = float((fs[:, :512].double() - z.gather(1, ams[:, None, :])[:, 0]).abs().max()) / scale
    e_mean = float((fs[:, 512:] - fd[:, 512:]).abs().max()) / mscale
    e_mean64 = float((fs[:, 512:].double() - z.mean(dim=1)).abs().max()) / mscale
    msg = (f"{label} max {e_max:.2e} own-argmax {e_own:.2e} mean {e_mean:.2e} (against fp64 {e_mean64:.2e}) "
           f"argmax differing {int((ams != amd).sum())} (under the gap: {int((~clear).sum())}) counters {cnt}")
    print(msg)
    assert e_max < FEAT_TOL and e_own < FEAT_TOL and e_mean < FEAT_TOL and e_mean64 < FEAT_TOL, msg
    assert torch.equal(ams[clear], amd[clear]), msg
    return cnt, fs, ams


@pytest.mark.parametrize("k", [-40, -20, 12, 24, 40])
def test_weight_range(base, k):
    """W3 and b3 times 2^k: below fp16's smallest subnormal, above its largest finite value, and in between.  Every layer-3
    value scales by exactly 2^k, so the features are 2^k times those at k = 0 bit for bit and the arg-max is the same."""
    w, pts, f0, a0, _ = base
    wk = with_w3(w, w["W3"] * 2.0 ** k, w["b3"] * 2.0 ** k)
    cnt, fs, ams = check_scaled(wk, pts, GAP * 2.0 ** k, f"2^{k}")
    assert cnt[1] == 0, cnt
    assert torch.equal(fs, f0 * 2.0 ** k)
    assert torch.equal(ams, a0)


def test_mixed_magnitudes_in_a_row(base):
    """Channels 0-31: every other entry of the row is 2^-20 of the row's largest (a small fp16 value after scaling).  Channels
    32-63: one entry 2^10 times the rest.  Channels 64-79, beyond what the issue asks: one entry 2^28 times the rest, which
    are subnormal in fp16, or flushed, after scaling.  The rest is scaled DOWN, so the feature scale of the tolerance stays."""
    w, pts, _, _, _ = base
    W3 = w["W3"].clone()
    top = W3[:32].abs().max(dim=1, keepdim=True)[0]
    W3[:32, ::2] = torch.sign(W3[:32, ::2]) * top * 2.0 ** -20
    for rows, k in ((slice(32, 64), -10), (slice(64, 80), -28)):
        keep = W3[rows, 5].clone()
        W3[rows] = W3[rows] * 2.0 ** k
        W3[rows, 5] = keep
    check_against_dense(with_w3(w, W3), pts, label="mixed magnitudes")


def test_zero_row_and_single_entry_row(base):
    """Row 100 all zero (the scale exponent is clamped; z~ = b3 for every point, the tie goes to point 0 and the feature is b3
    exactly); row 101 a single non-zero entry."""
    w, pts, _, _, _ = base
    W3 = w["W3"].clone()
    W3[100] = 0
    W3[101] = 0
    W3[101, 77] = 0.03
    wz = with_w3(w, W3)
    cnt, fs, ams = check_against_dense(wz, pts, label="zero row")
    assert torch.equal(fs[:, 100], wz["b3"][100].expand(B))
    assert int(ams[:, 100].abs().max()) == 0


def test_more_survivors_than_the_previous_cap(base):
    """The first tile's 64 points made equal in pairs (32 distinct points, each twice): every channel keeps both members of its
    leading pair, so a wave has at least 128 survivors in that tile, and more with the near-ties.  No fallback: the finish
    handled them.  The lower index of each pair must win."""
    w, pts, _, _, _ = base
    p2 = pts.clone()
    p2[:, 1:64:2] = p2[:, 0:64:2]
    cnt, fs, ams = check_against_dense(w, p2, label="pairs in the first tile")
    print("counters", cnt)
    assert cnt[1] == 0, cnt
    assert cnt[0] > 128 * 8 * B / 2, cnt
    first = ams < 64
    assert int(first.sum()) > 0 and int((ams[first] % 2).sum()) == 0
