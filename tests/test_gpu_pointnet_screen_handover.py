"""The hand-over of the screened PointNet forward's survivor finish (csrc/pointnet_enc_screen.h): the eight-lane sum on DPP moves,
and the running (maximum, point) of every channel kept as one packed 64-bit LDS word that the finish raises with an atomic
maximum.  Neither may change a bit of the outputs.  GPU box only.

Shapes: 3 clouds; 64 points (one tile: every channel starts from the slot's initial (-inf, point 0)) and 128 points (two tiles: the
maximum is carried in LDS, read back by the second tile's select pass and by the epilogue); 3 and 4 coordinates (the two
specialised layer-1 paths).

Bounds: bit equality with the host replay of the documented finish order (test_gpu_pointnet_screen_order.py) and with the dense
kernel where the kernel header promises it; the arg-max equals the dense kernel's wherever the fp64 top-2 gap exceeds 1e-5, as in
test_gpu_pointnet_screen.py; there is no tolerance to choose.

test_zero_row_returns_the_bias: the chain of a zero row is +0 (fmaf(0, h, +0) = +0 for either sign of h) and a plain add gives
(+0) + (-0) = +0, which is what the dense kernel returns for b3 = -0.0 (bits 0x00000000, measured) and what the finish returned
until it was given the rule `a zero sum returns b3 itself`; with it the feature is b3's bits, sign included, as the test asks."""
import numpy as np
import pytest
import torch

from tests.test_gpu_pointnet_screen import GAP, clouds, forward, repack, weights
from tests.test_gpu_pointnet_screen_order import replay

pytestmark = pytest.mark.gpu
B = 3
SHAPES = [(64, 3), (128, 3), (64, 4), (128, 4)]


def bits(x):
    return x.contiguous().view(torch.int32)


def assert_follows_the_order(w, pts, fs, ams, h2s, label):
    """Every max feature is the documented chain at the returned arg-max, bit for bit."""
    h = h2s.gather(1, ams[:, :, None].expand(-1, -1, 256)).reshape(-1, 256).cpu().numpy()
    n = pts.shape[0]
    want, _ = replay(h, np.tile(w["W3"].cpu().numpy(), (n, 1)), np.tile(w["b3"].cpu().numpy(), n))
    got = fs[:, :512].reshape(-1).cpu().numpy()
    same = got.view(np.uint32) == want.view(np.uint32)
    print(f"{label}: max features bit-equal to the replay {same.mean():.4f}")
    assert same.all()


def assert_argmax_as_dense(w, ams, amd, h2d):
    z = h2d.double() @ w["W3"].double().t() + w["b3"].double()
    top2 = z.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > GAP
    assert torch.equal(ams[clear], amd[clear])


@pytest.mark.parametrize("P,C", SHAPES)
def test_random_clouds(P, C):
    w = weights(C, 10 * C + 2)
    pts = clouds(B, P, C, 3 * P + C)
    fs, ams, h2s, cnt = forward(w, pts, True, count=True)
    assert cnt[1] == 0, cnt                                   # every max feature comes from the finish
    fd, amd, h2d, _ = forward(w, pts, False)
    assert_follows_the_order(w, pts, fs, ams, h2s, f"random P={P} C={C} counters {cnt}")
    assert_argmax_as_dense(w, ams, amd, h2d)


@pytest.mark.parametrize("P,C", SHAPES)
def test_repeated_points_lowest_index_wins(P, C):
    """Points 0-15 again at 32-47 of the first tile and (P = 128) at 64-79 of the second: wherever one of them holds a channel's
    maximum the channel has two survivors with the same value in one pass or in neighbouring passes, and a third that ties the
    carried maximum from the next tile.  The copies never win; the values follow the order."""
    w = weights(C, 10 * C + 3)
    pts = clouds(B, P, C, 5 * P + C)
    pts[:, 32:48] = pts[:, 0:16]
    if P == 128:
        pts[:, 64:80] = pts[:, 0:16]
    fs, ams, h2s, cnt = forward(w, pts, True, count=True)
    assert cnt[1] == 0, cnt
    held = int((ams < 16).sum())
    copies = ((ams >= 32) & (ams < 48)) | ((ams >= 64) & (ams < 80))
    print(f"repeated P={P} C={C}: {held} of {B * 512} channels won by a repeated point, counters {cnt}")
    assert bool((ams < 16).any(dim=1).all())                  # 16 of the 48 / 96 distinct points: every cloud has such channels
    assert not bool(copies.any())
    assert_follows_the_order(w, pts, fs, ams, h2s, f"repeated P={P} C={C}")
    fd, amd, _, _ = forward(w, pts, False)
    assert not bool((((amd >= 32) & (amd < 48)) | ((amd >= 64) & (amd < 80))).any())      # the dense kernel's rule is the same


@pytest.mark.parametrize("P,C", SHAPES)
def test_nan_coordinate(P, C):
    w = weights(C, 10 * C + 4)
    pts = clouds(B, P, C, 7 * P + C)
    clean = forward(w, pts, True)
    bad = pts.clone()
    bad[1, P - 3, C - 1] = float("nan")                       # the last tile of cloud 1; clouds 0 and 2 stay clean
    f, am, _, _ = forward(w, bad, True)
    fd, amd, _, _ = forward(w, bad, False)
    assert torch.isnan(f[1]).all()
    assert torch.equal(torch.isnan(f), torch.isnan(fd))
    for b in (0, 2):
        assert torch.equal(bits(f[b]), bits(clean[0][b])) and torch.equal(am[b], clean[1][b]), b


@pytest.mark.parametrize("P,C", SHAPES)
def test_infinite_weight_both_signs(P, C):
    """W3[77, k0] = +inf and W3[301, k1] = -inf, k0 and k1 the first two columns of h2 that take both signs in every cloud: the
    two channels' values are infinities of both signs."""
    w = weights(C, 10 * C + 5)
    pts = clouds(B, P, C, 11 * P + C)
    h2 = forward(w, pts, True)[2]
    both = ((h2 > 0).any(dim=1) & (h2 < 0).any(dim=1)).all(dim=0).nonzero().flatten().tolist()
    assert len(both) >= 2
    w2 = dict(w, W3=w["W3"].clone())
    w2["W3"][77, both[0]] = float("inf")
    w2["W3"][301, both[1]] = float("-inf")
    repack(w2)
    fs, ams, h2s, _ = forward(w2, pts, True)
    fd, amd, _, _ = forward(w2, pts, False)
    assert torch.equal(torch.isnan(fs), torch.isnan(fd))
    assert torch.equal(torch.isinf(fs), torch.isinf(fd))
    inf = torch.isinf(fd)
    assert torch.equal(torch.sign(fs[inf]), torch.sign(fd[inf]))
    assert int((~torch.isfinite(fs[:, :512])).sum()) >= 2 * B     # the two poisoned channels of every cloud
    ok = torch.isfinite(fd[:, :512])
    w_ok = dict(w2, W3=torch.nan_to_num(w2["W3"], posinf=0.0, neginf=0.0))     # the replay of the finite channels only
    h = h2s.gather(1, ams[:, :, None].expand(-1, -1, 256)).reshape(-1, 256).cpu().numpy()
    want, _ = replay(h, np.tile(w_ok["W3"].cpu().numpy(), (B, 1)), np.tile(w["b3"].cpu().numpy(), B))
    got = fs[:, :512].reshape(-1).cpu().numpy()
    m = ok.reshape(-1).cpu().numpy()
    assert (got.view(np.uint32)[m] == want.view(np.uint32)[m]).all()


@pytest.mark.parametrize("sign", ["plus", "minus"])
@pytest.mark.parametrize("P,C", SHAPES)
def test_zero_row_returns_the_bias(P, C, sign):
    """W3[100, :] = 0 and b3[100] = +0.0 / -0.0: every point of the channel ties at zero.  The feature is b3 bit for bit, sign
    included, and the arg-max is point 0.  (minus: the finish's own rule for a zero sum; the dense kernel returns +0.)"""
    w = weights(C, 10 * C + 6)
    pts = clouds(B, P, C, 13 * P + C)
    w2 = dict(w, W3=w["W3"].clone(), b3=w["b3"].clone())
    w2["W3"][100] = 0.0
    w2["b3"][100] = 0.0 if sign == "plus" else -0.0
    repack(w2)
    fs, ams, _, cnt = forward(w2, pts, True, count=True)
    fd, amd, _, _ = forward(w2, pts, False)
    print(f"zero row P={P} C={C} b3 bits {int(bits(w2['b3'])[100]):#x}: screened {[hex(int(v) & 0xffffffff) for v in bits(fs[:, 100])]} "
          f"arg-max {ams[:, 100].tolist()}; dense {[hex(int(v) & 0xffffffff) for v in bits(fd[:, 100])]} arg-max {amd[:, 100].tolist()}; "
          f"counters {cnt}")
    assert cnt[1] == 0, cnt
    assert ams[:, 100].tolist() == [0] * B
    assert torch.equal(bits(fs[:, 100]), bits(w2["b3"][100]).expand(B))


@pytest.mark.parametrize("P,C", SHAPES)
def test_all_equal_cloud_is_the_dense_kernel(P, C):
    """One point repeated: every (wave, tile) pair exceeds the survivor cap and folds the dense layer 3's winner into the slot."""
    w = weights(C, 10 * C + 7)
    pts = clouds(B, 1, C, 17 * P + C).repeat(1, P, 1)
    fs, ams, _, cnt = forward(w, pts, True, count=True)
    fd, amd, _, _ = forward(w, pts, False)
    assert cnt[1] == B * (P // 64) * 8, cnt
    assert torch.equal(bits(fs[:, :512]), bits(fd[:, :512]))
    assert int(ams.max()) == 0 and int(amd.max()) == 0
