"""Op-level tests of csrc/bn_pool2d.hip (batch norm, 3 x 3 / 2 max pool, global average pool, the stem's patch matrix) against
torch in float64, by the project's rule: max |hip - out64| <= 4 x what torch's own float32 evaluation loses (helpers.within).

The batch-norm backward takes its ReLU mask from the layer's output as the kernels do; the reference is given THAT mask (the
HIP forward's), so that the comparison is one of arithmetic and not of which side of zero a value at round-off fell."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import npy, same_bits, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1
BN_CASES = [(2, 64, 64), (37, 64, 80), (4609, 128, 128), (36, 512, 512)]


def _ws():
    from partmanip_amd import ops
    return ops.Workspace(torch.device(DEV))


def _strided(rows, C, ld, fill=None, src=None):
    """A (rows, C) view of a (rows, ld) device buffer whose padding columns hold a sentinel."""
    buf = torch.full((rows, ld), -777.25, device=DEV)
    v = buf[:, :C]
    if src is not None:
        v.copy_(src)
    elif fill is not None:
        v.fill_(fill)
    return buf, v


def bn_inputs(rows, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 0.7 + 0.3
    x[:, 0] = 0.7                                                       # a constant channel: variance 0
    x[:, 1] = 0.3 + 1.5 * torch.rand(rows, generator=g)                 # a depth-image channel: values near 1 ...
    x[::5, 1] = 100.0                                                   # ... with a fifth of them at the far plane
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    res = torch.randn(rows, C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    dy2 = torch.randn(rows, C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return x, gamma, beta, res, dy, dy2, rm, rv


def hip_bn(x, gamma, beta, res, rm, rv, ld, relu, use_res):
    from partmanip_amd import ops
    rows, C = x.shape
    _, xv = _strided(rows, C, ld, src=x)
    ybuf, yv = _strided(rows, C, ld)
    rbuf, rvw = _strided(rows, C, ld, src=res)
    mean, var, invstd = (torch.empty(C, device=DEV) for _ in range(3))
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
    ops.bn2d_stats(xv, EPS, mean, invstd, _ws(), var=var, running_mean=rm_d, running_var=rv_d, num_batches_tracked=nbt, momentum=MOM)
    ops.bn2d_apply(xv, mean, invstd, gamma.to(DEV), beta.to(DEV), yv, rvw if use_res else None, relu)
    return dict(xv=xv, yv=yv, ybuf=ybuf, mean=mean, var=var, invstd=invstd, rm=rm_d, rv=rv_d, nbt=nbt, res=rvw)


def ref_bn(x, gamma, beta, res, rm, rv, relu, use_res, dtype, training=True):
    x, gamma, beta, res, rm, rv = (v.to(dtype).clone() for v in (x, gamma, beta, res, rm, rv))
    y = F.batch_norm(x, rm, rv, gamma, beta, training, MOM, EPS)
    if use_res:
        y = y + res
    if relu:
        y = F.relu(y)
    return y, rm, rv


@pytest.mark.parametrize("rows,C,ld", BN_CASES)
@pytest.mark.parametrize("relu,use_res", [(False, False), (True, False), (False, True), (True, True)])
def test_bn_forward_statistics_and_running_update(rows, C, ld, relu, use_res):
    x, gamma, beta, res, _, _, rm, rv = bn_inputs(rows, C)
    h = hip_bn(x, gamma, beta, res, rm, rv, ld, relu, use_res)
    y32, rm32, rv32 = ref_bn(x, gamma, beta, res, rm, rv, relu, use_res, torch.float32)
    y64, rm64, rv64 = ref_bn(x, gamma, beta, res, rm, rv, relu, use_res, torch.float64)
    name = f"bn2d {rows}x{C} ld {ld} relu {int(relu)} res {int(use_res)}"
    x64 = x.double()
    within(name, "mean", npy(h["mean"]), x.mean(0).numpy(), x64.mean(0).numpy())
    within(name, "var", npy(h["var"]), x.var(0, unbiased=False).numpy(), x64.var(0, unbiased=False).numpy())
    within(name, "invstd", npy(h["invstd"]), (1 / torch.sqrt(x.var(0, unbiased=False) + EPS)).numpy(),
           (1 / torch.sqrt(x64.var(0, unbiased=False) + EPS)).numpy())
    within(name, "y", npy(h["yv"]), y32.numpy(), y64.numpy())
    within(name, "running_mean", npy(h["rm"]), rm32.numpy(), rm64.numpy())
    within(name, "running_var", npy(h["rv"]), rv32.numpy(), rv64.numpy())
    assert int(h["nbt"]) == 4
    # the constant channel: variance exactly 0, its mean exact, its output exactly beta [+ residual]
    assert float(h["var"][0]) == 0.0 and float(h["mean"][0]) == np.float32(0.7)
    want0 = beta[0] + (res[:, 0] if use_res else torch.zeros(rows))
    assert torch.equal(h["yv"][:, 0].cpu(), F.relu(want0) if relu else want0)
    if ld > C:
        assert torch.all(h["ybuf"][:, C:] == -777.25)                   # the padding columns are nobody's


@pytest.mark.parametrize("rows,C,ld", BN_CASES)
@pytest.mark.parametrize("relu,use_res", [(False, False), (True, True)])
def test_bn_backward(rows, C, ld, relu, use_res):
    from partmanip_amd import ops
    x, gamma, beta, res, dy, dy2, rm, rv = bn_inputs(rows, C, seed=1)
    h = hip_bn(x, gamma, beta, res, rm, rv, ld, relu, use_res)
    _, dyv = _strided(rows, C, ld, src=dy)
    _, dy2v = _strided(rows, C, ld, src=dy2)
    dxbuf, dxv = _strided(rows, C, ld)
    _, dmv = _strided(rows, C, ld)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.bn2d_bwd(dyv, h["xv"], h["yv"], h["mean"], h["invstd"], gamma.to(DEV), dgamma, dbeta, dxv, _ws(), relu=relu,
                 dy2=dy2v if use_res else None, dy_masked=dmv)
    # the reference is handed the mask the kernels used (y > 0 of the HIP forward)
    mask = (h["yv"] > 0).cpu() if relu else torch.ones(rows, C, dtype=torch.bool)
    dtot = (dy + dy2) if use_res else dy
    dm = torch.where(mask, dtot, torch.zeros(()))
    assert same_bits(npy(dmv), dm.numpy())
    out = {}
    for dtype in (torch.float32, torch.float64):
        xx, gg, bb = (v.detach().to(dtype).clone().requires_grad_(True) for v in (x, gamma, beta))
        y = F.batch_norm(xx, None, None, gg, bb, True, MOM, EPS)
        y.backward(dm.to(dtype))
        out[dtype] = (xx.grad.numpy(), gg.grad.numpy(), bb.grad.numpy())
    name = f"bn2d_bwd {rows}x{C} ld {ld} relu {int(relu)} res {int(use_res)}"
    within(name, "dx", npy(dxv), out[torch.float32][0], out[torch.float64][0])
    within(name, "dgamma", npy(dgamma), out[torch.float32][1], out[torch.float64][1])
    within(name, "dbeta", npy(dbeta), out[torch.float32][2], out[torch.float64][2])
    if ld > C:
        assert torch.all(dxbuf[:, C:] == -777.25)


@pytest.mark.parametrize("rows,C,ld", BN_CASES)
def test_bn_two_runs_give_the_same_bits(rows, C, ld):
    from partmanip_amd import ops
    x, gamma, beta, res, dy, dy2, rm, rv = bn_inputs(rows, C, seed=2)
    runs = []
    for _ in range(2):
        h = hip_bn(x, gamma, beta, res, rm, rv, ld, True, True)
        dx, dm = torch.empty(rows, C, device=DEV), torch.empty(rows, C, device=DEV)
        dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ops.bn2d_bwd(dy.to(DEV), h["xv"], h["yv"], h["mean"], h["invstd"], gamma.to(DEV), dgamma, dbeta, dx, _ws(), relu=True,
                     dy2=dy2.to(DEV), dy_masked=dm)
        runs.append([npy(v) for v in (h["mean"], h["var"], h["invstd"], h["yv"], h["rm"], h["rv"], dx, dm, dgamma, dbeta)])
    for a, b in zip(*runs):
        assert same_bits(a, b)


def test_bn_nan_propagates_and_stays_in_its_channel():
    rows, C = 37, 64
    x, gamma, beta, res, _, _, rm, rv = bn_inputs(rows, C, seed=3)
    clean = hip_bn(x, gamma, beta, res, rm, rv, C, True, True)
    x2 = x.clone()
    x2[3, 5] = float("nan")
    h = hip_bn(x2, gamma, beta, res, rm, rv, C, True, True)
    for k in ("mean", "var", "invstd", "rm", "rv"):
        assert torch.isnan(h[k][5]), k
    assert torch.isnan(h["yv"][:, 5]).all()                             # through the ReLU too, as torch.relu
    keep = [c for c in range(C) if c != 5]
    for k in ("mean", "var", "invstd", "rm", "rv"):
        assert same_bits(npy(h[k])[keep], npy(clean[k])[keep]), k
    assert same_bits(npy(h["yv"])[:, keep], npy(clean["yv"])[:, keep])


def test_bn_training_statistics_refuse_a_single_value_per_channel():
    from partmanip_amd import ops
    x = torch.randn(1, 64, device=DEV)
    mean, invstd = torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    with pytest.raises(RuntimeError, match="PM_EINVAL"):
        ops.bn2d_stats(x, EPS, mean, invstd, _ws())
    with pytest.raises(ValueError):                                     # torch refuses the same case
        F.batch_norm(torch.randn(1, 64), None, None, None, None, True, MOM, EPS)


@pytest.mark.parametrize("rows,C,ld", BN_CASES)
def test_bn_eval_mode_with_given_running_statistics(rows, C, ld):
    from partmanip_amd import ops
    x, gamma, beta, res, _, _, rm, rv = bn_inputs(rows, C, seed=4)
    _, xv = _strided(rows, C, ld, src=x)
    _, yv = _strided(rows, C, ld)
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    invstd = ops.bn2d_invstd(rv_d, EPS, torch.empty(C, device=DEV))
    ops.bn2d_apply(xv, rm_d, invstd, gamma.to(DEV), beta.to(DEV), yv, res.to(DEV), True)
    y32, rm32, rv32 = ref_bn(x, gamma, beta, res, rm, rv, True, True, torch.float32, training=False)
    y64, _, _ = ref_bn(x, gamma, beta, res, rm, rv, True, True, torch.float64, training=False)
    within(f"bn2d eval {rows}x{C} ld {ld}", "y", npy(yv), y32.numpy(), y64.numpy())
    assert same_bits(npy(rm_d), rm.numpy()) and same_bits(npy(rv_d), rv.numpy()) and torch.equal(rm32, rm) and torch.equal(rv32, rv)


def test_bn_wrappers_check_their_arguments():
    from partmanip_amd import ops
    x = torch.randn(8, 64, device=DEV)
    v = torch.empty(64, device=DEV)
    with pytest.raises(ValueError):
        ops.bn2d_stats(x[:, :62], EPS, v, v, _ws())                     # C % 4
    with pytest.raises(ValueError):
        ops.bn2d_stats(x, EPS, v[:32], v, _ws())                        # a per-channel vector of the wrong length
    with pytest.raises(ValueError):
        ops.bn2d_apply(x, v, v, v, v, torch.empty(4, 64, device=DEV))   # rows
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bn2d_apply(x.cpu(), v, v, v, v, x)


# ------------------------------------------------------------------------------------------------------------------------- pools
def pool_input(kind, B, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    if kind == "ties":
        x = torch.round(x * 2) / 2                                       # a handful of levels: every window holds exact ties
    elif kind == "negative":
        x = -x.abs() - 1.0                                               # zero padding would win; torch pads with -inf
    elif kind == "nan":
        x.view(-1)[torch.randperm(x.numel(), generator=g)[: x.numel() // 50]] = float("nan")
    return x


def rows_of(x_nchw):
    B, C, H, W = x_nchw.shape
    return x_nchw.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


@pytest.mark.parametrize("H,W", [(5, 7), (36, 64)])
@pytest.mark.parametrize("kind", ["random", "ties", "negative", "nan"])
def test_max_pool_forward_equals_torch(H, W, kind):
    from partmanip_amd import ops
    B, C = 2, 64
    x = pool_input(kind, B, C, H, W)
    want, widx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    Ho, Wo = want.shape[2:]
    assert (Ho, Wo) == (ops.pool2d_out(H), ops.pool2d_out(W))
    y = torch.empty(B * Ho * Wo, C, device=DEV)
    idx = torch.empty(B * Ho * Wo, C, dtype=torch.int32, device=DEV)
    ops.pool2d_max_fwd(rows_of(x).to(DEV), B, H, W, y, idx)
    assert same_bits(npy(y), rows_of(want).numpy())
    assert np.array_equal(npy(idx), rows_of(widx).numpy())
    if kind == "nan":
        assert np.isnan(npy(y)).any()


@pytest.mark.parametrize("H,W", [(5, 7), (36, 64)])
@pytest.mark.parametrize("kind", ["random", "ties"])
def test_max_pool_backward(H, W, kind):
    from partmanip_amd import ops
    B, C = 2, 64
    x = pool_input(kind, B, C, H, W, seed=1)
    g = torch.Generator().manual_seed(5)
    Ho, Wo = ops.pool2d_out(H), ops.pool2d_out(W)
    dy, dy2 = torch.randn(B, C, Ho, Wo, generator=g), torch.randn(B, C, Ho, Wo, generator=g)
    y = torch.empty(B * Ho * Wo, C, device=DEV)
    idx = torch.empty(B * Ho * Wo, C, dtype=torch.int32, device=DEV)
    ops.pool2d_max_fwd(rows_of(x).to(DEV), B, H, W, y, idx)
    for second in (False, True):
        dtot = dy + dy2 if second else dy
        out = {}
        for dtype in (torch.float32, torch.float64):
            xx = x.detach().to(dtype).clone().requires_grad_(True)
            F.max_pool2d(xx, 3, 2, 1).backward(dtot.to(dtype))
            out[dtype] = rows_of(xx.grad).numpy()
        dx = torch.full((B * H * W, C), -777.25, device=DEV)
        ops.pool2d_max_bwd(rows_of(dy).to(DEV), idx, B, H, W, dx, dy2=rows_of(dy2).to(DEV) if second else None)
        within(f"pool2d_max_bwd {H}x{W} {kind}", "dx (dy + dy2)" if second else "dx", npy(dx), out[torch.float32], out[torch.float64])
        dx2 = torch.empty_like(dx)
        ops.pool2d_max_bwd(rows_of(dy).to(DEV), idx, B, H, W, dx2, dy2=rows_of(dy2).to(DEV) if second else None)
        assert same_bits(npy(dx), npy(dx2))


def test_global_average_pool():
    from partmanip_amd import ops
    B, C, H, W, tail = 2, 512, 3, 4, 5
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, C, H, W, generator=g) + 0.5
    fbuf = torch.full((B, C + tail), -777.25, device=DEV)
    ops.pool2d_avg_fwd(rows_of(x).to(DEV), B, H * W, fbuf)
    within("pool2d_avg", "y", npy(fbuf[:, :C]), x.mean(dim=(2, 3)).numpy(), x.double().mean(dim=(2, 3)).numpy())
    assert torch.all(fbuf[:, C:] == -777.25)
    dy = torch.randn(B, C + tail, generator=g)
    dx = torch.empty(B * H * W, C, device=DEV)
    ops.pool2d_avg_bwd(dy.to(DEV), B, H * W, dx)
    want = lambda dt: rows_of((dy[:, :C].to(dt) / (H * W))[:, :, None, None].expand(B, C, H, W)).numpy()     # noqa: E731
    within("pool2d_avg", "dx", npy(dx), want(torch.float32), want(torch.float64))


def test_stem_patch_matrix_equals_unfold():
    from partmanip_amd import ops
    B, H, W, tail = 3, 72, 128, 5
    g = torch.Generator().manual_seed(7)
    obs = torch.rand(B, H * W + tail, generator=g)
    cols = torch.full((B * 36 * 64, 64), -777.25, device=DEV)
    ops.im2col2d_c1(obs.to(DEV)[:, :H * W], H, W, 7, 2, 3, cols)
    want = F.unfold(obs[:, :H * W].view(B, 1, H, W), 7, padding=3, stride=2).transpose(1, 2).reshape(B * 36 * 64, 49)
    assert same_bits(npy(cols[:, :49]), want.numpy())
    assert torch.all(cols[:, 49:] == 0)
