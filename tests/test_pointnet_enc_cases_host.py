"""The case table of the op-level PointNet encoder tests (tests/pointnet_enc_cases.py), checked on the host: the float64
backward against torch autograd, the exact cases inside the range where every float32 summation order is exact, their ties,
the coverage of the kernel list, and the top-2 gaps of the float cases."""
import numpy as np
import pytest
import torch

from tests import pointnet_enc_cases as PC
from tests import linear_variant_cases as LV

LIMIT = 2.0 ** 24


@pytest.mark.parametrize("act", [PC.TANH, PC.RELU, PC.ELU], ids=lambda a: PC.ACT_NAME[a])
@pytest.mark.parametrize("sub_mean", [False, True])
@pytest.mark.parametrize("max_mean", [False, True])
def test_backward64_is_autograd_through_a_gather_at_the_pinned_indices(act, sub_mean, max_mean):
    B, P, C = 3, 64, 4
    g = torch.Generator().manual_seed(7 + act)
    x = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    shapes = ((PC.C1, C), (PC.C1,), (PC.C2, PC.C1), (PC.C2,), (PC.C3, PC.C2), (PC.C3,))
    w = [(torch.randn(s, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True) for s in shapes]
    am = torch.randint(0, P, (B, PC.C3), generator=g)
    dfeat = torch.randn(B, PC.C3 * (2 if max_mean else 1), generator=g, dtype=torch.float64)
    h1 = PC._act(PC.centre(x, sub_mean) @ w[0].t() + w[1], act)
    h2 = PC._act(h1 @ w[2].t() + w[3], act)
    z3 = h2 @ w[4].t() + w[5]
    feat = z3.gather(1, am[:, None, :])[:, 0]
    if max_mean:
        feat = torch.cat([feat, z3.mean(dim=1)], dim=1)
    ref = torch.autograd.grad((feat * dfeat).sum(), w)
    wn = tuple(t_.detach().numpy() for t_ in w)
    for h2_in in (None, h2.detach().numpy()):
        got = PC.backward64(x.numpy(), wn, act, sub_mean, max_mean, am.numpy(), dfeat.numpy(), h2=h2_in)
        for k, r in zip(("dW1", "db1", "dW2", "db2", "dW3", "db3"), ref):
            r = r.numpy()
            assert np.abs(got[k] - r).max() <= 1e-12 * max(np.abs(r).max(), 1.0), k


def _ints(a):
    assert np.array_equal(a, np.rint(a)), "not integer-valued"
    return np.abs(a)


def _budget(c, d):
    """Every accumulation of the forward and the backward of an exact case with its terms replaced by their absolute values, as
    {name: largest sum}.  All values are integers far below 2^53, so the float64 products here ARE the int64 ones (checked by
    converting); a kernel may add the terms of any of these sums in any order and stay exact while the sum of |terms| < 2^24."""
    x, (W1, b1, W2, b2, W3, b3), P = d["x"], d["w"], c["P"]
    B = x.shape[0]
    xc = PC.centre(torch.from_numpy(x.copy()), c["sub_mean"]).numpy()
    a = lambda v: _ints(np.asarray(v))                                                                      # noqa: E731
    h1 = np.maximum(xc @ W1.T + b1, 0)
    h2 = np.maximum(h1 @ W2.T + b2, 0)
    out = {"centre": a(x[..., :3]).sum(axis=1).max() if c["sub_mean"] else 0,
           "layer 1": (a(xc) @ a(W1).T + a(b1)).max(), "layer 2": (a(h1) @ a(W2).T + a(b2)).max(), "layer 3": (a(h2) @ a(W3).T + a(b3)).max(),
           "mean column sums": a(d["fwd"]["z3"]).sum(axis=1).max(), "h2 column sums": a(h2).sum(axis=1).max()}
    if "bwd" in d:
        bw, df = d["bwd"], d["dfeat_t"]
        assert np.array_equal(bw["h2"].reshape(B, P, -1), h2)
        G, dz2, dz1 = a(bw["G"]), a(bw["dz2"]), a(bw["dz1"])
        dmean = a(df[:, PC.C3:]) if c["max_mean"] else np.zeros((B, PC.C3))
        out.update({"U": (dmean @ a(W3)).max(), "dh2": (G @ a(W3)).max(), "dW3": (G.T @ a(h2).reshape(B * P, -1)).max(), "db3": G.sum(0).max(),
                    "db3 as the kernel adds it (dmax + dmean)": (a(df[:, :PC.C3]) + dmean).sum(0).max(),
                    "dW2": (dz2.T @ a(bw["h1"])).max(), "db2": dz2.sum(0).max(), "dh1": (dz2 @ a(W2)).max(),
                    "dW1": (dz1.T @ a(bw["xc"])).max(), "db1": dz1.sum(0).max()})
        for k in PC.GRADS:
            _ints(bw[k])
    return {k: int(np.int64(v)) for k, v in out.items()}


@pytest.mark.parametrize("c", PC.EXACT_FWD + PC.EXACT_BWD, ids=lambda c: c["id"])
def test_exact_case_is_exact_under_any_summation_order(c):
    d = PC.reference(c["id"])
    for k, v in _budget(c, d).items():
        assert v < LIMIT, (c["id"], k, v)
    if c["sub_mean"]:
        assert np.array_equal(d["x"][..., :3].sum(axis=1) % c["P"], np.zeros((d["x"].shape[0], 3)))


@pytest.mark.parametrize("c", PC.EXACT_FWD, ids=lambda c: c["id"])
def test_exact_forward_case_holds_ties_of_every_kind(c):
    """A tie = a (cloud, channel) pair whose maximum is reached at its first index p and again at q: q = p + 32 inside one 64-point
    tile (the lane-half exchange of the kernels), q in a later tile (there is one only where P > 64), and p = 0 with q = P - 1."""
    z, am, P = PC.reference(c["id"])["fwd"]["z3"], PC.reference(c["id"])["fwd"]["argmax"], c["P"]
    at_max = z == z.max(axis=1, keepdims=True)                                   # (B, P, 512)
    b, ch = np.nonzero(am < P - 32)
    p = am[b, ch]
    lane_half = ((p % 64) < 32) & at_max[b, p + 32, ch]
    assert lane_half.any()
    tiles = at_max.reshape(z.shape[0], P // 64, 64, -1).any(axis=2)              # (B, tiles, 512)
    if P > 64:
        assert (tiles.sum(axis=1) > 1).any()
    assert ((am == 0) & at_max[:, P - 1]).any()
    print(c["id"], "pairs with a tie:", float((at_max.sum(axis=1) > 1).mean()))


def test_every_listed_kernel_is_exercised():
    fwd, bwd = set(), set()
    for c in PC.EXACT_FWD + PC.F64_FWD:
        fwd |= {k for _, k in PC.fwd_entries(c)}
    for c in PC.EXACT_BWD + PC.F64_BWD:
        bwd |= {k for _, k in PC.bwd_entries(c)}
    assert len(PC.FWD_KERNELS) == 6 + 6 + 3 + 3 and len(PC.BWD_KERNELS) == 12 + 6 + 3
    uncovered = [k for k in PC.FWD_KERNELS if k not in fwd] + [k for k in PC.BWD_KERNELS if k not in bwd]
    assert not uncovered, "kernels no case runs:\n" + "\n".join(uncovered)
    assert fwd <= set(PC.FWD_KERNELS) and bwd <= set(PC.BWD_KERNELS)
    # the generic instantiations by an exact case, the tanh ones by an fp64 case
    assert all("generic" in k for c in PC.EXACT_FWD + PC.EXACT_BWD for _, k in PC.fwd_entries(c) + PC.bwd_entries(c))
    # every table on every backward entry, at the walk-two-clouds batches too
    for cases in (PC.EXACT_BWD, PC.F64_BWD):
        for P in (64, 128, 512, 4096):
            assert {t_ for c in cases if c["P"] == P for t_ in PC.tables_of(c, PC.batch(c))} == set(PC.TABLES), P
        assert {PC.batch(c) for c in cases if c["P"] == 64} >= {3, 256 + 3, PC.BWD_MAXG + 3}
    assert all(c["ldf"] >= 1024 and c["tail"] > 0 for c in PC.ALL) and {c["ldf"] > 1024 for c in PC.ALL} == {True, False}


@pytest.mark.parametrize("c", PC.F64_FWD + PC.F64_BWD, ids=lambda c: c["id"])
def test_float_case_has_few_near_ties(c):
    """At most 5e-2 of the (cloud, channel) pairs under the 1e-5 top-2 gap: the cap of test_pointnet_forward_backward."""
    z = np.sort(PC.reference(c["id"])["fwd"]["z3"], axis=1)
    gap = z[:, -1] - z[:, -2]
    assert (gap < 1e-5).mean() <= 5e-2, (c["id"], float((gap < 1e-5).mean()))


def test_nan_row_linear_shapes_name_the_three_paths():
    by_id = {c["id"]: c for c in LV.CASES}
    for cid, path in PC.LINEAR_NAN_SHAPES.items():
        c = by_id[cid]
        assert c["kind"] == "fwd" and c["expect"]["path"] == path and len(c["probs"]) == 1, cid
    M, N, K = (by_id["fwd-skinny-M256-N16"]["probs"][0][k] for k in "MNK")
    assert N <= 16 and M >= 256
