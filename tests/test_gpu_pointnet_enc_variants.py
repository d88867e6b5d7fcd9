"""Every PointNet encoder kernel at the level of its entry point (ops.pointnet_enc_*), on the cases of tests/pointnet_enc_cases.py.
GPU box only.

Exact tier (ReLU, the generic instantiations): integer data on which every float32 summation order is exact, so features,
arg-max (ties included: the lowest index), saved layer 2 and the six gradients are compared BIT FOR BIT with the float64
restatement; the backward runs on hand-made arg-max tables.  fp64 tier (tanh, the production kernels): the stated tolerances of
tests/test_gpu_pointnet_screen.py, test_pointnet_forward_backward, test_pointnet_bf16x3_forward and
test_pointnet_bf16x6_backward_has_fp32_class_error against float64, plus a per-row bound on dW3 from a float32 torch-CPU
evaluation of the same algebra.  Non-finite tier: NaN / inf coordinates through the ReLU and ELU kernels and a NaN row through
the three Linear forward paths, against torch.

Every input is a view surrounded by NaN (x rows carry a NaN tail: ldx > P * C), every output a view inside a sentinel-filled
buffer that must come back untouched outside the view; feat / dfeat rows are 1024 floats apart or more.  dW1 is (128, C) with no
pad columns: the kernels keep 8 columns per channel in their partial sums and pn_bwd_reduce2_kernel writes the first C only.

Observed on MI355X (worst over the fp64 cases; every test prints its own and records them with tests.helpers.record_margin):
  forward, max feature / mean against fp64 layer 3 of the kernel's own h2, tolerance 3e-6 (bf16x3: 1e-4)
    pn_fwd_kernel 6.1e-07 / 8.0e-07    pn_fwd_screen_kernel 1.5e-07 / 8.2e-08 (both schedules bit-equal)
    pn_fwd_bf6_kernel 4.9e-07 / 8.0e-07    pn_fwd_bf3_kernel 3.9e-06 / 2.4e-06; against the whole network in fp64: 7.2e-07 (bf16x3 5.4e-06)
  backward, worst tensor (max abs / max|ref|; gate 1e-4), float32 torch-CPU on the same algebra: 4.7e-06
    pn_bwd16_kernel 3.2e-06    pn_bwd_kernel recompute and saved 5.6e-06 (db2 at P = 4096)    pn_bwd_bf6_kernel 3.1e-06
  worst row of dW3: kernels 1.0e-06 .. 2.1e-06, float32 torch-CPU 2.7e-06; at most 0.28 of the bound 4 x yardstick + 1 ulp
The exact tier found nothing wrong in the encoder kernels; the non-finite tier fails without the NaN rule of pm_act's ReLU."""
import functools

import numpy as np
import pytest
import torch

from partmanip_amd import ops
from tests import linear_variant_cases as LV
from tests import pointnet_enc_cases as PC
from tests.exact_gemm import DEV, SENT, GUARD, _view, _input, _outside_intact
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@functools.lru_cache(maxsize=1)
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ref_of(c):
    return PC.reference(c["id"], cu_count())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32_of(ref64):
    return (np.asarray(ref64) + 0.0).astype(np.float32)              # a zero is +0: every kernel sum starts from +0


def out(shape, ld=0):
    """(buffer, view, the view's place for _outside_intact) of an output inside a SENT-filled buffer."""
    buf, v = _view(shape, ld, 0, SENT)
    rows, cols = shape if len(shape) == 2 else (1, shape[0])
    return buf, v, [(GUARD, rows, cols, max(ld, cols))]


class Operands:
    """The device side of a case: NaN-surrounded inputs and the packed operands of every kernel family (built on demand)."""

    def __init__(self, c, x, w):
        self.c, self.B, self.P, self.C = c, x.shape[0], c["P"], c["C"]
        self.x = _input(x.reshape(self.B, -1), self.P * self.C + c["tail"], 0)
        assert self.x.stride(0) > self.P * self.C
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = (_input(a, 0, 0) for a in w)
        self.packed = torch.empty(ops.pointnet_packed_elems(), device=DEV)
        ops.pointnet_pack(self.W2, self.W3, self.packed)
        self.ws = ops.Workspace(DEV)

    @functools.cached_property
    def packed_s(self):
        p = torch.empty(ops.pointnet_packed_screen_bytes(), dtype=torch.uint8, device=DEV)
        ops.pointnet_pack_screen(self.W3, self.b3, p)
        return p

    @functools.cached_property
    def packed3(self):
        p = torch.empty(int(ops.lib.pm_pointnet_packed_bf3_bytes()), dtype=torch.uint8, device=DEV)
        ops.pointnet_pack_bf3(self.W2, self.W3, p)
        return p

    @functools.cached_property
    def packed6(self):
        p = torch.empty(int(ops.lib.pm_pointnet_packed_bf6_bytes()), dtype=torch.uint8, device=DEV)
        ops.pointnet_pack_bf6(self.W2, self.W3, p)
        return p

    @functools.cached_property
    def packed6b(self):
        p = torch.empty(int(ops.lib.pm_pointnet_packed_bwd_bf6_bytes()), dtype=torch.uint8, device=DEV)
        ops.pointnet_pack_bwd_bf6(self.W2, p)
        return p

    def forward(self, entry, save_h2=True, act=None, x=None):
        """Runs one forward entry into poisoned outputs, checks that nothing outside them changed; numpy (feat, argmax, h2)."""
        c, B, P, C = self.c, self.B, self.P, self.C
        x = self.x if x is None else x
        ncol = PC.C3 * (2 if c["max_mean"] else 1)
        fbuf, feat, fpl = out((B, ncol), c["ldf"])
        abuf, am = PC.argmax_buffer(B)
        hbuf, h2, hpl = out((B * P, PC.C2)) if save_h2 else (None, None, None)
        act = c["act"] if act is None else act
        a = (x, P, C, c["sub_mean"], self.W1, self.b1, self.b2, self.b3)
        if entry == "f32":
            ops.pointnet_enc_fwd(*a, self.packed, c["max_mean"], feat, am, h2, act=act)
        elif entry in ("screen0", "screen1"):
            ops.pointnet_enc_fwd_screen(*a, self.packed, self.packed_s, c["max_mean"], feat, am, h2, schedule=int(entry[-1]))
        elif entry == "bf3":
            ops.pointnet_enc_fwd_bf3(*a, self.packed3, c["max_mean"], feat, am, h2)
        elif entry == "bf6":
            ops.pointnet_enc_fwd_bf6(*a, self.packed6, c["max_mean"], feat, am, h2)
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
        assert _outside_intact(fbuf, fpl), f"{entry}: wrote outside feat"
        assert PC.argmax_outside_intact(abuf, B), f"{entry}: wrote outside argmax"
        if save_h2:
            assert _outside_intact(hbuf, hpl), f"{entry}: wrote outside h2_save"
        return feat.cpu().numpy(), am.cpu().numpy(), (h2.cpu().numpy().reshape(B, P, PC.C2) if save_h2 else None)

    def backward(self, entry, argmax, dfeat, h2):
        """Runs one backward entry (h2: the float32 layer 2 handed to the saved-layer-2 kernels) into poisoned outputs, checks that
        nothing outside them changed; {name: numpy gradient}."""
        c, B, P, C = self.c, self.B, self.P, self.C
        shapes = dict(dW1=(PC.C1, C), db1=(PC.C1,), dW2=(PC.C2, PC.C1), db2=(PC.C2,), dW3=(PC.C3, PC.C2), db3=(PC.C3,))
        o = {k: out(s) for k, s in shapes.items()}
        g = [o[k][1] for k in PC.GRADS]
        df = _input(dfeat, c["ldf"], 0)
        am = torch.from_numpy(np.array(argmax, dtype=np.int32)).to(DEV)
        h2d = None if entry == "recompute" else _input(np.asarray(h2).reshape(B * P, PC.C2), 0, 0)
        a = (self.x, P, C, c["sub_mean"], self.W1, self.b1, self.b2, self.W3, self.packed)
        if entry == "bf6":
            ops.pointnet_enc_bwd_bf6(*a, self.packed6b, c["max_mean"], df, am, *g, self.ws, h2d)
        else:
            ops.pointnet_enc_bwd(*a, c["max_mean"], df, am, *g, self.ws, h2_saved=h2d, act=c["act"], four_wave=(entry == "saved4"))
        torch.cuda.synchronize()
        for k in PC.GRADS:
            assert _outside_intact(o[k][0], o[k][2]), f"{entry}: wrote outside {k}"
        return {k: o[k][1].cpu().numpy() for k in PC.GRADS}


# ================================================================================================ exact tier
@pytest.mark.parametrize("save_h2", [True, False], ids=["h2_save", "no_h2"])
@pytest.mark.parametrize("c", PC.EXACT_FWD, ids=lambda c: c["id"])
def test_exact_forward(c, save_h2):
    d = ref_of(c)
    r = d["fwd"]
    feat, am, h2 = Operands(c, d["x"], d["w"]).forward("f32", save_h2)
    assert np.array_equal(am, r["argmax"]), f"arg-max differs at {int((am != r['argmax']).sum())} pairs (ties go to the lowest index)"
    assert np.array_equal(bits(feat[:, :PC.C3]), bits(f32_of(r["max"])))
    if c["max_mean"]:
        assert np.array_equal(bits(feat[:, PC.C3:]), bits(f32_of(r["mean"])))
    if save_h2:
        assert np.array_equal(bits(h2), bits(f32_of(r["h2"])))


@pytest.mark.parametrize("c", PC.EXACT_BWD, ids=lambda c: c["id"])
def test_exact_backward_on_the_argmax_tables(c):
    d = ref_of(c)
    dv = Operands(c, d["x"], d["w"])
    for entry, kernel in PC.bwd_entries(c):
        got = dv.backward(entry, d["argmax"], d["dfeat_t"], d["fwd"]["h2"])
        for k in PC.GRADS:
            want = f32_of(d["bwd"][k])
            same = bits(got[k]) == bits(want)
            assert same.all(), (f"{kernel} {k}: {int((~same).sum())} of {same.size} values differ, first at {np.argwhere(~same)[0].tolist()} "
                                f"(got {got[k][~same][0]}, want {want[~same][0]}); tables {''.join(PC.tables_of(c, dv.B))}")


# ================================================================================================ fp64 tier
FEAT_TOL, GAP = 3e-6, 1e-5                     # tests/test_gpu_pointnet_screen.py
BF3_TOL, BF3_GAP = 1e-4, 1e-3                  # test_pointnet_bf16x3_forward


@pytest.mark.parametrize("c", PC.F64_FWD, ids=lambda c: c["id"])
def test_fp64_forward_of_every_entry(c):
    d = ref_of(c)
    r = d["fwd"]
    dv = Operands(c, d["x"], d["w"])
    W3, b3 = d["w"][4].astype(np.float64), d["w"][5].astype(np.float64)
    res = {}
    for entry, kernel in PC.fwd_entries(c):
        tol, gap = (BF3_TOL, BF3_GAP) if entry == "bf3" else (FEAT_TOL, GAP)
        feat, am, h2 = dv.forward(entry)
        res[entry] = (feat, am, h2)
        z = h2.astype(np.float64) @ W3.T + b3                                  # float64 layer 3 of this kernel's own saved h2
        zs = np.sort(z, axis=1)
        clear = (zs[:, -1] - zs[:, -2]) > gap
        scale = np.abs(z.max(axis=1)).max()
        assert am.min() >= 0 and am.max() < c["P"]
        e_max = np.abs(feat[:, :PC.C3] - z.max(axis=1)).max() / scale
        e_own = np.abs(feat[:, :PC.C3] - np.take_along_axis(z, am[:, None, :].astype(np.int64), 1)[:, 0]).max() / scale
        e_net = np.abs(feat[:, :PC.C3] - r["max"]).max() / np.abs(r["max"]).max()      # the whole network in float64
        msg = f"{c['id']} {kernel}: max {e_max:.2e} own-argmax {e_own:.2e} whole-net {e_net:.2e} under the gap {int((~clear).sum())}"
        record_margin(f"{kernel} max feature vs fp64 layer 3 of own h2", e_max, tol)
        assert np.array_equal(am[clear], z.argmax(axis=1)[clear]), msg
        if c["max_mean"]:
            mscale = np.abs(z.mean(axis=1)).max()
            e_mean = np.abs(feat[:, PC.C3:] - z.mean(axis=1)).max() / mscale
            msg += f" mean {e_mean:.2e}"
            record_margin(f"{kernel} mean feature vs fp64 layer 3 of own h2", e_mean, tol)
            assert e_mean < tol, msg
        print(msg)
        assert e_max < tol and e_own < tol and e_net < tol, msg
    for entry in ("screen0", "screen1"):                                       # layers 1-2 are the dense kernel's; the schedules agree
        assert np.array_equal(bits(res[entry][2]), bits(res["f32"][2])), entry
    assert np.array_equal(bits(res["screen0"][0]), bits(res["screen1"][0])) and np.array_equal(res["screen0"][1], res["screen1"][1])


def _rel_max(got, ref):
    s = np.abs(ref).max()
    return float(np.abs(got - ref).max() / s) if s > 0 else float(np.abs(got).max())


def _rel_l2(got, ref):
    s = np.linalg.norm(ref)
    return float(np.linalg.norm(got - ref) / s) if s > 0 else float(np.linalg.norm(got))


def _row_err(got, ref):
    """Per row of dW3: max |got - ref| over the row / max |ref| over the row."""
    return np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)


@pytest.mark.parametrize("c", PC.F64_BWD, ids=lambda c: c["id"])
def test_fp64_backward_on_the_argmax_tables(c):
    """Every backward entry on the hand-made tables with random float dfeat, against backward64 fed the float32 layer 2 that the
    fp32 forward saved.  Beside the project's gates, per row of dW3: error <= 4 x the worst row of the float32 torch-CPU
    evaluation of the same algebra (the yardstick, never the kernel) + one float32 ulp of the row's scale."""
    d = ref_of(c)
    dv = Operands(c, d["x"], d["w"])
    _, _, h2 = dv.forward("f32")
    args = (d["x"], d["w"], c["act"], c["sub_mean"], c["max_mean"], d["argmax"], d["dfeat_t"])
    ref = PC.backward64(*args, h2=h2)
    yard = PC.backward64(*args, h2=h2, dtype=torch.float32)
    zero = all(np.abs(ref[k]).max() == 0 for k in PC.GRADS)                     # a batch of one cloud under table f
    y_rows = _row_err(yard["dW3"].astype(np.float64), ref["dW3"])
    y_worst = float(y_rows.max()) if not zero else 0.0
    e32 = None
    for entry, kernel in PC.bwd_entries(c):
        got = {k: v.astype(np.float64) for k, v in dv.backward(entry, d["argmax"], d["dfeat_t"], h2).items()}
        l2 = {k: _rel_l2(got[k], ref[k]) for k in PC.GRADS}
        if entry == "saved16":
            e32 = l2
        line = []
        for k in PC.GRADS:
            e, ey = _rel_max(got[k], ref[k]), _rel_max(yard[k].astype(np.float64), ref[k])
            line.append(f"{k} {e:.1e} (f32 torch {ey:.1e})")
            record_margin(f"{kernel} {k} vs fp64 (max abs / max|ref|); float32 torch-CPU: {ey:.2e}", e, 1e-4, yardstick=ey, case=c["id"])
            if entry == "bf6":
                tol = max(1.5 * e32[k] + 2e-7, 2e-6)
                record_margin(f"{kernel} {k} vs fp64, relative L2 (fp32 kernel: {e32[k]:.2e})", l2[k], tol, case=c["id"])
                assert l2[k] <= tol and l2[k] < 2e-4, (c["id"], kernel, k, l2[k], e32[k])
            else:
                assert e < 1e-4, (c["id"], kernel, k, e)
        rows = _row_err(got["dW3"], ref["dW3"]) if not zero else np.zeros(PC.C3)
        bound = 4 * y_worst + ULP
        record_margin(f"{kernel} worst dW3 row vs fp64; float32 torch-CPU worst row: {y_worst:.2e}", float(rows.max()), bound, case=c["id"])
        print(f"{c['id']} {kernel}: " + ", ".join(line) + f"; worst dW3 row {rows.max():.1e} (f32 torch {y_worst:.1e})")
        assert (rows <= bound).all(), (c["id"], kernel, int(rows.argmax()), float(rows.max()), y_worst)


# ================================================================================================ non-finite tier
NONFINITE = PC.NONFINITE


@pytest.mark.parametrize("act", [PC.RELU, PC.ELU], ids=lambda a: PC.ACT_NAME[a])
def test_nan_coordinate_poisons_its_cloud_like_torch(act):
    """A NaN coordinate at points 5 and 200 of cloud 1: torch's max / mean over the points give NaN for every channel of that cloud
    and torch.max the index of the first NaN; the other clouds must not change by a bit."""
    c = NONFINITE
    d = ref_of(c)
    dv = Operands(c, d["x"], d["w"])
    clean = dv.forward("f32", act=act)
    x = d["x"].copy()
    x[1, 5, 1] = x[1, 200, 0] = np.nan
    bad = dv.forward("f32", act=act, x=_input(x.reshape(dv.B, -1), dv.P * dv.C + c["tail"], 0))
    assert np.isnan(bad[0][1]).all(), f"{int((~np.isnan(bad[0][1])).sum())} of 1024 features of the NaN cloud are not NaN"
    assert (bad[1][1] == 5).all()
    for b in (0, 2):
        assert np.array_equal(bits(bad[0][b]), bits(clean[0][b])) and np.array_equal(bad[1][b], clean[1][b]), b
        assert np.array_equal(bits(bad[2][b]), bits(clean[2][b])), b
    x32 = torch.from_numpy(x).float()
    t_ref = PC.forward64(x32, *d["w"], act, False, True, dtype=torch.float32)
    assert np.isnan(t_ref["max"][1]).all() and np.isnan(t_ref["mean"][1]).all() and (t_ref["argmax"][1] == 5).all()


@pytest.mark.parametrize("act", [PC.RELU, PC.ELU], ids=lambda a: PC.ACT_NAME[a])
def test_infinite_coordinates_give_torchs_pattern(act):
    """+inf in one coordinate of a point, -inf in one of another, through integer weights chosen so that all four outcomes occur
    whatever the summation order: W1, W2 all +1 (layer 2 of the +inf point is +inf everywhere; ReLU / ELU make the -inf point
    finite), W3 row c all +1 (c % 4 == 0: +inf max and mean), all -1 (1: finite max, -inf mean), +1 with zeros (2: 0 * inf = NaN),
    +1 and -1 mixed (3: inf - inf = NaN).  The pattern of NaN / +inf / -inf of feat against torch CPU float32."""
    c = NONFINITE
    d = ref_of(c)
    rng = np.random.default_rng(9)
    W3 = np.ones((PC.C3, PC.C2))
    W3[1::4] = -1
    W3[2::4] = rng.integers(0, 2, size=(PC.C3 // 4, PC.C2))
    W3[3::4] = rng.integers(0, 2, size=(PC.C3 // 4, PC.C2)) * 2 - 1
    w = (np.ones((PC.C1, c["C"])), d["w"][1], np.ones((PC.C2, PC.C1)), d["w"][3], W3, d["w"][5])
    x = d["x"].copy()
    x[0, 300, 2] = np.inf
    x[2, 9, 0] = -np.inf
    x[2, 77, 1] = np.inf
    feat, am, _ = Operands(c, x, w).forward("f32", act=act)
    r = PC.forward64(torch.from_numpy(x).float(), *w, act, False, True, dtype=torch.float32)
    want = np.concatenate([r["max"], r["mean"]], axis=1)
    assert np.array_equal(np.isnan(feat), np.isnan(want)), int((np.isnan(feat) != np.isnan(want)).sum())
    assert np.array_equal(np.isinf(feat), np.isinf(want)) and np.array_equal(np.sign(feat[np.isinf(want)]), np.sign(want[np.isinf(want)]))
    for kind in (np.isnan(want), want == np.inf, want == -np.inf, np.isfinite(want)):
        assert kind[0].any() and kind[2].any()                                   # all four outcomes, in both touched clouds
    assert np.isfinite(want[1]).all()
    first_nan = np.isnan(r["z3"]).argmax(axis=1)
    nan_ch = np.isnan(want[:, :PC.C3])
    assert np.array_equal(am[nan_ch], first_nan[nan_ch])                         # the index of the first NaN, as torch.max


@pytest.mark.parametrize("cid", list(PC.LINEAR_NAN_SHAPES), ids=lambda s: PC.LINEAR_NAN_SHAPES[s])
def test_linear_forward_nan_row_propagates_like_torch(cid):
    """Row 7 of X holds a NaN: row 7 of Y is NaN wherever torch's is (everywhere: no weight is zero), for each of the seven
    activations, and every other row is bit-equal to the clean run."""
    p = {c["id"]: c for c in LV.CASES}[cid]["probs"][0]
    M, N, K = p["M"], p["N"], p["K"]
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2, torch.randn(N, generator=g)
    xb = x.clone()
    xb[7, K // 2] = float("nan")
    fns = {0: lambda z: z, 1: torch.tanh, 2: torch.relu, 3: torch.nn.functional.leaky_relu, 4: torch.nn.functional.elu,
           5: torch.nn.functional.selu, 6: torch.sigmoid}
    wd, bd = w.to(DEV), b.to(DEV)
    for act, fn in fns.items():
        ys = []
        for xi in (x, xb):
            y = torch.full((M, N), SENT, device=DEV)
            ops.linear_fwd(xi.to(DEV), wd, bd, y, act)
            torch.cuda.synchronize()
            ys.append(y.cpu())
        want_nan = torch.isnan(fn(torch.nn.functional.linear(xb, w, b)))
        assert want_nan[7].all() and not want_nan[torch.arange(M) != 7].any()
        assert torch.equal(torch.isnan(ys[1]), want_nan), (cid, act, int(torch.isnan(ys[1][7]).sum()), N)
        keep = torch.arange(M) != 7
        assert torch.equal(ys[1][keep].view(torch.int32), ys[0][keep].view(torch.int32)), (cid, act)
