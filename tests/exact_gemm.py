"""What the exact known-answer GEMM tests share (tests/test_gpu_linear_variants.py, tests/test_gpu_sparse_conv_variants.py):
operands as views inside poisoned device buffers, integer data whose products and sums are exact in float32, the float64
reference, and the activation references with their documented error figures."""
import numpy as np
import torch

DEV = "cuda:0"
SENT = -777.25
GUARD = 64                                   # floats (256 bytes: keeps the 16-byte phase of the allocation)
NONE, TANH, RELU, LRELU, ELU, SELU, SIGMOID = range(7)
ACT_NAMES = {NONE: "none", TANH: "tanh", RELU: "relu", LRELU: "lrelu", ELU: "elu", SELU: "selu", SIGMOID: "sigmoid"}
SELU_L, SELU_A = np.float32(1.0507009873554804934193349852946), np.float32(1.6732632423543772848170429916717)


# ------------------------------------------------------------------------------------------------ poisoned buffers
def _view(shape, ld, off, fill, extra=0):
    """(buffer, view): the view has `shape` (1-D or 2-D, row stride ld), starts `off` floats past a 16-byte boundary and lies in a
    buffer of `fill`: GUARD floats before it, two more rows (+ `extra` floats: the slabs of a grouped weight gradient) and GUARD
    floats after."""
    rows, cols = shape if len(shape) == 2 else (1, shape[0])
    ld = max(ld, cols)
    buf = torch.full((GUARD + off + (rows + 2) * ld + extra + GUARD,), fill, device=DEV)
    v = buf.as_strided((rows, cols), (ld, 1), GUARD + off)
    assert (v.data_ptr() - 4 * off) % 16 == 0
    return buf, (v if len(shape) == 2 else v[0])


def _input(a, ld, off):
    """The integer-valued array `a` as a device view surrounded by NaN."""
    _, v = _view(a.shape, ld, off, float("nan"))
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return v


def _outside_intact(buf, views):
    """Every float of `buf` outside the (start, rows, cols, ld) views still holds the sentinel."""
    a = buf.cpu().numpy()
    m = np.ones(a.shape, dtype=bool)
    for start, rows, cols, ld in views:
        np.lib.stride_tricks.as_strided(m[start:], (rows, cols), (ld, 1))[...] = False
    return bool(np.array_equal(a[m].view(np.uint32), np.full(int(m.sum()), SENT, dtype=np.float32).view(np.uint32)))


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _mm(a, b):
    """a @ b in float64 (exact here), a zero always +0: a kernel's accumulator starts at +0, so a sum of -0 products is +0 too."""
    return a.astype(np.float64) @ b.astype(np.float64) + 0.0


def _ulps(got, ref64):
    """|got - ref| in units of 2^-23 |ref| (floored at 1e-30, the convention of test_fast_tanh_accuracy)."""
    return np.abs(got.astype(np.float64) - ref64) / (np.maximum(np.abs(ref64), 1e-30) * 2.0 ** -23)


# ------------------------------------------------------------------------------------------------ activations
def _act64(z, act):
    z = z.astype(np.float64)
    if act == TANH:
        return np.tanh(z)
    if act == LRELU:
        return np.where(z > 0, z, np.float64(np.float32(0.01)) * z)      # the slope the kernels and torch hold: float32(0.01)
    if act == ELU:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    if act == SELU:
        return 1.0507009873554804934193349852946 * np.where(z > 0, z, 1.6732632423543772848170429916717 * np.expm1(np.minimum(z, 0)))
    if act == SIGMOID:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    raise ValueError(act)


def _act_torch32(z, act):
    t = torch.from_numpy(z)
    f = {LRELU: torch.nn.functional.leaky_relu, ELU: torch.nn.functional.elu, SELU: torch.nn.functional.selu, SIGMOID: torch.sigmoid}[act]
    return f(t).numpy()


# What the device's libm documents for expf and expm1f (HIP math API, float: 1 ulp each): the floor under 4 e_ref for the activations
# built on them, for the cases where torch's own CPU evaluation happens to be exact at these integer z.  lrelu is one multiplication,
# the same one torch does: no floor.
DOCUMENTED_ULP = {LRELU: 0.0, ELU: 1.0, SELU: 1.0, SIGMOID: 1.0}


def _dact64(h, act):
    h = h.astype(np.float64)
    if act == NONE:
        return np.ones_like(h)
    if act == TANH:
        return 1.0 - h * h
    if act == RELU:
        return np.where(h > 0, 1.0, 0.0)
    if act == ELU:
        return np.where(h > 0, 1.0, h + 1.0)
    if act == SIGMOID:
        return h * (1.0 - h)
    raise ValueError(act)
