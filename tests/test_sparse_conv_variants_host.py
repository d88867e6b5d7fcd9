"""The kernel selection of the sparse-convolution entry points, asked of the library on the host (ops.sparse_conv_variant: no
launch, no device): every case of tests/sparse_conv_variant_cases.py selects the variant it names, and the table reaches every
variant the selector can name."""
import itertools

import pytest

from tests import sparse_conv_variant_cases as SV

MB = 1 << 20


@pytest.fixture(scope="module")
def ops():
    from partmanip_amd import ops as o
    return o


@pytest.mark.parametrize("c", SV.CASES, ids=[c["id"] for c in SV.CASES])
def test_case_selects_the_variant_it_names(ops, c):
    for act, key in ((1, "expect"), (0, "expect_noact")):
        got = SV.host_query(ops, c, act)
        want = c[key]
        assert {k: got[k] for k in want} == want, (c["id"], key, got)
        assert len(got["splits"]) == 1 and got["kchunk"][0] % 32 == 0 and got["kchunk"][0] > 0
        if c["kind"] != "bwd_weight":
            assert got["splits"] == [1]


def _case_bytes(c):
    total = 4 * c["rows"] * c["J"]                                       # the index table
    for name in SV.OPERANDS[c["kind"]]:
        shape = SV.operand_shape(c, name)
        total += 4 * shape[0] * (SV.ld_of(c, name) if len(shape) == 2 else 1)
    return total


def test_case_table_stays_small():
    """The cap tests/test_linear_variants_host.py states: 76 MB of operands per case, the index table counted."""
    for c in SV.CASES:
        assert _case_bytes(c) < 76 * MB, (c["id"], _case_bytes(c) / MB)


def test_weight_gradient_query_reports_the_slabs_the_call_chooses(ops):
    """splits and kchunk as the call's own heuristic picks them: one slab up to 64 rows; 100 rows over a 32 x 96 gradient are 2
    slabs of 64 rows, the last with 36 live ones; 65 rows leave the last slab a single row."""
    q = lambda rows, N, J, Cc: ops.sparse_conv_variant("bwd_weight", dict(                   # noqa: E731
        dY=SV.BASE_ADDR, lddy=N, src=SV.BASE_ADDR, lds=Cc, idx=SV.BASE_ADDR, rows=rows, J=J, C=Cc, dW=SV.BASE_ADDR, lddw=J * Cc,
        db=SV.BASE_ADDR, N=N, zero=SV.BASE_ADDR, workspace=0))
    for rows in (1, 31, 32, 33, 63, 64):
        r = q(rows, 32, 3, 32)
        assert r["splits"] == [1] and r["kchunk"] == [(rows + 31) // 32 * 32], (rows, r)
    for rows in (65, 100, 129, 4096):
        r = q(rows, 32, 3, 32)
        S, kc = r["splits"][0], r["kchunk"][0]
        assert S > 1 and kc % 32 == 0 and (S - 1) * kc < rows <= S * kc, (rows, r)
    assert q(100, 32, 3, 32)["splits"] == [2] and q(100, 32, 3, 32)["kchunk"] == [64]
    assert q(65, 32, 3, 32)["splits"] == [2] and q(65, 32, 3, 32)["kchunk"] == [64]


def test_query_rejects_what_the_launch_rejects(ops):
    B = SV.BASE_ADDR
    fwd = dict(src=B, lds=8, idx=B, rows=4, J=4, C=8, W=B, ldw=32, b=B, Y=B, ldy=4, N=4, act=0, zero=B)
    bwd = dict(dY=B, lddy=8, idxT=B, rows=4, J=4, Cout=8, Wt=B, ldwt=32, H=0, ldh=0, dX=B, lddx=4, Cin=4, act=0, zero=B)
    sca = dict(dY=B, lddy=32, W=B, ldw=32, idx=B, rows=4, J=4, C=8, Cout=32, H=0, dX=B, act=0)
    wgt = dict(dY=B, lddy=4, src=B, lds=8, idx=B, rows=4, J=4, C=8, dW=B, lddw=32, db=B, N=4, zero=B, workspace=0)
    for kind, good in (("fwd", fwd), ("bwd_data", bwd), ("bwd_scatter", sca), ("bwd_weight", wgt)):
        assert ops.sparse_conv_variant(kind, good)["path"] == "dma"
    bad = [("fwd", dict(fwd, J=3, ldw=24), "PM_EINVAL"),                 # J * C % 32 != 0
           ("bwd_data", dict(bwd, J=3, ldwt=24), "PM_EINVAL"),
           ("fwd", dict(fwd, C=6, lds=6, J=16, ldw=96), "PM_EINVAL"),    # C % 4 != 0
           ("bwd_data", dict(bwd, Cout=6, lddy=8, J=16, ldwt=96), "PM_EINVAL"),
           ("bwd_scatter", dict(sca, C=6, ldw=24), "PM_EINVAL"),
           ("bwd_weight", dict(wgt, C=6, lddw=24), "PM_EINVAL"),
           ("fwd", dict(fwd, zero=B + 4), "PM_EALIGN"),                  # a misaligned zero
           ("bwd_data", dict(bwd, zero=B + 8), "PM_EALIGN"),
           ("bwd_weight", dict(wgt, zero=B + 4), "PM_EALIGN"),
           ("fwd", dict(fwd, ldw=28), "PM_EINVAL"),                      # ldw < J * C
           ("bwd_data", dict(bwd, ldwt=28), "PM_EINVAL"),
           ("bwd_scatter", dict(sca, ldw=28), "PM_EINVAL"),
           ("bwd_weight", dict(wgt, lddw=28), "PM_EINVAL"),
           ("bwd_scatter", dict(sca, dX=B + 4), "PM_EALIGN"),            # a scatter dX off 16 bytes
           ("bwd_scatter", dict(sca, H=B + 4, act=1), "PM_EALIGN"),
           ("fwd", dict(fwd, src=B + 4), "PM_EALIGN"),
           ("fwd", dict(fwd, zero=0), "PM_EINVAL"),
           ("bwd_weight", dict(wgt, N=6, lddy=8), "PM_EINVAL")]          # N % 4 != 0
    for kind, prob, err in bad:
        with pytest.raises(RuntimeError, match=err):
            ops.sparse_conv_variant(kind, prob)
    with pytest.raises(ValueError):
        ops.sparse_conv_variant("fwd", dict(fwd, workspace=0))           # a field of another kind


# ---------------------------------------------------------------------------------------------------------------- coverage
ROWS = (1, 32, 33, 64, 65, 100, 4096, 65409, 65536, 300000)
TAPS = ((1, 4), (8, 4), (1, 32), (2, 32), (3, 32), (8, 12), (1, 64), (1, 128), (27, 64), (16353, 4))
WIDTHS = (1, 4, 16, 32, 33, 36, 48, 64, 68, 128, 132, 2048, 65412)
# Variants the table leaves out: key -> (smallest selecting shape the sweep finds, its operand bytes), allowed only beyond 256 MB.
EXCLUDED = {}
# What the selector can name, read off gemm2_plan and the four select functions.  A gathered operand always takes the LDS-DMA
# kernels with 16-byte loads, so only the tile and the stores vary.
#   fwd, bwd_data (8 each): 64 x 64 small; big: 64 x 128 (N > 64), 64 x 64 (32 < N <= 64), 128 x 32 lay 2 (N <= 32); each with
#     16-byte or scalar stores.
#   bwd_weight (12): 64 x 64 and 32 x 128 (lay 1: N <= 32, J*C > 64) small; big: 128 x 128, 64 x 128 (32 < N <= 64), 128 x 64
#     (J*C <= 64), 32 x 128; each with 16-byte or scalar stores (scalar: a single slab stored to a misaligned dW).  A big 64 x 64
#     tile would need 512 slabs of one tile: the call never chooses more than 256.
#   bwd_scatter (5, always 16-byte stores): Cout % 32 == 0: LDS-DMA 64 x 64 small, 128 x 64 and 64 x 128 (rows <= 64) big;
#     else register-staged 64 x 64 small and 128 x 128 big.
REACHABLE = {"fwd": 8, "bwd_data": 8, "bwd_weight": 12, "bwd_scatter": 5}


def _sweep(ops):
    """rows x (J, C) x N x the alignment of every pointer that may be off through the queries: every distinct record (without
    grid, splits, kchunk) with the smallest shape that selects it."""
    B = SV.BASE_ADDR
    found = {}
    movable = {"fwd": ("b", "Y"), "bwd_data": ("H", "dX"), "bwd_scatter": (), "bwd_weight": ("dW", "db")}
    for kind in SV.KINDS:
        for rows, (J, Cc), N in itertools.product(ROWS, TAPS, WIDTHS):
            if kind == "bwd_scatter" and rows * J > 4 * MB:
                continue
            c = dict(kind=kind, rows=rows, J=J, C=Cc, N=N, nsrc=rows * J if kind == "bwd_scatter" else 67, ld={}, off={})
            nbytes = _case_bytes(c)
            if nbytes > 1024 * MB:
                continue
            for mis in itertools.product((0, 1), repeat=len(movable[kind])):
                c["off"] = dict(zip(movable[kind], mis))
                for act in ((0, 1) if kind == "bwd_data" and c["off"].get("H") else (1,)):
                    try:
                        rec = SV.host_query(ops, c, act)
                    except RuntimeError:
                        continue                                        # a shape the entry point rejects (J * C % 32, N % 4 ...)
                    for key in SV.variant_keys(kind, rec):
                        if key not in found or nbytes < found[key][1]:
                            found[key] = ((rows, J, Cc, N, mis, act), nbytes)
    return found


def test_case_table_covers_every_reachable_variant(ops):
    found = _sweep(ops)
    covered = set()
    for c in SV.CASES:
        for act in (0, 1):
            covered |= SV.variant_keys(c["kind"], SV.host_query(ops, c, act))
    for kind, n in REACHABLE.items():
        assert sum(k[0] == kind for k in found) >= n, (kind, sorted(k for k in found if k[0] == kind))
    missing = {k: v for k, v in found.items() if k not in covered}
    left_out = {k: v for k, v in missing.items() if k in EXCLUDED}
    uncovered = {k: v for k, v in missing.items() if k not in EXCLUDED}
    assert not uncovered, "variants no case selects (key: smallest shape, bytes):\n" + "\n".join(f"{k}: {v}" for k, v in sorted(uncovered.items()))
    for k, (shape, b) in left_out.items():
        assert b > 256 * MB and EXCLUDED[k] == (shape, b), (k, shape, b)
    assert set(EXCLUDED) <= set(missing), "an excluded variant is covered or unreachable: drop it from EXCLUDED"
