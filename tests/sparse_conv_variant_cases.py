"""One table of sparse-convolution problems (pm_sparse_conv_*), each with the kernel variant it is meant to select
(ops.sparse_conv_variant's record).

tests/test_sparse_conv_variants_host.py asks the selector for every case (no GPU) and checks that the table reaches every variant
the selector can name; tests/test_gpu_sparse_conv_variants.py runs every case on the device against exact integer answers.

A case is a dict: id, kind, rows, J, C, N, nsrc, absent (share of absent taps), mode (how the index table is filled), ld (operand
name -> leading dimension, default the operand's width), off (operand name -> offset of its first element from a 16-byte
boundary, in floats), expect (the variant record) and expect_noact (data gradients with PM_ACT_NONE, where H does not count).
rows x J is the index table.  C and N in the entry point's meaning:

  fwd          src (nsrc, C) gathered, W (N, J*C), b (N,), Y (rows, N)            GEMM rows x N over J*C
  bwd_data     dY (nsrc, C) gathered (C = Cout), Wt (N, J*C), H, dX (rows, N)     GEMM rows x N over J*C   (N = Cin)
  bwd_scatter  dY (rows, N), W (N, J*C), H, dX (nsrc, C) scattered (N = Cout)     GEMM rows x J*C over N
  bwd_weight   dY (rows, N), src (nsrc, C) gathered, dW (N, J*C), db (N,)         GEMM N x J*C over rows

Index modes: "random" (every tap a random live source row, absent with probability `absent`; the first entry points at source
row 0 and the last at the last live source row; with absent taps one whole row is absent), "one" (every tap of every row points
at one source row).  The scatter form needs every destination at most once: its table is a random injection into the nsrc rows.

Sizes are the smallest that select each variant: `big` needs 512 tiles of 128 x 128 and nothing more (65409 = 511 * 128 + 1 rows),
a gathered source stays a few hundred rows, and every case stays under the 76 MB tests/test_linear_variants_host.py allows.
"""
import numpy as np

KINDS = ("fwd", "bwd_data", "bwd_scatter", "bwd_weight")
OPERANDS = {"fwd": ("src", "W", "b", "Y"), "bwd_data": ("dY", "Wt", "H", "dX"), "bwd_scatter": ("dY", "W", "H", "dX"),
            "bwd_weight": ("dY", "src", "dW", "db")}


def operand_shape(c, name):
    rows, J, Cc, N, nsrc = c["rows"], c["J"], c["C"], c["N"], c["nsrc"]
    k = c["kind"]
    if name in ("W", "Wt", "dW"):
        return (N, J * Cc)
    if name in ("b", "db"):
        return (N,)
    if name == "src" or (name == "dY" and k == "bwd_data") or (k == "bwd_scatter" and name in ("H", "dX")):
        return (nsrc, Cc)
    return (rows, N)                        # Y; dY of the scatter form and the weight gradient; H and dX of the gathered data gradient


def V(tm=64, tn=64, lay=0, big=0, vecC=1, path="dma"):
    """A variant record.  Every gathered problem runs the LDS-DMA kernels (three-stage ring) with 16-byte loads."""
    return dict(path=path, tm=tm, tn=tn, lay=lay, stages=3 if path == "dma" else 0, vec=1, big=big, vecC=[vecC])


CASES = []
DEFAULT_NSRC = 67


def case(id_, kind, rows, J, C, N, expect, nsrc=None, absent=0.3, mode="random", ld=None, off=None, expect_noact=None):
    assert all(c["id"] != id_ for c in CASES), id_
    if nsrc is None:
        nsrc = rows * J + 3 if kind == "bwd_scatter" else DEFAULT_NSRC
    CASES.append(dict(id=id_, kind=kind, rows=rows, J=J, C=C, N=N, nsrc=nsrc, absent=absent, mode=mode, ld=dict(ld or {}),
                      off=dict(off or {}), expect=expect, expect_noact=expect_noact or expect))


BIG_M = 511 * 128 + 1                       # 512 row tiles of 128 (1023 of 64), the last one with a single live row
BIG_N = 65536 - 124                         # 512 column tiles of 128, the last one four columns wide
# (J, C) with J * C % 32 == 0.  Powers of two: eight taps per 32-wide K-step down to a quarter tap; the others take the division form
TAPS_POW2 = [(8, 4), (4, 8), (2, 16), (1, 32), (1, 64), (1, 128)]
TAPS_DIV = [(8, 12), (8, 20), (4, 24), (2, 48)]
# reduction lengths in K-steps: 1, 2, 3, 4, 5 and 54
TAPS_NK = [(1, 32), (2, 32), (3, 32), (4, 32), (5, 32), (27, 64)]
RAG_ROWS = (1, 63, 65, 127)                  # 1, T - 1, T + 1, 2T - 1 next to the 64-row tile
WIDTHS = (4, 28, 36, 60, 68, 124, 132)

# ------------------------------------------------------------------------------------------------------------ forward / gathered data gradient
for kind, out in (("fwd", "Y"), ("bwd_data", "dX")):
    for i, (J, Cc) in enumerate(TAPS_POW2 + TAPS_DIV + TAPS_NK):
        rows, n = RAG_ROWS[i % 4], WIDTHS[i % 7]
        case(f"{kind}-64-J{J}-C{Cc}-rows{rows}-N{n}", kind, rows, J, Cc, n, V())
    for i, n in enumerate((36, 60, 68, 124, 132, 4, 28)):       # every width with every row count of the ragged set once more
        case(f"{kind}-64-rows{RAG_ROWS[(i + 1) % 4]}-N{n}-J3-C32", kind, RAG_ROWS[(i + 1) % 4], 3, 32, n, V())
    for n in (1, 3, 17, 33, 63) if kind == "fwd" else (1, 3, 33):          # scalar stores
        case(f"{kind}-64-scalar-N{n}", kind, 65, 2, 48, n, V(vecC=0))
    case(f"{kind}-64-{out}-off1", kind, 65, 4, 8, 64, V(vecC=0), off={out: 1})
    case(f"{kind}-64-{out}-ld+1", kind, 63, 2, 32, 60, V(vecC=0), ld={out: 61})
    case(f"{kind}-64-{out}-ld+4", kind, 127, 2, 32, 60, V(), ld={out: 64})
    g, w = ("src", "W") if kind == "fwd" else ("dY", "Wt")
    case(f"{kind}-64-{g}-ld+4", kind, 65, 8, 12, 36, V(), ld={g: 16})
    case(f"{kind}-64-{w}-ld+4", kind, 65, 8, 12, 36, V(), ld={w: 100})
    case(f"{kind}-64-{g}-{w}-ld+8", kind, 127, 3, 32, 68, V(), ld={g: 40, w: 104})
    # index tables
    case(f"{kind}-64-none-absent", kind, 65, 8, 4, 36, V(), absent=0.0)
    case(f"{kind}-64-all-absent", kind, 65, 8, 4, 36, V(), absent=1.0)
    case(f"{kind}-64-one-source-row", kind, 127, 5, 32, 28, V(), mode="one", absent=0.0)
    case(f"{kind}-64-nsrc1", kind, 65, 3, 32, 60, V(), nsrc=1)
    case(f"{kind}-64-nsrc-above-rows", kind, 5, 8, 20, 124, V(), nsrc=301)
    # big grids: 64 x 128 (more than 64 output columns), 64 x 64 (33 .. 64), 128 x 32 (up to 32)
    case(f"{kind}-big64x128-N128", kind, BIG_M, 1, 32, 128, V(64, 128, big=1))
    case(f"{kind}-big64x128-N68-rows65535", kind, 65535, 8, 4, 68, V(64, 128, big=1))
    case(f"{kind}-big64x128-N132-J8-C12", kind, 32641 + 64, 8, 12, 132, V(64, 128, big=1))
    case(f"{kind}-big64x128-rows1", kind, 1, 1, 32, BIG_N, V(64, 128, big=1))
    case(f"{kind}-big64x128-rows63-N65411", kind, 63, 2, 16, 65411, V(64, 128, big=1, vecC=0))
    case(f"{kind}-big64x64-N64", kind, BIG_M, 2, 32, 64, V(64, 64, big=1))
    case(f"{kind}-big64x64-N36-rows65473", kind, BIG_M + 64, 4, 24, 36, V(64, 64, big=1))
    case(f"{kind}-big64x64-N33", kind, 65535, 1, 32, 33, V(64, 64, big=1, vecC=0))
    case(f"{kind}-lay2-N32", kind, BIG_M, 2, 32, 32, V(128, 32, lay=2, big=1))
    case(f"{kind}-lay2-N4-rows65535", kind, 65535, 8, 4, 4, V(128, 32, lay=2, big=1))
    case(f"{kind}-lay2-N28-rows65537-J8-C20", kind, BIG_M + 128, 8, 20, 28, V(128, 32, lay=2, big=1))
    case(f"{kind}-lay2-N17", kind, BIG_M + 127, 1, 64, 17, V(128, 32, lay=2, big=1, vecC=0))
    case(f"{kind}-lay2-{out}-off1", kind, BIG_M, 1, 32, 32, V(128, 32, lay=2, big=1, vecC=0), off={out: 1})
case("fwd-64-b-off1", "fwd", 65, 4, 8, 64, V(vecC=0), off={"b": 1})
case("fwd-big64x128-b-off1", "fwd", BIG_M, 1, 32, 128, V(64, 128, big=1, vecC=0), off={"b": 1})
# H unaligned counts under an activation only
case("bwd_data-64-H-off1", "bwd_data", 65, 4, 8, 64, V(vecC=0), off={"H": 1}, expect_noact=V())
case("bwd_data-64-H-ld+1", "bwd_data", 65, 4, 8, 64, V(vecC=0), ld={"H": 65}, expect_noact=V())
case("bwd_data-64-H-ld+4", "bwd_data", 65, 4, 8, 64, V(), ld={"H": 68})

# ------------------------------------------------------------------------------------------------------------ scatter
# C (channels per tap of dX) x J = the GEMM's columns; the reduction is Cout = N: a multiple of 32 runs the LDS-DMA kernels,
# 16 and 48 the register-staged ones.  J * C on both sides of 64 and 128.
for i, (J, Cc) in enumerate([(8, 4), (15, 4), (17, 4), (5, 12), (31, 4), (33, 4), (3, 20), (7, 24), (2, 48), (1, 128), (3, 64)]):
    for n, path in ((16, "reg"), (32, "dma"), (48, "reg"), (64, "dma")):
        if (i + n // 16) % 2 == 0 or i < 2:
            case(f"bwd_scatter-{path}64-J{J}-C{Cc}-Cout{n}-rows{RAG_ROWS[i % 4]}", "bwd_scatter", RAG_ROWS[i % 4], J, Cc, n, V(path=path))
case("bwd_scatter-dma64-none-absent", "bwd_scatter", 65, 8, 4, 32, V(), absent=0.0)
case("bwd_scatter-dma64-all-absent", "bwd_scatter", 65, 8, 4, 32, V(), absent=1.0)
case("bwd_scatter-reg64-all-absent", "bwd_scatter", 65, 8, 4, 16, V(path="reg"), absent=1.0)
case("bwd_scatter-reg64-none-absent", "bwd_scatter", 127, 3, 12, 48, V(path="reg"), absent=0.0)
case("bwd_scatter-dma64-Cout96-nsrc-above", "bwd_scatter", 63, 5, 8, 96, V(), nsrc=1000)
case("bwd_scatter-dma64-dY-W-ld+4", "bwd_scatter", 65, 9, 4, 32, V(), ld={"dY": 36, "W": 40})
case("bwd_scatter-reg64-dY-W-ld+4", "bwd_scatter", 65, 9, 4, 16, V(path="reg"), ld={"dY": 20, "W": 40})
case("bwd_scatter-big-dma128x64-J2-C4", "bwd_scatter", BIG_M, 2, 4, 32, V(128, 64, big=1))
case("bwd_scatter-big-dma128x64-J5-C16-Cout64", "bwd_scatter", BIG_M, 5, 16, 64, V(128, 64, big=1))
case("bwd_scatter-big-dma128x64-J11-C12", "bwd_scatter", 32641 + 64, 11, 12, 32, V(128, 64, big=1))
case("bwd_scatter-big-dma128x64-rows65535-C20", "bwd_scatter", 65535, 1, 20, 32, V(128, 64, big=1))             # 127 live rows in the last tile
case("bwd_scatter-big-dma64x128", "bwd_scatter", 64, BIG_N // 4, 4, 32, V(64, 128, big=1))
case("bwd_scatter-big-dma64x128-rows1-C12", "bwd_scatter", 1, BIG_N // 12, 12, 64, V(64, 128, big=1))
case("bwd_scatter-big-reg128-Cout16", "bwd_scatter", BIG_M, 2, 4, 16, V(128, 128, big=1, path="reg"))
case("bwd_scatter-big-reg128-Cout48-J11-C12", "bwd_scatter", 32641 + 64, 11, 12, 48, V(128, 128, big=1, path="reg"))
case("bwd_scatter-big-reg128-rows65535-Cout48", "bwd_scatter", 65535, 3, 4, 48, V(128, 128, big=1, path="reg"))
case("bwd_scatter-big-reg128-rows63", "bwd_scatter", 63, BIG_N // 4, 4, 16, V(128, 128, big=1, path="reg"))

# ------------------------------------------------------------------------------------------------------------ weight gradient
# N x J*C over the rows.  Up to 64 rows the call stores to dW itself; from 65 on it reduces slabs of its own through the workspace.
for i, rows in enumerate((1, 31, 32, 33, 63, 65)):
    J, Cc = (TAPS_POW2 + TAPS_DIV)[i]
    case(f"bwd_weight-64-rows{rows}-J{J}-C{Cc}-N36", "bwd_weight", rows, J, Cc, 36, V())
    J, Cc = (TAPS_DIV + [(1, 128), (3, 32)])[i]                          # more than 64 columns
    case(f"bwd_weight-lay1-rows{rows}-J{J}-C{Cc}-N28", "bwd_weight", rows, J, Cc, 28, V(32, 128, lay=1))
for i, (J, Cc) in enumerate(TAPS_POW2 + TAPS_DIV + TAPS_NK):
    n = WIDTHS[(i + 3) % 7]
    rows = (96, 100, 127, 129, 160, 193)[i % 6]
    lay1 = n <= 32 and J * Cc > 64
    case(f"bwd_weight-{'lay1' if lay1 else '64'}-J{J}-C{Cc}-N{n}-rows{rows}", "bwd_weight", rows, J, Cc, n,
         V(32, 128, lay=1) if lay1 else V())
# split-K in 2 slabs of 64 rows: 65 .. 68 rows leave the last slab 1 to 4 live rows, 97 .. 100 leave its last 32-row step as many
for rows in (65, 66, 67, 68, 97, 98, 100):
    case(f"bwd_weight-lay1-last-slab-rows{rows}", "bwd_weight", rows, 3, 32, 32, V(32, 128, lay=1))
    case(f"bwd_weight-64-last-slab-rows{rows}", "bwd_weight", rows, 3, 32, 36, V())
case("bwd_weight-64-K4-J1-C4", "bwd_weight", 65, 1, 4, 4, V())                     # J * C need be no multiple of 32 here
case("bwd_weight-64-K36-J3-C12", "bwd_weight", 63, 3, 12, 68, V())
case("bwd_weight-lay1-K100-J5-C20", "bwd_weight", 129, 5, 20, 32, V(32, 128, lay=1))
case("bwd_weight-64-dW-off1", "bwd_weight", 33, 2, 32, 36, V(vecC=0), off={"dW": 1})
case("bwd_weight-64-dW-ld+1", "bwd_weight", 63, 2, 32, 36, V(vecC=0), ld={"dW": 65})
case("bwd_weight-64-dW-ld+4", "bwd_weight", 31, 2, 32, 36, V(), ld={"dW": 68})
case("bwd_weight-64-slabs-dW-off1", "bwd_weight", 129, 2, 32, 36, V(), off={"dW": 1})          # slabs go to the workspace: dW's alignment does not count
case("bwd_weight-lay1-dW-off1", "bwd_weight", 64, 3, 32, 32, V(32, 128, lay=1, vecC=0), off={"dW": 1})
case("bwd_weight-lay1-dY-src-ld+4", "bwd_weight", 100, 8, 12, 32, V(32, 128, lay=1), ld={"dY": 36, "src": 16})
case("bwd_weight-64-dY-src-dW-ld+4", "bwd_weight", 64, 8, 12, 68, V(), ld={"dY": 72, "src": 16, "dW": 100})
case("bwd_weight-64-none-absent", "bwd_weight", 100, 8, 4, 36, V(), absent=0.0)
case("bwd_weight-64-all-absent", "bwd_weight", 100, 8, 4, 36, V(), absent=1.0)
case("bwd_weight-lay1-one-source-row", "bwd_weight", 127, 5, 32, 28, V(32, 128, lay=1), mode="one", absent=0.0)
case("bwd_weight-64-nsrc1", "bwd_weight", 65, 3, 32, 60, V(), nsrc=1)
case("bwd_weight-64-nsrc-above-rows", "bwd_weight", 5, 8, 20, 124, V(), nsrc=301)
# big by the size of the gradient itself (one slab: the stores go to dW)
case("bwd_weight-big128-N2048-K4096", "bwd_weight", 32, 1024, 4, 2048, V(128, 128, big=1))
case("bwd_weight-big128-N132-C12-rows33", "bwd_weight", 33, BIG_N // 12, 12, 132, V(128, 128, big=1))
case("bwd_weight-big128-N124-rows31", "bwd_weight", 31, BIG_N // 4, 4, 124, V(128, 128, big=1))               # T - 4 rows of dW, one row tile
case("bwd_weight-big128-dW-ld+1", "bwd_weight", 1, 1024, 4, 2048, V(128, 128, big=1, vecC=0), ld={"dW": 4097})
case("bwd_weight-big128x64-K64", "bwd_weight", 32, 16, 4, BIG_N, V(128, 64, big=1))
case("bwd_weight-big128x64-K60-dW-off2", "bwd_weight", 31, 5, 12, BIG_N, V(128, 64, big=1, vecC=0), off={"dW": 2})
case("bwd_weight-big64x128-N64", "bwd_weight", 32, BIG_N // 4, 4, 64, V(64, 128, big=1))
case("bwd_weight-big64x128-N36-dW-off1", "bwd_weight", 63, BIG_N // 4, 4, 36, V(64, 128, big=1, vecC=0), off={"dW": 1})
case("bwd_weight-big-lay1-N32", "bwd_weight", 32, BIG_N // 4, 4, 32, V(32, 128, lay=1, big=1))
case("bwd_weight-big-lay1-N4-C12-dW-off1", "bwd_weight", 65, BIG_N // 12, 12, 4, V(32, 128, lay=1, big=1, vecC=0), off={"dW": 1})


# ------------------------------------------------------------------------------------------------------------ index tables
def live_rows(c):
    """(rows of the gathered source tensor, the ones an index may name, the trap rows).  A gathered source has nsrc live rows: one
    more row behind them and, from four rows on, one in the middle are traps that no index names (NaN in the tests)."""
    n = c["nsrc"]
    if c["kind"] == "bwd_scatter":
        return n, np.arange(n), np.array([n, n + 1])                     # destination rows; the traps lie behind the view
    if n < 4:
        return n + 1, np.arange(n), np.array([n])
    live = np.array([r for r in range(n + 1) if r != n // 2])            # n live rows out of n + 1, the middle one a trap
    return n + 2, live, np.array([n // 2, n + 1])


def make_index(c, rng):
    """The (rows, J) int32 table of case c."""
    rows, J = c["rows"], c["J"]
    _, live, _ = live_rows(c)
    if c["kind"] == "bwd_scatter":
        assert len(live) >= rows * J
        idx = rng.permutation(len(live))[:rows * J].astype(np.int32).reshape(rows, J)
    elif c["mode"] == "one":
        idx = np.full((rows, J), live[len(live) // 2], np.int32)
    else:
        idx = live[rng.integers(0, len(live), size=(rows, J))].astype(np.int32)
    if c["absent"] >= 1.0:
        idx[...] = -1
    elif c["absent"] > 0:
        idx[rng.random((rows, J)) < c["absent"]] = -1
        if rows >= 3:
            idx[rows // 2] = -1                                          # one row with no neighbour at all
    if c["absent"] < 1.0 and c["kind"] != "bwd_scatter" and c["mode"] != "one":
        idx.flat[0], idx.flat[-1] = live[0], live[-1]                    # source row 0 and the last live one
    return idx


def variant_keys(kind, rec):
    """What the coverage test counts: the record without the grid size, the split count and kchunk."""
    return {(kind, rec["path"], rec["tm"], rec["tn"], rec["lay"], rec["stages"], rec["vec"], rec["big"], c) for c in rec["vecC"]}


BASE_ADDR = 0x10000000                      # the made-up 16-byte aligned address the host tests hang the operands' offsets on


def ld_of(c, name):
    return c["ld"].get(name, operand_shape(c, name)[-1])


def query_problem(c, ptr, act=1):
    """The argument dict ops.sparse_conv_variant takes for case c; ptr(name) -> address or tensor of operand `name` (the operands
    of the kind, "idx" and "zero")."""
    k, rows, J, Cc, N = c["kind"], c["rows"], c["J"], c["C"], c["N"]
    ld = lambda n: ld_of(c, n)                                                              # noqa: E731
    if k == "fwd":
        return dict(src=ptr("src"), lds=ld("src"), idx=ptr("idx"), rows=rows, J=J, C=Cc, W=ptr("W"), ldw=ld("W"), b=ptr("b"), Y=ptr("Y"),
                    ldy=ld("Y"), N=N, act=act, zero=ptr("zero"))
    if k == "bwd_data":
        return dict(dY=ptr("dY"), lddy=ld("dY"), idxT=ptr("idx"), rows=rows, J=J, Cout=Cc, Wt=ptr("Wt"), ldwt=ld("Wt"), H=ptr("H") if act else 0,
                    ldh=ld("H") if act else 0, dX=ptr("dX"), lddx=ld("dX"), Cin=N, act=act, zero=ptr("zero"))
    if k == "bwd_scatter":
        return dict(dY=ptr("dY"), lddy=ld("dY"), W=ptr("W"), ldw=ld("W"), idx=ptr("idx"), rows=rows, J=J, C=Cc, Cout=N, H=ptr("H") if act else 0,
                    dX=ptr("dX"), act=act)
    return dict(dY=ptr("dY"), lddy=ld("dY"), src=ptr("src"), lds=ld("src"), idx=ptr("idx"), rows=rows, J=J, C=Cc, dW=ptr("dW"), lddw=ld("dW"),
                db=ptr("db"), N=N, zero=ptr("zero"), workspace=0)


def host_query(ops, c, act=1):
    """The selector's record for case c with made-up addresses (no GPU)."""
    return ops.sparse_conv_variant(c["kind"], query_problem(c, lambda n: BASE_ADDR + 4 * c["off"].get(n, 0), act))
