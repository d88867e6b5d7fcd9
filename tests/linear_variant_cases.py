"""One table of Linear problems, each with the kernel variant it is meant to select (ops.linear_variant's record).

tests/test_linear_variants_host.py asks the selector for every case (no GPU) and checks that the table reaches every variant the
selector can name; tests/test_gpu_linear_variants.py runs every case on the device against exact integer answers.

A case is a dict: id, kind ("fwd", "bwd_data", "bwd_weight" or their "_group" forms), probs (a list of problems, one for the
single-problem kinds), splits (grouped weight gradient), expect (the record with an activation) and expect_noact (data gradients
with PM_ACT_NONE, where H does not count).  A problem is a dict M, N, K in the meaning of the entry point, ld (operand name ->
leading dimension, default the operand's width), off (operand name -> offset of the operand's first element from a 16-byte boundary,
in floats) and, for grouped weight gradients, cols (dY / X -> readable row width, the header's dy_cols / x_cols).

Operand names and shapes: fwd X (M, K), W (N, K), b (N,), Y (M, N); bwd_data dY (M, N), W (N, K), H (M, K), dX (M, K);
bwd_weight dY (M, N), X (M, K), dW (N, K), db (N,).  The GEMM behind them: forward M x N over K; data gradient M x K over N;
weight gradient N x K over M.

Sizes are the smallest that select each variant: `big` needs 512 tiles of 128 x 128 and nothing more (65409 = 511 * 128 + 1 rows: a
last tile with one live row); a case stays at about 64 MB of operands at the most (the smallest big data gradient has 33 MB in dX and
as much in H: 76 MB is what tests/test_linear_variants_host.py allows).
"""

OPERANDS = {"fwd": ("X", "W", "b", "Y"), "bwd_data": ("dY", "W", "H", "dX"), "bwd_weight": ("dY", "X", "dW", "db")}
OUTPUTS = {"fwd": ("Y",), "bwd_data": ("dX",), "bwd_weight": ("dW", "db")}


def base_kind(kind):
    return kind[:-6] if kind.endswith("_group") else kind


def operand_shape(kind, name, p):
    M, N, K = p["M"], p["N"], p["K"]
    return {"X": (M, K), "W": (N, K), "b": (N,), "Y": (M, N), "dY": (M, N), "H": (M, K), "dX": (M, K), "dW": (N, K), "db": (N,)}[name]


def V(path, tm=0, tn=0, lay=0, vec=1, big=0, vecC=1):
    """A variant record; vecC: one value for every problem or a list.  The LDS-DMA kernels run a three-stage ring."""
    return dict(path=path, tm=tm, tn=tn, lay=lay, stages=3 if path == "dma" else 0, vec=vec, big=big, vecC=vecC)


def P(M, N, K, ld=None, off=None, cols=None):
    return dict(M=M, N=N, K=K, ld=dict(ld or {}), off=dict(off or {}), cols=dict(cols or {}))


CASES = []


def case(id_, kind, probs, expect, expect_noact=None, splits=1):
    probs = probs if isinstance(probs, list) else [probs]
    for e in (expect, expect_noact):
        if e is not None and not isinstance(e["vecC"], list):
            e["vecC"] = [e["vecC"]] * len(probs)
    assert all(c["id"] != id_ for c in CASES), id_
    CASES.append(dict(id=id_, kind=kind, probs=probs, splits=splits, expect=expect, expect_noact=expect_noact or expect))


BIG_M = 511 * 128 + 1                       # 512 row tiles of 128, the last one with a single live row
RAG_ODD = [(1, 127), (63, 65), (65, 63), (127, 1)]         # (rows, cols) next to the 64 x 64 tile: 1, T - 1, T + 1, 2T - 1
RAG_4 = [(1, 124), (63, 68), (65, 60), (127, 4)]           # the same with columns that are multiples of 4 (16-byte stores)

# ------------------------------------------------------------------------------------------------------------ forward
for k in (1, 2, 3, 31, 33, 63):             # K % 4 != 0: scalar loads; odd N: scalar stores
    for m, n in RAG_ODD:
        case(f"fwd-reg64-scalar-M{m}-N{n}-K{k}", "fwd", P(m, n, k), V("reg", 64, 64, vec=0, vecC=0))
for k in (4, 36, 60):                       # K % 4 == 0 but no multiple of 32: 16-byte loads through registers
    for m, n in RAG_4:
        case(f"fwd-reg64-vec-M{m}-N{n}-K{k}", "fwd", P(m, n, k), V("reg", 64, 64))
    case(f"fwd-reg64-vec-M65-N63-K{k}", "fwd", P(65, 63, k), V("reg", 64, 64, vecC=0))
case("fwd-reg64-scalar-M65-N64-K33", "fwd", P(65, 64, 33), V("reg", 64, 64, vec=0, vecC=1))
for k in (32, 64, 96):                      # K % 32 == 0: LDS-DMA
    for m, n in RAG_4:
        case(f"fwd-dma64-M{m}-N{n}-K{k}", "fwd", P(m, n, k), V("dma", 64, 64))
    case(f"fwd-dma64-M65-N63-K{k}", "fwd", P(65, 63, k), V("dma", 64, 64, vecC=0))
# big: 512 tiles of 128 x 128
case("fwd-reg128-scalar-K6", "fwd", P(BIG_M, 128, 6), V("reg", 128, 128, vec=0, big=1))
case("fwd-reg128-scalar-K6-N127", "fwd", P(BIG_M, 127, 6), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("fwd-reg128-scalar-K33-N129", "fwd", P(32641, 129, 33), V("reg", 128, 128, vec=0, big=1, vecC=0))    # 256 x 2 tiles, ragged in both
case("fwd-reg128-vec-K36", "fwd", P(BIG_M, 128, 36), V("reg", 128, 128, big=1))
case("fwd-reg128-vec-K36-N126", "fwd", P(65535, 126, 36), V("reg", 128, 128, big=1, vecC=0))
case("fwd-dma128x64-K32-N128", "fwd", P(BIG_M, 128, 32), V("dma", 128, 64, big=1))
case("fwd-dma128x64-K64-N64", "fwd", P(65535, 64, 64), V("dma", 128, 64, big=1))
case("fwd-dma128x64-K64-N65", "fwd", P(BIG_M, 65, 64), V("dma", 128, 64, big=1, vecC=0))
case("fwd-dma128x64-K32-N36", "fwd", P(BIG_M, 36, 32), V("dma", 128, 64, big=1))
case("fwd-lay2-K64-N32", "fwd", P(BIG_M, 32, 64), V("dma", 128, 32, lay=2, big=1))
case("fwd-lay2-K32-N31", "fwd", P(65535, 31, 32), V("dma", 128, 32, lay=2, big=1, vecC=0))
case("fwd-lay2-K32-N17", "fwd", P(BIG_M + 128, 17, 32), V("dma", 128, 32, lay=2, big=1, vecC=0))       # (N <= 16 here is the skinny kernels')
case("fwd-dma64x128-M64", "fwd", P(64, 65536 - 124, 32), V("dma", 64, 128, big=1))
case("fwd-dma64x128-M63-N65411", "fwd", P(63, 65411, 32), V("dma", 64, 128, big=1, vecC=0))
# the skinny kernels' boundary: M >= 256, N <= 16, N * K * 4 <= 64 KB, 16-byte loadable X and W
case("fwd-skinny-M256-N16", "fwd", P(256, 16, 512), V("skinny", vecC=0))
case("fwd-skinny-M257-N1", "fwd", P(257, 1, 512), V("skinny", vecC=0))
case("fwd-skinny-M255-N16", "fwd", P(255, 16, 512), V("dma", 64, 64))
case("fwd-skinny-M256-N17", "fwd", P(256, 17, 512), V("dma", 64, 64, vecC=0))
case("fwd-skinny-N16-K1024", "fwd", P(256, 16, 1024), V("skinny", vecC=0))             # N * K * 4 = 64 KB exactly
case("fwd-skinny-N16-K1028", "fwd", P(256, 16, 1028), V("reg", 64, 64))                # 64 KB + 64 B
case("fwd-skinny-X-off1", "fwd", P(256, 16, 512, off={"X": 1}), V("reg", 64, 64, vec=0))
case("fwd-skinny-big-N10", "fwd", P(BIG_M, 10, 128), V("skinny", vecC=0))

# ------------------------------------------------------------------------------------------------------------ data gradient
for n in (1, 2, 3, 31, 33, 63):             # the reduction is N here
    for m, k in RAG_ODD:
        case(f"bwd_data-reg64-scalar-M{m}-K{k}-N{n}", "bwd_data", P(m, n, k), V("reg", 64, 64, vec=0, vecC=0))
for n in (4, 36, 60):
    for m, k in RAG_4:
        case(f"bwd_data-reg64-vec-M{m}-K{k}-N{n}", "bwd_data", P(m, n, k), V("reg", 64, 64))
case("bwd_data-reg64-scalar-M65-K64-N33", "bwd_data", P(65, 33, 64), V("reg", 64, 64, vec=0, vecC=1))
for n in (32, 64, 96):
    for m, k in RAG_4:
        case(f"bwd_data-dma64-M{m}-K{k}-N{n}", "bwd_data", P(m, n, k), V("dma", 64, 64))
case("bwd_data-reg128-scalar-N18", "bwd_data", P(BIG_M, 18, 128), V("reg", 128, 128, vec=0, big=1))
case("bwd_data-reg128-scalar-N6-K127", "bwd_data", P(BIG_M, 6, 127), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_data-reg128-scalar-N33-K129", "bwd_data", P(32641, 33, 129), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_data-reg128-vec-N36", "bwd_data", P(BIG_M, 36, 128), V("reg", 128, 128, big=1))
case("bwd_data-dma128x64-N32-K128", "bwd_data", P(BIG_M, 32, 128), V("dma", 128, 64, big=1))
case("bwd_data-dma128x64-N64-K64", "bwd_data", P(65535, 64, 64), V("dma", 128, 64, big=1))
case("bwd_data-dma128x64-N32-K68", "bwd_data", P(BIG_M, 32, 68), V("dma", 128, 64, big=1))
case("bwd_data-dma64x128-M64", "bwd_data", P(64, 32, 65536 - 124), V("dma", 64, 128, big=1))
case("bwd_data-dma64x128-M63", "bwd_data", P(63, 64, 65536), V("dma", 64, 128, big=1))
case("bwd_data-dma64x128-dX-off1", "bwd_data", P(64, 32, 65536 - 124, off={"dX": 1}), V("dma", 64, 128, big=1, vecC=0))
case("bwd_data-skinny-M256-N16", "bwd_data", P(256, 16, 512), V("skinny"))
case("bwd_data-skinny-M255-N16", "bwd_data", P(255, 16, 512), V("reg", 64, 64))
case("bwd_data-skinny-M256-N17", "bwd_data", P(256, 17, 512), V("reg", 64, 64, vec=0))
case("bwd_data-skinny-N16-K1024", "bwd_data", P(256, 16, 1024), V("skinny"))
case("bwd_data-skinny-N16-K1028", "bwd_data", P(256, 16, 1028), V("reg", 64, 64))
case("bwd_data-skinny-N1", "bwd_data", P(300, 1, 512), V("skinny"))
# H unaligned under an activation: the data gradient falls back to the GEMM (scalar epilogue); without one, H does not count
case("bwd_data-skinny-H-off1", "bwd_data", P(256, 16, 512, off={"H": 1}), V("reg", 64, 64, vecC=0), V("skinny"))
case("bwd_data-skinny-H-ld+1", "bwd_data", P(256, 16, 512, ld={"H": 513}), V("reg", 64, 64, vecC=0), V("skinny"))

# ------------------------------------------------------------------------------------------------------------ weight gradient
# (single call: the split count is the heuristic's -- 2 slabs from 65 rows on, so these also reduce slabs)
for m in (1, 2, 3, 31, 33, 63):             # the reduction is the batch M; N x K next to the 64 x 64 tile
    for n, k in RAG_ODD:
        case(f"bwd_weight-reg64-scalar-N{n}-K{k}-M{m}", "bwd_weight", P(m, n, k), V("reg", 64, 64, vec=0, vecC=0))
for m in (1, 31, 33, 65, 97):
    for n, k in [(4, 124), (60, 68), (68, 60), (124, 4)]:
        case(f"bwd_weight-reg64-vec-N{n}-K{k}-M{m}", "bwd_weight", P(m, n, k), V("reg", 64, 64))
case("bwd_weight-reg64-scalar-N63-K64-M97", "bwd_weight", P(97, 63, 64), V("reg", 64, 64, vec=0, vecC=1))
for m in (32, 64, 96, 160):
    for n, k in [(68, 60), (124, 4), (4, 64), (60, 68)]:
        case(f"bwd_weight-dma64-N{n}-K{k}-M{m}", "bwd_weight", P(m, n, k), V("dma", 64, 64))
# <= 32 output rows and more than 64 columns: the 32 x 128 tile
for m in (32, 96, 2048):
    for n, k in [(4, 68), (28, 124), (32, 132), (32, 252)]:
        case(f"bwd_weight-lay1-N{n}-K{k}-M{m}", "bwd_weight", P(m, n, k), V("dma", 32, 128, lay=1))
case("bwd_weight-lay1-not-N36", "bwd_weight", P(96, 36, 132), V("dma", 64, 64))
case("bwd_weight-lay1-not-K64", "bwd_weight", P(96, 32, 64), V("dma", 64, 64))
case("bwd_weight-lay1-not-M100", "bwd_weight", P(100, 32, 132), V("reg", 64, 64))
# big by the size of the gradient itself
case("bwd_weight-dma128-N2048-K4096", "bwd_weight", P(32, 2048, 4096), V("dma", 128, 128, big=1))
case("bwd_weight-dma128-ragged", "bwd_weight", P(64, 2048 - 124, 4096 - 124), V("dma", 128, 128, big=1))
case("bwd_weight-reg128-vec-M33", "bwd_weight", P(33, 2048, 4096 - 124), V("reg", 128, 128, big=1))
case("bwd_weight-reg128-scalar-N2047", "bwd_weight", P(33, 2047, 4096), V("reg", 128, 128, vec=0, big=1))
case("bwd_weight-reg128-scalar-K4095", "bwd_weight", P(3, 2048, 4095), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-dma128x64-K64", "bwd_weight", P(32, 65536 - 124, 64), V("dma", 128, 64, big=1))
case("bwd_weight-dma64x128-N64", "bwd_weight", P(32, 64, 65536 - 124), V("dma", 64, 128, big=1))
case("bwd_weight-lay1-big", "bwd_weight", P(32, 32, 65536 - 124), V("dma", 32, 128, lay=1, big=1))
case("bwd_weight-lay1-big-dW-off1", "bwd_weight", P(32, 32, 65536 - 124, off={"dW": 1}), V("dma", 32, 128, lay=1, big=1, vecC=0))
case("bwd_weight-dma128x64-dW-off2", "bwd_weight", P(32, 65536 - 124, 64, off={"dW": 2}), V("dma", 128, 64, big=1, vecC=0))

# ------------------------------------------------------------------------------------------------------------ ragged edges of the big tiles
# Rows x columns next to the 128 x 128 tile (1, T - 1, T + 1, 2T - 1 in either dimension, the other one long enough for 512
# tiles) for the register-staged 128 x 128 kernels, with every reduction length they admit.
RAG128 = [(1, BIG_M), (127, 65535), (129, 32641), (255, 32767), (32641, 255), (BIG_M, 129), (65535, 127), (BIG_M, 1)]
for i, k in enumerate((1, 2, 3, 31, 33, 63)):                     # scalar loads: any K
    for m, n in (RAG128[i], RAG128[(i + 3) % 8], RAG128[(i + 6) % 8]):
        case(f"fwd-reg128-scalar-M{m}-N{n}-K{k}", "fwd", P(m, n, k), V("reg", 128, 128, vec=0, big=1, vecC=0))
    # the data gradient's output is M x K over N; odd K: W is not 16-byte loadable, so N <= 16 does not go to the skinny kernel.
    # (Reductions from 31 on keep to the shapes of up to 32641 rows: with 65409 rows dY alone would add 8 to 16 MB to dX and H.)
    for m, n in ((RAG128[i], RAG128[(i + 3) % 8], RAG128[(i + 6) % 8]) if k < 31 else (RAG128[i % 5], RAG128[(i + 2) % 5], RAG128[(i + 4) % 5])):
        case(f"bwd_data-reg128-scalar-M{m}-K{n}-N{k}", "bwd_data", P(m, k, n), V("reg", 128, 128, vec=0, big=1, vecC=0))
# 16-byte loads through registers: K (forward) or N (data gradient) a multiple of 4 but not of 32; columns multiples of 4.  (Forward
# N <= 16 with M >= 256, and data-gradient N <= 16 with M >= 256, belong to the skinny kernels: those pairs are left out.)
RAG128_4 = [(1, 65536 - 124), (127, 65536), (129, 32768 - 124), (255, 32768), (32641, 252), (BIG_M, 132), (65535, 124)]
for i, k in enumerate((60, 4, 36)):
    for m, n in (RAG128_4[i], RAG128_4[i + 2], RAG128_4[i + 4]):
        case(f"fwd-reg128-vec-M{m}-N{n}-K{k}", "fwd", P(m, n, k), V("reg", 128, 128, big=1))
        if not (k <= 16 and m >= 256):
            case(f"bwd_data-reg128-vec-M{m}-K{n}-N{k}", "bwd_data", P(m, k, n), V("reg", 128, 128, big=1))
# the LDS-DMA tiles (reduction a multiple of 32, columns a multiple of 4: an odd column count cannot select them)
case("fwd-dma64x128-M1", "fwd", P(1, 65536 - 124, 32), V("dma", 64, 128, big=1))
case("fwd-dma64x128-M33-N65532", "fwd", P(33, 65536 - 4, 64), V("dma", 64, 128, big=1))
case("fwd-dma128x64-N124", "fwd", P(BIG_M, 124, 32), V("dma", 128, 64, big=1))
case("fwd-dma128x64-N252", "fwd", P(32641 + 128, 252, 64), V("dma", 128, 64, big=1))
case("fwd-dma128x64-N60", "fwd", P(65535, 60, 32), V("dma", 128, 64, big=1))
case("bwd_data-dma64x128-M1", "bwd_data", P(1, 32, 65536 - 124), V("dma", 64, 128, big=1))
case("bwd_data-dma64x128-M33-K65532", "bwd_data", P(33, 64, 65536 - 4), V("dma", 64, 128, big=1))
case("bwd_data-dma128x64-K60", "bwd_data", P(65535, 32, 60), V("dma", 128, 64, big=1))
case("bwd_data-dma128x64-K124", "bwd_data", P(BIG_M, 32, 124), V("dma", 128, 64, big=1))
case("bwd_data-dma128x64-K132", "bwd_data", P(BIG_M, 32, 132), V("dma", 128, 64, big=1))
case("bwd_data-dma128x64-K252", "bwd_data", P(32641 + 128, 32, 252), V("dma", 128, 64, big=1))
# weight gradients, N x K over the batch M: the 128 x 128 tiles at T - 4 in both dimensions, the register-staged one with every
# batch next to the 32-row step, and gradients with fewer rows or columns than a tile
case("bwd_weight-dma128-N2044-K4092", "bwd_weight", P(64, 2048 - 4, 4096 - 4), V("dma", 128, 128, big=1))
case("bwd_weight-dma128-N132-K65412", "bwd_weight", P(32, 132, 65536 - 124), V("dma", 128, 128, big=1))
case("bwd_weight-reg128-vec-M1", "bwd_weight", P(1, 2048 - 4, 4096 - 4), V("reg", 128, 128, big=1))
case("bwd_weight-reg128-vec-M31", "bwd_weight", P(31, 2048, 4096), V("reg", 128, 128, big=1))
case("bwd_weight-reg128-vec-M63", "bwd_weight", P(63, 2048 - 124, 4096), V("reg", 128, 128, big=1))
case("bwd_weight-reg128-scalar-M1", "bwd_weight", P(1, 2048, 4095), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-reg128-scalar-M2", "bwd_weight", P(2, 2047, 4096 - 124), V("reg", 128, 128, vec=0, big=1))
case("bwd_weight-reg128-scalar-M31-N127", "bwd_weight", P(31, 127, BIG_M), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-reg128-scalar-M63-N255", "bwd_weight", P(63, 255, 32641), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-reg128-scalar-M3-N1", "bwd_weight", P(3, 1, BIG_M), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-reg128-scalar-M33-K129", "bwd_weight", P(33, BIG_M, 129), V("reg", 128, 128, vec=0, big=1, vecC=0))
case("bwd_weight-reg128-scalar-M2-K1", "bwd_weight", P(2, BIG_M, 1), V("reg", 128, 128, vec=0, big=1, vecC=0))

# ------------------------------------------------------------------------------------------------------------ alignment lattice
# Offsets of 0 / 1 / 2 / 4 floats and leading dimensions of width / width + 1 / width + 4, one operand at a time, on a base of
# every path that can lose something: an operand off its 16-byte grid drops the 16-byte LOADS of the whole launch (and with them
# the LDS-DMA path); a result, bias or H off it drops the 16-byte STORES of that problem only.
LATTICE_BASES = {
    # kind: [(name, problem, record when everything is aligned, record when the loads drop)]
    "fwd": [("dma64", (65, 64, 64), V("dma", 64, 64), V("reg", 64, 64, vec=0)),
            ("reg64", (65, 64, 36), V("reg", 64, 64), V("reg", 64, 64, vec=0)),
            ("dma128x64", (BIG_M, 128, 32), V("dma", 128, 64, big=1), V("reg", 128, 128, vec=0, big=1)),
            ("lay2", (BIG_M, 32, 32), V("dma", 128, 32, lay=2, big=1), V("reg", 128, 128, vec=0, big=1)),
            ("dma64x128", (64, 65536 - 124, 32), V("dma", 64, 128, big=1), V("reg", 128, 128, vec=0, big=1)),
            ("reg128", (BIG_M, 128, 36), V("reg", 128, 128, big=1), V("reg", 128, 128, vec=0, big=1))],
    "bwd_data": [("dma64", (65, 64, 64), V("dma", 64, 64), V("reg", 64, 64, vec=0)),
                 ("reg64", (65, 36, 64), V("reg", 64, 64), V("reg", 64, 64, vec=0)),
                 ("dma128x64", (BIG_M, 32, 128), V("dma", 128, 64, big=1), V("reg", 128, 128, vec=0, big=1)),
                 ("dma64x128", (64, 32, 65536 - 124), V("dma", 64, 128, big=1), V("reg", 128, 128, vec=0, big=1)),
                 ("reg128", (BIG_M, 36, 128), V("reg", 128, 128, big=1), V("reg", 128, 128, vec=0, big=1))],
    "bwd_weight": [("dma64", (96, 64, 64), V("dma", 64, 64), V("reg", 64, 64, vec=0)),
                   ("reg64", (97, 64, 64), V("reg", 64, 64), V("reg", 64, 64, vec=0)),
                   ("lay1", (96, 32, 132), V("dma", 32, 128, lay=1), V("reg", 64, 64, vec=0)),
                   ("dma128", (32, 2048, 4096), V("dma", 128, 128, big=1), V("reg", 128, 128, vec=0, big=1)),
                   ("dma128x64", (32, 65536 - 124, 64), V("dma", 128, 64, big=1), V("reg", 128, 128, vec=0, big=1)),
                   ("dma64x128", (32, 64, 65536 - 124), V("dma", 64, 128, big=1), V("reg", 128, 128, vec=0, big=1)),
                   ("reg128", (33, 2048, 4096), V("reg", 128, 128, big=1), V("reg", 128, 128, vec=0, big=1))],
}
LOADED = {"fwd": ("X", "W"), "bwd_data": ("dY", "W"), "bwd_weight": ("dY", "X")}       # the operands whose alignment decides the loads
# the operands whose alignment decides the stores (db is stored element by element: its alignment never counts)
STORED = {"fwd": ("b", "Y"), "bwd_data": ("H", "dX"), "bwd_weight": ("dW",)}


def _lattice():
    for kind, bases in LATTICE_BASES.items():
        for name, mnk, aligned, dropped in bases:
            small = not aligned["big"]
            for op in OPERANDS[kind]:
                vector = op in ("b", "db")
                steps = [("off", 1), ("off", 2), ("off", 4)] + ([] if vector else [("ld", 1), ("ld", 4)])
                if not small and op == "db":
                    # left out on the big bases: the selector never reads db's address (every small base runs db at offsets 1, 2
                    # and 4 and keeps its record, and the host sweep finds no variant that depends on it), and the kernels
                    # store db one float at a time whatever the tile
                    steps = []
                for what, d in steps:
                    p = P(*mnk)
                    if what == "off":
                        p["off"][op] = d
                    else:
                        p["ld"][op] = operand_shape(kind, op, p)[1] + d
                    breaks = d in (1, 2)
                    e = dict(aligned)
                    e_no = None
                    if breaks and op in LOADED[kind]:
                        e = dict(dropped)
                    elif breaks and op in STORED[kind]:
                        e = dict(aligned, vecC=0)
                        if op == "H":
                            e_no = dict(aligned)
                    # single weight gradients in slabs store to the workspace (aligned, ld = K): dW's own alignment does not count
                    if kind == "bwd_weight" and op == "dW" and name in ("dma64", "reg64", "lay1"):
                        e = dict(aligned)
                    case(f"{kind}-lattice-{name}-{op}-{what}+{d}", kind, p, e, e_no)


_lattice()
# single-slab weight gradients (up to 64 rows of batch) store to dW itself: its alignment counts
case("bwd_weight-1slab-dW-off1", "bwd_weight", P(64, 64, 64, off={"dW": 1}), V("dma", 64, 64, vecC=0))
case("bwd_weight-1slab-dW-ld+1", "bwd_weight", P(64, 64, 64, ld={"dW": 65}), V("dma", 64, 64, vecC=0))
case("bwd_weight-1slab-dW-ld+4", "bwd_weight", P(33, 64, 64, ld={"dW": 68}), V("reg", 64, 64))

# ------------------------------------------------------------------------------------------------------------ groups
# three one-tile problems: 3 live work-groups in a grid of 24 (every problem's range is padded to 8)
case("fwd_group-3x1tile", "fwd_group", [P(64, 64, 64), P(1, 4, 32), P(33, 60, 96)], V("dma", 64, 64))
case("bwd_data_group-3x1tile", "bwd_data_group", [P(64, 64, 64), P(1, 32, 4), P(33, 96, 60)], V("dma", 64, 64))
case("bwd_weight_group-3x1tile", "bwd_weight_group", [P(64, 64, 64), P(32, 4, 8), P(96, 60, 36)], V("dma", 64, 64))
# 8 problems of every size around the tile
_EIGHT = [(64, 64, 64), (1, 4, 32), (65, 68, 96), (127, 124, 32), (130, 60, 64), (63, 128, 128), (200, 8, 32), (7, 132, 64)]
case("fwd_group-8", "fwd_group", [P(m, n, k) for m, n, k in _EIGHT], V("dma", 64, 64))
case("bwd_data_group-8", "bwd_data_group", [P(m, k, n) for m, n, k in _EIGHT], V("dma", 64, 64))
_EIGHT_W = [(96, 64, 64), (160, 4, 32), (192, 68, 96), (96, 124, 32), (160, 60, 64), (192, 128, 128), (96, 8, 32), (160, 132, 64)]
case("bwd_weight_group-8-splits3", "bwd_weight_group", [P(m, n, k) for m, n, k in _EIGHT_W], V("dma", 64, 64), splits=3)
# one unaligned problem among aligned ones: scalar loads for all of them; its own misaligned result: scalar stores for it alone
case("fwd_group-8-one-unaligned", "fwd_group", [P(m, n, k, off={"X": 1} if i == 5 else ({"Y": 2} if i == 2 else {}))
                                                for i, (m, n, k) in enumerate(_EIGHT)],
     V("reg", 64, 64, vec=0, vecC=[1, 1, 0, 1, 1, 1, 1, 1]))
case("bwd_data_group-8-one-unaligned", "bwd_data_group", [P(m, k, n, off={"W": 1} if i == 5 else ({"H": 1} if i == 2 else {}))
                                                          for i, (m, n, k) in enumerate(_EIGHT)],
     V("reg", 64, 64, vec=0, vecC=[1, 1, 0, 1, 1, 1, 1, 1]), V("reg", 64, 64, vec=0))
case("bwd_weight_group-8-one-unaligned", "bwd_weight_group",
     [P(96, n, k, ld={"X": k + 1} if i == 5 else ({"dW": k + 1} if i == 2 else {})) for i, (m, n, k) in enumerate(_EIGHT_W)],
     V("reg", 64, 64, vec=0, vecC=[1, 1, 0, 1, 1, 1, 1, 1]), splits=2)
case("fwd_group-K-odd-among-dma", "fwd_group", [P(64, 64, 64), P(64, 64, 36)], V("reg", 64, 64))     # one K % 32 != 0: no LDS-DMA for anyone
# small problems that are big only by their sum: 8 x 64 tiles of 128 x 128
case("fwd_group-big-by-sum", "fwd_group", [P(8192 - (i % 2) * 127, 128, 32) for i in range(8)], V("dma", 128, 64, big=1))
case("fwd_group-big-by-sum-reg", "fwd_group", [P(8192 - (i % 2) * 127, 128, 6) for i in range(8)], V("reg", 128, 128, vec=0, big=1))
case("bwd_data_group-big-by-sum", "bwd_data_group", [P(8192 - (i % 2) * 127, 32, 128) for i in range(8)], V("dma", 128, 64, big=1))
case("fwd_group-7-not-big", "fwd_group", [P(8192, 128, 32) for i in range(7)], V("dma", 64, 64))
# grouped weight gradients choose their slabs: 64 x 64 and 128-wide tiles that are big by their slabs alone
case("bwd_weight_group-big-64x64", "bwd_weight_group", [P(64 * 32, 64, 64) for i in range(8)], V("dma", 64, 64, big=1), splits=64)
case("bwd_weight_group-big-128", "bwd_weight_group", [P(64 * 32, 128, 132) for i in range(4)], V("dma", 128, 128, big=1), splits=64)
case("bwd_weight_group-big-128-reg", "bwd_weight_group", [P(64 * 32 - (31 if i == 1 else 0), 128, 132) for i in range(4)],
     V("reg", 128, 128, big=1), splits=64)
case("bwd_weight_group-big-128x64", "bwd_weight_group", [P(128 * 32, 132, 64) for i in range(2)], V("dma", 128, 64, big=1), splits=128)
case("bwd_weight_group-big-64x128", "bwd_weight_group", [P(128 * 32, 64, 132) for i in range(2)], V("dma", 64, 128, big=1), splits=128)
case("bwd_weight_group-big-64x64-dW-ld+1", "bwd_weight_group", [P(64 * 32, 64, 64, ld={"dW": 65} if i == 3 else {}) for i in range(8)],
     V("dma", 64, 64, big=1, vecC=[1, 1, 1, 0, 1, 1, 1, 1]), splits=64)
case("bwd_weight_group-big-64x128-dW-off1", "bwd_weight_group", [P(128 * 32, 64, 132, off={"dW": 1} if i == 1 else {}) for i in range(2)],
     V("dma", 64, 128, big=1, vecC=[1, 0]), splits=128)
case("bwd_weight_group-big-64x64-reg-scalar", "bwd_weight_group", [P(64 * 32, 63, 64) for i in range(8)],
     V("reg", 128, 128, vec=0, big=1), splits=64)
case("bwd_weight_group-big-128-reg-scalar-stores", "bwd_weight_group", [P(511 * 32 + 1, 127, 129)],
     V("reg", 128, 128, vec=0, big=1, vecC=0), splits=512)
# split-K edges: a last slab of a single 32-row step, and a batch of S * kchunk - 31
case("bwd_weight_group-last-slab-1-step", "bwd_weight_group", [P(3 * 64 + 32, 64, 64), P(3 * 64 + 32, 32, 132)], V("dma", 64, 64), splits=4)
case("bwd_weight_group-lay1-last-slab-1-step", "bwd_weight_group", [P(3 * 64 + 32, 32, 132)], V("dma", 32, 128, lay=1), splits=4)
case("bwd_weight_group-M-Sxkchunk-31", "bwd_weight_group", [P(4 * 64 - 31, 64, 64), P(4 * 64 - 31, 28, 132)], V("reg", 64, 64), splits=4)
case("bwd_weight_group-M-Sxkchunk-31-scalar", "bwd_weight_group", [P(4 * 64 - 31, 63, 65)], V("reg", 64, 64, vec=0, vecC=0), splits=4)
# rows of 10 / 53 floats inside 16- / 56-float strides, the padding readable (dy_cols / x_cols): 16-byte loads all the same
case("bwd_weight_group-padded-cols", "bwd_weight_group", [P(2048, 10, 53, ld={"dY": 16, "X": 56}, cols={"dY": 16, "X": 56})],
     V("dma", 64, 64, vecC=0), splits=8)
case("bwd_weight_group-padded-cols-1slab", "bwd_weight_group", [P(96, 10, 53, ld={"dY": 16, "X": 56}, cols={"dY": 16, "X": 56})],
     V("dma", 64, 64, vecC=0))
case("bwd_weight_group-padded-cols-lay1", "bwd_weight_group", [P(2048, 10, 133, ld={"dY": 16, "X": 136}, cols={"dY": 16, "X": 136})],
     V("dma", 32, 128, lay=1, vecC=0), splits=8)
case("bwd_weight_group-padded-cols-reg", "bwd_weight_group", [P(2047, 10, 53, ld={"dY": 16, "X": 56}, cols={"dY": 16, "X": 56})],
     V("reg", 64, 64, vecC=0), splits=8)
case("bwd_weight_group-unpadded-cols", "bwd_weight_group", [P(2048, 10, 53, ld={"dY": 16, "X": 56})],
     V("reg", 64, 64, vec=0, vecC=0), splits=8)


def variant_keys(kind, rec):
    """What the coverage test counts: the record without the grid size, the split count and kchunk, once per value of vecC."""
    return {(base_kind(kind), rec["path"], rec["tm"], rec["tn"], rec["lay"], rec["stages"], rec["vec"], rec["big"], c) for c in rec["vecC"]}


BASE_ADDR = 0x10000000                      # the made-up 16-byte aligned address the host tests hang the operands' offsets on


def query_problem(kind, p, ptr, act=1, slab_stride=0):
    """The descriptor dict ops.linear_variant takes for problem p; ptr(name) -> address or tensor of the operand (None: absent)."""
    b = base_kind(kind)
    ld = lambda n: p["ld"].get(n, operand_shape(b, n, p)[-1])                                # noqa: E731
    if b == "fwd":
        return dict(X=ptr("X"), ldx=ld("X"), W=ptr("W"), ldw=ld("W"), b=ptr("b"), Y=ptr("Y"), ldy=ld("Y"), M=p["M"], N=p["N"], K=p["K"], act=act)
    if b == "bwd_data":
        return dict(dY=ptr("dY"), lddy=ld("dY"), W=ptr("W"), ldw=ld("W"), H=ptr("H") if act else 0, ldh=ld("H") if act else 0, dX=ptr("dX"),
                    lddx=ld("dX"), M=p["M"], N=p["N"], K=p["K"], act=act)
    d = dict(dY=ptr("dY"), lddy=ld("dY"), X=ptr("X"), ldx=ld("X"), dW=ptr("dW"), lddw=ld("dW"), db=ptr("db"), M=p["M"], N=p["N"], K=p["K"])
    if kind.endswith("_group"):
        d.update(slab_stride=slab_stride, dy_cols=p["cols"].get("dY", 0), x_cols=p["cols"].get("X", 0))
    return d


def slab_stride(p, splits):
    """Distance between the slabs of a grouped weight gradient: the N x K block with its row stride, a gap of 8 floats (sentinels
    the kernels must leave alone) -- a multiple of 4 when the row stride is one, so that 16-byte stores stay possible."""
    if splits == 1:
        return 0
    return p["N"] * p["ld"].get("dW", p["K"]) + 8


def host_query(ops, c, act=1):
    """The selector's record for case c with made-up addresses (no GPU)."""
    kind = c["kind"]
    probs = [query_problem(kind, p, lambda n, p=p: BASE_ADDR + 4 * p["off"].get(n, 0), act, slab_stride(p, c["splits"])) for p in c["probs"]]
    if kind.endswith("_group"):
        return ops.linear_variant(kind, probs, splits=c["splits"])
    return ops.linear_variant(kind, probs[0], workspace=BASE_ADDR)
