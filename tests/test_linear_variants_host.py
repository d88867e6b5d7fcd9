"""The Linear kernel selection, asked of the library on the host (ops.linear_variant: no launch, no device): every case of
tests/linear_variant_cases.py selects the variant it names, and the table reaches every variant the selector can name."""
import itertools

import pytest

from tests import linear_variant_cases as LV

MB = 1 << 20


@pytest.fixture(scope="module")
def ops():
    from partmanip_amd import ops as o
    return o


@pytest.mark.parametrize("c", LV.CASES, ids=[c["id"] for c in LV.CASES])
def test_case_selects_the_variant_it_names(ops, c):
    for act, key in ((1, "expect"), (0, "expect_noact")):
        got = LV.host_query(ops, c, act)
        want = c[key]
        assert {k: got[k] for k in want} == want, (c["id"], key, got)
        assert len(got["splits"]) == len(c["probs"]) and all(k % 32 == 0 for k in got["kchunk"])
        if c["kind"] == "bwd_weight_group":
            assert got["splits"] == [c["splits"]] * len(c["probs"])


def test_case_table_stays_small():
    """About 64 MB of operands per case at the most (a test takes seconds, its fp64 reference included): 76 MB, because the smallest
    `big` data gradient, 512 tiles of 128 x 128, has 33 MB in dX and as much in H beside its dY."""
    for c in LV.CASES:
        total = 0
        for p in c["probs"]:
            for name in LV.OPERANDS[LV.base_kind(c["kind"])]:
                shape = LV.operand_shape(LV.base_kind(c["kind"]), name, p)
                total += 4 * shape[0] * (p["ld"].get(name, shape[-1]) if len(shape) == 2 else 1) * (c["splits"] if name in ("dW", "db") else 1)
        assert total < 76 * MB, (c["id"], total / MB)


def test_group_grid_pads_every_problem_to_eight(ops):
    """Three one-tile problems: a grid of 24 work-groups, 21 of them idle."""
    for c in LV.CASES:
        if c["id"].endswith("-3x1tile"):
            assert LV.host_query(ops, c)["grid"] == 24, c["id"]


def test_query_rejects_what_the_launch_rejects(ops):
    B = LV.BASE_ADDR
    with pytest.raises(RuntimeError, match="PM_EINVAL"):
        ops.linear_variant("fwd", dict(X=B, ldx=3, W=B, ldw=4, b=B, Y=B, ldy=4, M=4, N=4, K=4, act=0))         # ldx < K
    with pytest.raises(RuntimeError, match="PM_EINVAL"):
        ops.linear_variant("bwd_data", dict(dY=B, lddy=4, W=B, ldw=4, H=0, ldh=0, dX=B, lddx=4, M=4, N=4, K=4, act=1))   # act without H
    with pytest.raises(RuntimeError, match="PM_EINVAL"):
        ops.linear_variant("bwd_weight_group", [dict(dY=B, lddy=4, X=B, ldx=4, dW=B, lddw=4, db=B, M=64, N=4, K=4, slab_stride=32)], splits=3)


# ---------------------------------------------------------------------------------------------------------------- coverage
SIZES = (1, 4, 32, 33, 36, 64, 68, 132, 256, 1028, 4096, 65536)
# Variants the table leaves out: key -> (smallest selecting shape the sweep finds, its operand bytes), allowed only beyond 256 MB.
EXCLUDED = {}


def _bytes(kind, M, N, K):
    return 4 * {"fwd": M * K + N * K + N + M * N, "bwd_data": M * N + N * K + 2 * M * K, "bwd_weight": M * N + M * K + N * K + N}[kind]


def _sweep(ops):
    """Orientation x alignment x sizes through the query: every distinct record (without grid, splits, kchunk) with the smallest
    shape that selects it."""
    B = LV.BASE_ADDR
    found = {}

    def note(kind, rec, M, N, K, extra):
        for key in LV.variant_keys(kind, rec):
            b = _bytes(kind, M, N, K)
            if key not in found or b < found[key][1]:
                found[key] = ((M, N, K) + extra, b)

    for M, N, K in itertools.product(SIZES, repeat=3):
        for kind in ("fwd", "bwd_data", "bwd_weight"):
            if _bytes(kind, M, N, K) > 1024 * MB:
                continue
            names = LV.OPERANDS[kind]
            for mis in itertools.product((0, 1), repeat=4):
                if kind == "bwd_weight" and mis[3]:
                    continue                                        # db: never looked at
                p = LV.P(M, N, K, off={n: m for n, m in zip(names, mis)})
                ptr = lambda n: B + 4 * p["off"][n]                                                        # noqa: E731
                for act in ((0, 1) if kind == "bwd_data" and mis[2] else (1,)):
                    note(kind, ops.linear_variant(kind, LV.query_problem(kind, p, ptr, act), workspace=B), M, N, K, (mis, act))
                if kind == "bwd_weight" and not mis[3]:             # the grouped form chooses its slabs
                    for S in (4, 64, 512):
                        kc = (-(-M // S) + 31) // 32 * 32
                        if (S - 1) * kc < M:
                            d = LV.query_problem("bwd_weight_group", p, ptr, 1, N * K + 8)
                            note(kind, ops.linear_variant("bwd_weight_group", [d], splits=S), M, N, K, (mis, S))
    return found


def test_case_table_covers_every_reachable_variant(ops):
    found = _sweep(ops)
    covered = set()
    for c in LV.CASES:
        for act in (0, 1):
            covered |= LV.variant_keys(c["kind"], LV.host_query(ops, c, act))
    assert len(found) >= 40, len(found)                             # the sweep itself reaches the family
    missing = {k: v for k, v in found.items() if k not in covered}
    left_out = {k: v for k, v in missing.items() if k in EXCLUDED}
    uncovered = {k: v for k, v in missing.items() if k not in EXCLUDED}
    assert not uncovered, "variants no case selects (key: smallest shape, bytes):\n" + "\n".join(f"{k}: {v}" for k, v in sorted(uncovered.items()))
    for k, (shape, b) in left_out.items():
        assert b > 256 * MB and EXCLUDED[k] == (shape, b), (k, shape, b)
    assert set(EXCLUDED) <= set(missing), "an excluded variant is covered or unreachable: drop it from EXCLUDED"
