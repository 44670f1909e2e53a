"""The built systems of tests/sparse_cases.py, checked without a GPU: a case whose predicate does not hold fails HERE, not on the GPU by
an unexplained counter.  Per case: the preconditions enqueue_forward sets for k_block_sparse, the predicate that forces the branch (the
ranks and depths of the construction, walked by `predict`, arrive at every expected counter), and that the oracle's rank, status and
dimension are what the construction says."""
import pytest

from oracle import gf2_oracle as O
from tests import sparse_cases as SC


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_is_what_it_claims(name):
    case = SC.cases()[name]
    case.check_preconditions()
    aug = case.aug()
    rows = aug.shape[0]
    assert rows == len(case.coefficient_rows()) and (rows <= 20000 or name == "beyond_window")
    want = O.solve_words(aug, rows, case.cols, 1)
    if case.diagonal:
        got = SC.predict(case)
        assert SC.holds(got, case.expect) == [], got["trace"]
        assert got["sparse_giveup_why"][0] == 0 and got["sparse_giveup_why"][3] == 0
        assert want["rank"] == case.rank()
    else:
        assert want["rank"] == case.cols          # (the panel-confined rows alone have full rank)
    assert (want["status"] == 0) == case.consistent
    if case.consistent:
        assert want["dim"] == case.cols - want["rank"]


def test_names_and_table_agree():
    assert list(SC.cases()) == SC.NAMES


def test_the_predicates_that_separate_neighbouring_branches():
    """What the table's rows rest on, spelled out once: ranks of the first 64 / first 512 entries and of the truncated pools."""
    C = SC.cases()

    def entries(case, b, g, pool=None):
        rows = case.blocks[b][:pool]
        return [w for q, w in rows if q == g]

    for name, entry in (("absorb_100", 100), ("absorb_511", 511), ("absorb_512", 512)):
        e = entries(C[name], 1, 2)
        assert SC.rank_of(e[:64]) == 63 and SC.rank_of(e[:entry]) == 63 and SC.rank_of(e[:entry + 1]) == 64
        assert (SC.rank_of(e[:SC.SP_NE]) == 64) == (entry < SC.SP_NE)
    # the cycle: every block from 2 to 8 WOULD complete each panel from its first 64 entries
    for b in range(2, 9):
        assert all(SC.rank_of(entries(C["cycle"], b, g)[:64]) == 64 for g in range(SC.G))
    # truncated: more rows than the small pool, the pivots inside it
    t = C["truncated"].blocks[1]
    assert len(t) > SC.POOLS[0] and all(SC.rank_of(entries(C["truncated"], 1, g, SC.POOLS[0])[:64]) == 64 for g in range(SC.G))
    # depths: the pool that misses the decisive row has rank 63 on its panel, the next size has 64
    for name, b, small, large in (("escalate_middle", 1, 0, 1), ("escalate_middle", 2, 0, 1), ("escalate_largest", 2, 1, 2),
                                  ("escalate_largest", 3, 1, 2), ("pipelined", 5, 0, 1)):
        assert SC.rank_of(entries(C[name], b, 3, SC.POOLS[small])) == 63 and SC.rank_of(entries(C[name], b, 3, SC.POOLS[large])) == 64
    assert SC.NZ_LARGEST < len(C["straight_to_largest"].blocks[1]) and len(C["escalate_middle"].blocks[2]) <= SC.NZ_LARGEST
    # no pool completes a deficient block; reasons 5 and 2
    for b in (1, 2, 3):
        assert SC.rank_of(entries(C["strikes_probed"], b, 1)) == 63
    r = C["reasons_5_and_2"]
    assert len(entries(r, 1, 2)) < 64 <= 64 * SC.G <= len(r.blocks[1]) and len(r.blocks[2]) < 64 * SC.G
    # alive bound: block 9's rows are rows 0..255 of alive_top and its only ones; the reverse order; a bound of 1 behind block 1
    a = C["alive_top"]
    assert a.block_start(9) == 0 and len(a.blocks[9]) == 64 * SC.G
    rev = C["alive_reverse"]
    assert [rev.block_start(b) for b in range(1, 9)] == sorted((rev.block_start(b) for b in range(1, 9)), reverse=True)
    m = C["alive_min_free"]
    assert m.block_start(1) == 0 and m.blocks[1][0] == m.blocks[1][1]
    # ... with teeth: rows 0 and 1 agree on block 1's window, and whichever of them block 1 leaves untaken is the only row of the
    # system with a bit in column 7 of block 5's panel 2
    t = C["alive_min_free_row_in_two_blocks"].coefficient_rows()
    win1 = ((1 << 256) - 1) << 256
    col = 64 * (SC.G * 5 + 2) + 7
    assert isinstance(t[0], int) and isinstance(t[1], int) and t[0] & win1 == t[1] & win1 != 0 and (t[0] ^ t[1]) >> col & 1
    assert not any(r[0] == SC.G * 5 + 2 and r[1] >> 7 & 1 for r in t[2:] if isinstance(r, tuple))
    # beyond the window: block 8's rows start past every mask word the kernel can look at while a zero row is alive below them
    w = C["beyond_window"]
    zero0 = next(i for i, r in enumerate(w.coefficient_rows()) if r is None)
    assert w.block_start(8) >= (zero0 // 64 + SC.SP_NW) * 64 and w.block_start(8) - zero0 == 66000
