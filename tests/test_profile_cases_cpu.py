"""tests/profile_cases.py checked before the GPU tests trust it: every case against the CPU oracle in both modes, the property each case
is named for recomputed from its pivots, the fast applier against KA.apply_numpy word for word, the append pair and the right-hand sides."""
import numpy as np
import pytest

from oracle import gf2_oracle as O
from tests import known_answer as KA
from tests import profile_cases as PC


@pytest.mark.parametrize("name", list(PC.TABLE))
def test_known_answer_equals_the_oracle(name):
    """(for small_300x200 and small_905x831, with fewer than cols + 128 rows, this is also what says that the unedited columns are
    independent)"""
    c = PC.case(name)
    assert c.aug.shape == (c.rows, O.words_for(c.cols)) and c.rows <= 2700 and c.rows >= c.cols + 64
    assert c.want["status"] == (1 if name.startswith("inconsistent") else 0)
    for mode in (0, 1):
        KA.assert_same(O.solve_words(c.aug, c.rows, c.cols, mode), c.want, mode)


@pytest.mark.parametrize("name", list(PC.TABLE))
def test_fast_applier_equals_apply_numpy(name):
    c = PC.case(name)
    assert np.array_equal(KA.apply_numpy(O.gen_synthetic(c.rows, c.cols, c.seed), c.cols, c.spec), c.aug)


def test_fast_applier_on_a_padded_stride_and_a_row_range():
    c = PC.case("last_word_1279")                              # the RHS is bit 63 of the last word
    wide = O.gen_synthetic(c.rows, c.cols, c.seed, O.words_for(c.cols) + 3)
    got = PC.apply_fast(wide, c.cols, c.spec)
    assert np.array_equal(got[:, :c.aug.shape[1]], c.aug) and not got[:, c.aug.shape[1]:].any()
    raw = O.gen_synthetic(c.rows, c.cols, c.seed)
    assert np.array_equal(PC.apply_fast(raw[100:333], c.cols, c.spec), c.aug[100:333])


def test_every_free_column_is_dense():
    """what zero and copied columns do not give: a kernel vector per free column with about half of the pivots left of it"""
    for name in PC.NAMES:
        c = PC.case(name)
        sizes = {op[1]: len(op[2]) for op in c.spec if op[0] == "col_xor"}
        for f in c.free:
            left = f - sum(1 for g in c.free if g < f)
            if left >= 40:
                assert .3 * left < sizes[f] < .7 * left, (name, f, left, sizes.get(f))
        assert [op[1] for op in c.spec if op[0] == "zero_col"] in ([], [0])


def _masks(name):
    c = PC.case(name)
    return c, PC.panel_masks(c.want["pivcols"], c.cols)


@pytest.mark.parametrize("name", list(PC.MASKS))
def test_named_pivot_masks(name):
    c, masks = _masks(name)
    for p, m in enumerate(masks):
        assert m == PC.MASKS[name].get(p, PC.full_mask(p, c.cols)), (name, p, hex(m))
    assert masks[0] == PC.ALL and masks[len(masks) - 2] == PC.ALL       # full panels left and right of the holes
    nb = (c.cols + PC.B - 1) // PC.B
    holes = sorted({f // PC.B for f in c.free})
    assert 0 < holes[0] and holes[-1] < nb - 1


def test_alternate_has_32_pivots_in_each_of_four_panels():
    c, masks = _masks("alternate")
    assert [bin(m).count("1") for m in masks[4:8]] == [32] * 4 and c.want["dim"] == 128


def test_every_5th_drifts_across_every_panel_block_and_group():
    c, masks = _masks("every_5th")
    assert c.want["dim"] == 440 and c.want["rank"] == 2060
    assert all(m == PC.ALL for m in masks[:4]) and all(12 <= 64 - bin(m).count("1") <= 13 for m in masks[5:39])
    piv = c.want["pivcols"]
    drift = piv - np.arange(len(piv))
    assert drift[0] == 0 and drift[-1] == 440 and len(set(drift.tolist())) == 441      # rank index k and column differ by 0 .. 440
    k = PC.case("inconsistent")
    assert k.free == c.free and k.want["status"] == 1 and np.array_equal(k.want["pivcols"], piv)


def test_group_edge():
    c, masks = _masks("group_edge")
    assert c.want["dim"] == 28
    low14 = (1 << 50) - 1                                      # columns 1010 .. 1023 are bits 50 .. 63 of panel 15; 960 is its bit 0
    assert masks[15] == low14 & ~1
    assert masks[16] == PC.ALL & ~0x7F & ~(1 << 63)            # columns 1024 .. 1030 and 1087
    single = {p: bin(PC.full_mask(p, c.cols) & ~m).count("1") for p, m in enumerate(masks) if p not in (15, 16)}
    assert {p for p, n in single.items() if n} == {2, 5, 7, 9, 12} and set(single.values()) == {0, 1}


@pytest.mark.parametrize("name", list(PC.DIMS))
def test_dim_cases_hold_exactly_n_holes_between_pivots(name):
    c, masks = _masks(name)
    n = PC.DIMS[name]
    assert c.want["dim"] == n == len(c.free)
    assert len({f >> 6 for f in c.free}) == min(n, len(masks)) and len(masks) == 21       # spread over all panels
    piv = set(c.want["pivcols"].tolist())
    between = [f for f in c.free if any(p in piv for p in range(f & ~63, f)) and any(p in piv for p in range(f + 1, (f | 63) + 1))]
    assert len(between) >= 2


@pytest.mark.parametrize("cols", [1217, 1279, 1280])
def test_last_word_cases(cols):
    c, masks = _masks(f"last_word_{cols}")
    last = (cols - 1) // 64
    assert set(c.free) == {0, last * 64, cols - 2, cols - 1} and c.spec[-1][0] == "col_xor"
    assert ("zero_col", 0) in c.spec and masks[0] == PC.ALL & ~1
    want_last = PC.full_mask(last, cols) & ~1 & ~(1 << ((cols - 1) & 63)) & ~((1 << ((cols - 2) & 63)) if (cols - 2) >> 6 == last else 0)
    assert masks[last] == want_last


@pytest.mark.parametrize("name", ["small_300x200", "small_905x831"])
def test_small_cases(name):
    c, masks = _masks(name)
    every_third = sum(1 << b for b in range(64) if b % 3)
    assert masks[0] == PC.ALL & ~(1 << 63) and masks[1] == every_third and masks[2] & 1 == 0
    assert (c.cols - 1 in c.free) == (name == "small_905x831") and c.rows < c.cols + 128


def test_append_pair():
    p = PC.append_pair()
    assert p.a.shape[0] == 1100 and p.b.shape[0] == 400 and len(p.free2) == 20 and set(p.free2) < set(p.free1)
    assert p.free1 == PC.case("alternate").free and np.array_equal(p.a, PC.case("alternate").aug[:1100])
    assert p.want["dim"] == 20 and np.array_equal(p.want["origin"], PC.case("alternate").want["origin"])
    for mode in (0, 1):
        KA.assert_same(O.solve_words(p.stacked, p.rows, p.cols, mode), p.want, mode)
    # A alone: 1100 equations of rank 1100 in 1300 unknowns, F1's kernel vectors among its 200
    padded = np.vstack([p.a, np.zeros((p.cols - 1100, p.a.shape[1]), dtype=np.uint64)])
    got = O.solve_words(padded, p.cols, p.cols, 1)
    assert (got["status"], got["rank"], got["dim"]) == (0, 1100, 200)
    full = PC.case("alternate").want["basis"]
    rows_of = {int(np.flatnonzero(np.unpackbits(v.view(np.uint8), bitorder="little"))[-1]): v for v in got["basis"]}
    for v in full:
        top = int(np.flatnonzero(np.unpackbits(v.view(np.uint8), bitorder="little"))[-1])
        assert np.array_equal(rows_of[top], v)


@pytest.mark.parametrize("name", ["group_edge", "every_5th", "edges"])
def test_right_hand_sides(name):
    c = PC.case(name)
    bits, want = PC.rhs_bits(name), PC.rhs_oracle(name)
    assert bits.shape == (65, c.rows) and PC.rhs_words(bits).shape == (65, (c.rows + 63) // 64)
    assert [w["status"] for w in want] == [1 if j in PC.BAD_RHS else 0 for j in range(65)]
    assert len({w["origin"].tobytes() for w in want}) >= 60
    for w in want:
        assert np.array_equal(w["pivcols"], c.want["pivcols"])
        if w["status"] == 0:
            assert np.array_equal(w["basis"], c.want["basis"])
