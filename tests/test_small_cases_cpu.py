"""The built systems of tests/small_cases.py, checked without a GPU: a case whose premise does not hold fails HERE, not on the GPU by an
unexplained counter.  Per case: the construction rule, one (passes, kinds, rank) over the arrival orders, the model's rank and pivot
columns against the oracle, the property the case is named after, and that the one-launch kernel is eligible for it.  Then the two
facts the constructions rest on, the shapes the entries can reach, and plain-integer models of the two digit loaders (the load of
k_small_solve, k_pack_digits) against the definition for every digit width."""
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import small_cases as SC


@pytest.fixture(scope="module")
def cases():
    return SC.cases()


def test_names_and_table_agree(cases):
    assert list(cases) == SC.NAMES
    # the table of tests/small_cases.py: which counters are exact and which are contained
    assert [n for n, c in cases.items() if not c.exact] == [n for n in SC.NAMES if n.startswith("wide")]


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_is_what_it_claims(name, cases):
    case = cases[name]
    assert SC.eligible(case.rows, case.cols) and case.rows >= case.cols
    SC.check_construction(case)
    designed = 1 if case.mixed else None              # mixed: the designed panel is the first; the later ones are ordinary
    assert not case.mixed or case.panel == 0
    seen = set()
    for order in case.orders():
        m = SC.model(case.coef, case.cols, order, panels=designed)
        seen.add((m["passes"], m["kinds"], m["rank"]))
    assert len(seen) == 1, seen
    passes, kinds, rank = seen.pop()
    assert (passes, kinds) == (case.passes, case.kinds)
    # every wavefront finished before the next looks: nothing but "candidates were left out" may move
    for order in case.orders(20):
        m = SC.model(case.coef, case.cols, order, serial=True, panels=designed)
        assert (m["passes"], m["rank"]) == (passes, rank)
        assert m["kinds"] | SC.KIND_LEFT_OUT == kinds | SC.KIND_LEFT_OUT and m["kinds"] & ~kinds == 0
    # the whole solve against the oracle: rank and the pivot columns
    aug = case.aug()
    want = O.solve_words(aug, case.rows, case.cols, 1)
    full = SC.model(case.coef, case.cols)
    assert full["rank"] == want["rank"] and sorted(full["pivrow"]) == list(want["pivcols"])
    assert want["status"] == 0 and want["dim"] == case.cols - want["rank"]
    assert case.holds(full["passes"], full["kinds"])
    if case.mixed:
        # every later column gets a pivot, so every row's later words are consumed: a row whose other words did not follow its
        # combination ends as a non-pivot row that is not zero, or with the wrong constant (the planted solution decides)
        assert full["per_panel"][0] == case.passes and want["rank"] == rank + case.cols - 64
    else:
        # confined: no row has bits in two panels
        for a in case.coef:
            assert sum(1 for q in range((case.cols + 63) // 64) if (a >> (64 * q)) & SC.M64) <= 1


def panel_words(case, q=0):
    return [(a >> (64 * q)) & SC.M64 for a in case.coef]


def rank_of(words):
    basis = {}
    for w in words:
        while w:
            h = w.bit_length() - 1
            if h not in basis:
                basis[h] = w
                break
            w ^= basis[h]
    return len(basis)


def test_the_properties_the_cases_are_named_after(cases):
    C = cases
    # the 4 / 5 edge: every stripe of first_k is full, has rank k, and holds a row with all k bits (the row the bit loops must not
    # shorten to four pivot rows); the twins differ in k alone
    for name, k in (("first_3", 3), ("first_4", 4), ("first_5", 5), ("wide13_first_3", 3), ("wide13_first_5", 5), ("wide12_first_4", 4)):
        w = panel_words(C[name])
        span = 0
        for x in w:
            span |= x
        assert bin(span).count("1") == k and C[name].plant & span == span
        for r0 in range(0, len(w) - 63, 64):
            st = w[r0:r0 + 64]
            assert all(st) and rank_of(st) == k and span in st
        assert (C[name].kinds & SC.KIND_FIRST_FEW != 0) == (k <= 4) and (C[name].kinds & SC.KIND_FIRST_TABLES != 0) == (k > 4)
    assert (C["first_4"].rows, C["first_4"].cols) == (C["first_5"].rows, C["first_5"].cols)
    # later_tables / later_few: the second pass's pivots are in rows >= 1024 only, and every stripe below is full
    for name, low_rank, n2 in (("later_tables", 32, 64), ("later_few", 62, 3)):
        w = panel_words(C[name])
        assert all(w[:1024]) and rank_of(w[:1024]) == low_rank and rank_of(w) == 64 and len(w) - 1024 == n2
        assert all(rank_of(w[r0:r0 + 64]) == low_rank for r0 in range(0, 1024, 64))
    assert any(bin(x).count("1") > 1 for x in panel_words(C["later_few"])[:64])          # sums among the stripe's rows
    # slots_40: identical stripes, 40 independent vectors then zero rows
    w = panel_words(C["slots_40"])
    assert all(w[r0:r0 + 64] == w[:64] for r0 in range(0, len(w), 64)) and rank_of(w[:40]) == 40 and not any(w[40:64]) and len(w) <= 1024
    # second_stripe_first_pass: fewer than 64 candidates below row 1024, the rest of the basis above, in two wavefronts' second stripes
    w = panel_words(C["second_stripe_first_pass"])
    low, high = [x for x in w[:1024] if x], [x for x in w[1024:] if x]
    assert len(low) + len(high) < 64 and rank_of(low) == len(low) == 20 and rank_of(low + high) == 60
    assert {r // 64 for r in range(1024, len(w)) if w[r]} == {16, 17}
    # last_stripe_4096: every non-zero row is in wavefront 15's fourth stripe
    c = C["last_stripe_4096"]
    assert c.rows == 4096 and SC.words_of(c.cols) <= 2 and not any(c.coef[:4032]) and all(c.coef[4032:])
    # deficient_then_empty: rank 30, no bit at all, a full panel
    c = C["deficient_then_empty"]
    assert [rank_of(panel_words(c, q)) for q in range(3)] == [30, 0, 64] and sum(1 for x in panel_words(c, 0) if x) == 50
    # partial_last_panel: the constant's bit shares the last panel's word, for 63 columns at bit 63
    for name, rem in (("partial_last_1", 1), ("partial_last_63", 63)):
        c = C[name]
        assert c.cols % 64 == rem and c.panel == c.cols // 64 == (c.cols + 63) // 64 - 1 and rank_of(panel_words(c, c.panel)) == rem
        assert any(int(x) >> rem & 1 for x in c.aug()[:, c.panel])
    # the second pass below 1024 rows: stripe s carries its own column 32 + s, and a pass takes one stripe
    for name, own in (("wide13_later_tables", 9), ("wide13_later_few", 4)):
        w = panel_words(C[name])
        for s, r0 in enumerate(range(0, len(w), 64)):
            st = w[r0:r0 + 64]
            assert all(st) and rank_of(st) == min(len(st), 32 + (s < own))
        assert rank_of(w) == 32 + own and (own - 1 <= 4) == (C[name].kinds & SC.KIND_LATER_FEW != 0)


def test_a_full_stripe_pass_takes_one_whole_stripe_and_never_looks_above_row_1024():
    """Fact (F): every stripe below row 1024 holds 64 candidates -> the list is one whole stripe, the winner's, for every arrival order
    and interleaving, and no row >= 1024 enters."""
    rows = 1300
    stripe = lambda r0: list(range(r0, min(r0 + 64, rows)))
    rng = random.Random(1)
    for t in range(200):
        order = list(range(SC.NW))
        rng.shuffle(order)
        for serial in (False, True):
            lst, ncand = SC.gather(stripe, rows, order, serial)
            assert lst == stripe(64 * order[0]) and max(lst) < 1024
            assert ncand == (64 if serial else 1024)


def test_panel_confined_rows_make_the_panels_independent(cases):
    """Fact: rows with support inside one panel -> a panel's passes are those of the panel alone, whatever the other panels hold."""
    for name in ("one_pass_64", "deficient_then_empty", "partial_last_1", "last_stripe_4096"):
        c = cases[name]
        whole = SC.model(c.coef, c.cols)
        npan = (c.cols + 63) // 64
        alone = [SC.model([a & (SC.M64 << (64 * q)) for a in c.coef], c.cols)["passes"] for q in range(npan)]
        assert whole["per_panel"] == alone and whole["passes"] == sum(alone)


def test_the_entries_reach_at_most_13_words_per_row():
    """rows >= cols (check_shape) and eligibility together: 13 words is the widest row, 905 x 831 its largest system; the room the kernel
    keeps for 14-16 words cannot be entered, and the entries say so before any device is touched."""
    widest = max(SC.words_of(cols) for cols in range(1, SC.MAXCOLS + 1) if SC.eligible(cols, cols))
    assert widest == 13 and SC.largest_rows(13) == 905 and SC.eligible(905, 831) and not SC.eligible(906, 831)
    for wt in (14, 15, 16):
        rows, cols = SC.largest_rows(wt), 64 * wt - 1
        assert SC.eligible(rows, cols) and rows < 64 * (wt - 1)          # fewer rows than the width's smallest column count
        with pytest.raises(ValueError, match="greater than or equal"):
            hip.solve_words(np.zeros((rows, wt), dtype=np.uint64), rows, cols, 1)
    assert SC.largest_rows(16) == 572


# ---- the digit loaders ---------------------------------------------------------------------------------------------------------------

def small_word(d, bpd, w, cols):
    """word w of a row as the load phase of k_small_solve forms it from the digits d"""
    wt, nd = SC.words_of(cols), len(d)
    p0 = w * 64 + 1
    di0, sh, filled, v = p0 // bpd, p0 % bpd, 0, 0
    dg = [d[di0 + u] if di0 + u < nd else 0 for u in range(4)]
    first = d[0] if nd > 0 else 0
    for u in range(4):
        if filled < 64:
            v |= ((dg[u] >> sh) << filled) & SC.M64
            filled += bpd - sh
            sh = 0
    di = di0 + 4
    while filled < 64 and di < nd:          # (bpd < 22 needs more than four digits per word: the tail, one by one)
        v |= (d[di] << filled) & SC.M64
        filled += bpd
        di += 1
    c0 = w * 64
    if c0 + 64 > cols:
        v &= SC.e(cols - c0) - 1 if cols - c0 > 0 else 0
    if w == cols >> 6 and first & 1:
        v |= SC.e(cols & 63)
    topmask = SC.e((cols + 1) & 63) - 1 if (cols + 1) & 63 else SC.M64
    return v & topmask if w == wt - 1 else v


def pack_word(d, bpd, w, cols):
    """... and as k_pack_digits forms it"""
    nd, val, c0 = len(d), 0, w * 64
    if c0 < cols:
        p0 = c0 + 1
        di, sh, filled = p0 // bpd, p0 % bpd, 0
        while filled < 64 and di < nd:
            val |= ((d[di] >> sh) << filled) & SC.M64
            filled += bpd - sh
            sh = 0
            di += 1
        if cols - c0 < 64:
            val &= SC.e(cols - c0) - 1
    if w == cols >> 6 and nd > 0:
        val |= (d[0] & 1) << (cols & 63)
    return val


@pytest.mark.parametrize("bpd", range(1, 33))
def test_both_digit_loaders_follow_the_definition(bpd):
    """bit 0 of the integer = the constant (column `cols`), bit k = column k - 1, bits above cols ignored; rows with no digits are 0"""
    rng = random.Random(bpd)
    for cols in (1, 5, 62, 63, 64, 65, 127, 128, 129, 200, 831, 1023):
        wt = SC.words_of(cols)
        for nbits in (0, 1, 2, cols // 2, cols, cols + 1, cols + 40, cols + 1 + 4 * bpd):
            v = rng.getrandbits(nbits) | (SC.e(nbits - 1) if nbits else 0)
            dig, off = SC.digits([v], bpd)
            d = [int(x) for x in dig]
            assert len(d) == (nbits + bpd - 1) // bpd == off[1]
            full = ((v >> 1) & (SC.e(cols) - 1)) | ((v & 1) << cols)
            for w in range(wt):
                want = (full >> (64 * w)) & SC.M64
                assert small_word(d, bpd, w, cols) == want and pack_word(d, bpd, w, cols) == want, (cols, nbits, w)
