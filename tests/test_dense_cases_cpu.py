"""The built systems of tests/dense_cases.py, checked without a GPU: a case whose claim does not hold fails HERE, not on the GPU by an
unexplained counter.  Per case: every row is confined to one block, the claim the case is named for holds under `simulate`, the model
arrives at the table's `==` / `>=` entry, and the oracle's rank and pivots are what the construction says.  The model's pivot sets are
checked against an independent rank computation (rank_of on the words each panel looked at), its used rows against the blocks' home
rows, and its combinations against the source words they are said to combine."""
import numpy as np
import pytest

from oracle import gf2_oracle as O
from tests import dense_cases as DC
from tests.sparse_cases import FAST_NC, G, TWO_LEVEL_MIN_BYTES, rank_of

# the table: what gf2bv_stats::fast_blocks must read.  Every entry is exact: a case whose count the general path's verdict could move
# has its case block where no search can follow (see dense_cases._late) or gives up where every later block is out of reach as well
TABLE = {"plain": ("==", 10), "chain": ("==", 9), "giveup_then_back": ("==", 9), "first_block_refused": ("==", 9),
         "anchor_zero_row": ("==", 7), "anchor_edge_2047": ("==", 9), "anchor_edge_2048": ("==", 8), "tail_320": ("==", 10),
         "tail_319": ("==", 9), "leftover_low": ("==", 10), "leftover_mid": ("==", 10), "seven_blocks": ("==", 6),
         "dense_48": ("==", 9), "dense_47": ("==", 8), "dense_13": ("==", 9), "dense_12": ("==", 8), "dense_carry_48": ("==", 9),
         "dense_carry_47": ("==", 8), "giveup_panel0": ("==", 8), "giveup_panel2": ("==", 8), "giveup_panel3": ("==", 8),
         "absorb_incomplete_g0": ("==", 8), "absorb_last_lane_g0": ("==", 9), "absorb_incomplete_g2": ("==", 8),
         "absorb_last_lane_g2": ("==", 9)}
TABLE.update({f"miss_{k}_g{g}": ("==", 9) for k in (1, 2, 4, 7, 8) for g in range(G)})
TABLE.update({f"miss_9_g{g}": ("==", 8) for g in range(G)})


def test_names_and_table_agree():
    assert list(DC.cases()) == DC.NAMES and sorted(TABLE) == sorted(DC.NAMES)
    for name, case in DC.cases().items():
        assert case.expect == {"fast_blocks": TABLE[name]}, name


@pytest.mark.parametrize("name", DC.NAMES)
def test_case_is_what_it_claims(name):
    case = DC.cases()[name]
    aug = case.aug()
    rows, wt = aug.shape
    assert rows == len(case.rows) and 64 * G * case.full_blocks == case.cols <= 4096 and case.nblocks == case.full_blocks + 1
    assert rows * wt * 8 < TWO_LEVEL_MIN_BYTES, "a one-level plan unless forced"
    # every row is confined to one block: its coefficient words lie in one aligned group of four
    coef = aug[:, :case.cols // 64]
    nz = coef != 0
    for i in np.flatnonzero(nz.any(axis=1)):
        w = np.flatnonzero(nz[i])
        assert w[0] // G == w[-1] // G == case.rows[i][0], (name, i)
    assert [i for i in range(rows) if case.rows[i] is None] == list(np.flatnonzero(~nz.any(axis=1)))
    # home rows: 256 per block, independent (one short where the case says so); every other row is a zero row
    for b in range(case.full_blocks):
        home = [sum(int(w) << (64 * e) for e, w in enumerate(r[1])) for r in case.rows if r is not None and r[0] == b]
        assert len(home) == 64 * G and rank_of(home) == 64 * G - (case.deficit if b == case.block else 0), (name, b)
    # the claim, and the table's entry -- the same count with and without the optimistic enqueue
    for optimistic in (True, False):
        m = case.model(optimistic)
        assert m["fast_blocks"] == case.expect["fast_blocks"], (name, optimistic, m["low"], m["high"])
    case.claim(case.model(True)["trace"])
    # the oracle: full rank, every column a pivot -- but one column of the case block's panel where it is rank deficient
    want = O.solve_words(aug, rows, case.cols, 1)
    assert want["status"] == 0 and want["rank"] == case.cols - case.deficit and want["dim"] == case.deficit
    missing = sorted(set(range(case.cols)) - set(int(c) for c in want["pivcols"]))
    assert len(missing) == case.deficit
    if case.deficit:
        g = int(name[-1])
        assert 64 * (G * case.block + g) <= missing[0] < 64 * (G * case.block + g + 1)


@pytest.mark.parametrize("name", DC.NAMES)
def test_model_against_independent_ranks(name):
    """What `simulate` says a panel found, from ranks alone: the main chunk's pivots number the rank of its words, the panel is
    complete exactly when the two chunks together have rank 64, a taken block used exactly its 256 home rows, and new_first is the
    first alive row that was not used."""
    case = DC.cases()[name]
    trace = case.model(True)["trace"]
    dead = set()
    for r in trace:
        b = r["block"]
        for p in r["panels"]:
            g = p["g"]
            if p["why"] == "gate":
                assert p["dense"] < DC.DENSE_WORDS
                continue
            assert p["dense"] >= DC.DENSE_WORDS and len(p["main_pivots"]) == rank_of(p["main"])
            if p["why"] == "few":
                assert rank_of(p["main"]) < 64 - DC.FEW_MISSING
                continue
            assert rank_of(p["main"]) >= 64 - DC.FEW_MISSING
            both = rank_of(p["main"] + p["next"])
            assert (p["why"] is None) == (both == 64) and len(p["main_pivots"]) + len(p["absorbed"]) == both
            if p["why"] is None:
                cand = r["candidates"]
                for col, comb in p["comb"].items():       # a combination names home rows of the block, out of the panel's two chunks
                    assert all(case.rows[cand[s]] is not None and case.rows[cand[s]][0] == b and s // 64 in (g, g + 1) for s in DC.bits(comb))
        if r["taken"]:
            home = {i for i, row in enumerate(case.rows) if row is not None and row[0] == b}
            assert set(r["used"]) == home and len(r["used"]) == 64 * G
            assert r["candidates"] == [i for i in range(r["first"], len(case.rows)) if i not in dead][:FAST_NC]
            assert r["candidates"][-1] - r["first"] < DC.REACH
            dead |= home
            assert r["new_first"] == min(i for i in r["candidates"] if i not in home)
        else:
            dead |= {i for i, row in enumerate(case.rows) if row is not None and row[0] == b}


def test_pivot_rows_are_the_reduced_echelon_form():
    """The model's arithmetic (gj_columns, find_absorb's reduced bit, the narrow step it carries from panel to panel, combinations x
    sources) against a direct computation on the rows as they were WRITTEN: the XOR of the written rows a pivot's combination names,
    cleared left of its panel by the earlier panels' pivot rows, must be the unit bit in the panel's word and, right of it, the pivot
    row the model formed from the candidates' narrowed words."""
    for name in ("miss_8_g0", "miss_8_g1", "miss_7_g2", "miss_8_g3", "chain", "absorb_last_lane_g0", "dense_carry_48", "plain",
                 "anchor_zero_row", "leftover_mid"):
        case = DC.cases()[name]
        r = case.model(True)["trace"][max(case.block, 0) if name != "anchor_zero_row" else 6]
        assert r["taken"]
        cand, fwd = r["candidates"], {}
        for p in r["panels"]:
            g = p["g"]
            for col, comb in p["comb"].items():
                v = [0] * G
                for s in DC.bits(comb):
                    v = [a ^ b for a, b in zip(v, case.rows[cand[s]][1])]
                for e in range(g):
                    for q in DC.bits(v[e]):
                        v = [a ^ b for a, b in zip(v, fwd[(e, q)])]
                assert v == [0] * g + [1 << col] + p["pivot_rows"][col][g + 1:], (name, g, col)
            fwd.update({(g, col): [0] * g + [1 << col] + words[g + 1:] for col, words in p["pivot_rows"].items()})
        assert len(fwd) == 64 * G


def test_twins_differ_in_the_one_property_they_are_named_for():
    C = DC.cases()
    for taken, given_up in DC.TWINS:
        a, b = C[taken], C[given_up]
        ta, tb = a.model(True)["trace"], b.model(True)["trace"]
        assert a.cols == b.cols and a.expect["fast_blocks"][1] == b.expect["fast_blocks"][1] + 1, (taken, given_up)
        blk = next(i for i, (x, y) in enumerate(zip(ta, tb)) if x["taken"] != y["taken"])
        assert ta[blk]["taken"] and not tb[blk]["taken"] and all(x["taken"] and y["taken"] for x, y in zip(ta[:blk], tb[:blk]))
    for g in range(G):          # nine zero candidates against eight, the same eight among them; the same completing lanes + 1
        pa, pb = C[f"miss_8_g{g}"].model()["trace"][DC.LATE]["panels"][g], C[f"miss_9_g{g}"].model()["trace"][DC.LATE]["panels"][g]
        za, zb = {l for l, w in enumerate(pa["main"]) if not w}, {l for l, w in enumerate(pb["main"]) if not w}
        assert len(za) == 8 and len(zb) == 9 and za < zb and len(pa["main_pivots"]) == 56 and len(pb["main_pivots"]) == 55
    for g in (0, 2):            # the same main chunk and the same completing word, as lane 63 of chunk g + 1 or as candidate 0 of chunk g + 2
        a, b = C[f"absorb_last_lane_g{g}"], C[f"absorb_incomplete_g{g}"]
        pa, pb = a.model()["trace"][DC.LATE]["panels"][g], b.model()["trace"][DC.LATE]["panels"][g]
        assert pa["main"] == pb["main"]
        far = b.plans[DC.LATE]["comp"][g]
        assert far == [64 * (g + 2)] and a.plans[DC.LATE]["comp"][g] == [64 * (g + 1) + 63]
        wb = b.rows[2048 + far[0]][1][g]
        assert rank_of(pb["main"] + [wb]) == 64 and rank_of(pa["main"] + [pa["next"][63]]) == 64
    for x, y, g in (("dense_48", "dense_47", 0), ("dense_13", "dense_12", 2), ("dense_carry_48", "dense_carry_47", 1)):
        pa, pb = C[x].model()["trace"][DC.LATE]["panels"][g], C[y].model()["trace"][DC.LATE]["panels"][g]
        diff = [l for l in range(64) if pa["main"][l] != pb["main"][l]]
        assert len(diff) == 1 and (pa["dense"], pb["dense"]) == (48, 47)
        wa, wb = pa["main"][diff[0]], pb["main"][diff[0]]
        assert DC.popcount(wb) == 12 and DC.popcount(wa) > 12
        if x == "dense_13":
            assert DC.popcount(wa) == 13 and wb == wa & (wa - 1)
    a, b = C["anchor_edge_2047"], C["anchor_edge_2048"]
    assert len(a.rows) == len(b.rows) and a.rows.index(None) == 320 and b.rows.index(None) == 319
    assert len(C["tail_320"].rows) == len(C["tail_319"].rows) + 1 == 2560 + 64


def test_the_gang_cases_share_a_shape():
    shapes = {(len(DC.cases()[n].rows), DC.cases()[n].cols) for n in ("leftover_low", "anchor_edge_2048", "anchor_zero_row")}
    assert shapes == {(2560 + 1 + DC.TAIL, 2560)}
