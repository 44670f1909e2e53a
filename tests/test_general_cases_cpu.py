"""The built systems of tests/general_cases.py, checked without a GPU: a case whose predicate does not hold fails HERE, not on the GPU
by an unexplained counter.  Per case: the model arrives at every expected counter and at the claim the case is named for; the model's
ranks and pivot rows against an independent rank computation on the rows as written; the oracle's rank, status and dimension.  The
twins differ in the one counter they are named for, and each of the four mutants moves a prediction."""
import time

import pytest

from oracle import gf2_oracle as O
from tests import general_cases as GC


@pytest.mark.parametrize("name", GC.NAMES)
def test_case_is_what_it_claims(name):
    case = GC.cases()[name]
    got = case.model()
    assert GC.holds(got, case.expect) == []
    assert set(case.expect) == set(GC.COUNTERS) and all(op == "==" for op, _ in case.expect.values()), "every count is exact"
    case.claim(got)
    npanels = (case.cols + 63) // 64
    assert got["general_unit0"] + got["general_adopted"] + got["general_merged"] == npanels == len(got["trace"])
    assert got["general_group_adopted"] + got["general_group_merged"] == sum(len(p["groups"]) for p in got["trace"])
    assert got["units"] == GC.units_of(len(case.rows)) and len(case.rows) >= case.cols
    # not the one-workgroup path (small_eligible): more than 4096 rows, or (rows + 512) x (words | 1) beyond 18432 words of LDS
    wt = (case.cols + 1 + 63) // 64
    assert len(case.rows) > 4096 or (len(case.rows) + 512) * (wt | 1) > 18432


@pytest.mark.parametrize("name", GC.NAMES)
def test_model_ranks_and_pivot_rows(name):
    """per panel: the model's pivot rows are rows written for that panel, alive, as many as the panel's rank over ALL its rows (computed
    apart from the model, on the rows as written), and independent"""
    case = GC.cases()[name]
    got = case.model()
    seen = set()
    for p in got["trace"]:
        j = p["j"]
        words = [case.rows[r][1] for r in p["srow"]]
        assert all(case.rows[r] is not None and case.rows[r][0] == j for r in p["srow"])
        assert p["p"] == len(set(p["srow"])) == GC.rank_of(words) == case.panel_rank(j)
        assert not seen & set(p["srow"])
        seen |= set(p["srow"])
        # the bound is a bound: no alive row lies below it
        assert all(r in seen for r in range(p["new_first"])), (j, p["new_first"])
    assert got["rank"] == case.rank()


@pytest.mark.parametrize("name", GC.NAMES)
def test_the_oracle_solves_it(name):
    case = GC.cases()[name]
    aug = case.aug()
    t0 = time.perf_counter()
    want = O.solve_words(aug, aug.shape[0], case.cols, 1)
    took = time.perf_counter() - t0
    assert want["status"] == 0 and want["rank"] == case.rank() and want["dim"] == case.cols - want["rank"]
    assert took < 5.0, f"{took:.1f} s on the CPU oracle: thin the columns"


def test_names_and_table_agree():
    assert list(GC.cases()) == GC.NAMES
    assert [c.name for c in GC.cases().values() if c.tall] == ["tall_256_units", "tall_plain"]


@pytest.mark.parametrize("name", GC.NAMES)
def test_shipped_model_accounts_for_every_panel(name):
    """the model with the dense block search in front: a taken block is four full panels and adds nothing to general_*; `fast_off`
    before a block is what the block before left"""
    case = GC.cases()[name]
    got = case.shipped()
    npanels = (case.cols + 63) // 64
    assert got["general_unit0"] + got["general_adopted"] + got["general_merged"] + GC.G * got["fast_blocks"] == npanels
    assert got["rank"] == case.rank() and len(got["blocks"]) == (case.cols // (64 * GC.G) if len(case.rows) >= 320 else 0)
    for b in got["blocks"]:
        assert b["taken"] == (b["why"] is None) and (b["why"] == "fast_off") == bool(b["fast_off_before"])


def test_fast_off_twins():
    """st->fast_off from the last panel of a block: both twins' block 0 goes to the general steps (a gate miss in panel 2); it ends easy
    and full in one and with a merged panel of 63 pivots in the other, and only then is block 1 withheld from the dense search -- which
    would have taken it: with the flag ignored the model takes three blocks in both"""
    C = GC.cases()
    a, b = C["fast_off_cleared"].shipped(), C["fast_off_stands"].shipped()
    assert [(x["taken"], x["why"]) for x in a["blocks"]] == [(False, "gate 2"), (True, None), (True, None), (True, None)]
    assert [(x["taken"], x["why"]) for x in b["blocks"]] == [(False, "gate 2"), (False, "fast_off"), (True, None), (True, None)]
    assert (a["fast_blocks"], b["fast_blocks"]) == (3, 2)
    assert a["trace"][3]["fast_off"] == 0 and b["trace"][3]["fast_off"] == 1 and b["trace"][7]["fast_off"] == 0
    assert GC.simulate(C["fast_off_stands"], fast=True, heed_fast_off=False)["fast_blocks"] == 3
    # the other case in which the flag withholds a block: tall_256_units, whose panel 3 is merged
    t = C["tall_256_units"].shipped()
    assert [x["why"] for x in t["blocks"]] == ["incomplete 0", "fast_off"] and t["trace"][3]["fast_off"] == 1


def test_twins_differ_in_what_they_are_named_for():
    C = GC.cases()
    for a, b, differ in GC.TWINS:
        ma, mb = C[a].model(), C[b].model()
        assert {k for k in GC.COUNTERS if ma[k] != mb[k]} == differ, (a, b)
        assert [p["srow"] for p in ma["trace"][:7]] == [p["srow"] for p in mb["trace"][:7]] and ma["rank"] == mb["rank"]


@pytest.mark.parametrize("mutant", list(GC.MUTANTS))
def test_each_mutant_moves_a_prediction(mutant):
    """the model with the mutant's rule predicts another rank or other counters for the case that is there to catch it"""
    kw, name = GC.MUTANTS[mutant]
    case = GC.cases()[name]
    base, mut = case.model(), GC.simulate(case, **kw)
    assert any(base[k] != mut[k] for k in GC.COUNTERS + ("rank",)), mutant
    if mutant == "no carry":
        assert mut["rank"] == base["rank"] - 16          # the 16 carried rows are lost: a wrong rank, not only a wrong count
