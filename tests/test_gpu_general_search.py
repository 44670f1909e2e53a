"""The general panel search (search_panel and the narrow half of k_panel_step) branch by branch: the built systems of
tests/general_cases.py through hip.solve_words with the one-launch searches switched off (GF2BV_FAST=0, GF2BV_SPARSE_FAST=0: every panel
goes through search_panel) -- with flags, with events (GF2BV_FLAG_SYNC=0) and plain (GF2BV_PLAIN=1) -- and as shipped.  Per case, mode
and leg the oracle's answers (status, rank, pivots, origin, basis and its order) AND gf2bv_stats::general_*, which say how each panel
was published: exact in every leg -- as shipped against the model with the dense block search in front of the general steps, which
also gives `fast_blocks`: which blocks that search is asked for is decided by `st->fast_off`, which search_panel's last panel of a
block leaves (the twins fast_off_cleared / fast_off_stands).  Three systems as a gang with counters per member, one under a forced two-level plan, three through a kept
factorization, which replays slot_row / comb / src_mult as a merge or a group record wrote them."""
import functools
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import general_cases as GC
from tests.test_gpu_parity import assert_same
from tests.test_gpu_rhs import _make_rhs, _rhs_words, _with_rhs, assert_same_solution

pytestmark = pytest.mark.gpu

OFF = {"GF2BV_FAST": "0", "GF2BV_SPARSE_FAST": "0"}
LEGS = (("general", OFF), ("general, events", {**OFF, "GF2BV_FLAG_SYNC": "0"}), ("general, plain", {**OFF, "GF2BV_PLAIN": "1"}), ("shipped", {}))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _oracle(name: str, mode: int) -> dict:
    case = GC.cases()[name]
    aug = case.aug()
    return O.solve_words(aug, aug.shape[0], case.cols, mode)


def _line(name, mode, leg, st):
    print(f"[general] {name} mode {mode} {leg}: rows {st['rows']} " + " ".join(f"{k[8:]} {st[k]}" for k in GC.COUNTERS)
          + f" | fast_blocks {st['fast_blocks']} sparse {st['sparse_blocks']} handovers {st['search_handovers']}")


def _accounted(st: dict, cols: int) -> None:
    """what holds whoever took the blocks: every panel was published by search_panel or belongs to a block of a one-launch search"""
    assert st["general_unit0"] + st["general_adopted"] + st["general_merged"] + GC.G * st["fast_blocks"] == (cols + 63) // 64
    assert st["general_two_level"] <= st["general_wide"] and st["general_gj_kept"] + st["general_gj_redone"] <= st["general_unit0"] + st["general_adopted"]
    assert st["general_group_adopted"] + st["general_group_merged"] >= 2 * st["general_two_level"]
    assert st["handover_retries"] == 0 and st["small_path"] == 0


def _shipped(st: dict, case) -> None:
    """as shipped these systems (fewer than 8 blocks) get k_block_fast with the general steps behind it for every full block: the model
    with the dense search in front says which blocks it takes -- `st->fast_off`, left by each block's last general panel, decides
    whether it is asked at all -- and gives the general_* counts of the blocks it leaves"""
    want = case.shipped()
    assert st["fast_blocks"] == want["fast_blocks"] and st["sparse_blocks"] == [0, 0, 0]
    assert {k: st[k] for k in GC.COUNTERS} == {k: want[k] for k in GC.COUNTERS}


def _exact(st: dict, case) -> None:
    assert GC.holds(st, case.expect) == []
    assert st["fast_blocks"] == 0 and st["sparse_blocks"] == [0, 0, 0] and st["small_path"] == 0 and st["handover_retries"] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", GC.NAMES)
def test_case_answers_and_branches(monkeypatch, name, mode):
    case = GC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    want = _oracle(name, mode)
    for leg, env in LEGS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = hip.solve_words(aug, rows, cols, mode)
        st = got.stats
        _line(name, mode, leg, st)
        assert_same(got, want, mode)
        _accounted(st, cols)
        if env:
            _exact(st, case)
        else:
            _shipped(st, case)


GANG = ("merge_carry_40_40_40", "adopt_unit3", "gj_55_redone")          # one shape (2048 x 512): a merge with a carry, an adoption, a redone first chunk


@pytest.mark.parametrize("mode", [0, 1])
def test_a_gang_of_three(monkeypatch, mode):
    """three systems of one shape in lock-step, the general steps for every member (blockIdx.y picks the system and its SolveState):
    each member against the oracle and against ITS row of the table; then as shipped (k_block_fast in front of the general steps)"""
    cs = [GC.cases()[n] for n in GANG]
    augs = np.stack([c.aug() for c in cs])
    monkeypatch.setenv("GF2BV_GANG", "3")
    for leg, env in (("gang, general", OFF), ("gang, shipped", {})):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = hip.solve_batch_words(augs, augs.shape[1], cs[0].cols, mode)
        assert len(got) == 3
        for name, case, g in zip(GANG, cs, got):
            _line(name, mode, leg, g.stats)
            assert_same(g, _oracle(name, mode), mode)
            assert g.stats["gang_systems"] == 3 and g.stats["sparse_blocks"] == [0, 0, 0]
            _accounted(g.stats, case.cols)
            if env:
                _exact(g.stats, case)
            else:
                _shipped(g.stats, case)


@pytest.mark.parametrize("mode", [0, 1])
def test_forced_two_level_plan(monkeypatch, mode):
    """outer panels of two blocks over the 16 panels of dead_blocks_1024: the panel steps are the one-level plan's, and so are the counts"""
    name = "dead_blocks_1024"
    case = GC.cases()[name]
    aug = case.aug()
    for k, v in {**OFF, "GF2BV_TWO_LEVEL": "2"}.items():
        monkeypatch.setenv(k, v)
    got = hip.solve_words(aug, aug.shape[0], case.cols, mode)
    _line(name, mode, "two-level", got.stats)
    assert_same(got, _oracle(name, mode), mode)
    assert got.stats["outer_blocks"] > 0
    _accounted(got.stats, case.cols)
    _exact(got.stats, case)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["merge_carry_40_40_40", "two_level_20_units", "deficient_30_then_empty"])
def test_kept_factorization_replays_what_the_search_wrote(monkeypatch, name, mode):
    """hip.factor_words through the general steps, then four right-hand sides (two planted, two random): result for result what
    solve_rhs_words gives, and for a planted and a random one the oracle's answer.  A handle carries no stats: that its factorization
    took the merge / the group records rests on factor_words and solve_words sharing enqueue_forward, so the solve of the same matrix
    is asked for its counters first."""
    case = GC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    for k, v in OFF.items():
        monkeypatch.setenv(k, v)
    rng = random.Random(len(name) * 1000 + mode)
    rhs_bits = _make_rhs(rng, aug, rows, cols, 4)
    rhs = _rhs_words(rhs_bits)
    want = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    _exact(hip.solve_words(aug, rows, cols, mode).stats, case)
    with hip.factor_words(aug, rows, cols, mode) as f:
        assert f.rank == _oracle(name, mode)["rank"]
        got = f.solve(rhs)
        again = f.solve(rhs[::-1].copy())[::-1]
    assert len(got) == len(want) == 4
    for j in range(4):
        assert_same_solution(got[j], want[j], mode)
        assert_same_solution(again[j], want[j], mode)
        if j < 2:
            assert_same(got[j], O.solve_words(_with_rhs(aug, cols, rhs_bits[j]), rows, cols, mode), mode)
    assert got[0].status == 0 and got[2].status == 0                      # the planted ones are consistent
