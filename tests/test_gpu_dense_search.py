"""The one-launch dense block search (block_fast_body) branch by branch: the built systems of tests/dense_cases.py through
hip.solve_words in every form the search runs in -- the fused launch as shipped, k_block_fast + k_narrow_all (GF2BV_FUSED_NARROW=0),
k_block_fast with the general steps behind it (GF2BV_OPTIMISTIC=0, GF2BV_PLAIN=1), events instead of flags, and switched off.  Per case,
mode and leg the oracle's answers (status, rank, pivots, origin, basis and its order) AND gf2bv_stats::fast_blocks, which says whether
the branch the case was built for ran: exact wherever tests/dense_cases.py's model fixes it.  Three of the systems as a gang, three under
a forced two-level plan (a give-up inside an outer panel), three through a kept factorization, which replays slot_row / comb / src_mult
as this kernel wrote them."""
import functools
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import dense_cases as DC
from tests.test_gpu_rhs import _make_rhs, _rhs_words, _with_rhs, assert_same_oracle, assert_same_solution

pytestmark = pytest.mark.gpu

LEGS = (("shipped", {}, True), ("two launches", {"GF2BV_FUSED_NARROW": "0"}, True), ("not optimistic", {"GF2BV_OPTIMISTIC": "0"}, False),
        ("events", {"GF2BV_FLAG_SYNC": "0"}, True), ("plain", {"GF2BV_PLAIN": "1"}, False), ("switched off", {"GF2BV_FAST": "0"}, None))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _oracle(name: str, mode: int) -> dict:
    case = DC.cases()[name]
    aug = case.aug()
    return O.solve_words(aug, aug.shape[0], case.cols, mode)


def _line(name, mode, leg, st, want):
    print(f"[dense] {name} mode {mode} {leg}: rows {st['rows']} fast_blocks {st['fast_blocks']} want {want} sparse {st['sparse_blocks']} "
          f"outer_blocks {st['outer_blocks']} handover_retries {st['handover_retries']} small_path {st['small_path']}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", DC.NAMES)
def test_case_answers_and_branches(monkeypatch, name, mode):
    case = DC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    want = _oracle(name, mode)
    for leg, env, optimistic in LEGS:
        with monkeypatch.context() as m:
            for k, v in {**case.env, **env}.items():
                m.setenv(k, v)
            got = hip.solve_words(aug, rows, cols, mode)
        st = got.stats
        expect = {"fast_blocks": DC.eq(0)} if optimistic is None else {"fast_blocks": case.model(optimistic)["fast_blocks"]}
        _line(name, mode, leg, st, expect["fast_blocks"])
        assert_same_oracle(got, want, mode)
        assert st["handover_retries"] == 0 and st["small_path"] == 0
        assert st["sparse_blocks"] == [0, 0, 0]
        # every panel was published by the general search or belongs to a block the dense search took (which adds nothing to general_*)
        assert st["general_unit0"] + st["general_adopted"] + st["general_merged"] + DC.G * st["fast_blocks"] == (cols + 63) // 64
        assert DC.holds(st, expect) == [], leg
        if optimistic is not None:
            assert expect == case.expect


GANG = ("leftover_low", "anchor_edge_2048", "anchor_zero_row")      # one shape: every block taken, a give-up out of reach, the anchored bound


@pytest.mark.parametrize("mode", [0, 1])
def test_a_gang_of_three(monkeypatch, mode):
    """three systems of one shape in lock-step (a gang never takes the optimistic enqueue: k_block_fast with the general steps behind
    it, one workgroup per system); every member against the oracle, and its own count"""
    cs = [DC.cases()[n] for n in GANG]
    augs = np.stack([c.aug() for c in cs])
    monkeypatch.setenv("GF2BV_GANG", "3")
    got = hip.solve_batch_words(augs, augs.shape[1], cs[0].cols, mode)
    assert len(got) == 3
    for name, case, g in zip(GANG, cs, got):
        _line(name, mode, "gang", g.stats, case.model(False)["fast_blocks"])
        assert_same_oracle(g, _oracle(name, mode), mode)
        assert g.stats["gang_systems"] == 3 and g.stats["sparse_blocks"] == [0, 0, 0]
        assert DC.holds(g.stats, {"fast_blocks": case.model(False)["fast_blocks"]}) == []


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["miss_8_g1", "giveup_panel2", "anchor_zero_row"])
def test_forced_two_level_plan(monkeypatch, name, mode):
    """outer panels of two blocks: the give-ups fall inside an outer panel (recover cuts the plan back to what has run)"""
    case = DC.cases()[name]
    aug = case.aug()
    monkeypatch.setenv("GF2BV_TWO_LEVEL", "2")
    got = hip.solve_words(aug, aug.shape[0], case.cols, mode)
    _line(name, mode, "two-level", got.stats, case.expect["fast_blocks"])
    assert_same_oracle(got, _oracle(name, mode), mode)
    assert got.stats["outer_blocks"] > 0 and got.stats["sparse_blocks"] == [0, 0, 0] and got.stats["handover_retries"] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["miss_8_g0", "chain", "giveup_then_back"])
def test_kept_factorization_replays_what_the_search_wrote(name, mode):
    """hip.factor_words, then four right-hand sides (two planted, two random): result for result what solve_rhs_words gives, and for a
    planted and a random one the oracle's answer.  A handle carries no stats: that its factorization went through the search rests on
    factor_words and solve_words sharing enqueue_forward, so the solve of the same matrix is asked for its counter first."""
    case = DC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    rng = random.Random(len(name) * 1000 + mode)
    rhs_bits = _make_rhs(rng, aug, rows, cols, 4)
    rhs = _rhs_words(rhs_bits)
    want = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    assert DC.holds(hip.solve_words(aug, rows, cols, mode).stats, case.expect) == []
    with hip.factor_words(aug, rows, cols, mode) as f:
        assert f.rank == _oracle(name, mode)["rank"]
        got = f.solve(rhs)
        again = f.solve(rhs[::-1].copy())[::-1]
    assert len(got) == len(want) == 4
    for j in range(4):
        assert_same_solution(got[j], want[j], mode)
        assert_same_solution(again[j], want[j], mode)
        if j < 2:
            assert_same_oracle(got[j], O.solve_words(_with_rhs(aug, cols, rhs_bits[j]), rows, cols, mode), mode)
    assert got[0].status == 0 and got[2].status == 0                      # the planted ones are consistent
