"""k_block_sparse branch by branch: the built systems of tests/sparse_cases.py through hip.solve_words as shipped.  Per case and mode the
oracle's answers (status, rank, pivots, origin, basis and its order) AND the counters that say which branch ran
(gf2bv_stats::sparse_*: pool size, selection outcome per panel, give-ups by reason, probed or met after submission) -- exact where the construction
fixes them.  The same systems with the search switched off (all its counters zero) and with events instead of flags; three of them
through a kept factorization, which replays slot_row / comb / src_mult as this kernel wrote them."""
import functools
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import sparse_cases as SC
from tests.test_gpu_rhs import _make_rhs, _rhs_words, _with_rhs, assert_same_oracle, assert_same_solution

pytestmark = pytest.mark.gpu

COUNTERS = ("sparse_blocks", "sparse_panels_first64", "sparse_panels_absorb", "sparse_panels_rounds", "sparse_giveups",
            "sparse_giveup_why", "sparse_nz_max")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _oracle(name: str, mode: int) -> dict:
    case = SC.cases()[name]
    aug = case.aug()
    return O.solve_words(aug, aug.shape[0], case.cols, mode)


def _line(name, mode, leg, st):
    print(f"[sparse] {name} mode {mode} {leg}: rows {st['rows']} blocks {st['sparse_blocks']} first64 {st['sparse_panels_first64']} "
          f"absorb {st['sparse_panels_absorb']} rounds {st['sparse_panels_rounds']} giveups {st['sparse_giveups']} "
          f"why {st['sparse_giveup_why']} nz_max {st['sparse_nz_max']} fast_blocks {st['fast_blocks']}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SC.NAMES)
def test_case_answers_and_branches(monkeypatch, name, mode):
    case = SC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    want = _oracle(name, mode)
    for leg, env in (("shipped", {}), ("events", {"GF2BV_FLAG_SYNC": "0"}), ("switched off", {"GF2BV_SPARSE_FAST": "0"})):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = hip.solve_words(aug, rows, cols, mode)
        st = got.stats
        _line(name, mode, leg, st)
        assert_same_oracle(got, want, mode)
        assert st["handover_retries"] == 0 and st["small_path"] == 0
        # every panel was published by the general search or belongs to a block a one-launch search took (which adds nothing to general_*)
        assert st["general_unit0"] + st["general_adopted"] + st["general_merged"] + SC.G * st["fast_blocks"] == cols // 64
        if leg == "switched off":
            assert all(st[k] == 0 or st[k] == [0] * len(st[k]) for k in COUNTERS), st
        else:
            assert SC.holds(st, case.expect) == []
            assert st["sparse_giveup_why"][0] == 0 and st["sparse_giveup_why"][3] == 0
            assert st["sparse_giveups"] == sum(st["sparse_giveup_why"]) <= SC.STRIKES
            assert st["sparse_panels_first64"] + st["sparse_panels_absorb"] + st["sparse_panels_rounds"] == SC.G * sum(st["sparse_blocks"])
            assert st["fast_blocks"] >= sum(st["sparse_blocks"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["absorb_511", "escalate_middle", "alive_top"])
def test_kept_factorization_replays_what_the_search_wrote(name, mode):
    """hip.factor_words, then four right-hand sides (two planted, two random): result for result what solve_rhs_words gives, and for a
    planted and a random one the oracle's answer.  A handle carries no stats: that its factorization went through k_block_sparse rests
    on factor_words and solve_words sharing enqueue_forward, so the solve of the same matrix is asked for its counters first."""
    case = SC.cases()[name]
    aug = case.aug()
    rows, cols = aug.shape[0], case.cols
    rng = random.Random(len(name) * 1000 + mode)
    rhs_bits = _make_rhs(rng, aug, rows, cols, 4)
    rhs = _rhs_words(rhs_bits)
    want = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    assert SC.holds(hip.solve_words(aug, rows, cols, mode).stats, case.expect) == []
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
