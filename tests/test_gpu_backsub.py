"""The back-substitution behind every solving entry (gf2_solver.hip: BackSub, backsub_begin, enqueue_backward_parity, enqueue_backward).
One parity chain serves a single system and a whole gang (blockIdx.y = system); right-hand sides go through it in groups of GF2_BSV = 8,
more than GF2_BS_MAXRHS = 64 of them through the Y sweeps; and a Solver that is asked for a second back-substitution -- a kept
factorization, a slab handle solved twice -- first gives back what the first one took.  Every result is compared bit for bit."""
import functools
import gc
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import hip, slab
from oracle import gf2_oracle as O
from tests import thread_jobs as J
from tests import threads as T
from tests.systems import random_system

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


# -- the gang's chain against the single chain --------------------------------------------------------------------------------------------
# rows x cols: one panel and one word; exactly one group of 16 panels; 18 panels = a full and a ragged group; rank below cols (in mode 1
# a kernel of 200 vectors and more, which the views send through the Y sweeps).  The entries refuse rows < cols ("try pad with zeros"), so
# the 900 equations in 1100 unknowns are passed as the library asks: followed by 200 zero rows.
GANG_SHAPES = {"70x63": (70, 63, 0), "1100x1024": (1100, 1024, 0), "1200x1100": (1200, 1100, 0), "900x1100": (1100, 1100, 200)}


@functools.lru_cache(maxsize=None)
def _batch(rows: int, cols: int, zero_rows: int):
    """five systems of mixed rank, the fourth inconsistent (its last equation is its first with the other constant), and the oracle's
    answers in both modes"""
    rng = random.Random(rows * 10007 + cols)
    live = rows - zero_rows
    full = min(live, cols)
    systems = [random_system(rng, rows, cols, .5, cap, True, zero_rows) for cap in (None, full - 1, full - 5, None, full - 40)]
    systems[3][live - 1] = systems[3][0] ^ 1
    augs = np.stack([O.eqs_to_aug(e, cols) for e in systems])
    want = {mode: tuple(T.oracle_key(O.solve_words(a, rows, cols, mode), mode) for a in augs) for mode in (0, 1)}
    assert [w[0] for w in want[0]] == [0, 0, 0, 1, 0]
    return augs, want


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", list(GANG_SHAPES))
def test_gang_chain_equals_one_chain_per_system(monkeypatch, shape, mode):
    """5 systems = gangs of 3 + 2: solve_batch_words as shipped (one chain per gang), with GF2BV_GANG_BS=0 (one chain per view) and a loop
    of solve_words on the blocked path (the single chain) agree with each other and with the oracle"""
    rows, cols, zero_rows = GANG_SHAPES[shape]
    augs, want = _batch(rows, cols, zero_rows)
    gang = hip.solve_batch_words(augs, rows, cols, mode)
    assert [g.stats["gang_systems"] for g in gang] == [3, 3, 3, 2, 2]
    monkeypatch.setenv("GF2BV_GANG_BS", "0")
    per_view = hip.solve_batch_words(augs, rows, cols, mode)
    monkeypatch.delenv("GF2BV_GANG_BS")
    monkeypatch.setenv("GF2BV_SMALL", "0")                 # (70 x 63 would take the one-launch small solve, which has no chain)
    single = [hip.solve_words(a, rows, cols, mode) for a in augs]
    assert not any(s.stats["small_path"] for s in single)
    for name, got in (("gang", gang), ("per view", per_view), ("single", single)):
        assert J.solve_many(got, mode) == want[mode], name


# -- groups of right-hand sides ---------------------------------------------------------------------------------------------------------------
RHS_SHAPES = [(70, 63), (1200, 1100)]
NRHS = (1, 8, 9, 64, 65)                                   # either side of GF2_BSV = 8 and of GF2_BS_MAXRHS = 64 (the Y sweeps take over)


@functools.lru_cache(maxsize=None)
def _rhs_case(rows: int, cols: int):
    """a matrix five short of full rank, 65 right-hand sides (planted and random in turn), and what solve_words -- switches unset -- returns
    for each augmented system in both modes"""
    rng = random.Random(rows * 31 + cols)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cols - 5, True, 0), cols)
    bits = J.make_rhs(rng, aug, rows, cols, max(NRHS))
    want = {mode: tuple(T.solution_key(hip.solve_words(J.with_rhs(aug, cols, b), rows, cols, mode), mode) for b in bits) for mode in (0, 1)}
    assert {w[0] for w in want[0]} == {0, 1}                 # consistent and inconsistent ones
    return aug, bits, want


@pytest.mark.parametrize("inv", [None, "0", "1"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", RHS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_groups_of_right_hand_sides(monkeypatch, shape, mode, inv):
    """solve_rhs_words with the first nrhs of the 65 right-hand sides: result j is what solve_words returns for system j alone, with
    GF2BV_BS_INV unset, 0 (k_bs_near) and 1 (k_bs_inv + k_bs_near2)"""
    rows, cols = shape
    aug, bits, want = _rhs_case(rows, cols)                # (the reference is taken before the switch is set)
    if inv is not None:
        monkeypatch.setenv("GF2BV_BS_INV", inv)
    for nrhs in NRHS:
        got = hip.solve_rhs_words(aug, rows, cols, J.rhs_words(bits[:nrhs]), mode)
        assert J.solve_many(got, mode) == want[mode][:nrhs], nrhs


# -- repeated back-substitutions on one Solver give back what they take -------------------------------------------------------------------------
def in_use(collect: bool = False) -> dict:
    if collect:
        gc.collect()
    return hip.pool_in_use(0)


def test_kept_handle_is_balanced_after_every_back_substitution():
    """mode 1: a solve pass's back-substitution, and the kernel basis's at factor and append time, leave the pool's numbers where the
    open handle put them; close returns the rest"""
    rows, cols = 300, 200
    rng = random.Random(61)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, 150, True, 0), cols)
    base = in_use(collect=True)
    f = hip.factor_words(aug, rows, cols, 1)
    f.append_words(np.zeros((2, aug.shape[1]), dtype=np.uint64))       # (the first append outgrows the factored rows: the handle takes a buffer more)
    assert f.rank == 150
    held = in_use()
    for nrhs in (1, 9, 65):
        bits = J.make_rhs(rng, aug, rows, cols, nrhs)
        padded = np.concatenate([bits, np.zeros((nrhs, 2), dtype=np.uint8)], axis=1)          # (the two appended equations are 0 = 0)
        got = J.solve_many(f.solve(J.rhs_words(padded)), 1)
        assert got == J.oracle_rhs(aug, rows, cols, bits, 1), nrhs
        del got
        assert in_use() == held, nrhs
    more = O.eqs_to_aug(random_system(rng, 3, cols, .5, None, True, 0), cols)
    f.append_words(more)
    assert f.rank == 153 and in_use() == held
    all_rows = np.concatenate([aug, more])
    bits = J.make_rhs(rng, all_rows, rows + 3, cols, 3)
    with_zero_rows = np.concatenate([bits[:, :rows], np.zeros((3, 2), dtype=np.uint8), bits[:, rows:]], axis=1)
    assert J.solve_many(f.solve(J.rhs_words(with_zero_rows)), 1) == J.oracle_rhs(all_rows, rows + 3, cols, bits, 1)
    assert in_use() == held
    f.close()
    del f
    assert in_use(collect=True) == base


def test_slab_handle_solved_twice():
    """gf2bv_slab_solve twice on one handle (world size 1): the second back-substitution first returns the first one's buffers and takes no
    second export event, so the answers are equal and close() leaves the pool's numbers where they were.  (Before BackSub the second
    call overwrote the pointers: three buffers and an event stayed handed out for ever.)"""
    rows, cols = 1200, 1100
    eqs = random_system(random.Random(62), rows, cols, .5, cols - 5, True, 0)
    stride = hip.padded_stride(cols)
    aug = torch.from_numpy(O.eqs_to_aug(eqs, cols, stride).view(np.int64).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    base = in_use(collect=True)
    eng = slab.HipSlabEngine(aug.data_ptr(), rows, cols, stride, 1, 0, 0)
    try:
        for b in range(eng.nblocks):
            eng.apply(b, eng.factor(b))
        eng.finish_local()
        first, second = eng.solve(), eng.solve()
    finally:
        eng.close()
    after = in_use()
    want = T.oracle_key(O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, 0), 0)
    assert T.solution_key(first, 0) == want
    assert T.solution_key(second, 0) == want
    assert after == base
