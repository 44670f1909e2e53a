"""The unrolling entries (gf2bv_compose_unroll_*) and gf2bv_amd.unroll on the GPU, bit for bit against the host twin of
tests/unroll_terms.py, which substitutes one time step after the other: every boundary of the doubling schedule with its product
count, start and step, blocks that cross a row group and two slices, garbage and padding, answers that owe nothing to this code (an
LFSR's register and period, xoshiro256's steps), the rows of host stepping, the device entry and its stream ordering, two threads,
and the example."""
import importlib.util
import os
import random
import sys
import threading

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedBitVec, PackedLinearSystem, hip, unroll
from tests import compose_terms as T
from tests import unroll_terms as U
from tests.harness_models import FibonacciLFSR, GaloisLFSR, Xoshiro256starstar
from tests.test_compose_cpu import xoshiro_step_map
from tests.test_gpu_compose import _delayed_copy, _dev, _even, _host, cut, cycles, dense, invertible_affine, stream  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPE = hip.compose_shape()
S, RG, TW = SHAPE["slice_bits"], SHAPE["rows_per_workgroup"], SHAPE["tile_words"]
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _example(name: str):
    """an example module, with examples/ importable while it loads (they import each other by bare name)"""
    sys.path.insert(0, EXAMPLES)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLES, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(EXAMPLES)
    return mod


# -- the doubling boundaries ------------------------------------------------------------------------------------------------------------
N65 = 65                                                      # two words, an odd word count


@pytest.fixture(scope="module")
def affine65():
    return invertible_affine(65, N65)


@pytest.fixture(scope="module")
def watched65():
    return cut(dense(66, 3, T.form_words(N65)), N65 + 1)


@pytest.fixture(scope="module")
def twin65(affine65, watched65):
    """the twin's 17 time steps of the three watched forms, computed once: every shorter count is a prefix, one form a row subset"""
    want = U.unroll(watched65, N65, affine65, 0, 1, 17)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("ra", [1, 3])
@pytest.mark.parametrize("count", [0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17])
def test_doubling_boundaries(affine65, watched65, twin65, ra, count):
    assert (affine65[:, 0] & np.uint64(1)).any(), "the map needs a constant: the unit row has to matter"
    got = hip.compose_unroll_words(watched65[:ra], N65, affine65, count)
    assert hip.compose_last_times()["products"] == U.products(0, 1, count)
    w = T.form_words(N65)
    want = twin65.reshape(17, 3, w)[:count, :ra].reshape(count * ra, w)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("start, step", [(0, 1), (5, 1), (0, 3), (7, 2), ((1 << 64) + 3, (1 << 64) + 1)])
def test_start_and_step(affine65, watched65, start, step):
    got = hip.compose_unroll_words(watched65, N65, affine65, 5, start=start, step=step)
    assert hip.compose_last_times()["products"] == U.products(start, step, 5)
    assert np.array_equal(got, U.unroll(watched65, N65, affine65, start, step, 5))


def test_no_forms_and_no_times(affine65, watched65):
    assert hip.compose_unroll_words(watched65[:0], N65, affine65, 4).shape == (0, 2)
    assert hip.compose_unroll_words(watched65, N65, affine65, 0, start=3, step=2).shape == (0, 2)
    assert hip.compose_last_times()["products"] == 0


# -- a block that crosses a row group and two slices --------------------------------------------------------------------------------
N_BIG, RA_BIG = S + 1, 65


@pytest.fixture(scope="module")
def big():
    """(a, b, the twin's 129 time steps): dense random, computed once"""
    w = T.form_words(N_BIG)
    a, b = cut(dense(7, RA_BIG, w), N_BIG + 1), cut(dense(8, N_BIG, w), N_BIG + 1)
    want = U.unroll(a, N_BIG, b, 0, 1, 129)
    want.setflags(write=False)
    return a, b, want


@pytest.mark.parametrize("count", [127, 129])
def test_blocks_across_row_groups_and_slices(big, count):
    a, b, want = big
    assert 63 * RA_BIG < RG < 64 * RA_BIG and 127 * RA_BIG > 2 * RG and N_BIG + 1 > S
    got = hip.compose_unroll_words(a, N_BIG, b, count)
    assert hip.compose_last_times()["products"] == U.products(0, 1, count)
    assert np.array_equal(got, want[:count * RA_BIG])


# -- garbage and padding --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 2])
def test_garbage_is_ignored_and_padding_is_zero(affine65, watched65, twin65, start):
    w = T.form_words(N65)
    dirty_a = np.concatenate([watched65 | (dense(1, 3, w) & ~cut(~np.zeros((3, w), dtype=np.uint64), N65 + 1)), dense(2, 3, 2)], axis=1)
    dirty_b = np.concatenate([affine65 | (dense(3, N65, w) & ~cut(~np.zeros((N65, w), dtype=np.uint64), N65 + 1)), dense(4, N65, 1)], axis=1)
    assert np.array_equal(cut(dirty_a[:, :w], N65 + 1), watched65) and not np.array_equal(dirty_a[:, :w], watched65)
    assert np.array_equal(cut(dirty_b[:, :w], N65 + 1), affine65) and not np.array_equal(dirty_b[:, :w], affine65)
    got = hip.compose_unroll_words(dirty_a, N65, dirty_b, 6, start=start, stride_words=w + 3)
    assert got.shape == (18, w + 3) and not got[:, w:].any(), "every word behind W must be zero"
    assert np.array_equal(got[:, :w], twin65[3 * start:3 * (start + 6)])


# -- answers that owe nothing to this code ----------------------------------------------------------------------------------------------
def _lfsr16_step():
    lin = PackedLinearSystem([16])
    (x,) = lin.gens()
    reg = GaloisLFSR(16, 0xB400, x)
    reg()
    return x, reg.state


def test_lfsr_against_the_concrete_register():
    x, step = _lfsr16_step()
    items = unroll((x,), (step,), 40)
    assert len(items) == 40 and all(isinstance(it, tuple) and len(it) == 1 and len(it[0]) == 16 for it in items)
    rng = random.Random(40)
    for _ in range(3):
        seed = rng.getrandbits(16)
        reg = GaloisLFSR(16, 0xB400, seed)
        for t in range(40):
            assert items[t][0].evaluate(seed) == reg.state, t
            reg()


def test_lfsr_period_steps_are_the_identity():
    """x^16 + x^14 + x^13 + x^11 + 1 (taps 0xB400) is primitive: the step map has order 65535"""
    x, step = _lfsr16_step()
    items = unroll(x, (step,), 3, step=65535)
    assert len(items) == 3 and all(np.array_equal(v._rows, x._rows) for v in items)
    assert not np.array_equal(unroll(x, (step,), 2, step=255)[1]._rows, x._rows)


def test_xoshiro_against_concrete_stepping():
    lin, images = xoshiro_step_map()
    items = unroll(lin.gens(), images, 8)
    assert len(items) == 8 and all([len(v) for v in it] == [64] * 4 for it in items)
    rng = random.Random(256)
    for _ in range(3):
        state = [rng.getrandbits(64) for _ in range(4)]
        x = sum(w << (64 * i) for i, w in enumerate(state))
        gen = Xoshiro256starstar(state)
        for t in range(8):
            assert [v.evaluate(x) for v in items[t]] == gen.s, t
            gen.step()


# -- the rows of host stepping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [GaloisLFSR, FibonacciLFSR])
def test_rows_equal_host_stepping(kind):
    base = _example("nlfsr_recovery")
    lin = PackedLinearSystem([base.N_BITS])
    (x,) = lin.gens()
    sym = kind(base.N_BITS, base.TAPS, x)
    sym()
    items = unroll([x[i] for i in base.SELECT], (sym.state,), 300, start=1)
    assert len(items) == 300
    host = kind(base.N_BITS, base.TAPS, x)
    for t in range(300):
        host()
        assert len(items[t]) == 5
        for got, i in zip(items[t], base.SELECT):
            assert np.array_equal(got._rows, host.state[i]._rows), (t, i)
    # one vector in, one out; the items look into one array
    whole = unroll(x, (sym.state,), 3, start=299)
    assert isinstance(whole[0], PackedBitVec) and np.array_equal(whole[1]._rows, host.state._rows)
    assert not whole[0]._rows.flags.owndata and np.shares_memory(whole[0]._rows.base, whole[2]._rows.base)


# -- the device entry ---------------------------------------------------------------------------------------------------------------------------
N_DEV, RA_DEV, COUNT_DEV = S + 40, 70, 9                      # two slices; 9 time steps: blocks of 1, 2, 4 and a tail of 1


def test_unroll_device_matches_words_and_is_stream_ordered(stream, cycles):
    w = T.form_words(N_DEV)
    new_a, old_a = _even(dense(1, RA_DEV, w)), _even(dense(2, RA_DEV, w))
    new_b, old_b = _even(dense(3, N_DEV, w)), _even(dense(4, N_DEV, w))
    for start, step in ((0, 1), (3, 2)):
        want = hip.compose_unroll_words(new_a, N_DEV, new_b, COUNT_DEV, start=start, step=step)
        assert not np.array_equal(want, hip.compose_unroll_words(old_a, N_DEV, new_b, COUNT_DEV, start=start, step=step))
        assert not np.array_equal(want, hip.compose_unroll_words(new_a, N_DEV, old_b, COUNT_DEV, start=start, step=step))
        # the forms and the map in one tensor (rows of the same even stride), so that one delayed copy brings both
        d_in, d_new = _dev(np.concatenate([old_a, old_b])), _dev(np.concatenate([new_a, new_b]))
        d_a, d_b = d_in[:RA_DEV], d_in[RA_DEV:]
        out_stride = w + 1 if w % 2 else w + 2
        d_out = _dev(dense(5, COUNT_DEV * RA_DEV, out_stride))    # (junk: every word must be written)
        _delayed_copy(stream, cycles, d_in, d_new)
        hip.compose_unroll_device(d_a.data_ptr(), RA_DEV, new_a.shape[1], N_DEV, d_b.data_ptr(), new_b.shape[1], COUNT_DEV, d_out.data_ptr(),
                                  out_stride, start=start, step=step, stream=stream.cuda_stream)
        assert hip.compose_last_times()["products"] == U.products(start, step, COUNT_DEV)
        stream.synchronize()
        # the inputs may go once the stream is through
        d_in.zero_()
        torch.cuda.synchronize()
        got = _host(d_out)
        assert np.array_equal(got[:, :w], want) and not got[:, w:].any()


# -- two threads ---------------------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_their_own_answers():
    n, count = S + 9, 6
    jobs = []
    for t in range(2):
        a, b = cut(dense(20 + t, 40, T.form_words(n)), n + 1), cut(dense(30 + t, n, T.form_words(n)), n + 1)
        jobs.append((a, b, U.unroll(a, n, b, 1, 1, count)))
    results = [[] for _ in jobs]
    go = threading.Barrier(len(jobs))

    def work(i):
        a, b, _ = jobs[i]
        images = [PackedBitVec(b[:100]), PackedBitVec(b[100:])]
        go.wait()
        for _ in range(8):
            items = unroll(PackedBitVec(a), images, count, start=1)
            results[i].append(np.concatenate([v._rows for v in items]))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not np.array_equal(jobs[0][2], jobs[1][2])
    for (_, _, want), got in zip(jobs, results):
        assert len(got) == 8 and all(np.array_equal(g, want) for g in got)


# -- the example -----------------------------------------------------------------------------------------------------------------------------------
def test_nlfsr_recovery_unrolled_example():
    mod = _example("nlfsr_recovery_unrolled")
    secret = mod.recover(GaloisLFSR, 1, 2 ** 14 + 1000, time_host=False)
    assert secret == random.Random(1).getrandbits(mod.N_BITS)
