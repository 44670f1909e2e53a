"""Stream ordering of the device entries.  The contract (include/gf2bv_hip.h): an entry that reads device memory reads what the
caller's stream (NULL = the null stream) has produced when the call is made, even though it does its work on the library's own
streams.  Each case makes the window real: on the caller's stream a spin of ~100 ms, then the producer -- a device-to-device copy
of the NEW content over the OLD one -- and the library call while the producer is still pending (asserted before every call, so
no case can pass because the window was missed).  Every result must be the CPU oracle's answer for NEW, and the oracle's answers
for OLD and NEW are asserted to differ, so a stale read cannot match by chance.  Every case runs on the null stream (torch's
default stream) and on a side stream whose handle is passed explicitly."""
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import hip, slab
from oracle import gf2_oracle as O
from tests.known_answer import assert_same
from tests.systems import random_system
from tests.test_gpu_rhs import _bits, _make_rhs, _rhs_words, _with_rhs

pytestmark = pytest.mark.gpu

DELAY_MS = 100.0            # the spin in front of every producer
BUDGET_MS = 6000.0          # all the spins of the module together
_spent_ms = [0.0]

R, C, CAP, OLD_CAP = 1100, 1023, 900, 800      # the blocked-path shape; OLD's lower rank cap makes every answer differ
SR, SC, SCAP = 600, 500, 450                    # the handle of Factor.solve_device (65 oracle solves per stream)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(scope="module", autouse=True)
def _warm(_need_gpu):
    """The library's first calls load its code and fill its pools: done here, before any window is timed, so that no case's
    ~100 ms go to them."""
    a = _aug(0, R, C, CAP)
    hip.solve_words(a, R, C, 1)
    with hip.factor_words(a, R, C, 1) as f:
        f.solve(_rhs_words(_make_rhs(random.Random(0), a, R, C, 2)))


@pytest.fixture(scope="module")
def cycles():
    """torch.cuda._sleep cycles for DELAY_MS, measured once with timing events (the clock64 rate of the chip is not assumed)."""
    torch.cuda._sleep(1000)                     # (the spin kernel loaded)
    torch.cuda.synchronize()
    trial = 10_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(trial)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 1.0, f"a spin of {trial} cycles took {ms} ms"
    return int(trial * DELAY_MS / ms)


@pytest.fixture(params=["null", "side"])
def stream(request):
    """The caller's stream: torch's default stream (the null stream, handle 0) or a side stream."""
    if request.param == "null":
        s = torch.cuda.default_stream()
        assert s.cuda_stream == 0
    else:
        s = torch.cuda.Stream()
        assert s.cuda_stream != 0
    torch.cuda.synchronize()
    yield s
    torch.cuda.synchronize()                    # nothing pending outlives the case


def _dev(a: np.ndarray) -> torch.Tensor:
    """uint64 host array -> int64 device tensor of the same shape (complete when this returns)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def _stage(old: np.ndarray, new: np.ndarray):
    """The buffer the entry reads, holding OLD, and NEW on the device ready to be copied over it."""
    assert old.shape == new.shape
    return _dev(old), _dev(new)


def _delayed_copy(s: torch.cuda.Stream, cycles: int, dst: torch.Tensor, src: torch.Tensor) -> torch.cuda.Event:
    """On `s`: a spin of `cycles`, then dst.copy_(src).  Returns the event recorded after the copy, checked to be pending."""
    assert _spent_ms[0] + DELAY_MS <= BUDGET_MS, "the module's spins exceed their budget"
    _spent_ms[0] += DELAY_MS
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        dst.copy_(src)
        ev.record(s)
    assert not ev.query(), "the producer finished before the call: the window is not there"
    return ev


def _differs(x: dict, y: dict) -> bool:
    return any(not np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in ("status", "rank", "pivcols", "origin", "basis"))


def _assert_old_differs(olds, news):
    """at least one oracle answer for OLD differs from NEW's: a result read from OLD cannot pass"""
    assert any(_differs(o, n) for o, n in zip(olds, news)), "OLD and NEW have the same answers"


def _aug(seed: int, rows: int, cols: int, cap) -> np.ndarray:
    return O.eqs_to_aug(random_system(random.Random(seed), rows, cols, .5, cap, True, 0), cols, hip.padded_stride(cols))


def _rhs_pair(seed: int, aug: np.ndarray, rows: int, cols: int, nrhs: int):
    """NEW and OLD right-hand-side bits: NEW planted at even j and random at odd j, OLD the other way round"""
    rng = random.Random(seed)
    return _make_rhs(rng, aug, rows, cols, nrhs), _make_rhs(rng, aug, rows, cols, nrhs + 1)[1:]


def _oracles(aug: np.ndarray, rows: int, cols: int, bits: np.ndarray, mode: int) -> list:
    return [O.solve_words(_with_rhs(aug, cols, b), rows, cols, mode) for b in bits]


def _handle(s: torch.cuda.Stream) -> int:
    return s.cuda_stream


# -- the single-matrix solve ----------------------------------------------------------------------------------------------
def test_solve_device_small_path(stream, cycles):
    rows, cols = 640, 256
    new, old = _aug(1, rows, cols, None), _aug(2, rows, cols, 200)
    want = O.solve_words(new, rows, cols, 1)
    _assert_old_differs([O.solve_words(old, rows, cols, 1)], [want])
    buf, src = _stage(old, new)
    _delayed_copy(stream, cycles, buf, src)
    got = hip.solve_device(buf.data_ptr(), rows, cols, new.shape[1], 1, stream=_handle(stream))
    assert got.stats["small_path"] == 1
    assert_same(got, want, 1)


def test_solve_device_blocked_path(stream, cycles):
    new, old = _aug(3, R, C, CAP), _aug(4, R, C, OLD_CAP)
    want = O.solve_words(new, R, C, 1)
    _assert_old_differs([O.solve_words(old, R, C, 1)], [want])
    buf, src = _stage(old, new)
    _delayed_copy(stream, cycles, buf, src)
    got = hip.solve_device(buf.data_ptr(), R, C, new.shape[1], 1, stream=_handle(stream))
    assert got.stats["small_path"] == 0
    assert_same(got, want, 1)


def test_solve_batch_device(stream, cycles):
    news = [_aug(10 + i, R, C, CAP) for i in range(3)]
    olds = [_aug(20 + i, R, C, OLD_CAP) for i in range(3)]
    wants = [O.solve_words(a, R, C, 1) for a in news]
    _assert_old_differs([O.solve_words(a, R, C, 1) for a in olds], wants)
    stride = news[0].shape[1]
    buf, src = _stage(np.concatenate(olds), np.concatenate(news))
    _delayed_copy(stream, cycles, buf, src)
    got = hip.solve_batch_device(buf.data_ptr(), 3, R * stride, R, C, stride, 1, stream=_handle(stream))
    assert max(g.stats["gang_systems"] for g in got) > 1                 # (the systems did run as a gang)
    for g, w in zip(got, wants):
        assert_same(g, w, 1)


# -- many right-hand sides of one matrix ----------------------------------------------------------------------------------
@pytest.mark.parametrize("delayed", ["matrix", "rhs"])
def test_solve_rhs_device(stream, cycles, delayed):
    nrhs = 9
    new = _aug(30, R, C, CAP)
    bits, old_bits = _rhs_pair(31, new, R, C, nrhs)
    wants = _oracles(new, R, C, bits, 1)
    rw = (R + 63) // 64
    if delayed == "matrix":
        old = _aug(32, R, C, OLD_CAP)
        _assert_old_differs(_oracles(old, R, C, bits, 1), wants)
        buf, src = _stage(old, new)
        rhs = _dev(_rhs_words(bits))
        mat, rhs_ptr = buf, rhs.data_ptr()
    else:
        _assert_old_differs(_oracles(new, R, C, old_bits, 1), wants)
        buf, src = _stage(_rhs_words(old_bits), _rhs_words(bits))
        mat, rhs_ptr = _dev(new), buf.data_ptr()
    _delayed_copy(stream, cycles, buf, src)
    got = hip.solve_rhs_device(mat.data_ptr(), R, C, new.shape[1], rhs_ptr, nrhs, rw, 1, stream=_handle(stream))
    assert len(got) == nrhs
    for g, w in zip(got, wants):
        assert_same(g, w, 1)


# -- the kept factorization -----------------------------------------------------------------------------------------------
def _check_factor(f: hip.Factor, aug: np.ndarray, rows: int, cols: int, mode: int, seed: int):
    """rank, pivots and host-RHS solves of the handle against the oracle of `aug`"""
    want = O.solve_words(aug, rows, cols, mode)
    assert f.rank == want["rank"]
    assert np.array_equal(f.pivots, want["pivcols"][:want["rank"]])
    bits = _make_rhs(random.Random(seed), aug, rows, cols, 6)
    got = f.solve(_rhs_words(bits))
    for g, w in zip(got, _oracles(aug, rows, cols, bits, mode)):
        assert_same(g, w, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_factor_device(stream, cycles, mode):
    new, old = _aug(40, R, C, CAP), _aug(41, R, C, OLD_CAP)
    _assert_old_differs([O.solve_words(old, R, C, mode)], [O.solve_words(new, R, C, mode)])
    buf, src = _stage(old, new)
    _delayed_copy(stream, cycles, buf, src)
    f = hip.factor_device(buf.data_ptr(), R, C, new.shape[1], mode, stream=_handle(stream))
    try:
        torch.cuda.synchronize()
        _check_factor(f, new, R, C, mode, 42)
    finally:
        f.close()


@pytest.mark.parametrize("nrhs", [1, 65])          # 65: two passes of 64 slots
def test_factor_solve_device(stream, cycles, nrhs):
    a = _aug(50, SR, SC, SCAP)
    bits, old_bits = _rhs_pair(51, a, SR, SC, nrhs)
    wants = _oracles(a, SR, SC, bits, 1)
    _assert_old_differs(_oracles(a, SR, SC, old_bits[:1], 1), wants[:1])
    rw = (SR + 63) // 64
    buf, src = _stage(_rhs_words(old_bits), _rhs_words(bits))
    f = hip.factor_words(a, SR, SC, 1)
    try:
        _delayed_copy(stream, cycles, buf, src)
        got = f.solve_device(buf.data_ptr(), nrhs, rw, stream=_handle(stream))
        assert len(got) == nrhs
        for g, w in zip(got, wants):
            assert_same(g, w, 1)
    finally:
        f.close()


def _rows(seed: int, k: int, cols: int) -> np.ndarray:
    return O.eqs_to_aug(random_system(random.Random(seed), k, cols, .5, None, True, 0), cols, hip.padded_stride(cols))


def test_factor_append_device(stream, cycles):
    k = 120
    a = _aug(60, R, C, CAP)                                               # rank 900: the new rows add pivots
    new, old = _rows(61, k, C), _rows(62, k, C)
    stacked, stacked_old = np.concatenate((a, new)), np.concatenate((a, old))
    bits = _make_rhs(random.Random(63), stacked, R + k, C, 6)
    _assert_old_differs(_oracles(stacked_old, R + k, C, bits, 1), _oracles(stacked, R + k, C, bits, 1))
    buf, src = _stage(old, new)
    f = hip.factor_words(a, R, C, 1)
    try:
        _delayed_copy(stream, cycles, buf, src)
        f.append_device(buf.data_ptr(), k, new.shape[1], stream=_handle(stream))
        torch.cuda.synchronize()
        assert f.rows == R + k
        _check_factor(f, stacked, R + k, C, 1, 63)
    finally:
        f.close()


# -- the handle keeps no pointer to the caller's buffers --------------------------------------------------------------------
def _on_stream(s: torch.cuda.Stream, a: np.ndarray) -> torch.Tensor:
    """`a` in a buffer allocated on `s` (so that freeing it there hands its memory to the next allocation on `s`), complete"""
    with torch.cuda.stream(s):
        t = torch.empty(a.shape, dtype=torch.int64, device="cuda")
        t.copy_(_dev(a))
    torch.cuda.synchronize()
    return t


def test_factor_device_keeps_no_pointer_to_its_input(stream):
    """after factor_device returns, its input is overwritten and freed on the caller's stream, and the memory reused"""
    new, old = _aug(70, R, C, CAP), _aug(71, R, C, OLD_CAP)
    held = [_on_stream(stream, new)]
    junk = _dev(old)
    f = hip.factor_device(held[0].data_ptr(), R, C, new.shape[1], 1, stream=_handle(stream))
    try:
        with torch.cuda.stream(stream):
            held[0].copy_(junk)
            held.clear()
            reuse = torch.empty(junk.shape, dtype=torch.int64, device="cuda")
            reuse.copy_(junk)
        torch.cuda.synchronize()
        _check_factor(f, new, R, C, 1, 72)
        del reuse
    finally:
        f.close()


def test_factor_append_device_keeps_no_pointer_to_its_rows(stream):
    """the same for the rows given to append_device"""
    k = 120
    a = _aug(73, R, C, CAP)
    new, old = _rows(74, k, C), _rows(75, k, C)
    held = [_on_stream(stream, new)]
    junk = _dev(old)
    f = hip.factor_words(a, R, C, 1)
    try:
        f.append_device(held[0].data_ptr(), k, new.shape[1], stream=_handle(stream))
        with torch.cuda.stream(stream):
            held[0].copy_(junk)
            held.clear()
            reuse = torch.empty(junk.shape, dtype=torch.int64, device="cuda")
            reuse.copy_(junk)
        torch.cuda.synchronize()
        _check_factor(f, np.concatenate((a, new)), R + k, C, 1, 76)
        del reuse
    finally:
        f.close()


# -- the checker and the column-slab engine ---------------------------------------------------------------------------------
def _host_residual(aug: np.ndarray, rows: int, cols: int, x: np.ndarray) -> int:
    """rows where A x != b, counted on the host"""
    A = _bits(aug, rows, cols).astype(np.int64)
    xb = np.unpackbits(np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8), bitorder="little")[:cols].astype(np.int64)
    b = (aug[:rows, cols // 64] >> np.uint64(cols % 64)) & np.uint64(1)
    return int((((A @ xb) & 1) != b.astype(np.int64)).sum())


def test_residual_device(stream, cycles):
    new, old = _aug(80, R, C, CAP), _aug(81, R, C, OLD_CAP)
    x = O.solve_words(new, R, C, 0)["origin"]
    want = _host_residual(new, R, C, x)
    assert want == 0 and _host_residual(old, R, C, x) != want
    buf, src = _stage(old, new)
    _delayed_copy(stream, cycles, buf, src)
    assert hip.residual_device(buf.data_ptr(), R, C, new.shape[1], x, stream=_handle(stream)) == want


def test_slab_engine_world_1(stream, cycles):
    """slab.HipSlabEngine driven as run_schedule drives it at world size 1 (no process group).  The engine follows torch's
    current stream, so it is built and run inside `with torch.cuda.stream(...)`."""
    n = 3000
    stride = hip.padded_stride(n)
    new, old = O.gen_synthetic(n, n, 90, stride), O.gen_synthetic(n, n, 91, stride)
    want = O.solve_words(new, n, n, 0)
    _assert_old_differs([O.solve_words(old, n, n, 0)], [want])
    buf, src = _stage(old, new)
    with torch.cuda.stream(stream):
        _delayed_copy(stream, cycles, buf, src)
        eng = slab.HipSlabEngine(buf.data_ptr(), n, n, stride, 1, 0, 0)
        try:
            for b in range(eng.nblocks):
                eng.apply(b, eng.factor(b))
            eng.finish_local()
            got = eng.solve()
        finally:
            eng.close()
    assert_same(got, want, 0)
