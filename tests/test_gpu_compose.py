"""k_compose and the entries above it on the GPU, bit for bit: every selector position by construction, the boundary shapes (taken
from gf2bv_compose_shape, not copied) against the numpy twin of tests/compose_terms.py, powers, answers that owe nothing to this
code (an LFSR's period, xoshiro256's published jumps), the device entries and their stream ordering, and two threads."""
import importlib.util
import os
import random
import threading

import numpy as np
import pytest
import torch

import gf2bv_amd
from gf2bv_amd import PackedBitVec, PackedLinearSystem, hip, power, substitute
from tests import compose_terms as T
from tests.harness_models import GaloisLFSR, Xoshiro256starstar
from tests.test_compose_cpu import JUMP, LONG_JUMP, reference_jump, xoshiro_step_map

pytestmark = pytest.mark.gpu

SHAPE = hip.compose_shape()
S, RG, TW = SHAPE["slice_bits"], SHAPE["rows_per_workgroup"], SHAPE["tile_words"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def dense(seed: int, rows: int, words: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(rows, words), dtype=np.uint64)


def cut(rows: np.ndarray, nbits: int, words=None) -> np.ndarray:
    """the rows with every bit from nbits on cleared"""
    return T.words_of(T.bits_of(rows, nbits), rows.shape[1] if words is None else words)


# -- every selector position, by construction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", [2, 9, 65, S + 1, 2 * S + 1])
def test_unit_rows_select_every_row_of_b(n1):
    """A = one row per bit k of a form, only bit k set; B dense: C[k] is row k of B~ -- every table, every entry bit, every slice"""
    n = n1 - 1
    nb = 2 * 64 * TW + 37                                     # three tiles, the last one half
    a = T.words_of(np.eye(n1, dtype=np.uint8), T.form_words(n))
    b = dense(n1, n, T.form_words(nb))
    got = hip.compose_words(a, n, b, nb)
    unit = np.zeros((1, T.form_words(nb)), dtype=np.uint64)
    unit[0, 0] = 1
    assert np.array_equal(got, np.concatenate([unit, cut(b, nb + 1)]))


@pytest.mark.parametrize("n1", [2, 9, 65, S + 1, 2 * S + 1])
def test_identity_images_return_a(n1):
    n = n1 - 1
    a = dense(100 + n1, 77, T.form_words(n))
    assert np.array_equal(hip.compose_words(a, n, T.identity(n), n), cut(a, n1))


def test_zero_and_constant_forms():
    n, nb = S + 5, 200
    b = dense(3, n, T.form_words(nb))
    a = np.zeros((70, T.form_words(n)), dtype=np.uint64)
    assert not hip.compose_words(a, n, b, nb).any()
    a[::2, 0] = 1                                             # the constant alone: the unit form comes back
    got = hip.compose_words(a, n, b, nb)
    assert np.array_equal(got[:, 0], a[:, 0]) and not got[:, 1:].any()
    assert hip.compose_words(a[:0], n, b, nb).shape == (0, T.form_words(nb))


# -- boundaries against the twin ------------------------------------------------------------------------------------------------
N1 = [2, 8, 9, 63, 64, 65, S - 1, S, S + 1, 2 * S, 2 * S + 1]
RA = [1, 63, 64, 65, RG - 1, RG, RG + 1, 2 * RG + 1]
NB1 = [2, 64, 65, 128, 129, 193]


def _boundary_cases() -> list:
    """a chosen list, not the cross product: every value of each axis several times, the corners together"""
    cases = []
    for i in range(24):
        cases.append((N1[i % len(N1)], RA[(3 * i + 1) % len(RA)], NB1[(5 * i + 2) % len(NB1)]))
    for i, ra in enumerate(RA):
        cases.append((N1[(4 * i + 6) % len(N1)], ra, NB1[i % len(NB1)]))
    cases += [(2, 1, 2), (2 * S + 1, 2 * RG + 1, 193), (S + 1, RG + 1, 129), (S, RG, 128), (S - 1, RG - 1, 64), (65, 65, 65),
              (2 * S, 64, 193), (9, 2 * RG + 1, 2), (2 * S + 1, 1, 65)]
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


BOUNDARY = _boundary_cases()


def test_boundary_list_covers_every_value():
    assert 38 <= len(BOUNDARY) <= 44
    assert {c[0] for c in BOUNDARY} == set(N1) and {c[1] for c in BOUNDARY} == set(RA) and {c[2] for c in BOUNDARY} == set(NB1)


@pytest.mark.parametrize("n1, ra, nb1", BOUNDARY)
def test_boundary_against_twin(n1, ra, nb1):
    """dense random, with garbage above n in A and above nb in B (whole words of it too) and an output stride above Wb"""
    n, nb = n1 - 1, nb1 - 1
    wa, wb = T.form_words(n), T.form_words(nb)
    a = dense(n1 * 7 + ra, ra, wa + 1)                        # (a word the forms do not own: ignored)
    b = dense(nb1 * 11 + n1, n, wb + 2)
    want = T.substitute(a, n, b, nb, wb + 3)
    got = hip.compose_words(a, n, b, nb, stride_words=wb + 3)
    assert not got[:, wb:].any(), "the padding behind Wb must be zero"
    assert np.array_equal(got, want)
    # the same forms without the garbage, the plain stride
    assert np.array_equal(hip.compose_words(cut(a, n1, wa), n, cut(b, nb1, wb), nb), want[:, :wb])


# -- powers -------------------------------------------------------------------------------------------------------------------------
def invertible_affine(seed: int, n: int) -> np.ndarray:
    """a dense invertible linear part (unit lower x unit upper triangular) and a random constant, as n image rows"""
    rng = np.random.default_rng(seed)
    lo = np.tril(rng.integers(0, 2, (n, n)), -1) + np.eye(n, dtype=np.int64)
    up = np.triu(rng.integers(0, 2, (n, n)), 1) + np.eye(n, dtype=np.int64)
    bits = np.concatenate([rng.integers(0, 2, (n, 1)), (lo @ up) & 1], axis=1).astype(np.uint8)
    return T.words_of(bits, T.form_words(n))


@pytest.fixture(scope="module")
def affine65():
    return invertible_affine(65, 65)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, (1 << 64) + 3])
def test_power_against_twin(affine65, k):
    got = hip.compose_power_words(affine65, 65, k)
    assert np.array_equal(got, T.power(affine65, 65, k))
    assert hip.compose_last_times()["products"] == (k.bit_length() - 1 + bin(k).count("1") if k else 0)


def test_power_pads_and_ignores_garbage(affine65):
    dirty = affine65.copy()
    dirty[:, 1] |= dense(1, 65, 1)[:, 0] << np.uint64(2)      # (66 live bits: everything from bit 2 of word 1 on is garbage)
    assert np.array_equal(cut(dirty, 66), affine65) and not np.array_equal(dirty, affine65)
    got = hip.compose_power_words(np.concatenate([dirty, dense(2, 65, 1)], axis=1), 65, 3, stride_words=5)
    assert not got[:, 2:].any() and np.array_equal(got[:, :2], T.power(affine65, 65, 3))


def _vec(rows: np.ndarray) -> tuple:
    return (PackedBitVec(rows),)


def test_powers_add(affine65):
    m = _vec(affine65)
    for a, b in ((2, 3), (7, 1), (0, 4), ((1 << 64) + 1, 6)):
        lhs = substitute(power(m, a), power(m, b))
        assert isinstance(lhs, tuple) and len(lhs) == 1
        assert np.array_equal(lhs[0]._rows, power(m, a + b)[0]._rows)


def test_affine_lfsr_against_concrete_iteration():
    """Galois LFSR step XOR a constant: the unit row matters at every product"""
    const = 0x9d2c
    lin = PackedLinearSystem([16])
    reg = GaloisLFSR(16, 0xB400, lin.gens()[0])
    reg()
    step = (reg.state ^ const,)
    rng = random.Random(16)
    for k in (1, 2, 77, 1000):
        pk = power(step, k)[0]
        for _ in range(3):
            x = rng.getrandbits(16)
            c = GaloisLFSR(16, 0xB400, x)
            for _ in range(k):
                c()
                c.state ^= const
            assert pk.evaluate(x) == c.state


# -- known answers that owe nothing to this code --------------------------------------------------------------------------------------
def test_lfsr_period():
    """x^16 + x^14 + x^13 + x^11 + 1 (taps 0xB400) is primitive: the step map has order 65535"""
    lin = PackedLinearSystem([16])
    reg = GaloisLFSR(16, 0xB400, lin.gens()[0])
    reg()
    ident = lin.gens()[0]._rows
    assert np.array_equal(power((reg.state,), 65535)[0]._rows, ident)
    assert not np.array_equal(power((reg.state,), 255)[0]._rows, ident)
    assert np.array_equal(power((reg.state,), 0)[0]._rows, ident)


@pytest.mark.parametrize("k, poly", [(1 << 128, JUMP), (1 << 192, LONG_JUMP)], ids=["jump", "long_jump"])
def test_xoshiro_jumps(k, poly):
    _, images = xoshiro_step_map()
    jumped = power(images, k)
    assert [len(v) for v in jumped] == [64] * 4
    rng = random.Random(k.bit_length())
    for _ in range(3):
        state = [rng.getrandbits(64) for _ in range(4)]
        x = sum(w << (64 * i) for i, w in enumerate(state))
        assert [v.evaluate(x) for v in jumped] == reference_jump(state, poly)


def test_xoshiro_jump_recovery_example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "xoshiro_jump_recovery.py")
    spec = importlib.util.spec_from_file_location("xoshiro_jump_recovery", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seed = [0x0123456789abcdef, 0xfedcba9876543210, 0x0f1e2d3c4b5a6978, 0x8796a5b4c3d2e1f0]
    outs = mod.observe(seed)
    assert mod.recover(outs) == tuple(seed)


# -- device entries ---------------------------------------------------------------------------------------------------------------------
def _dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _even(rows: np.ndarray) -> np.ndarray:
    """the rows with an even word stride, as the device entries want them"""
    if rows.shape[1] % 2 == 0:
        return rows
    return np.concatenate([rows, np.zeros((len(rows), 1), dtype=np.uint64)], axis=1)


@pytest.fixture(params=["null", "side"])
def stream(request):
    s = torch.cuda.default_stream() if request.param == "null" else torch.cuda.Stream()
    assert (s.cuda_stream == 0) == (request.param == "null")
    torch.cuda.synchronize()
    yield s
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cycles():
    """torch.cuda._sleep cycles for ~100 ms, measured once with timing events"""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    trial = 10_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(trial)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 1.0
    return int(trial * 100.0 / ms)


def _delayed_copy(s, cycles: int, dst: torch.Tensor, src: torch.Tensor):
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        dst.copy_(src)
        ev.record(s)
    assert not ev.query(), "the producer finished before the call: the window is not there"


N_DEV, NB_DEV, RA_DEV = S + 40, 150, 300                      # two slices, two tiles (one half), one row group


def test_compose_device_matches_words_and_is_stream_ordered(stream, cycles):
    wa, wb = T.form_words(N_DEV), T.form_words(NB_DEV)
    new, old = _even(dense(1, RA_DEV, wa)), _even(dense(2, RA_DEV, wa))
    b = _even(dense(3, N_DEV, wb))
    want = hip.compose_words(new, N_DEV, b, NB_DEV)
    assert not np.array_equal(want, hip.compose_words(old, N_DEV, b, NB_DEV))
    d_a, d_new, d_b = _dev(old), _dev(new), _dev(b)
    out_stride = wb + 1 if wb % 2 else wb + 2
    d_out = _dev(dense(4, RA_DEV, out_stride))                # (junk: every word must be written)
    _delayed_copy(stream, cycles, d_a, d_new)
    hip.compose_device(d_a.data_ptr(), RA_DEV, new.shape[1], N_DEV, d_b.data_ptr(), b.shape[1], NB_DEV, d_out.data_ptr(), out_stride,
                       stream=stream.cuda_stream)
    stream.synchronize()
    # the inputs may go once the stream is through
    d_a.copy_(d_out[:, :1].expand(-1, d_a.shape[1]))
    d_b.zero_()
    torch.cuda.synchronize()
    got = _host(d_out)
    assert np.array_equal(got[:, :wb], want) and not got[:, wb:].any()


def test_compose_power_device_matches_words_and_is_stream_ordered(stream, cycles):
    n, k = 65, 11
    new, old = invertible_affine(7, n), invertible_affine(8, n)
    want = hip.compose_power_words(new, n, k)
    assert not np.array_equal(want, hip.compose_power_words(old, n, k))
    d_b, d_new = _dev(old), _dev(new)
    d_out = _dev(dense(5, n, 4))
    _delayed_copy(stream, cycles, d_b, d_new)
    hip.compose_power_device(d_b.data_ptr(), 2, n, k, d_out.data_ptr(), 4, stream=stream.cuda_stream)
    stream.synchronize()
    d_b.zero_()
    torch.cuda.synchronize()
    got = _host(d_out)
    assert np.array_equal(got[:, :2], want) and not got[:, 2:].any()
    assert hip.compose_last_times()["products"] == 3 + 3


def test_compose_power_device_in_place():
    n = 65
    m = invertible_affine(9, n)
    d = _dev(m)
    hip.compose_power_device(d.data_ptr(), 2, n, 6, d.data_ptr(), 2)
    torch.cuda.synchronize()
    assert np.array_equal(_host(d), T.power(m, n, 6))


# -- two threads ---------------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_their_own_answers():
    n, nb = S + 9, 140
    jobs = []
    for t in range(2):
        a, b = dense(20 + t, 500, T.form_words(n)), dense(30 + t, n, T.form_words(nb))
        jobs.append((cut(a, n + 1), cut(b, nb + 1), T.substitute(a, n, b, nb)))
    results = [[] for _ in jobs]
    go = threading.Barrier(len(jobs))

    def work(i):
        a, b, _ = jobs[i]
        images = [PackedBitVec(b[:100]), PackedBitVec(b[100:])]
        go.wait()
        for _ in range(8):
            results[i].append(substitute(PackedBitVec(a), images)._rows.copy())

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not np.array_equal(jobs[0][2], jobs[1][2])
    for (_, _, want), got in zip(jobs, results):
        assert len(got) == 8 and all(np.array_equal(g, want) for g in got)
