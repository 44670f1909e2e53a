"""Equations appended to a kept factorization (gf2bv_factor_append_*, gf2bv_factor_copy, Factorization.append / copy,
hip.Factor.append_*, FactoredSystem.add / copy).  The contract: after appending B1 .. Bm to a handle of A, every result is
bit-identical to gf2bv_solve_rhs_words on the stacked matrix [A; B1; ..; Bm] -- status, rank, pivots, dimension, origin, basis."""
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import LinearSystem, QuadraticSystem, hip
from oracle import gf2_oracle as O
from tests import harness as H
from tests.harness_models import MT19937
from tests.systems import random_system
from tests.test_gpu_rhs import _make_rhs, _rhs_words, _with_rhs, assert_same_oracle, assert_same_solution

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(params=["default", "plain"])
def heuristics(request, monkeypatch):
    """As shipped and with GF2BV_PLAIN=1 (both panel paths for every block, events instead of gates)."""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


def _check_stacked(f: hip.Factor, aug, cols, mode, rng, nrhs=6, oracle=False):
    """f against solve_rhs_words on the stacked matrix `aug` (planted and random right-hand sides)"""
    rows = aug.shape[0]
    assert f.rows == rows
    bits = _make_rhs(rng, aug, rows, cols, nrhs)
    rhs = _rhs_words(bits)
    got = f.solve(rhs)
    want = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    assert len(got) == len(want) == nrhs
    for g, w in zip(got, want):
        assert_same_solution(g, w, mode)
        assert g.dimension == w.dimension
    assert f.rank == want[0].rank
    assert np.array_equal(f.pivots, want[0].pivots)
    if oracle:
        for j in (0, 1):
            assert_same_oracle(got[j], O.solve_words(_with_rhs(aug, cols, bits[j]), rows, cols, mode), mode)
    return got


def _base(rng, rows, cols, cap, early_free):
    """A rank-deficient A whose columns early_free are zero: an append gives them pivots before A's own"""
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cap, True, 0), cols)
    for c in early_free:
        if c < cols:
            aug[:, c // 64] &= ~np.uint64(1 << (c % 64))
    return aug


def _batch(rng, kind, k, aug_so_far, cols, words):
    """k new equations: 'rand' dense random, 'span' XOR combinations of the rows so far (rank unchanged), 'sparse' with zero rows"""
    if kind == "span":
        out = np.zeros((k, words), dtype=np.uint64)
        n = aug_so_far.shape[0]
        for i in range(k):
            for _ in range(3):
                out[i] ^= aug_so_far[rng.randrange(n)]
        return out
    eqs = []
    for _ in range(k):
        if kind == "sparse" and rng.random() < 0.4:
            eqs.append(0)
        elif kind == "sparse":
            eqs.append(sum(1 << (1 + rng.randrange(cols)) for _ in range(3)) | rng.getrandbits(1))
        else:
            eqs.append(rng.getrandbits(cols + 1))
    a = O.eqs_to_aug(eqs, cols)
    out = np.zeros((k, words), dtype=np.uint64)
    out[:, :a.shape[1]] = a[:, :words]
    return out


# rows, cols, rank cap of A: cols % 64 in {0, 1, 63}, rank-deficient, small enough for the oracle first
SHAPES = [(70, 64, 40), (80, 65, 60), (140, 127, 100), (1100, 1000, 700), (2100, 2049, 1900)]
KS = [1, 63, 64, 65, 300]
KINDS = ["span", "sparse", "rand", "span", "rand"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", [0, 1])
def test_appends_match_stacked(shape, mode, heuristics):
    rows, cols, cap = shape
    rng = random.Random(rows * 7 + cols + mode)
    aug = _base(rng, rows, cols, cap, [0, 1, 5, 64, 66, cols - 1])
    words = aug.shape[1]
    oracle = rows * cols <= 200 * 200
    batches = []
    stacked = aug
    for kind, k in zip(KINDS, KS):
        b = _batch(rng, kind, k, stacked, cols, words)
        batches.append(b)
        stacked = np.vstack([stacked, b])
    # in several calls, with a solve after each (the first one grows the handle, the later ones fit its rounded capacity)
    with hip.factor_words(aug, rows, cols, mode) as f:
        _check_stacked(f, aug, cols, mode, rng, oracle=oracle)
        so_far = aug
        for b in batches:
            f.append_words(b)
            so_far = np.vstack([so_far, b])
            _check_stacked(f, so_far, cols, mode, rng, oracle=oracle)
    # in one call
    with hip.factor_words(aug, rows, cols, mode) as f:
        f.append_words(stacked[rows:])
        _check_stacked(f, stacked, cols, mode, rng, oracle=oracle)


@pytest.mark.parametrize("mode", [0, 1])
def test_multi_chunk_append_and_second_grow(mode):
    """1500 rows in one call (two elimination chunks of at most 1024 rows, the handle grown to 3072 rows), then an append that fits
    the capacity, then one that crosses it (a second grow: re-tiled from a slab with spare rows, the row records replaced)."""
    rng = random.Random(31 + mode)
    rows, cols = 1100, 1000
    aug = _base(rng, rows, cols, 200, [0, 1, 63, 64, 500])
    words = aug.shape[1]
    b1 = np.vstack([_batch(rng, "sparse", 700, aug, cols, words), _batch(rng, "rand", 800, aug, cols, words)])
    b2 = _batch(rng, "span", 300, aug, cols, words)
    b3 = _batch(rng, "rand", 400, aug, cols, words)
    with hip.factor_words(aug, rows, cols, mode) as f:
        f.append_words(b1)
        stacked = np.vstack([aug, b1])
        got = _check_stacked(f, stacked, cols, mode, rng)
        assert got[0].rank == cols
        bytes_after_grow = f.device_bytes
        f.append_words(b2)
        stacked = np.vstack([stacked, b2])
        _check_stacked(f, stacked, cols, mode, rng)
        assert f.device_bytes == bytes_after_grow                         # (it fit: rows 2900 of 3072)
        f.append_words(b3)
        stacked = np.vstack([stacked, b3])
        _check_stacked(f, stacked, cols, mode, rng)
        assert f.device_bytes > bytes_after_grow                          # (3300 rows: grown again)
    # two chunks that both find pivots: A of rank 200, 1500 sparse rows
    b = _batch(rng, "sparse", 1500, aug, cols, words)
    with hip.factor_words(aug, rows, cols, mode) as f:
        f.append_words(b)
        _check_stacked(f, np.vstack([aug, b]), cols, mode, rng)


def test_internal_append_array_form_equals_list_form():
    """Factorization.append with an n x words uint64 array (equation-int bit order: bit 0 = constant) equals the list form."""
    from gf2bv_amd import _internal
    rng = random.Random(17)
    rows, cols = 400, 330
    eqs = random_system(rng, rows, cols, .5, 250, True, 0)
    more = [rng.getrandbits(cols + 1) for _ in range(120)] + [0, 1]
    words = (cols + 1 + 63) // 64
    arr = np.array([[(e >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(words)] for e in more], dtype=np.uint64)
    # two planted right-hand sides and a random one (bit r = the constant of stacked equation r)
    rhs = []
    for _ in range(2):
        x = rng.getrandbits(cols)
        rhs.append(sum((bin((e >> 1) & x).count("1") & 1) << r for r, e in enumerate(eqs + more)))
    rhs.append(rng.getrandbits(rows + len(more)))
    for mode in (0, 1):
        f1 = _internal.m4ri_factor(eqs, cols, mode)
        f2 = _internal.m4ri_factor(eqs, cols, mode)
        f1.append(more)
        f2.append(arr)
        assert f1.rows == f2.rows == rows + len(more)
        assert f1.rank == f2.rank and f1.pivots == f2.pivots
        got1, got2 = f1.solve(rhs), f2.solve(rhs)
        want = _internal.m4ri_solve_rhs(eqs + more, cols, mode, rhs)
        assert any(w is not None for w in want)
        for a, b, w in zip(got1, got2, want):
            if mode == 0 or w is None:
                assert a == b == w
            else:
                assert (a.origin, a.basis, a.dimension) == (b.origin, b.basis, b.dimension) == (w.origin, w.basis, w.dimension)
        f1.close()
        f2.close()


def test_span_keeps_rank_and_turns_inconsistent():
    """B inside A's row space: the rank stays, and a right-hand side that contradicts it on the new rows is inconsistent."""
    rng = random.Random(4)
    rows, cols = 600, 500
    aug = _base(rng, rows, cols, 400, [])
    b = _batch(rng, "span", 100, aug, cols, aug.shape[1])
    stacked = np.vstack([aug, b])
    for mode in (0, 1):
        with hip.factor_words(aug, rows, cols, mode) as f:
            r0 = f.rank
            f.append_words(b)
            assert f.rank == r0
            got = _check_stacked(f, stacked, cols, mode, rng, nrhs=8)
            assert any(g.status == 1 for g in got[1::2])                   # the random ones
            assert all(g.status == 0 for g in got[0::2])                   # the planted ones


def test_append_makes_full_rank_and_digits_form():
    rng = random.Random(8)
    rows, cols = 700, 640
    aug = _base(rng, rows, cols, 500, [3, 70, 639])
    b = _batch(rng, "rand", 200, aug, cols, aug.shape[1])
    stacked = np.vstack([aug, b])
    with hip.factor_words(aug, rows, cols, 1) as f:
        g = hip.factor_words(aug, rows, cols, 1)
        f.append_words(b)
        assert f.rank == cols
        _check_stacked(f, stacked, cols, 1, rng)
        # the same rows as equation ints in 32-bit digits (bit 0 = constant), and from the device
        nd = (cols + 1 + 31) // 32
        raw = bytearray()
        for row in b:
            v = int.from_bytes(row.tobytes(), "little")
            raw += ((((v & ((1 << cols) - 1)) << 1) | ((v >> cols) & 1)).to_bytes(nd * 4, "little"))
        digits = np.frombuffer(bytes(raw), dtype=np.uint32)
        offs = np.arange(b.shape[0] + 1, dtype=np.int64) * nd
        g.append_digits(digits, offs, 32, b.shape[0])
        _check_stacked(g, stacked, cols, 1, rng)
        g.close()
    stride = hip.padded_stride(cols)
    t = torch.zeros((b.shape[0], stride), dtype=torch.int64, device="cuda")
    t[:, :b.shape[1]] = torch.from_numpy(b.view(np.int64)).cuda()
    torch.cuda.synchronize()
    with hip.factor_words(aug, rows, cols, 0) as f:
        f.append_device(t.data_ptr(), b.shape[0], stride)
        _check_stacked(f, stacked, cols, 0, rng)
    del t


def test_forced_two_level_plan(monkeypatch, heuristics):
    monkeypatch.setenv("GF2BV_TWO_LEVEL", "2")
    rows, cols, cap = 2600, 2500, 2300
    rng = random.Random(rows + cols + 1)
    aug = _base(rng, rows, cols, cap, [10, 700])
    b = _batch(rng, "rand", 250, aug, cols, aug.shape[1])
    for mode in (0, 1):
        with hip.factor_words(aug, rows, cols, mode) as f:
            f.append_words(b[:50])
            _check_stacked(f, np.vstack([aug, b[:50]]), cols, mode, rng)
            f.append_words(b[50:])
            got = _check_stacked(f, np.vstack([aug, b]), cols, mode, rng)
            assert got[0].rank == cols


def test_failed_append_leaves_handle_intact():
    rng = random.Random(12)
    rows, cols = 300, 250
    aug = _base(rng, rows, cols, 200, [])
    b = _batch(rng, "rand", 20, aug, cols, aug.shape[1])
    with hip.factor_words(aug, rows, cols, 1) as f:
        before = _check_stacked(f, aug, cols, 1, random.Random(1))
        with pytest.raises(ValueError):
            f.append_words(b, rows=0)
        with pytest.raises(ValueError):
            f.append_words(b[:, :1])                                       # the stride does not cover cols + 1 bits
        with pytest.raises(ValueError):
            f.append_device(0, 4, hip.padded_stride(cols))                 # null device pointer
        with pytest.raises(ValueError):
            f.append_device(8, 4, 3)                                       # odd stride / misaligned
        assert f.rows == rows and f.rank == before[0].rank
        after = _check_stacked(f, aug, cols, 1, random.Random(1))
        for g, w in zip(after, before):
            assert_same_solution(g, w, 1)
        f.append_words(b)                                                  # still usable
        _check_stacked(f, np.vstack([aug, b]), cols, 1, rng)


def test_copy_is_independent():
    rng = random.Random(21)
    rows, cols = 1050, 1000
    aug = _base(rng, rows, cols, 800, [2, 900])
    b1 = _batch(rng, "rand", 120, aug, cols, aug.shape[1])
    b2 = _batch(rng, "sparse", 500, aug, cols, aug.shape[1])
    for mode in (0, 1):
        with hip.factor_words(aug, rows, cols, mode) as f:
            f.append_words(b1)
            c = f.copy()
            assert c.rows == f.rows and c.rank == f.rank
            c.append_words(b2)
            _check_stacked(f, np.vstack([aug, b1]), cols, mode, rng)
            _check_stacked(c, np.vstack([aug, b1, b2]), cols, mode, rng)
            f.append_words(b2[:7])
            _check_stacked(f, np.vstack([aug, b1, b2[:7]]), cols, mode, rng)
            _check_stacked(c, np.vstack([aug, b1, b2]), cols, mode, rng)
            c.close()


@pytest.mark.parametrize("two_level", [None, "2"])
@pytest.mark.parametrize("mode", [0, 1])
def test_copy_outlives_its_original(mode, two_level, monkeypatch):
    """A copy owns everything it works on: the original (grown by an append: it has row records of its own) is closed first and a
    second factorization of the same shape takes its buffers from the pool and overwrites them; the copy still answers, and still
    appends.  GF2BV_TWO_LEVEL=2: the first two of the four blocks form an outer panel (T matrices, row lists, 2K multiplier sets)."""
    if two_level:
        monkeypatch.setenv("GF2BV_TWO_LEVEL", two_level)
    rng = random.Random(77 + mode)
    rows, cols = 1050, 1000
    aug = _base(rng, rows, cols, 800, [2, 900])
    other = _base(rng, rows, cols, 900, [7])
    b1 = _batch(rng, "rand", 120, aug, cols, aug.shape[1])
    b2 = _batch(rng, "sparse", 500, aug, cols, aug.shape[1])
    f = hip.factor_words(aug, rows, cols, mode)
    f.append_words(b1)
    c = f.copy()
    f.close()
    g = hip.factor_words(other, rows, cols, mode)
    try:
        _check_stacked(c, np.vstack([aug, b1]), cols, mode, rng)
        c.append_words(b2)
        _check_stacked(c, np.vstack([aug, b1, b2]), cols, mode, rng)
        _check_stacked(g, other, cols, mode, rng)
    finally:
        c.close()
        g.close()


@pytest.mark.parametrize("bs", [32, 1])
def test_mt19937_outputs_arrive(bs):
    """Too few outputs factored, the rest appended in batches (FactoredSystem.add); the known answer of examples/mt.py."""
    lin = LinearSystem([32] * 624)
    mt = lin.gens()
    model = MT19937(mt)
    samples = 624 * 32 // bs
    outs = [model.getrandbits(bs) for _ in range(samples)]
    rand = random.Random(3142)
    state = tuple(rand.getstate()[1][:-1])
    values = [rand.getrandbits(bs) for _ in range(samples)]
    first = samples - (16 if bs == 32 else 600)
    step = 4 if bs == 32 else 150
    with lin.factor([mt[0]] + outs[:first]) as fs:
        vals = [0x80000000] + values[:first]
        assert fs.solve_raw_one_rhs([vals]) == lin.solve_raw_one_rhs([mt[0]] + outs[:first], [vals])
        for i in range(first, samples, step):
            fs.add(outs[i:i + step])
            vals += values[i:i + step]
        assert fs.solve_one(vals) == state
        exprs = [mt[0]] + outs
        assert fs.solve_raw_one_rhs([vals]) == lin.solve_raw_one_rhs(exprs, [vals])


def test_quadratic_guesses_on_copies():
    for c3 in (0, 1):
        q, zeros = H.quadratic_small_system((0, 0, 0, c3))
        assert isinstance(q, QuadraticSystem)
        x, y = q.gens()
        base = zeros[:3]
        with q.factor(base) as fs:
            fs.solve_one([0] * len(base))                                  # (the handle exists before the copies)
            for a in (x[0], x[1], x[2], y[0], y[1]):
                for v in (0, 1):
                    guess = list(q.bit_assert(a, v))
                    c = fs.copy()
                    c.add(guess)
                    assert c.solve_one([0] * (len(base) + len(guess))) == q.solve_one(base + guess)
                    c.close()
            assert fs.solve_one([0] * len(base)) == q.solve_one(base)      # the base is as it was


def test_large_device_resident_append():
    """65536^2 bench system factored with its last 512 rows zeroed, those rows appended from the device (66048 stacked rows):
    full rank, x == planted, equal to solve_rhs_device on the stacked matrix."""
    n, seed, k = 65536, 1234, 512
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n + k, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    torch.cuda.synchronize()
    A[n:] = A[n - k:n]                                                     # the original rows, appended below
    A[n - k:n] = 0
    torch.cuda.synchronize()
    rw = (n + k + 63) // 64
    w = n // 64
    b = ((A[:, w] >> (n % 64)) & 1).clone()
    weights = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64, device=dev)
    pad = torch.zeros(rw * 64, dtype=torch.int64, device=dev)
    pad[:n + k] = b
    rhs = (pad.view(rw, 64) * weights).sum(dim=1).view(1, rw).contiguous()
    torch.cuda.synchronize()
    planted = hip.planted_solution(n, seed)
    f = hip.factor_device(A.data_ptr(), n, n, stride, 0)
    assert f.rank < n
    f.append_device(A[n:].data_ptr(), k, stride)
    assert f.rows == n + k and f.rank == n
    got = f.solve_device(rhs.data_ptr(), 1, rw)[0]
    f.close()
    want = hip.solve_rhs_device(A.data_ptr(), n + k, n, stride, rhs.data_ptr(), 1, rw, 0)[0]
    assert_same_solution(got, want, 0)
    assert got.status == 0 and np.array_equal(got.origin, planted)
    del A, rhs, pad, b
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
