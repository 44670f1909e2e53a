"""Hybrid degree-4 XL on cubic equations on the MI355X: guessed unknowns substituted into cubic rows (k_cubic_specialise), every
assignment's rows multiplied in one launch (k_xl4_cubic_expand_batch) and all systems solved as lock-step gangs.  The yardsticks are
the set-based substitution of tests/cubic_guess_terms.py, the set-based expansion of tests/cubic_xl4_terms.py and the CPU oracle on
their rows; every comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedCubicGuessSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols, xl4_cols
from oracle import gf2_oracle as O
from tests import cubic_guess_terms as CG
from tests import xl4_terms as X4
from tests.cubic_terms import (REGISTER_12, REGISTER_16, expand_ints, poly_int, poly_value, random_cubic_terms, register_zeros, row_polys,
                               to_aug)
from tests.known_answer import assert_same
from tests.test_gpu_stream_order import _delayed_copy, _handle, cycles, stream      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _w3(n: int) -> int:
    return (xl3_cols(n) + 1 + 63) // 64


def _dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).cuda()      # (a copy: the shared cases are read-only)
    torch.cuda.synchronize()
    return t


# -- 1. specialisation parity ----------------------------------------------------------------------------------------------------------------
# n' = 1 and 3 (no triple, one triple); f = 0; the constant on bit 63 and on bit 1 of a word; cols2' = 66 crossing a word inside the
# per-guess vectors; an unsorted guess; f = n - 1 (256 assignments); n' = 65: two words of linear columns
SPEC_CASES = [(2, (1,)), (4, (0,)), (5, ()), (8, (7,)), (11, (10, 0)), (13, (12, 0)), (12, (5, 11, 2)), (9, (0, 1, 2, 3, 4, 5, 6, 7)),
              (67, (66, 0))]


@functools.lru_cache(maxsize=None)
def _spec_case(n: int, guess: tuple):
    """(cubic source rows one spare word wide, the rows as sets of monomials): random factored rows expanded by the set product and a
    row with every coefficient set (three random rows alone at n = 67); made once, never changed"""
    polys = row_polys(n, *random_cubic_terms(random.Random(7000 + n + len(guess)), n, 3))
    if n < 60:
        polys.append(frozenset([frozenset()] + [frozenset((i,)) for i in range(n)] + [frozenset((i, j)) for i in range(n) for j in range(i)]
                               + [frozenset((i, j, l)) for i in range(n) for j in range(i) for l in range(j)]))
        polys.append(frozenset([frozenset()]))
    src = to_aug([poly_int(p, n) for p in polys], xl3_cols(n), _w3(n) + 1)
    src.setflags(write=False)
    return src, tuple(polys)


def _specialise_device(src: np.ndarray, n: int, guess, a0: int, na: int, stride: int, sys_stride: int) -> np.ndarray:
    """gf2bv_cubic_specialise_device into a buffer that held the sentinel in every word"""
    d_src = _dev(src)
    d_out = torch.full((max(na * sys_stride, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.cubic_specialise_device(d_src.data_ptr(), len(src), src.shape[1], n, guess, a0, na, d_out.data_ptr(), stride, sys_stride)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)[:na * sys_stride].reshape(na, sys_stride)


@pytest.mark.parametrize("n,guess", SPEC_CASES)
def test_specialisation_equals_set_substitution(n, guess):
    src, polys = _spec_case(n, guess)
    m, ns, total = len(polys), n - len(guess), 1 << len(guess)
    w = _w3(ns)
    want = CG.specialised_aug(polys, n, guess, 0, total)                   # [2^f, m, W3']
    assert want.any() and (ns < 3 or any(len(mono) == 3 for p in CG.specialise_polys(polys, n, guess, total - 1) for mono in p))
    got = hip.cubic_specialise_words(src, n, guess)
    assert got.shape == want.shape == (total, m, w)
    assert np.array_equal(got, want), (n, guess, np.argwhere(got != want)[:4])
    # an odd and an even stride with spare words (one word at a time / 16 bytes at a time), a sub-range of the assignments
    a0 = total // 3 + (total > 1)
    odd, even = w + 1 + (w & 1), w + 2 - (w & 1)
    assert odd & 1 and not even & 1 and 0 < a0 + (total == 1) <= total
    for stride in (odd, even):
        for first, count in ((0, total), (a0, total - a0)):
            g = hip.cubic_specialise_words(src, n, guess, first, count, stride_words=stride)
            assert g.shape == (count, m, stride)
            assert np.array_equal(g[:, :, :w], want[first:first + count]), (n, guess, stride, first)
            assert not g[:, :, w:].any()               # the spare words of the stride come back zero
    # the device entry: systems further apart than they need to be, nothing written between them
    for stride in (odd, even):
        sys_stride = m * stride + 2
        g = _specialise_device(src, n, guess, a0, total - a0, stride, sys_stride)
        rows = g[:, :m * stride].reshape(total - a0, m, stride)
        assert np.array_equal(rows[:, :, :w], want[a0:]) and not rows[:, :, w:].any()
        assert (g[:, m * stride:] == SENTINEL).all()
    assert hip.cubic_specialise_words(src[:0], n, guess).shape == (total, 0, w)
    assert hip.cubic_specialise_words(src, n, guess, 0, 0).shape == (0, m, w)


@pytest.mark.parametrize("n,guess", [(8, (7,)), (11, (10, 0)), (12, (5, 11, 2))])
def test_bits_behind_the_source_constant_are_ignored(n, guess):
    src, polys = _spec_case(n, guess)
    junk = np.array(src)
    for c in range(xl3_cols(n) + 1, 64 * junk.shape[1]):
        junk[:, c >> 6] |= np.uint64(1 << (c & 63))
    assert not np.array_equal(junk, src)
    total, w = 1 << len(guess), _w3(n - len(guess))
    want = CG.specialised_aug(polys, n, guess, 0, total)
    got = hip.cubic_specialise_words(junk, n, guess, stride_words=w + 2)
    assert np.array_equal(got[:, :, :w], want) and not got[:, :, w:].any()


# -- 2. the batched multiply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 2, 5])
def test_batch_expansion_equals_single_expansions(nsys):
    for n, m, pad in ((4, 3, 2), (9, 4, 3), (13, 2, 0)):
        rng = random.Random(100 * nsys + n)
        cols3 = xl3_cols(n)
        cubics = np.stack([to_aug([rng.getrandbits(cols3 + 1) for _ in range(m)], cols3, _w3(n) + 1) for _ in range(nsys)])
        rows = m * (n + 1) + pad
        stride = (xl4_cols(n) + 1 + 63) // 64 + (nsys & 1)
        sys_stride = rows * stride + 7
        got = hip.xl4_cubic_expand_batch_words(cubics, n, rows=rows, stride_words=stride, sys_stride_words=sys_stride)
        assert got.shape == (nsys, sys_stride)
        singles = [hip.xl4_cubic_expand_words(c, n, rows=rows, stride_words=stride) for c in cubics]
        for s in range(nsys):
            assert np.array_equal(got[s, :rows * stride].reshape(rows, stride), singles[s]), (nsys, n, s)
            assert not got[s, rows * stride:].any()    # (the binding's zeros: the entry writes nothing between the systems)
        tight = hip.xl4_cubic_expand_batch_words(cubics, n)
        assert np.array_equal(tight.reshape(nsys, m * (n + 1), -1), np.stack([hip.xl4_cubic_expand_words(c, n) for c in cubics]))
        # the device entry: sources and outputs both further apart than they need to be, every other word pre-filled
        qs = cubics.shape[2]
        csys, even = m * qs + 5, stride + (stride & 1)
        dsys = rows * even + 4
        src = np.full((nsys, csys), SENTINEL, dtype=np.uint64)
        src[:, :m * qs] = cubics.reshape(nsys, -1)
        d_src = _dev(src)
        out = torch.full((nsys * dsys,), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hip.xl4_cubic_expand_batch_device(d_src.data_ptr(), nsys, csys, m, qs, n, rows, out.data_ptr(), even, dsys)
        torch.cuda.synchronize()
        dev = out.cpu().numpy().view(np.uint64).reshape(nsys, dsys)
        for s in range(nsys):
            block = dev[s, :rows * even].reshape(rows, even)
            assert np.array_equal(block[:, :stride], singles[s]) and not block[:, stride:].any()
        assert (dev[:, rows * even:] == SENTINEL).all()
    assert hip.xl4_cubic_expand_batch_words(np.zeros((0, 2, 3), dtype=np.uint64), 9).shape == (0, 2 * 10 * 4)


# -- 3. hybrid solves against the CPU oracle on the helper's rows ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _register_case(secret: int, outputs: int):
    """(factored arrays, expanded cubic rows, the rows as sets of monomials) of REGISTER_12's first `outputs` equations"""
    n = 12
    p = PackedCubicGuessSystem([n])
    terms = p._terms(register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], outputs))
    polys = CG.register_case(secret, count=outputs, **REGISTER_12)
    cubic = to_aug([poly_int(q, n) for q in polys], xl3_cols(n), _w3(n))
    assert expand_ints(n, *terms) == [poly_int(q, n) for q in polys]       # the two ways of writing the register agree
    return terms, cubic, polys


@functools.lru_cache(maxsize=None)
def _planted_case(n: int, m: int, seed: int):
    """m random factored rows over n unknowns, every one vanishing at a planted point: (factored arrays, cubic rows, sets, point)"""
    rng = random.Random(seed)
    point = rng.getrandbits(n) | 2
    terms = random_cubic_terms(rng, n, m, max_terms=2)
    for r, p in enumerate(row_polys(n, *terms)):
        terms[0][r, 0] ^= np.uint64(poly_value(p, point))
    polys = tuple(row_polys(n, *terms))
    cubic = to_aug([poly_int(q, n) for q in polys], xl3_cols(n), _w3(n))
    return terms, cubic, polys, point


def _dims(want: list) -> list:
    return [w[1]["dim"] if w[1]["status"] == 0 else None for w in want]


def _check_hybrid(n: int, guess: tuple, terms, cubic, polys, dims):
    total = 1 << len(guess)
    want = [CG.oracle_guess(polys, n, guess, a) for a in range(total)]
    if dims is not None:
        assert _dims(want) == dims                     # (the CPU tests' rank facts: the cases are what their names say)
    for md in (0, 1):
        for got in (hip.solve_xl4_cubic_guess_words(cubic, n, guess, mode=md), hip.solve_xl4_cubic_guess_terms(*terms, n, guess, mode=md)):
            assert len(got) == total
            for a in range(total):
                assert_same(got[a], want[a][md], md)
    return want


# all deficient, then mixed, then one consistent
@pytest.mark.parametrize("outputs,dims", [(34, [11, 11, 11, 11]), (35, [None, 2, 1, 1]), (36, [None, 0, None, None])])
def test_register_12_two_guesses_equal_oracle(outputs, dims):
    _check_hybrid(12, (10, 11), *_register_case(0x52F, outputs), dims)


@pytest.mark.parametrize("outputs,dims", [(26, [None, 1, None, 3, None, 2, None, None]), (27, [None, 0] + [None] * 6)])
def test_register_12_three_guesses_equal_oracle(outputs, dims):
    _check_hybrid(12, (3, 7, 11), *_register_case(0x52F, outputs), dims)


def test_planted_system_equals_oracle():
    n, guess = 10, (9, 4)                              # n' = 8: 162 quartic columns, 9 rows an equation, 20 equations
    terms, cubic, polys, point = _planted_case(n, 20, 1020)
    want = _check_hybrid(n, guess, terms, cubic, polys, None)
    own = ((point >> 9) & 1) | (((point >> 4) & 1) << 1)
    assert want[own][1]["status"] == 0                 # the planted point's assignment is consistent
    for first, count in ((1, 2), (3, 1), (2, 0)):
        for md in (0, 1):
            for got in (hip.solve_xl4_cubic_guess_words(cubic, n, guess, first, count, md),
                        hip.solve_xl4_cubic_guess_terms(*terms, n, guess, first, count, md)):
                assert len(got) == count
                for s in range(count):
                    assert_same(got[s], want[first + s][md], md)


# -- 4. known answers through the front-end ------------------------------------------------------------------------------------------------
def _zero_set(polys, n: int) -> set:
    """the common zeros of the polynomials over all 2^n points"""
    x = np.arange(1 << n)
    bit = [(x >> g) & 1 for g in range(n)]
    alive = np.ones(1 << n, dtype=bool)
    for p in polys:
        v = np.zeros(1 << n, dtype=np.int64)
        for mono in p:
            t = np.ones(1 << n, dtype=np.int64)
            for g in mono:
                t &= bit[g]
            v ^= t
        alive &= v == 0
    return set(np.flatnonzero(alive).tolist())


def _oracle_points(polys, n: int, guess) -> list:
    """the consistent points of every assignment's space, in assignment order and within one in AffineSpace order"""
    ns = n - len(guess)
    cols4 = xl4_cols(ns)
    out = []
    for a in range(1 << len(guess)):
        ints = CG.quartic_ints(polys, n, guess, a)
        space = O.m4ri_solve(ints + [0] * max(0, cols4 - len(ints)), cols4, 1)
        if space is None:
            continue
        assert space.dimension <= 16
        for raw in space:
            y = raw & ((1 << ns) - 1)
            if X4.point_vector(y, ns) == raw:
                out.append((CG.scatter(y, n, guess, a),))
    return out


@pytest.mark.parametrize("secret", [0x52F, 0x3A1])
def test_register_12_known_answers(secret):
    """36 outputs and two guessed bits give exactly the secret where plain degree-4 XL needs 62; at 35 outputs the generator returns
    the brute-force zero set of the 2^12 points, in assignment and AffineSpace order"""
    n, guess = 12, (10, 11)
    p = PackedCubicGuessSystem([n])
    (x,) = p.gens()
    zeros = register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], 36)
    assert list(p.solve_all_xl4_guess(zeros, guess)) == [(secret,)]
    assert list(p.solve_all_xl4_guess(zeros, [x[10], x[11]])) == [(secret,)] and p.solve_one_xl4_guess(zeros, guess) == (secret,)
    own = (secret >> 10) & 3
    spaces = p.solve_raw_space_xl4_guess(zeros, guess)
    assert [sp is not None for sp in spaces] == [a == own for a in range(4)] and spaces[own].dimension == 0
    assert p.convert_sol_xl4_guess(spaces[own].origin, guess, own) == (secret,)
    assert p.solve_raw_one_xl4_guess(zeros, guess) == [None if sp is None else sp.origin for sp in spaces]
    with pytest.raises(DimensionTooLargeError):        # plain degree-4 XL on the same 36 outputs
        list(p.solve_all_xl4(zeros))
    polys = CG.register_case(secret, count=35, **REGISTER_12)
    truth = _zero_set(polys, n)
    want = _oracle_points(polys, n, guess)
    assert secret in truth and {s for (s,) in want} == truth and len(want) == len(truth)
    got = list(p.solve_all_xl4_guess(zeros[:35], guess))
    assert got == want
    assert list(p.solve_all_xl4_guess(zeros + [1], guess)) == [] and p.solve_one_xl4_guess(zeros + [1], guess) is None
    if secret == 0x52F:                                # 34 outputs: dimension 11 under every assignment
        with pytest.raises(DimensionTooLargeError, match="assignment 0") as e:
            list(p.solve_all_xl4_guess(zeros[:34], guess, max_dimension=10))
        assert e.value.space.dimension == 11


def test_register_16_from_62_outputs():
    """n = 16, guess x[12..15]: 16 systems of 806 x 793, one batch; plain degree-4 XL needs 149 outputs"""
    n, secret, guess = 16, 0x52E7, (12, 13, 14, 15)
    p = PackedCubicGuessSystem([n])
    zeros = register_zeros(p, secret, REGISTER_16["taps"], REGISTER_16["pos"], 62)
    assert xl4_cols(12) == 793 and len(p._terms(zeros)[0]) * 13 == 806
    assert list(p.solve_all_xl4_guess(zeros, guess)) == [(secret,)]
    spaces = p.solve_raw_space_xl4_guess(zeros, guess)
    assert [a for a, sp in enumerate(spaces) if sp is not None] == [secret >> 12] and spaces[secret >> 12].dimension == 0
    with pytest.raises(DimensionTooLargeError):
        list(p.solve_all_xl4(zeros))


def test_assignment_ranges_and_no_guess():
    n, guess = 12, (3, 7, 11)
    p = PackedCubicGuessSystem([n])
    zeros = register_zeros(p, 0x3A1, REGISTER_12["taps"], REGISTER_12["pos"], 26)          # consistent: assignments 1, 2, 3, 5, 7
    full = list(p.solve_all_xl4_guess(zeros, guess))
    spaces = p.solve_raw_space_xl4_guess(zeros, guess)
    assert [None if sp is None else sp.dimension for sp in spaces] == [None, 1, 1, 3, None, 1, None, 3] and full
    parts = [sol for a in range(0, 8, 3) for sol in p.solve_all_xl4_guess(zeros, guess, assignments=(a, min(3, 8 - a)))]
    assert parts == full
    key = lambda sp: None if sp is None else (sp.origin, tuple(sp.basis))          # noqa: E731
    assert [key(sp) for sp in p.solve_raw_space_xl4_guess(zeros, guess, assignments=(2, 4))] == [key(sp) for sp in spaces[2:6]]
    assert p.solve_raw_space_xl4_guess(zeros, guess, assignments=(5, 0)) == []
    # f = 0: the plain degree-4 XL system
    terms = _planted_case(10, 40, 1040)[0]
    (one,) = hip.solve_xl4_cubic_guess_terms(*terms, 10, [], mode=1)
    plain = hip.solve_xl4_cubic_terms(*terms, 10, 1)
    fields = lambda s: (s.status, s.rank, s.dimension, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())      # noqa: E731
    assert fields(one) == fields(plain) and plain.status == 0
    zs = register_zeros(p, 0x3A1, REGISTER_12["taps"], REGISTER_12["pos"], 60)             # dimension 13, one consistent point
    (sp,) = p.solve_raw_space_xl4_guess(zs, [])
    assert sp.dimension == 13 and key(sp) == key(p.solve_raw_space_xl4(zs))
    assert list(p.solve_all_xl4_guess(zs, [])) == list(p.solve_all_xl4(zs)) == [(0x3A1,)]


# -- 5. stream order -------------------------------------------------------------------------------------------------------------------------
def test_chain_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the cubic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then specialisation, batched multiply and the gang solve are enqueued there with no synchronisation anywhere."""
    n, m, guess = 12, 30, (1, 4, 7)                    # 8 systems over 9 unknowns: 300 live rows, 255 columns
    ns, na = n - len(guess), 8
    cols4 = xl4_cols(ns)
    rows, stride = 300 + 3, hip.padded_stride(cols4)
    ss = _w3(ns) + 1                                   # 4 words a specialised row
    new, old = _planted_case(n, m, 91)[1], _planted_case(n, m, 92)[1]
    want, stale = hip.solve_xl4_cubic_guess_words(new, n, guess, mode=1), hip.solve_xl4_cubic_guess_words(old, n, guess, mode=1)
    key = lambda sols: [(s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist()) for s in sols]     # noqa: E731
    assert any(s.status == 0 for s in want) and key(want) != key(stale), "the two systems have the same answers"
    buf, src = _dev(old), _dev(new)
    d_spec = torch.zeros(na * m * ss, dtype=torch.int64, device="cuda")
    d_xl = torch.zeros(na * rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _delayed_copy(stream, cycles, buf, src)
    hip.cubic_specialise_device(buf.data_ptr(), m, new.shape[1], n, guess, 0, na, d_spec.data_ptr(), ss, m * ss, stream=_handle(stream))
    hip.xl4_cubic_expand_batch_device(d_spec.data_ptr(), na, m * ss, m, ss, ns, rows, d_xl.data_ptr(), stride, rows * stride, stream=_handle(stream))
    got = hip.solve_batch_device(d_xl.data_ptr(), na, rows * stride, rows, cols4, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (the solve entry's 300 rows and these 303: zero rows change nothing)
