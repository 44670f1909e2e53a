"""Hybrid XL without a GPU: the set-based substitution of tests.xl_guess_terms against brute force, the CPU-oracle pipeline on the systems
the GPU tests use (the conditions that keep those from passing vacuously), gf2bv_xl3_guess_chunk, the argument checks of every new
C-ABI entry -- made before any device is touched -- and the front-ends' guess parsing and scatter."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd._internal import m4ri_solve_xl3_guess, m4ri_solve_xl3_guess_quad_packed
from gf2bv_amd.linsys import xl3_cols
from oracle import gf2_oracle as O
from tests import xl_guess_terms as G
from tests import xl_terms as X
from tests.quad_terms import random_terms


# -- 1. the helper against brute-force evaluation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,guess", [(2, (1,)), (3, (0, 2)), (5, ()), (5, (3,)), (6, (4, 1, 2)), (7, (6, 0)), (8, (7, 2, 3, 5)), (8, (0, 1, 2, 3, 4, 5, 6))])
def test_substitution_equals_evaluation(n, guess):
    rng = random.Random(80 + n + len(guess))
    cols2 = n + n * (n - 1) // 2
    eqs = [rng.getrandbits(cols2 + 1) for _ in range(4)] + [(1 << (cols2 + 1)) - 1, 0, 1]
    ns = n - len(guess)
    for a in range(1 << len(guess)):
        spec = G.specialise_ints(eqs, n, guess, a)
        assert len(spec) == len(eqs) and all(e >> (ns + ns * (ns - 1) // 2 + 1) == 0 for e in spec)
        for y in range(1 << ns):
            x = G.scatter(y, n, guess, a)
            assert all((x >> g) & 1 == (a >> t) & 1 for t, g in enumerate(guess))
            assert [G.evaluate(e, y, ns) for e in spec] == [G.evaluate(e, x, n) for e in eqs], (a, y)
    if not guess:
        assert G.specialise_ints(eqs, n, guess, 0) == eqs


# -- 2. the CPU-oracle pipeline on the GPU tests' systems --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,guess", list(G.CASES))
def test_oracle_pipeline_finds_exactly_the_solutions(n, m, guess):
    eqs = list(G.case_eqs(n, m, guess))
    rows = X.xl3_ints(eqs, n)
    plain = O.m4ri_solve(rows + [0] * max(0, xl3_cols(n) - len(rows)), xl3_cols(n), 1)
    assert plain is not None and plain.dimension > 16          # plain degree-3 XL gives up on it
    points, largest = G.oracle_points(eqs, n, guess)           # (asserts that no assignment exceeds dimension 16)
    truth = G.brute_force(eqs, n)
    assert truth and sorted(points) == truth and len(set(points)) == len(points)
    assert 0 <= largest <= 16
    if (n, m) == (9, 8):
        assert largest == 3                                    # spaces with points that are no monomial vectors: the filter's work


def test_no_guess_is_plain_xl():
    n, m = 9, 8
    eqs = list(G.case_eqs(n, m, (1, 8)))
    assert G.specialise_ints(eqs, n, (), 0) == eqs
    aug, rows, cols3 = G.cubic_aug(eqs, n)
    want = O.solve_words(aug, rows, cols3, 1)
    got = G.oracle_guess(eqs, n, (), 0)[1]
    assert (got["status"], got["rank"]) == (want["status"], want["rank"]) and np.array_equal(got["basis"], want["basis"])


# -- 3. the chunk ----------------------------------------------------------------------------------------------------------------------------
def test_guess_chunk():
    m, n, f = 192, 40, 8                               # n' = 32: 6336 rows of 86 words and 192 rows of 10 words a system
    per = 8 * (6336 * 86 + 192 * 10)
    assert hip.xl3_guess_chunk(m, n, f, 4 * per - 1) == 0
    assert hip.xl3_guess_chunk(m, n, f, 4 * per) == 1
    assert hip.xl3_guess_chunk(m, n, f, 4 * 200 * per + 5) == 200
    assert hip.xl3_guess_chunk(m, n, f, 1 << 50) == 256          # capped at 2^f
    assert hip.xl3_guess_chunk(m, n, 0, 1 << 50) == 1
    last = 0
    for free in range(0, 40 * per, per // 3):
        c = hip.xl3_guess_chunk(m, n, f, free)
        assert c >= last
        last = c
    assert last == 9
    assert hip.xl3_guess_chunk(100, 60, 30, 1 << 60) == (2 ** 31 - 65) // max(100 * 31, xl3_cols(30))      # rows of all systems < 2^31 - 64
    for bad in ((m, 0, 0, 1), (m, n, -1, 1), (m, n, n, 1), (m, 40, 31, 1), (-1, n, f, 1), (m, n, f, -1), (0, 3000, 0, 1)):
        with pytest.raises(ValueError):
            hip.xl3_guess_chunk(*bad)


# -- 4. the C ABI: GF2BV_ERR_ARG before any device ---------------------------------------------------------------------------------------
def test_entries_check_arguments_before_device_use():
    L = hip.lib()
    n, m, f = 12, 5, 3                                 # 78 quadratic columns (2 words); n' = 9: 45 columns (1 word), 129 cubic (3 words)
    rows = 130                                         # max(5 * 10, 129) and one more
    quad = np.zeros((4 * m + 1, 2), dtype=np.uint64)
    aug = np.zeros((4 * rows + 1, 4), dtype=np.uint64)
    Q, A = quad.ctypes.data, aug.ctypes.data
    A += -A % 16
    guess = np.array([3, 11, 0], dtype=np.int32)
    Gp = guess.ctypes.data
    arr = lambda *v: np.array(v, dtype=np.int32)       # noqa: E731
    lin, off, ta, tb = random_terms(random.Random(3), n, m)
    Lp, Op, Ap, Bp = lin.ctypes.data, off.ctypes.data, ta.ctypes.data, tb.ctypes.data
    hs = (ctypes.c_void_p * 8)()
    big = 2 ** 31 - 64

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    def guess_errors(call):
        """what every entry with a guess refuses: call(n_lin, guess pointer, nguess, a0, na)"""
        err(call(0, Gp, 0, 0, 1), "n_lin")
        err(call(n, None, f, 0, 8), "null")
        err(call(n, Gp, -1, 0, 1), "nguess")
        err(call(n, Gp, n, 0, 1), "nguess")
        err(call(40, Gp, 31, 0, 1), "nguess")
        err(call(n, arr(3, 12, 0).ctypes.data, f, 0, 8), "0 .. n_lin - 1")
        err(call(n, arr(3, -1, 0).ctypes.data, f, 0, 8), "0 .. n_lin - 1")
        err(call(n, arr(3, 0, 3).ctypes.data, f, 0, 8), "repeated")
        err(call(n, Gp, f, -1, 2), "assignments")
        err(call(n, Gp, f, 0, -1), "assignments")
        err(call(n, Gp, f, 2, 7), "assignments")
        err(call(n, Gp, f, 9, 0), "assignments")

    D = L.gf2bv_quad_specialise_device
    guess_errors(lambda nl, g, nf, a0, na: D(Q, m, 2, nl, g, nf, a0, na, A, 1, m, 0, None))
    err(D(None, m, 2, n, Gp, f, 0, 8, A, 1, m, 0, None), "null")
    err(D(Q, m, 2, n, Gp, f, 0, 8, None, 1, m, 0, None), "null")
    err(D(Q, -1, 2, n, Gp, f, 0, 8, A, 1, m, 0, None), "na x m")
    err(D(Q, big // 8 + 1, 2, n, Gp, f, 0, 8, A, 1, big, 0, None), "na x m")
    err(D(Q, m, 1, n, Gp, f, 0, 8, A, 1, m, 0, None), "quad_stride_words")
    err(D(Q, m, 2, n, Gp, f, 0, 8, A, 0, m, 0, None), "out_stride_words")                # short
    err(D(Q, m, 2, n, Gp, f, 0, 8, A, 1, m - 1, 0, None), "out_stride_words")            # sys_stride below m rows
    err(D(Q, m, 2, n, Gp, f, 0, 8, A + 4, 1, m, 0, None), "out_stride_words")            # not a word boundary
    err(D(Q, 0, 10000, 1100, Gp, f, 0, 8, A, 10000, 0, 0, None), "LDS")                  # a 75 KiB source row
    err(D(Q, 0, 5000, 750, Gp, 0, 0, 1, A, 5000, 0, 0, None), "LDS")                     # 35 KiB, but twice: source and specialised row

    W = L.gf2bv_quad_specialise_words
    guess_errors(lambda nl, g, nf, a0, na: W(Q, m, 2, nl, g, nf, a0, na, A, 1, 0))
    err(W(None, m, 2, n, Gp, f, 0, 8, A, 1, 0), "null")
    err(W(Q, m, 2, n, Gp, f, 0, 8, None, 1, 0), "null")
    err(W(Q, big // 8 + 1, 2, n, Gp, f, 0, 8, A, 1, 0), "na x m")
    err(W(Q, m, 1, n, Gp, f, 0, 8, A, 1, 0), "quad_stride_words")
    err(W(Q, m, 2, n, Gp, f, 0, 8, A, 0, 0), "out_stride_words")
    err(W(Q, 0, 10000, 1100, Gp, f, 0, 8, A, 10000, 0), "LDS")

    B = L.gf2bv_xl3_expand_batch_device                # 4 systems of m rows over 9 unknowns, 1 word each
    err(B(None, 4, m, m, 1, 9, rows, A, 4, rows * 4, 0, None), "null")
    err(B(Q, 4, m, m, 1, 9, rows, None, 4, rows * 4, 0, None), "null")
    err(B(Q, -1, m, m, 1, 9, rows, A, 4, rows * 4, 0, None), "nsys")
    err(B(Q, 4, m, m, 1, 0, rows, A, 4, rows * 4, 0, None), "n_lin")
    err(B(Q, 4, m, -1, 1, 9, rows, A, 4, rows * 4, 0, None), "m(n_lin + 1)")
    err(B(Q, 4, m, m, 1, 9, m * 10 - 1, A, 4, rows * 4, 0, None), "rows must")
    err(B(Q, big // rows + 1, m, m, 1, 9, rows, A, 4, rows * 4, 0, None), "all systems together")
    err(B(Q, 4, m, m, 0, 9, rows, A, 4, rows * 4, 0, None), "quad_stride_words")
    err(B(Q, 4, m - 1, m, 1, 9, rows, A, 4, rows * 4, 0, None), "quad_sys_stride_words")
    err(B(Q, 4, m, m, 1, 9, rows, A, 2, rows * 4, 0, None), "stride_words")              # short
    err(B(Q, 4, m, m, 1, 9, rows, A, 3, rows * 4, 0, None), "even")                      # odd
    err(B(Q, 4, m, m, 1, 9, rows, A, 4, rows * 4 - 2, 0, None), "sys_stride_words")      # systems overlap
    err(B(Q, 4, m, m, 1, 9, rows, A, 4, rows * 4 + 1, 0, None), "even")
    err(B(Q, 4, m, m, 1, 9, rows, A + 8, 4, rows * 4, 0, None), "16-byte alignment")
    err(B(Q, 1, 0, 0, 10000, 1100, 0, A, 2 ** 23, 0, 0, None), "LDS")

    V = L.gf2bv_xl3_expand_batch_words
    err(V(None, 4, m, m, 1, 9, rows, A, 3, rows * 3, 0), "null")
    err(V(Q, 4, m, m, 1, 9, rows, None, 3, rows * 3, 0), "null")
    err(V(Q, -1, m, m, 1, 9, rows, A, 3, rows * 3, 0), "nsys")
    err(V(Q, 4, m, m, 1, 0, rows, A, 3, rows * 3, 0), "n_lin")
    err(V(Q, 4, m, m, 1, 9, m * 10 - 1, A, 3, rows * 3, 0), "rows must")
    err(V(Q, big // rows + 1, m, m, 1, 9, rows, A, 3, rows * 3, 0), "all systems together")
    err(V(Q, 4, m, m, 0, 9, rows, A, 3, rows * 3, 0), "quad_stride_words")
    err(V(Q, 4, m - 1, m, 1, 9, rows, A, 3, rows * 3, 0), "quad_sys_stride_words")
    err(V(Q, 4, m, m, 1, 9, rows, A, 2, rows * 3, 0), "stride_words")
    err(V(Q, 4, m, m, 1, 9, rows, A, 3, rows * 3 - 1, 0), "sys_stride_words")

    S = L.gf2bv_solve_xl3_guess_words
    guess_errors(lambda nl, g, nf, a0, na: S(Q, m, 2, nl, g, nf, a0, na, 0, 0, hs))
    err(S(Q, m, 2, n, Gp, f, 0, 8, 0, 0, None), "null")
    err(S(None, m, 2, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(S(Q, m, 1, n, Gp, f, 0, 8, 0, 0, hs), "quad_stride_words")
    err(S(Q, m, 2, n, Gp, f, 0, 8, 3, 0, hs), "Invalid mode")
    err(S(Q, 0, 10000, 1100, Gp, f, 0, 8, 0, 0, hs), "LDS")
    wide = np.arange(20, dtype=np.int32)               # n' = 100: 166750 cubic columns a system, 2^20 systems
    err(S(Q, 0, 114, 120, wide.ctypes.data, 20, 0, 2 ** 20, 0, 0, (ctypes.c_void_p * 2 ** 20)()), "all assignments")

    T = L.gf2bv_solve_xl3_guess_quad_terms
    guess_errors(lambda nl, g, nf, a0, na: T(Lp, Op, Ap, Bp, m, nl, g, nf, a0, na, 0, 0, hs))
    err(T(Lp, Op, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, None), "null")
    err(T(None, Op, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(T(Lp, None, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(T(Lp, Op, None, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(T(Lp, Op, Ap, Bp, m, n, Gp, f, 0, 8, 5, 0, hs), "Invalid mode")
    dec = off.copy()
    dec[3] = dec[2] - 1
    err(T(Lp, dec.ctypes.data, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "must not decrease")
    assert not any(hs)                                 # nothing was made

    C = L.gf2bv_xl3_guess_chunk_device
    chunk = ctypes.c_int64(7)
    err(C(m, n, f, 0, None), "null")
    err(C(m, n, 12, 0, ctypes.byref(chunk)), "out of range")
    assert chunk.value == 0

    # the bindings and the extension: library errors as ValueError, shapes checked before the library sees them
    with pytest.raises(ValueError, match="repeated"):
        hip.quad_specialise_words(quad[:m], n, [1, 1])
    with pytest.raises(ValueError, match="2-D"):
        hip.solve_xl3_guess_words(quad.ravel(), n, [1])
    with pytest.raises(ValueError, match="3-D"):
        hip.xl3_expand_batch_words(quad, 9)
    with pytest.raises(ValueError, match="assignments"):
        hip.solve_xl3_guess_words(quad[:m], n, [1, 2], a0=3, na=2)
    with pytest.raises(ValueError, match="term_off"):
        hip.solve_xl3_guess_quad_terms(lin, off[:-1], ta, tb, n, [1])
    with pytest.raises(ValueError, match="nguess"):
        m4ri_solve_xl3_guess([6, 2], 3, [0, 1, 2], 0, 1, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl3_guess([6, 2], 3, [0], 0, 1, 2)
    with pytest.raises(ValueError, match="assignments"):
        m4ri_solve_xl3_guess([6, 2], 3, [0], 1, 2, 0)
    with pytest.raises(ValueError, match="n_lin - 1"):
        m4ri_solve_xl3_guess([6, 2], 3, [-1], 0, 1, 0)
    with pytest.raises(TypeError, match="sequence"):
        m4ri_solve_xl3_guess([6, 2], 3, 1, 0, 1, 0)
    with pytest.raises(TypeError, match="must be a list"):
        m4ri_solve_xl3_guess((6, 2), 3, [0], 0, 1, 0)
    assert m4ri_solve_xl3_guess([6, 2], 3, [0], 1, 0, 0) == []          # no assignment: no device is needed
    with pytest.raises(ValueError, match="repeated"):
        m4ri_solve_xl3_guess_quad_packed(lin, off, ta, tb, n, [4, 4], 0, 1, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl3_guess_quad_packed(lin, off, ta, tb, n, [4], 0, 1, 5)
    with pytest.raises(ValueError, match="one int64 per row"):
        m4ri_solve_xl3_guess_quad_packed(lin, off[:-1].copy(), ta, tb, n, [4], 0, 1, 0)


# -- 5. the front-ends: guess parsing and the scatter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
def test_guess_parsing(cls):
    q = cls([3, 4])                                    # unknowns 0..2 are x, 3..6 are y
    x, y = q.gens()
    assert q._parse_guess([]) == []
    assert q._parse_guess([5, 0]) == [5, 0]
    assert q._parse_guess([y[2], x[0], 6]) == [5, 0, 6]
    assert q._parse_guess((x[1], y[3:4])) == [1, 6]
    for bad in ([7], [-1], [1, 1], [x[0], 0], [x], [x[0] ^ x[1]], [x[0] ^ 1], [y[1] ^ y[1]], ["x"], [1.0], [True], [0, 1, 2, 3, 4, 5, 6]):
        with pytest.raises(ValueError):
            q._parse_guess(bad)
    with pytest.raises(ValueError, match="at most"):
        cls([40])._parse_guess(list(range(31)))
    with pytest.raises(ValueError, match="assignments"):
        q.solve_raw_space_xl_guess([], [0, 1], assignments=(2, 3))
    with pytest.raises(ValueError, match="degree 3"):
        list(q.solve_all_xl_guess([], [0], degree=4))
    if cls is QuadraticSystem:                         # the int front-end's shortcut: "1 = 0" under every assignment, no device asked
        assert q.solve_raw_space_xl_guess([1], [0, 5]) == [None] * 4
        assert q.solve_raw_one_xl_guess([1], [0, 5], assignments=(1, 2)) == [None] * 2
        assert list(q.solve_all_xl_guess([1], [y[0]])) == [] and q.solve_one_xl_guess([1], [y[0]]) is None


@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
def test_convert_sol_xl_guess(cls):
    n, rng = 9, random.Random(99)
    q = cls([4, 5])
    for guess in ((), (8,), (0, 1), (7, 2, 4), tuple(range(8))):
        ns = n - len(guess)
        for _ in range(4):
            a, y = rng.getrandbits(len(guess)), rng.getrandbits(ns)
            full = G.scatter(y, n, guess, a)
            raw = X.point_vector(y, ns)
            assert q.convert_sol_xl_guess(raw, guess, a) == (full & 15, full >> 4)
            for c in range(ns, xl3_cols(ns)):          # any single pair or triple coordinate flipped
                assert q.convert_sol_xl_guess(raw ^ (1 << c), guess, a) is None
    x, y = q.gens()
    assert q.convert_sol_xl_guess(X.point_vector(0b1010101, 7), [y[4], x[1]], 0b01) == (0b1001, 0b11010)
    assert set(q._xl_index_cache) >= {1, 6, 7, 8, 9}  # the index arrays, once per n'
    assert q.convert_sol_xl(X.point_vector(0x155, n)) == (5, 0x15)      # the unguessed check shares the cache


def test_no_device_no_answer():
    """without a GPU the hybrid entries say so; nothing is computed on the host"""
    if hip.device_count() > 0:
        return
    q = QuadraticSystem([4])
    (x,) = q.gens()
    with pytest.raises((RuntimeError, hip.HipError), match="no HIP device"):
        q.solve_one_xl_guess([q.mul_bit(x[0], x[1]) ^ x[2] ^ 1], [x[3]])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.quad_specialise_words(np.zeros((1, 1), dtype=np.uint64), 4, [0])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl3_guess_chunk(4, 4, 1)
