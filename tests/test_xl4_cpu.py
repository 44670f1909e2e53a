"""Degree-4 XL without a GPU: the column numbering, convert_sol_xl4, the host reference of tests.xl4_terms, the rank deficit of the
multiplied rows, the kernel's quartic root on the host, gf2bv_xl4_guess_chunk, and the argument checks of every xl4 C-ABI entry, which
are made before any device is touched."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd._internal import m4ri_solve_xl4, m4ri_solve_xl4_guess, m4ri_solve_xl4_guess_quad_packed, m4ri_solve_xl4_quad_packed
from gf2bv_amd.linsys import xl3_cols, xl3_pair_col, xl3_triple_col, xl4_cols, xl4_quad_col
from oracle import gf2_oracle as O
from tests import xl4_terms as X4
from tests import xl_terms as X
from tests.quad_terms import random_terms


# -- the columns ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 13))
def test_column_functions_are_a_bijection(n):
    want = X4.columns(n)                               # numbered by walking the monomials in order
    got = {frozenset([i]): i for i in range(n)}
    got.update({frozenset([i, j]): xl3_pair_col(n, i, j) for i in range(n) for j in range(i)})
    got.update({frozenset([i, j, l]): xl3_triple_col(n, i, j, l) for i in range(n) for j in range(i) for l in range(j)})
    got.update({frozenset([i, j, l, p]): xl4_quad_col(n, i, j, l, p) for i in range(n) for j in range(i) for l in range(j) for p in range(l)})
    assert got == want
    assert sorted(got.values()) == list(range(xl4_cols(n)))
    assert hip.xl4_cols(n) == xl4_cols(n) == X4.cols4(n)
    assert all(X4.column_of(mono, n) == c for mono, c in want.items())
    assert list(want.values())[:xl3_cols(n)] == list(X.columns(n).values())      # the first cols3 columns are degree 3's


def test_column_counts():
    assert [xl4_cols(n) for n in (1, 2, 3, 4, 5)] == [1, 3, 7, 15, 30]
    assert [hip.xl4_cols(n) for n in (12, 14, 16, 32)] == [793, 1470, 2516, 41448]
    assert X4.rows_per_equation(32) == 529 and X4.rows_per_equation(1) == 2


# -- convert_sol_xl4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
@pytest.mark.parametrize("n", [5, 8])
def test_convert_sol_xl4(cls, n):
    rng = random.Random(40 + n)
    q = cls([n])
    for x in [0, (1 << n) - 1] + [rng.getrandbits(n) for _ in range(3)]:
        raw = X4.point_vector(x, n)
        assert q.convert_sol_xl4(raw) == (x,)
        for c in range(n, xl4_cols(n)):                # any single pair, triple or quadruple coordinate flipped
            assert q.convert_sol_xl4(raw ^ (1 << c)) is None, (x, c)
    q2 = cls([3, n - 3])
    x = rng.getrandbits(n)
    assert q2.convert_sol_xl4(X4.point_vector(x, n)) == (x & 7, x >> 3)
    for guess in ((), (n - 1,), (0, 2)):               # the hybrid form: the check over the remaining unknowns, then the scatter
        ns = n - len(guess)
        y, a = rng.getrandbits(ns), rng.getrandbits(len(guess))
        from tests.xl_guess_terms import scatter       # noqa: PLC0415
        raw = X4.point_vector(y, ns)
        assert q.convert_sol_xl4_guess(raw, guess, a) == (scatter(y, n, guess, a),)
        for c in range(ns, xl4_cols(ns)):
            assert q.convert_sol_xl4_guess(raw ^ (1 << c), guess, a) is None


@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
def test_xl4_methods_take_no_degree(cls):
    q = cls([4])
    with pytest.raises(TypeError):
        list(q.solve_all_xl4([], degree=4))
    with pytest.raises(TypeError):
        list(q.solve_all_xl4_guess([], [0], degree=4))
    with pytest.raises(ValueError, match="assignments"):
        q.solve_raw_space_xl4_guess([], [0, 1], assignments=(2, 3))
    if cls is QuadraticSystem:                         # the int front-end's shortcut: "1 = 0", no device asked
        assert q.solve_raw_one_xl4([1]) is None and q.solve_raw_space_xl4([1]) is None
        assert list(q.solve_all_xl4([1])) == [] and q.solve_one_xl4([1]) is None
        assert q.solve_raw_space_xl4_guess([1], [0, 3]) == [None] * 4
        assert list(q.solve_all_xl4_guess([1], [2])) == [] and q.solve_one_xl4_guess([1], [2]) is None


# -- the host reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_rows_vanish_at_a_planted_point():
    n, rng = 8, random.Random(8)
    x = rng.getrandbits(n) | 1
    eqs = X.planted_dense(rng, n, 7, [x])
    rows, per = X4.xl4_ints(eqs, n), X4.rows_per_equation(n)
    assert per == 37 and len(rows) == 7 * per and rows[::per] == eqs              # the first cols2 columns are QuadraticSystem's
    cubic = X.xl3_ints(eqs, n)
    assert [rows[e * per + k] for e in range(7) for k in range(n + 1)] == cubic   # f and x_k f: degree 3's rows, no quadruple
    point = (X4.point_vector(x, n) << 1) | 1
    assert all(bin(r & point).count("1") % 2 == 0 for r in rows)
    other = (X4.point_vector(x ^ 2, n) << 1) | 1
    assert any(bin(r & other).count("1") % 2 for r in rows)
    assert all(r & 1 == 0 for k, r in enumerate(rows) if k % per)                 # the constant of every product is 0
    # x_2 x_0 (1 + x_0 + x_1 + x_1 x_3) = x_2 x_0 + x_2 x_0 + x_2 x_1 x_0 + x_3 x_2 x_1 x_0
    f = 1 | 1 << 1 | 1 << 2 | 1 << (1 + xl3_pair_col(n, 3, 1))
    got = X4.xl4_ints([f], n)[1 + n + 2 * 1 // 2 + 0]                             # offset 1 + n + C(2,2) + 0
    assert got == 1 << (1 + xl3_triple_col(n, 2, 1, 0)) | 1 << (1 + xl4_quad_col(n, 3, 2, 1, 0))
    aug = X4.xl4_aug(eqs, n, len(rows) + 3, O.words_for(xl4_cols(n)) + 1)         # the words form the GPU tests compare with
    assert np.array_equal(aug[:len(rows), :-1], O.eqs_to_aug(rows, xl4_cols(n))) and not aug[len(rows):].any() and not aug[:, -1].any()
    assert np.array_equal(X4.xl4_aug(eqs, n, len(rows) + 3, aug.shape[1], table=False), aug)


def test_rank_is_rows_minus_the_relations():
    """n = 16, m = 19: before saturation the rank is rows - m - C(m,2), because f_i f_i = f_i and f_i f_j = f_j f_i"""
    n, m = 16, 19
    rng = random.Random(400 * n + m)
    eqs = X.planted_dense(rng, n, m, [rng.getrandbits(n)])
    aug, rows, cols4 = X4.quartic_aug(eqs, n)
    res = O.solve_words(aug, rows, cols4, 1)
    assert (rows, cols4) == (2603, 2516)
    assert (res["status"], res["rank"], res["dim"]) == (0, 2603 - 19 - 19 * 18 // 2, 103) and res["rank"] == 2413


# -- the kernel's quartic root, compiled for the host ---------------------------------------------------------------------------------------
def test_quartic_root_against_integer_search():
    """every u below 300000 (i up to 53), and u = C(i,4) - 2 .. C(i,4) + 2 for every i with C(i,4) below 2^33 (i = 5 .. 675)"""
    root = hip.lib().gf2bv_xl4_quartic_root
    c4 = lambda i: i * (i - 1) * (i - 2) * (i - 3) // 24                           # noqa: E731
    i = 3
    for u in range(300000):
        while c4(i + 1) <= u:
            i += 1
        assert root(u) == i, u
    i = 5                                              # (C(5,4) = 5: the neighbourhood stays at u >= 0)
    while c4(i) < 2 ** 33:
        for u in range(c4(i) - 2, c4(i) + 3):
            assert root(u) == (i if u >= c4(i) else i - 1), (i, u)
        i += 1
    assert i == 676 and root(-1) == -1


# -- the chunk ------------------------------------------------------------------------------------------------------------------------------
def test_guess_chunk():
    m, n, f = 92, 40, 8                                # n' = 32: 92 * 529 = 48668 rows of 648 words and 92 rows of 10 words a system
    per = 8 * (48668 * 648 + 92 * 10)
    assert hip.xl4_guess_chunk(m, n, f, 4 * per - 1) == 0
    assert hip.xl4_guess_chunk(m, n, f, 4 * per) == 1
    assert hip.xl4_guess_chunk(m, n, f, 4 * 200 * per + 5) == 200
    assert hip.xl4_guess_chunk(m, n, f, 1 << 50) == 256            # capped at 2^f
    assert hip.xl4_guess_chunk(m, n, 0, 1 << 60) == 1
    last = 0
    for free in range(0, 40 * per, per // 3):          # a pure function of its arguments, monotone in the memory
        c = hip.xl4_guess_chunk(m, n, f, free)
        assert c >= last and c == hip.xl4_guess_chunk(m, n, f, free)
        last = c
    assert last == 9
    assert hip.xl4_guess_chunk(10, 60, 30, 1 << 60) == (2 ** 31 - 65) // max(10 * 466, xl4_cols(30))       # rows of all systems < 2^31 - 64
    for bad in ((m, 0, 0, 1), (m, n, -1, 1), (m, n, n, 1), (m, 40, 31, 1), (-1, n, f, 1), (m, n, f, -1), (0, 600, 0, 1)):
        with pytest.raises(ValueError):
            hip.xl4_guess_chunk(*bad)


# -- the C ABI: GF2BV_ERR_ARG before any device --------------------------------------------------------------------------------------------
def test_entries_check_arguments_before_device_use():
    L = hip.lib()
    n, m, f = 12, 5, 3                                 # 78 quadratic columns (2 words), 793 quartic ones (13 words), 5 * 79 = 395 live rows
    rows = 800
    quad = np.zeros((4 * m + 1, 2), dtype=np.uint64)
    aug = np.zeros((rows + 1, 14), dtype=np.uint64)
    Q, A = quad.ctypes.data, aug.ctypes.data
    A += -A % 16
    lin, off, ta, tb = random_terms(random.Random(3), n, m)
    Lp, Op, Ap, Bp = lin.ctypes.data, off.ctypes.data, ta.ctypes.data, tb.ctypes.data
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)
    hs = (ctypes.c_void_p * 8)()
    guess = np.array([3, 11, 0], dtype=np.int32)
    Gp = guess.ctypes.data
    arr = lambda *v: np.array(v, dtype=np.int32)       # noqa: E731
    big = 2 ** 31 - 64

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    D = L.gf2bv_xl4_expand_device
    err(D(None, m, 2, n, rows, A, 14, 0, None), "null")
    err(D(Q, m, 2, n, rows, None, 14, 0, None), "null")
    err(D(Q, m, 2, 0, rows, A, 14, 0, None), "n_lin")
    err(D(Q, m, 2, 600, big - 1, A, 2 ** 27, 0, None), "C(n_lin,4)")                   # 5.4e9 quartic columns
    err(D(Q, -1, 2, n, rows, A, 14, 0, None), "m(1 + n_lin + C(n_lin,2))")
    err(D(Q, big // 79 + 1, 2, n, big - 1, A, 14, 0, None), "m(1 + n_lin + C(n_lin,2))")
    err(D(Q, m, 2, n, big, A, 14, 0, None), "rows must")
    err(D(Q, m, 2, n, m * 79 - 1, A, 14, 0, None), "rows must")                        # degree 3's m(n + 1) rows are not enough
    err(D(Q, m, 1, n, rows, A, 14, 0, None), "quad_stride_words")
    err(D(Q, m, 2, n, rows, A, 13, 0, None), "stride")                                 # odd
    err(D(Q, m, 2, n, rows, A, 12, 0, None), "stride")                                 # short
    err(D(Q, m, 2, n, rows, A + 8, 14, 0, None), "16-byte alignment")

    W = L.gf2bv_xl4_expand_words
    err(W(None, m, 2, n, rows, A, 13, 0), "null")
    err(W(Q, m, 2, n, rows, None, 13, 0), "null")
    err(W(Q, m, 2, 0, rows, A, 13, 0), "n_lin")
    err(W(Q, m, 2, 600, big - 1, A, 2 ** 27, 0), "C(n_lin,4)")
    err(W(Q, big // 79 + 1, 2, n, big - 1, A, 13, 0), "m(1 + n_lin + C(n_lin,2))")
    err(W(Q, m, 2, n, big, A, 13, 0), "rows must")
    err(W(Q, m, 2, n, m * 79 - 1, A, 13, 0), "rows must")
    err(W(Q, m, 1, n, rows, A, 13, 0), "quad_stride_words")
    err(W(Q, m, 2, n, rows, A, 12, 0), "stride")

    S = L.gf2bv_solve_xl4_words
    err(S(Q, m, 2, n, 0, 0, None), "null")
    err(S(None, m, 2, n, 0, 0, H), "null")
    err(S(Q, m, 2, 0, 0, 0, H), "n_lin")
    err(S(Q, m, 2, 600, 0, 0, H), "C(n_lin,4)")
    err(S(Q, big // 79 + 1, 2, n, 0, 0, H), "m(1 + n_lin + C(n_lin,2))")
    err(S(Q, m, 1, n, 0, 0, H), "quad_stride_words")
    err(S(Q, m, 2, n, 3, 0, H), "Invalid mode")

    T = L.gf2bv_solve_xl4_quad_terms
    err(T(Lp, Op, Ap, Bp, m, n, 0, 0, None), "null")
    err(T(None, Op, Ap, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, None, Ap, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, Op, None, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, Op, Ap, None, m, n, 0, 0, H), "null")
    err(T(Lp, Op, Ap, Bp, m, 0, 0, 0, H), "n_lin")
    err(T(Lp, Op, Ap, Bp, 0, 600, 0, 0, H), "C(n_lin,4)")
    err(T(Lp, Op, Ap, Bp, m, n, 3, 0, H), "Invalid mode")
    bad0, dec = off.copy(), off.copy()
    bad0[0] = 1
    dec[3] = dec[2] - 1
    err(T(Lp, bad0.ctypes.data, Ap, Bp, m, n, 0, 0, H), "start at 0")
    err(T(Lp, dec.ctypes.data, Ap, Bp, m, n, 0, 0, H), "must not decrease")
    assert not h.value                                 # nothing was made

    def guess_errors(call):
        """what every entry with a guess refuses: call(n_lin, guess pointer, nguess, a0, na)"""
        err(call(0, Gp, 0, 0, 1), "n_lin")
        err(call(n, None, f, 0, 8), "null")
        err(call(n, Gp, -1, 0, 1), "nguess")
        err(call(n, Gp, n, 0, 1), "nguess")
        err(call(40, Gp, 31, 0, 1), "nguess")
        err(call(n, arr(3, 12, 0).ctypes.data, f, 0, 8), "0 .. n_lin - 1")
        err(call(n, arr(3, 0, 3).ctypes.data, f, 0, 8), "repeated")
        err(call(n, Gp, f, -1, 2), "assignments")
        err(call(n, Gp, f, 0, -1), "assignments")
        err(call(n, Gp, f, 2, 7), "assignments")

    brow = 260                                         # 4 systems of m rows over 9 unknowns: 5 * 46 = 230 live rows, 255 columns (4 words)
    B = L.gf2bv_xl4_expand_batch_device
    err(B(None, 4, m, m, 1, 9, brow, A, 6, brow * 6, 0, None), "null")
    err(B(Q, 4, m, m, 1, 9, brow, None, 6, brow * 6, 0, None), "null")
    err(B(Q, -1, m, m, 1, 9, brow, A, 6, brow * 6, 0, None), "nsys")
    err(B(Q, 4, m, m, 1, 0, brow, A, 6, brow * 6, 0, None), "n_lin")
    err(B(Q, 4, m, -1, 1, 9, brow, A, 6, brow * 6, 0, None), "m(1 + n_lin + C(n_lin,2))")
    err(B(Q, 4, m, m, 1, 9, m * 46 - 1, A, 6, brow * 6, 0, None), "rows must")
    err(B(Q, big // brow + 1, m, m, 1, 9, brow, A, 6, brow * 6, 0, None), "all systems together")
    err(B(Q, 4, m, m, 0, 9, brow, A, 6, brow * 6, 0, None), "quad_stride_words")
    err(B(Q, 4, m - 1, m, 1, 9, brow, A, 6, brow * 6, 0, None), "quad_sys_stride_words")
    err(B(Q, 4, m, m, 1, 9, brow, A, 2, brow * 6, 0, None), "stride_words")            # short: degree 3's stride
    err(B(Q, 4, m, m, 1, 9, brow, A, 5, brow * 6, 0, None), "even")                    # odd
    err(B(Q, 4, m, m, 1, 9, brow, A, 6, brow * 6 - 2, 0, None), "sys_stride_words")    # systems overlap
    err(B(Q, 4, m, m, 1, 9, brow, A, 6, brow * 6 + 1, 0, None), "even")
    err(B(Q, 4, m, m, 1, 9, brow, A + 8, 6, brow * 6, 0, None), "16-byte alignment")

    V = L.gf2bv_xl4_expand_batch_words
    err(V(None, 4, m, m, 1, 9, brow, A, 4, brow * 4, 0), "null")
    err(V(Q, 4, m, m, 1, 9, brow, None, 4, brow * 4, 0), "null")
    err(V(Q, -1, m, m, 1, 9, brow, A, 4, brow * 4, 0), "nsys")
    err(V(Q, 4, m, m, 1, 0, brow, A, 4, brow * 4, 0), "n_lin")
    err(V(Q, 4, m, m, 1, 9, m * 46 - 1, A, 4, brow * 4, 0), "rows must")
    err(V(Q, big // brow + 1, m, m, 1, 9, brow, A, 4, brow * 4, 0), "all systems together")
    err(V(Q, 4, m, m, 0, 9, brow, A, 4, brow * 4, 0), "quad_stride_words")
    err(V(Q, 4, m - 1, m, 1, 9, brow, A, 4, brow * 4, 0), "quad_sys_stride_words")
    err(V(Q, 4, m, m, 1, 9, brow, A, 3, brow * 4, 0), "stride_words")
    err(V(Q, 4, m, m, 1, 9, brow, A, 4, brow * 4 - 1, 0), "sys_stride_words")

    G = L.gf2bv_solve_xl4_guess_words
    guess_errors(lambda nl, g, nf, a0, na: G(Q, m, 2, nl, g, nf, a0, na, 0, 0, hs))
    err(G(Q, m, 2, n, Gp, f, 0, 8, 0, 0, None), "null")
    err(G(None, m, 2, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(G(Q, m, 1, n, Gp, f, 0, 8, 0, 0, hs), "quad_stride_words")
    err(G(Q, m, 2, n, Gp, f, 0, 8, 3, 0, hs), "Invalid mode")
    wide = np.arange(20, dtype=np.int32)               # n' = 40: 102090 quartic columns a system, 2^20 systems
    err(G(Q, 0, 30, 60, wide.ctypes.data, 20, 0, 2 ** 20, 0, 0, (ctypes.c_void_p * 2 ** 20)()), "all assignments")

    U = L.gf2bv_solve_xl4_guess_quad_terms
    guess_errors(lambda nl, g, nf, a0, na: U(Lp, Op, Ap, Bp, m, nl, g, nf, a0, na, 0, 0, hs))
    err(U(Lp, Op, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, None), "null")
    err(U(None, Op, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(U(Lp, Op, Ap, Bp, m, n, Gp, f, 0, 8, 5, 0, hs), "Invalid mode")
    err(U(Lp, dec.ctypes.data, Ap, Bp, m, n, Gp, f, 0, 8, 0, 0, hs), "must not decrease")
    assert not any(hs)                                 # nothing was made

    C = L.gf2bv_xl4_guess_chunk_device
    chunk = ctypes.c_int64(7)
    err(C(m, n, f, 0, None), "null")
    err(C(m, n, 12, 0, ctypes.byref(chunk)), "out of range")
    assert chunk.value == 0

    # the bindings and the extension: library errors as ValueError, shapes checked before the library sees them
    with pytest.raises(ValueError, match="quad_stride_words"):
        hip.xl4_expand_words(quad[:, :1], n)
    with pytest.raises(ValueError, match="rows must"):
        hip.xl4_expand_words(quad, n, rows=3)
    with pytest.raises(ValueError, match="2-D"):
        hip.solve_xl4_words(quad.ravel(), n)
    with pytest.raises(ValueError, match="term_off"):
        hip.solve_xl4_quad_terms(lin, off[:-1], ta, tb, n)
    with pytest.raises(ValueError, match="3-D"):
        hip.xl4_expand_batch_words(quad, 9)
    with pytest.raises(ValueError, match="assignments"):
        hip.solve_xl4_guess_words(quad[:m], n, [1, 2], a0=3, na=2)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl4([6, 2], 3, 2)
    with pytest.raises(ValueError, match="n_lin"):
        m4ri_solve_xl4([6, 2], 0, 0)
    with pytest.raises(TypeError, match="must be a list"):
        m4ri_solve_xl4((6, 2), 3, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        m4ri_solve_xl4_quad_packed(lin, off[:-1].copy(), ta, tb, n, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl4_quad_packed(lin, off, ta, tb, n, 5)
    with pytest.raises(ValueError, match="nguess"):
        m4ri_solve_xl4_guess([6, 2], 3, [0, 1, 2], 0, 1, 0)
    with pytest.raises(ValueError, match="assignments"):
        m4ri_solve_xl4_guess([6, 2], 3, [0], 1, 2, 0)
    assert m4ri_solve_xl4_guess([6, 2], 3, [0], 1, 0, 0) == []          # no assignment: no device is needed
    with pytest.raises(ValueError, match="repeated"):
        m4ri_solve_xl4_guess_quad_packed(lin, off, ta, tb, n, [4, 4], 0, 1, 0)


def test_no_device_no_answer():
    """without a GPU the degree-4 entries say so; nothing is computed on the host"""
    if hip.device_count() > 0:
        return
    q = QuadraticSystem([4])
    (x,) = q.gens()
    zeros = [q.mul_bit(x[0], x[1]) ^ x[2] ^ 1]
    with pytest.raises(RuntimeError, match="no HIP device"):
        q.solve_one_xl4(zeros)
    with pytest.raises((RuntimeError, hip.HipError), match="no HIP device"):
        q.solve_one_xl4_guess(zeros, [x[3]])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_expand_words(np.zeros((1, 1), dtype=np.uint64), 4)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_expand_batch_words(np.zeros((1, 1, 1), dtype=np.uint64), 4)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_guess_chunk(4, 4, 1)
