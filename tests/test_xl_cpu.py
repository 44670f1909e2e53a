"""Degree-3 XL without a GPU: the column numbering, convert_sol_xl, the host reference of tests.xl_terms, and the argument checks of the
four C-ABI entries, which are made before any device is touched."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd._internal import m4ri_solve_xl3, m4ri_solve_xl3_quad_packed
from gf2bv_amd.linsys import xl3_cols, xl3_pair_col, xl3_triple_col
from tests import xl_terms as X
from tests.quad_terms import random_terms


# -- the columns ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 13))
def test_column_functions_are_a_bijection(n):
    want = X.columns(n)                                # numbered by walking the monomials in order
    got = {frozenset([i]): i for i in range(n)}
    got.update({frozenset([i, j]): xl3_pair_col(n, i, j) for i in range(n) for j in range(i)})
    got.update({frozenset([i, j, l]): xl3_triple_col(n, i, j, l) for i in range(n) for j in range(i) for l in range(j)})
    assert got == want
    assert sorted(got.values()) == list(range(xl3_cols(n)))
    assert hip.xl3_cols(n) == xl3_cols(n) == X.cols3(n)


def test_column_counts():
    assert [xl3_cols(n) for n in (1, 2, 3, 32)] == [1, 3, 7, 5488]
    assert [hip.xl3_cols(n) for n in (1, 2, 3, 32)] == [1, 3, 7, 5488]
    assert xl3_cols(64) == 43744 and xl3_cols(24) == 2324 and xl3_cols(16) == 696


# -- convert_sol_xl -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
@pytest.mark.parametrize("n", [5, 9])
def test_convert_sol_xl(cls, n):
    rng = random.Random(50 + n)
    q = cls([n])
    for x in [0, (1 << n) - 1] + [rng.getrandbits(n) for _ in range(4)]:
        raw = X.point_vector(x, n)
        assert q.convert_sol_xl(raw) == (x,)
        for c in range(n, xl3_cols(n)):                # any single pair or triple coordinate flipped
            assert q.convert_sol_xl(raw ^ (1 << c)) is None, (x, c)
    sizes = [3, n - 3]
    q2 = cls(sizes)
    x = rng.getrandbits(n)
    assert q2.convert_sol_xl(X.point_vector(x, n)) == (x & 7, x >> 3)


@pytest.mark.parametrize("cls", [QuadraticSystem, PackedQuadraticSystem], ids=["int", "packed"])
def test_only_degree_3(cls):
    q = cls([4])
    for degree in (2, 4):
        with pytest.raises(ValueError, match="degree 3"):
            list(q.solve_all_xl([], degree=degree))
        with pytest.raises(ValueError, match="degree 3"):
            q.solve_one_xl([], degree=degree)


# -- the host reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_rows_vanish_at_a_planted_point():
    n, rng = 8, random.Random(8)
    x = rng.getrandbits(n) | 1
    eqs = X.planted_dense(rng, n, 9, [x])
    rows = X.xl3_ints(eqs, n)
    assert len(rows) == 9 * (n + 1) and rows[::n + 1] == eqs          # the first cols2 columns are QuadraticSystem's
    point = (X.point_vector(x, n) << 1) | 1
    assert all(bin(r & point).count("1") % 2 == 0 for r in rows)
    other = (X.point_vector(x ^ 2, n) << 1) | 1
    assert any(bin(r & other).count("1") % 2 for r in rows)
    assert all(r & 1 == 0 for k, r in enumerate(rows) if k % (n + 1))                  # the constant of x_k f is 0
    # x_0 (1 + x_0 + x_1 + x_1 x_2) = x_0 + x_0 + x_0 x_1 + x_0 x_1 x_2
    f = 1 | 1 << 1 | 1 << 2 | 1 << (1 + xl3_pair_col(n, 2, 1))
    assert X.xl3_ints([f], n)[1] == 1 << (1 + xl3_pair_col(n, 1, 0)) | 1 << (1 + xl3_triple_col(n, 2, 1, 0))


# -- the C ABI: GF2BV_ERR_ARG before any device --------------------------------------------------------------------------------------------
def test_entries_check_arguments_before_device_use():
    L = hip.lib()
    n, m = 12, 5                                       # 78 quadratic columns (2 words), 298 cubic ones (5 words), 65 live rows
    rows = 300
    quad = np.zeros((m + 1, 2), dtype=np.uint64)
    aug = np.zeros((rows + 1, 6), dtype=np.uint64)
    Q, A = quad.ctypes.data, aug.ctypes.data
    A += -A % 16
    lin, off, ta, tb = random_terms(random.Random(3), n, m)
    Lp, Op, Ap, Bp = lin.ctypes.data, off.ctypes.data, ta.ctypes.data, tb.ctypes.data
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)
    big = 2 ** 31 - 64

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    D = L.gf2bv_xl3_expand_device
    err(D(None, m, 2, n, rows, A, 6, 0, None), "null")
    err(D(Q, m, 2, n, rows, None, 6, 0, None), "null")
    err(D(Q, m, 2, 0, rows, A, 6, 0, None), "n_lin")
    err(D(Q, m, 2, 3000, big - 1, A, 2 ** 27, 0, None), "n_lin")                      # 4.5e9 cubic columns
    err(D(Q, -1, 2, n, rows, A, 6, 0, None), "m(n_lin + 1)")
    err(D(Q, big // 13 + 1, 2, n, big - 1, A, 6, 0, None), "m(n_lin + 1)")
    err(D(Q, m, 2, n, big, A, 6, 0, None), "rows must")
    err(D(Q, m, 2, n, m * (n + 1) - 1, A, 6, 0, None), "rows must")
    err(D(Q, m, 1, n, rows, A, 6, 0, None), "quad_stride_words")
    err(D(Q, m, 2, n, rows, A, 5, 0, None), "stride")                                 # odd
    err(D(Q, m, 2, n, rows, A, 4, 0, None), "stride")                                 # short
    err(D(Q, m, 2, n, rows, A + 8, 6, 0, None), "16-byte alignment")
    err(D(Q, 0, 10000, 1100, 0, A, 2 ** 23, 0, None), "LDS")                          # a 75 KiB source row

    W = L.gf2bv_xl3_expand_words
    err(W(None, m, 2, n, rows, A, 5, 0), "null")
    err(W(Q, m, 2, n, rows, None, 5, 0), "null")
    err(W(Q, m, 2, 0, rows, A, 5, 0), "n_lin")
    err(W(Q, m, 2, 3000, big - 1, A, 2 ** 27, 0), "n_lin")
    err(W(Q, big // 13 + 1, 2, n, big - 1, A, 5, 0), "m(n_lin + 1)")
    err(W(Q, m, 2, n, big, A, 5, 0), "rows must")
    err(W(Q, m, 2, n, m * (n + 1) - 1, A, 5, 0), "rows must")
    err(W(Q, m, 1, n, rows, A, 5, 0), "quad_stride_words")
    err(W(Q, m, 2, n, rows, A, 4, 0), "stride")
    err(W(Q, 0, 10000, 1100, 0, A, 2 ** 23, 0), "LDS")

    S = L.gf2bv_solve_xl3_words
    err(S(Q, m, 2, n, 0, 0, None), "null")
    err(S(None, m, 2, n, 0, 0, H), "null")
    err(S(Q, m, 2, 0, 0, 0, H), "n_lin")
    err(S(Q, m, 2, 3000, 0, 0, H), "n_lin")
    err(S(Q, big // 13 + 1, 2, n, 0, 0, H), "m(n_lin + 1)")
    err(S(Q, m, 1, n, 0, 0, H), "quad_stride_words")
    err(S(Q, 0, 10000, 1100, 0, 0, H), "LDS")
    err(S(Q, m, 2, n, 3, 0, H), "Invalid mode")

    T = L.gf2bv_solve_xl3_quad_terms
    err(T(Lp, Op, Ap, Bp, m, n, 0, 0, None), "null")
    err(T(None, Op, Ap, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, None, Ap, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, Op, None, Bp, m, n, 0, 0, H), "null")
    err(T(Lp, Op, Ap, None, m, n, 0, 0, H), "null")
    err(T(Lp, Op, Ap, Bp, m, 0, 0, 0, H), "n_lin")
    err(T(Lp, Op, Ap, Bp, 0, 3000, 0, 0, H), "n_lin")
    many = np.zeros(big // 1001 + 2, dtype=np.int64)                                   # (offsets the check may walk: no product anywhere)
    err(T(Lp, many.ctypes.data, Ap, Bp, big // 1001 + 1, 1000, 0, 0, H), "m(n_lin + 1)")
    err(T(Lp, Op, Ap, Bp, 0, 1100, 0, 0, H), "LDS")
    err(T(Lp, Op, Ap, Bp, m, n, 3, 0, H), "Invalid mode")
    bad0, dec = off.copy(), off.copy()
    bad0[0] = 1
    dec[3] = dec[2] - 1
    err(T(Lp, bad0.ctypes.data, Ap, Bp, m, n, 0, 0, H), "start at 0")
    err(T(Lp, dec.ctypes.data, Ap, Bp, m, n, 0, 0, H), "must not decrease")
    assert not h.value                                 # nothing was made

    # the bindings and the extension: library errors as ValueError, shapes checked before the library sees them
    with pytest.raises(ValueError, match="quad_stride_words"):
        hip.xl3_expand_words(quad[:, :1], n)
    with pytest.raises(ValueError, match="rows must"):
        hip.xl3_expand_words(quad, n, rows=3)
    with pytest.raises(ValueError, match="2-D"):
        hip.solve_xl3_words(quad.ravel(), n)
    with pytest.raises(ValueError, match="term_off"):
        hip.solve_xl3_quad_terms(lin, off[:-1], ta, tb, n)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl3([6, 2], 3, 2)
    with pytest.raises(ValueError, match="n_lin"):
        m4ri_solve_xl3([6, 2], 0, 0)
    with pytest.raises(TypeError, match="must be a list"):
        m4ri_solve_xl3((6, 2), 3, 0)
    with pytest.raises(TypeError, match="integers"):
        m4ri_solve_xl3([6, "x"], 3, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        m4ri_solve_xl3_quad_packed(lin, off[:-1].copy(), ta, tb, n, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_xl3_quad_packed(lin, off, ta, tb, n, 5)


def test_no_device_no_answer():
    """without a GPU the XL entries say so; nothing is computed on the host"""
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    q = QuadraticSystem([4])
    (x,) = q.gens()
    with pytest.raises(RuntimeError, match="no HIP device"):
        q.solve_one_xl([q.mul_bit(x[0], x[1]) ^ x[2] ^ 1])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl3_expand_words(np.zeros((1, 1), dtype=np.uint64), 4)
