"""Degree-4 XL on cubic equations without a GPU: the set-based reference of tests/cubic_xl4_terms.py itself (row order, columns, planted
points), the rank facts of the filtered register that the front-end's documentation quotes, convert_sol_xl4, and every argument
check of the four new entries."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import PackedCubicSystem, hip
from gf2bv_amd._internal import m4ri_solve_xl4_cubic_packed
from gf2bv_amd.linsys import xl3_cols, xl4_cols
from tests import xl4_terms as X4
from tests.cubic_terms import REGISTER_12, IntBasis, poly_int, poly_value, random_cubic_terms, row_polys
from tests.cubic_xl4_terms import poly_int4, register_polys, xl4_cubic_eqs, xl4_cubic_polys

M = lambda *v: frozenset(v)                            # noqa: E731  (a monomial)


def test_helper_row_order_and_columns():
    n = 6
    col = X4.columns(n)                                # the walked table of every monomial of degree 1..4
    assert len(col) == xl4_cols(n) == 56
    for mono, c in col.items():
        assert poly_int4(frozenset([mono]), n) == 1 << (1 + c)
    assert poly_int4(frozenset([M()]), n) == 1
    p = frozenset([M(), M(0), M(2, 1), M(4, 3, 2), M(5, 4, 1)])
    rows = xl4_cubic_polys(n, [p, frozenset([M(3)])])
    assert len(rows) == 2 * (n + 1) and rows[0] == p and rows[n + 1] == frozenset([M(3)])
    assert rows[1 + 2] == frozenset([M(2), M(2, 0), M(2, 1), M(4, 3, 2), M(5, 4, 2, 1)])          # x_2 p: x_2 x_2 = x_2
    assert rows[1 + 0] == frozenset([M(2, 1, 0), M(4, 3, 2, 0), M(5, 4, 1, 0)])                    # x_0 p: 1 x_0 ^ x_0 x_0 = 0
    assert rows[n + 1 + 1 + 3] == frozenset([M(3)]) and rows[n + 1 + 1 + 5] == frozenset([M(5, 3)])
    eqs = xl4_cubic_eqs(n, [p])
    assert eqs[0] == 1 | 1 << 1 | 1 << (1 + col[M(2, 1)]) | 1 << (1 + col[M(4, 3, 2)]) | 1 << (1 + col[M(5, 4, 1)])
    assert eqs[1 + 2] == sum(1 << (1 + col[m]) for m in rows[3])
    assert eqs[0] == poly_int(p, n)                    # degree <= 3: the cubic columns come first


@pytest.mark.parametrize("n", [5, 9])
def test_reference_rows_vanish_at_the_planted_point(n):
    rng = random.Random(n)
    point = rng.getrandbits(n) | 1
    terms = random_cubic_terms(rng, n, 8)
    polys = [p ^ frozenset([M()]) if poly_value(p, point) else p for p in row_polys(n, *terms)]
    raw = X4.point_vector(point, n)
    rows = xl4_cubic_polys(n, polys)
    assert any(len(m) == 4 for r in rows for m in r)
    for r, e in zip(rows, xl4_cubic_eqs(n, polys)):
        assert poly_value(r, point) == 0
        assert (bin((e >> 1) & raw).count("1") + e) & 1 == 0


@pytest.mark.parametrize("secret", [0x52F, 0x3A1])
def test_register_rank_facts(secret):
    """n = 12, 793 quartic columns: 59 / 60 / 62 outputs give 767 / 780 / 806 rows of rank 767 / 780 / 793 -- dimension 26 / 13 / 0 --
    where plain linearisation over the 298 cubic columns needs 298 outputs"""
    n = 12
    cols4 = xl4_cols(n)
    assert cols4 == 793 and xl3_cols(n) == 298
    eqs = xl4_cubic_eqs(n, register_polys(secret, count=62, **REGISTER_12))
    assert len(eqs) == 62 * 13
    raw = X4.point_vector(secret, n)
    basis, dims = IntBasis(), {}
    for r, e in enumerate(eqs):
        assert (bin((e >> 1) & raw).count("1") + e) & 1 == 0
        basis.add(e >> 1)
        if (r + 1) % 13 == 0:
            dims[(r + 1) // 13] = cols4 - len(basis)
    assert (dims[59], dims[60], dims[62]) == (26, 13, 0)
    assert dims[20] == cols4 - 20 * 13 and dims[59] == cols4 - 59 * 13      # the rows stay independent until the columns run out
    assert dims[61] == (0 if secret == 0x52F else 1)


def test_convert_sol_xl4():
    p = PackedCubicSystem([3, 5])
    n = 8
    for x in (0, 0xFF, 0xB5, 0x0F, 0x80):
        raw = X4.point_vector(x, n)
        assert p.convert_sol_xl4(raw) == (x & 7, x >> 3)
    raw = X4.point_vector(0xF3, n)
    cols3, cols4 = xl3_cols(n), xl4_cols(n)
    assert p.convert_sol_xl4(raw ^ (1 << (cols4 - 1))) is None                       # the quadruple (7, 6, 5, 4), set at this point
    assert p.convert_sol_xl4(raw ^ (1 << cols3)) is None                             # the quadruple (3, 2, 1, 0), clear at this point
    assert p.convert_sol_xl4(raw ^ (1 << (cols3 - 1))) is None and p.convert_sol_xl4(raw ^ (1 << n)) is None      # a triple, a pair
    assert p.convert_sol(raw & ((1 << cols3) - 1)) == (3, 0x1E)                      # the cubic part is convert_sol's point
    with pytest.raises(AssertionError, match="Invalid solution"):
        p.convert_sol_xl4(1 << cols4)


def test_entries_check_arguments_before_device_use():
    """every GF2BV_ERR_ARG case of the four entries returns 1 with its message, on a machine without a GPU too"""
    L = hip.lib()
    n, m = 9, 6                                        # 129 cubic columns (3 words), 255 quartic ones (4 words), 60 live rows
    w3, wt, live = 3, 4, m * (n + 1)
    rows = live + 2
    cubic = np.zeros((m, w3), dtype=np.uint64)
    aug = np.zeros((rows + 1, wt), dtype=np.uint64)
    C, A = cubic.ctypes.data, aug.ctypes.data
    A += -A % 16
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    D, W, S, T = L.gf2bv_xl4_cubic_expand_device, L.gf2bv_xl4_cubic_expand_words, L.gf2bv_solve_xl4_cubic_words, L.gf2bv_solve_xl4_cubic_terms
    big_m = (1 << 31) // (n + 1)
    # the shape rules the three entries on expanded rows share
    for f, tail in ((D, lambda rows=rows: (rows, A, wt, 0, None)), (W, lambda rows=rows: (rows, A, wt, 0)), (S, lambda rows=0: (0, 0, H))):
        err(f(None, m, w3, n, *tail()), "null")
        err(f(C, m, w3, 0, *tail()), "n_lin")
        err(f(C, m, w3, 500, *tail()), "C(n_lin,4) below 2^31 - 64")              # cols4 >= 2^31 - 64
        err(f(C, -1, w3, n, *tail()), "m(n_lin + 1)")
        err(f(C, big_m, w3, n, *tail()), "m(n_lin + 1) must stay below")
        err(f(C, m, w3 - 1, n, *tail()), "cubic_stride_words")
        err(f(C, m, 9000, 147, *tail(m * 148)), "cubic row of this n_lin does not fit")  # W3 = 8275 words: 66200 bytes of LDS
        err(f(C, m, 8106, 146, *tail(m * 147)), "cubic_stride_words")                    # n_lin = 146 (W3 = 8107) is past the LDS check
    err(D(C, m, w3, n, rows, None, wt, 0, None), "null")
    err(D(C, m, w3, n, live - 1, A, wt, 0, None), "rows must be at least m(n_lin + 1)")
    err(D(C, m, w3, n, rows, A, wt - 2, 0, None), "stride_words covering cols+1 bits")
    err(D(C, m, w3, n, rows, A, wt + 1, 0, None), "even stride_words")
    err(D(C, m, w3, n, rows, A + 8, wt, 0, None), "16-byte alignment")
    err(W(C, m, w3, n, rows, None, wt, 0), "null")
    err(W(C, m, w3, n, live - 1, A, wt, 0), "rows must be at least m(n_lin + 1)")
    err(W(C, m, w3, n, rows, A, wt - 1, 0), "stride_words does not cover")
    err(S(C, m, w3, n, 0, 0, None), "null")
    err(S(C, m, w3, n, 2, 0, H), "Invalid mode")
    err(S(C, m, w3, n, -1, 0, H), "Invalid mode")
    # the factored form
    terms = random_cubic_terms(random.Random(3), n, m)
    P = [a.ctypes.data for a in terms]
    swap = lambda k, v: P[:k] + [v] + P[k + 1:]        # noqa: E731
    for k in range(8):
        err(T(*swap(k, None), m, n, 0, 0, H), "null")
    err(T(*P, m, n, 0, 0, None), "null")
    err(T(*P, m, 0, 0, 0, H), "n_lin")
    err(T(*P, m, 500, 0, 0, H), "C(n_lin,4) below 2^31 - 64")
    err(T(*P, -1, n, 0, 0, H), "rows_live")
    err(T(*P, m, n, 2, 0, H), "Invalid mode")
    for k in (1, 4):
        start, dec = terms[k].copy(), terms[k].copy()
        start[0] = 1
        dec[3] = dec[2] - 1
        err(T(*swap(k, start.ctypes.data), m, n, 0, 0, H), "start at 0")
        err(T(*swap(k, dec.ctypes.data), m, n, 0, 0, H), "must not decrease")
    lin147, off = np.zeros((1, 3), dtype=np.uint64), np.zeros(2, dtype=np.int64)            # one linear row over 147 unknowns
    err(T(lin147.ctypes.data, off.ctypes.data, None, None, off.ctypes.data, None, None, None, 1, 147, 0, 0, H),
        "cubic row of this n_lin does not fit")
    assert not h.value
    # the bindings and the extension's entry
    with pytest.raises(ValueError, match="2-D"):
        hip.xl4_cubic_expand_words(np.zeros(3, dtype=np.uint64), n)
    with pytest.raises(ValueError, match="cubic_stride_words"):
        hip.xl4_cubic_expand_words(cubic[:, :2], n)
    with pytest.raises(ValueError, match="stride_words does not cover"):
        hip.xl4_cubic_expand_words(cubic, n, stride_words=3)
    with pytest.raises(ValueError, match="rows must be at least"):
        hip.xl4_cubic_expand_words(cubic, n, rows=live - 1)
    with pytest.raises(ValueError, match="null"):
        hip.xl4_cubic_expand_device(C, m, w3, n, rows, 0, wt)
    with pytest.raises(ValueError, match="Invalid mode"):
        hip.solve_xl4_cubic_words(cubic, n, mode=4)
    with pytest.raises(ValueError, match="off3"):
        hip.solve_xl4_cubic_terms(*terms[:4], terms[4][:-1], *terms[5:], n)
    with pytest.raises(ValueError, match="Invalid mode"):
        hip.solve_xl4_cubic_terms(*terms, n, mode=3)
    X = m4ri_solve_xl4_cubic_packed
    with pytest.raises(ValueError, match="Invalid mode"):
        X(*terms, n, 5)
    with pytest.raises(ValueError, match="n_lin"):
        X(*terms, 0, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        X(terms[0], terms[1][:-1].copy(), *terms[2:], n, 0)
    with pytest.raises(ValueError, match="same number"):
        X(*terms[:7], terms[7][:-1].copy(), n, 0)
    with pytest.raises(TypeError):
        X(*terms, n)


def test_no_device_no_answer():
    """without a GPU the new entries say so; nothing is computed on the host"""
    if hip.device_count() > 0:
        return
    p = PackedCubicSystem([4])
    (x,) = p.gens()
    zeros = [p.mul_bit(p.mul_bit(x[0], x[1]), x[2]) ^ x[3] ^ 1]
    with pytest.raises(RuntimeError, match="no HIP device"):
        p.solve_one_xl4(zeros)
    with pytest.raises(RuntimeError, match="no HIP device"):
        list(p.solve_all_xl4(zeros))
    with pytest.raises(RuntimeError, match="no HIP device"):
        p.solve_raw_space_xl4(zeros)
    with pytest.raises(hip.HipError, match="no HIP device"):
        p.get_eqs_xl4(zeros)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_cubic_expand_words(np.zeros((1, 1), dtype=np.uint64), 4)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.solve_xl4_cubic_words(np.zeros((1, 1), dtype=np.uint64), 4)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.solve_xl4_cubic_terms(*p._terms(zeros), 4)
