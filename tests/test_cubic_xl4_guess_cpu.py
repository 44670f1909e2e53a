"""Hybrid degree-4 XL on cubic equations without a GPU: the set-based substitution of tests/cubic_guess_terms.py against evaluation,
the rank facts of the filtered registers that the documentation quotes (outputs saved by guessing), convert_sol_xl4_guess and the guess
parsing of PackedCubicGuessSystem, gf2bv_xl4_cubic_guess_chunk, and every argument check of the new entries -- made before any device is
touched."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import PackedCubicGuessSystem, hip
from gf2bv_amd._internal import m4ri_solve_xl4_guess_cubic_packed
from gf2bv_amd.linsys import xl3_cols, xl4_cols
from tests import cubic_guess_terms as CG
from tests import xl4_terms as X4
from tests.cubic_terms import REGISTER_12, REGISTER_16, IntBasis, bits_of, poly_value, random_cubic_terms, row_polys

M = lambda *v: frozenset(v)                            # noqa: E731  (a monomial)


# -- 1. the helper against evaluation at every point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,guess", [(2, (1,)), (3, (0, 2)), (5, ()), (5, (3,)), (6, (4, 1, 2)), (7, (6, 0)), (8, (7, 2, 3, 5)), (8, (0, 1, 2, 3, 4, 5, 6))])
def test_substitution_equals_evaluation(n, guess):
    rng = random.Random(300 + n + len(guess))
    polys = row_polys(n, *random_cubic_terms(rng, n, 5))
    polys.append(frozenset([M()] + [M(i) for i in range(n)] + [M(i, j) for i in range(n) for j in range(i)]
                           + [M(i, j, l) for i in range(n) for j in range(i) for l in range(j)]))          # every coefficient set
    polys += [frozenset(), frozenset([M()])]
    ns = n - len(guess)
    for a in range(1 << len(guess)):
        spec = CG.specialise_polys(polys, n, guess, a)
        assert len(spec) == len(polys) and all(len(mono) <= 3 and all(0 <= u < ns for u in mono) for p in spec for mono in p)
        for y in range(1 << ns):
            x = CG.scatter(y, n, guess, a)
            assert all((x >> g) & 1 == (a >> t) & 1 for t, g in enumerate(guess))
            assert [poly_value(p, y) for p in spec] == [poly_value(p, x) for p in polys], (a, y)
    if not guess:
        assert CG.specialise_polys(polys, n, guess, 0) == polys
    assert n < 5 or any(len(mono) == 3 for p in polys[:5] for mono in p)


def test_substitution_by_hand():
    p = frozenset([M(), M(1), M(3, 0), M(4, 2, 1), M(4, 3, 2), M(5, 4, 3)])
    # x_4 = 1, x_1 = 0: 1 ^ x_3 x_0 ^ x_3 x_2 ^ x_5 x_3 over (0, 2, 3, 5) -> (0, 1, 2, 3)
    assert CG.substitute(p, 6, (4, 1), 0b01) == frozenset([M(), M(2, 0), M(2, 1), M(3, 2)])
    # x_4 = 1, x_1 = 1: the constant and x_1 cancel, x_4 x_2 x_1 becomes x_2
    assert CG.substitute(p, 6, (4, 1), 0b11) == frozenset([M(2, 0), M(1), M(2, 1), M(3, 2)])
    assert CG.substitute(p, 6, (4, 1), 0b00) == frozenset([M(), M(2, 0)])
    aug = CG.specialised_aug([p], 6, (4, 1), 1, 1)
    assert aug.shape == (1, 1, 1)                      # n' = 4: 14 cubic columns, the constant on bit 14
    assert int(aug[0, 0, 0]) == 1 << 14 | 1 << (4 + 1) | 1 << (4 + 2) | 1 << (4 + 5)      # pairs (2,0) (2,1) (3,2) at 4 + C(i,2) + j


# -- 2. what guessing saves: the rank facts of the filtered registers --------------------------------------------------------------------------
def _dimensions(polys, n: int, guess) -> list:
    """per assignment the dimension of its degree-4 XL system's solution space, None for an inconsistent one (an integer echelon
    basis over the equation ints: the constant is bit 0, so the row 1 appears exactly when the system is inconsistent)"""
    cols4 = xl4_cols(n - len(guess))
    out = []
    for a in range(1 << len(guess)):
        basis = IntBasis()
        for e in CG.quartic_ints(polys, n, guess, a):
            basis.add(e)
        out.append(None if 1 in basis.rows else cols4 - len(basis))
    return out


# (secret, guess, outputs) -> per assignment its dimension; plain degree-4 XL needs 62 outputs for either secret
REGISTER_12_FACTS = {
    (0x52F, (10, 11), 34): [11, 11, 11, 11],
    (0x52F, (10, 11), 35): [None, 2, 1, 1],
    (0x52F, (10, 11), 36): [None, 0, None, None],
    (0x3A1, (10, 11), 35): [1, 2, None, 0],
    (0x3A1, (10, 11), 36): [0, None, None, None],
    (0x52F, (3, 7, 11), 26): [None, 1, None, 3, None, 2, None, None],
    (0x52F, (3, 7, 11), 27): [None, 0, None, None, None, None, None, None],
    (0x3A1, (3, 7, 11), 26): [None, 1, 1, 3, None, 1, None, 3],
    (0x3A1, (3, 7, 11), 27): [None, None, 0, None, None, None, None, None],
}


@pytest.mark.parametrize("secret,guess,outputs", list(REGISTER_12_FACTS))
def test_register_12_rank_facts(secret, guess, outputs):
    n = 12
    assert xl4_cols(n - len(guess)) == {2: 385, 3: 255}[len(guess)]
    polys = CG.register_case(secret, count=outputs, **REGISTER_12)
    want = REGISTER_12_FACTS[(secret, guess, outputs)]
    assert _dimensions(polys, n, guess) == want
    own = sum(((secret >> g) & 1) << t for t, g in enumerate(guess))      # the secret's own assignment is never inconsistent
    assert want[own] is not None


def test_register_16_falls_to_62_outputs():
    """n = 16, guess x[12..15]: 16 systems of 62 * 13 = 806 rows over the 793 quartic columns of 12 unknowns; only the secret's
    assignment is consistent, with dimension 0 (plain degree-4 XL needs 149 outputs, plain linearisation 696)"""
    n, secret, guess = 16, 0x52E7, (12, 13, 14, 15)
    assert xl4_cols(12) == 793 and xl4_cols(16) == 2516 and xl3_cols(16) == 696
    polys = CG.register_case(secret, count=62, **REGISTER_16)
    assert len(CG.quartic_ints(polys, n, guess, 0)) == 806
    assert _dimensions(polys, n, guess) == [0 if a == secret >> 12 else None for a in range(16)]


# -- 3. the front-end: convert_sol_xl4_guess and guess parsing ------------------------------------------------------------------------------
def test_convert_sol_xl4_guess():
    n, rng = 9, random.Random(77)
    p = PackedCubicGuessSystem([4, 5])
    for guess in ((), (8,), (0, 1), (7, 2, 4), tuple(range(8))):
        ns = n - len(guess)
        for _ in range(3):
            a, y = rng.getrandbits(len(guess)), rng.getrandbits(ns)
            full = CG.scatter(y, n, guess, a)
            raw = X4.point_vector(y, ns)
            assert p.convert_sol_xl4_guess(raw, guess, a) == (full & 15, full >> 4)          # the generators' values, no trailing block
            for c in range(ns, xl4_cols(ns)):          # any single pair, triple or quadruple coordinate flipped
                assert p.convert_sol_xl4_guess(raw ^ (1 << c), guess, a) is None
    x, y = p.gens()
    assert p.convert_sol_xl4_guess(X4.point_vector(0b1010101, 7), [y[4], x[1]], 0b01) == (0b1001, 0b11010)
    assert p.convert_sol_xl4_guess(X4.point_vector(0x155, n), [], 0) == p.convert_sol_xl4(X4.point_vector(0x155, n)) == (5, 0x15)
    with pytest.raises(AssertionError, match="Invalid solution"):
        p.convert_sol_xl4_guess(1 << xl4_cols(7), [0, 1], 0)


def test_the_hybrid_class_is_a_cubic_system_with_five_methods_more():
    import gf2bv_amd
    from gf2bv_amd import PackedCubicSystem
    public = lambda cls: {name for name in dir(cls) if not name.startswith("_")}
    assert issubclass(PackedCubicGuessSystem, PackedCubicSystem) and "PackedCubicGuessSystem" in gf2bv_amd.__all__
    assert public(PackedCubicGuessSystem) - public(PackedCubicSystem) == {
        "convert_sol_xl4_guess", "solve_all_xl4_guess", "solve_one_xl4_guess", "solve_raw_one_xl4_guess", "solve_raw_space_xl4_guess"}
    assert not public(PackedCubicSystem) - public(PackedCubicGuessSystem)
    p, q = PackedCubicSystem([3, 4]), PackedCubicGuessSystem([3, 4])
    (x, y), (u, v) = p.gens(), q.gens()
    assert bits_of(q.mul_bit(x[0], q.mul_bit(u[1], y[2])) ^ v[3]) == bits_of(p.mul_bit(x[0], p.mul_bit(x[1], y[2])) ^ y[3])
    with pytest.raises(TypeError, match="not built"):
        q.factor([u[0]])


def test_guess_parsing():
    p = PackedCubicGuessSystem([3, 4])                      # unknowns 0..2 are x, 3..6 are y
    x, y = p.gens()
    assert p._parse_guess([]) == []
    assert p._parse_guess([5, 0]) == [5, 0]
    assert p._parse_guess([y[2], x[0], 6]) == [5, 0, 6]
    assert p._parse_guess((x[1], y[3:4])) == [1, 6]
    for bad in ([7], [-1], [1, 1], [x[0], 0], [x], [x[0] ^ x[1]], [x[0] ^ 1], [y[1] ^ y[1]], ["x"], [1.0], [True], [0, 1, 2, 3, 4, 5, 6],
                [p.mul_bit(x[0], x[1])]):
        with pytest.raises(ValueError):
            p._parse_guess(bad)
    with pytest.raises(ValueError, match="at most"):
        PackedCubicGuessSystem([40])._parse_guess(list(range(31)))
    for method in (p.solve_raw_space_xl4_guess, p.solve_raw_one_xl4_guess):
        with pytest.raises(ValueError, match="assignments"):
            method([], [0, 1], assignments=(2, 3))
    with pytest.raises(ValueError, match="assignments"):
        list(p.solve_all_xl4_guess([], [0, 1], assignments=(-1, 2)))
    with pytest.raises(ValueError, match="guessed twice"):
        p.solve_one_xl4_guess([], [y[0], 3])
    gen = p.solve_all_xl4_guess([x[0]], ["x"])         # a generator: nothing is looked at before the first point is asked for
    with pytest.raises(ValueError):
        next(gen)


# -- 4. the chunk ----------------------------------------------------------------------------------------------------------------------------
def test_guess_chunk():
    m, n, f = 100, 24, 8                               # n' = 16: 697 cubic bits (11 words, 12 held), 2516 rows of 40 words a system
    per = 8 * (2516 * 40 + 100 * 12)
    chunk = hip.xl4_cubic_guess_chunk
    assert chunk(m, n, f, 4 * per - 1) == 0
    assert chunk(m, n, f, 4 * per) == 1
    assert chunk(m, n, f, 4 * 200 * per + 5) == 200
    assert chunk(m, n, f, 1 << 50) == 256              # capped at 2^f
    assert chunk(m, n, 0, 1 << 50) == 1
    last = 0
    for free in range(0, 40 * per, per // 3):
        c = chunk(m, n, f, free)
        assert c >= last
        last = c
    assert last == 9
    assert chunk(200, n, f, 4 * per) == 0 and chunk(200, n, f, 4 * 8 * (3400 * 40 + 200 * 12)) == 1      # 200 * 17 live rows above the columns
    assert chunk(10, 50, 30, 1 << 62) == (2 ** 31 - 65) // xl4_cols(20)          # rows of all systems < 2^31 - 64
    for bad in ((m, 0, 0, 1), (m, n, -1, 1), (m, n, n, 1), (m, 40, 31, 1), (-1, n, f, 1), (m, n, f, -1), (0, 500, 0, 1), (0, 147, 0, 1)):
        with pytest.raises(ValueError):
            chunk(*bad)


# -- 5. the C ABI: GF2BV_ERR_ARG before any device ---------------------------------------------------------------------------------------
def test_entries_check_arguments_before_device_use():
    L = hip.lib()
    n, m, f = 12, 5, 3                                 # 298 cubic columns (5 words); n' = 9: 129 cubic (3 words), 255 quartic (4 words)
    w3, w3s, wt = 5, 3, 4
    rows = 256                                         # max(5 * 10, 255) and one more
    cubic = np.zeros((4 * m + 1, w3), dtype=np.uint64)
    aug = np.zeros((4 * rows + 1, wt), dtype=np.uint64)
    Q, A = cubic.ctypes.data, aug.ctypes.data
    A += -A % 16
    guess = np.array([3, 11, 0], dtype=np.int32)
    Gp = guess.ctypes.data
    arr = lambda *v: np.array(v, dtype=np.int32)       # noqa: E731
    terms = random_cubic_terms(random.Random(3), n, m)
    P = [a.ctypes.data for a in terms]
    swap = lambda k, v: P[:k] + [v] + P[k + 1:]        # noqa: E731
    hs = (ctypes.c_void_p * 8)()
    big = 2 ** 31 - 64

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    def guess_errors(call):
        """what every entry with a guess refuses: call(n_lin, guess pointer, nguess, a0, na)"""
        err(call(0, Gp, 0, 0, 1), "n_lin")
        err(call(2400, Gp, 0, 0, 1), "C(n_lin,3) below 2^31 - 64")
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

    D = L.gf2bv_cubic_specialise_device
    guess_errors(lambda nl, g, nf, a0, na: D(Q, m, w3, nl, g, nf, a0, na, A, w3s, m * w3s, 0, None))
    err(D(None, m, w3, n, Gp, f, 0, 8, A, w3s, m * w3s, 0, None), "null")
    err(D(Q, m, w3, n, Gp, f, 0, 8, None, w3s, m * w3s, 0, None), "null")
    err(D(Q, -1, w3, n, Gp, f, 0, 8, A, w3s, m * w3s, 0, None), "na x m")
    err(D(Q, big // 8 + 1, w3, n, Gp, f, 0, 8, A, w3s, 3 * big, 0, None), "na x m")
    err(D(Q, m, w3 - 1, n, Gp, f, 0, 8, A, w3s, m * w3s, 0, None), "cubic_stride_words")
    err(D(Q, m, w3, n, Gp, f, 0, 8, A, w3s - 1, m * w3s, 0, None), "out_stride_words")           # short
    err(D(Q, m, w3, n, Gp, f, 0, 8, A, w3s, m * w3s - 1, 0, None), "out_stride_words")           # sys_stride below m rows
    err(D(Q, m, w3, n, Gp, f, 0, 8, A + 4, w3s, m * w3s, 0, None), "out_stride_words")           # not a word boundary
    err(D(Q, 0, 9000, 147, Gp, f, 0, 8, A, 9000, 0, 0, None), "cubic row, its specialised form")  # a 66200-byte source row
    err(D(Q, 0, 4502, 120, Gp, 0, 0, 1, A, 4502, 0, 0, None), "LDS")                             # 36016 bytes, but twice: source and specialised row
    # f = 30 over 100 unknowns: 435 pair vectors of 2 + 1 words, 30 vectors of 39 words, rows of 2606 and 895 words -- 47 KiB, accepted
    wide = np.arange(30, dtype=np.int32)
    err(D(Q, m, 2606, 100, wide.ctypes.data, 30, 0, 8, A, 894, m * 894, 0, None), "out_stride_words")

    W = L.gf2bv_cubic_specialise_words
    guess_errors(lambda nl, g, nf, a0, na: W(Q, m, w3, nl, g, nf, a0, na, A, w3s, 0))
    err(W(None, m, w3, n, Gp, f, 0, 8, A, w3s, 0), "null")
    err(W(Q, m, w3, n, Gp, f, 0, 8, None, w3s, 0), "null")
    err(W(Q, big // 8 + 1, w3, n, Gp, f, 0, 8, A, w3s, 0), "na x m")
    err(W(Q, m, w3 - 1, n, Gp, f, 0, 8, A, w3s, 0), "cubic_stride_words")
    err(W(Q, m, w3, n, Gp, f, 0, 8, A, w3s - 1, 0), "out_stride_words")
    err(W(Q, 0, 9000, 147, Gp, f, 0, 8, A, 9000, 0), "LDS")

    B = L.gf2bv_xl4_cubic_expand_batch_device          # 4 systems of m rows over 9 unknowns, 3 words each
    q = m * w3s
    err(B(None, 4, q, m, w3s, 9, rows, A, wt, rows * wt, 0, None), "null")
    err(B(Q, 4, q, m, w3s, 9, rows, None, wt, rows * wt, 0, None), "null")
    err(B(Q, -1, q, m, w3s, 9, rows, A, wt, rows * wt, 0, None), "nsys")
    err(B(Q, 4, q, m, w3s, 0, rows, A, wt, rows * wt, 0, None), "n_lin")
    err(B(Q, 4, q, m, w3s, 500, rows, A, wt, rows * wt, 0, None), "C(n_lin,4) below 2^31 - 64")
    err(B(Q, 4, q, -1, w3s, 9, rows, A, wt, rows * wt, 0, None), "m(n_lin + 1)")
    err(B(Q, 4, q, m, w3s, 9, m * 10 - 1, A, wt, rows * wt, 0, None), "rows must")
    err(B(Q, big // rows + 1, q, m, w3s, 9, rows, A, wt, rows * wt, 0, None), "all systems together")
    err(B(Q, 4, q, m, w3s - 1, 9, rows, A, wt, rows * wt, 0, None), "cubic_stride_words")
    err(B(Q, 4, q - 1, m, w3s, 9, rows, A, wt, rows * wt, 0, None), "cubic_sys_stride_words")
    err(B(Q, 4, q, m, w3s, 9, rows, A, wt - 2, rows * wt, 0, None), "stride_words")              # short
    err(B(Q, 4, q, m, w3s, 9, rows, A, wt + 1, rows * (wt + 1), 0, None), "even")                # odd
    err(B(Q, 4, q, m, w3s, 9, rows, A, wt, rows * wt - 2, 0, None), "sys_stride_words")          # systems overlap
    err(B(Q, 4, q, m, w3s, 9, rows, A, wt, rows * wt + 1, 0, None), "even")
    err(B(Q, 4, q, m, w3s, 9, rows, A + 8, wt, rows * wt, 0, None), "16-byte alignment")
    err(B(Q, 1, 0, 0, 9000, 147, 0, A, 2 ** 23, 0, 0, None), "cubic row of this n_lin does not fit")

    V = L.gf2bv_xl4_cubic_expand_batch_words
    err(V(None, 4, q, m, w3s, 9, rows, A, wt, rows * wt, 0), "null")
    err(V(Q, 4, q, m, w3s, 9, rows, None, wt, rows * wt, 0), "null")
    err(V(Q, -1, q, m, w3s, 9, rows, A, wt, rows * wt, 0), "nsys")
    err(V(Q, 4, q, m, w3s, 0, rows, A, wt, rows * wt, 0), "n_lin")
    err(V(Q, 4, q, m, w3s, 9, m * 10 - 1, A, wt, rows * wt, 0), "rows must")
    err(V(Q, big // rows + 1, q, m, w3s, 9, rows, A, wt, rows * wt, 0), "all systems together")
    err(V(Q, 4, q, m, w3s - 1, 9, rows, A, wt, rows * wt, 0), "cubic_stride_words")
    err(V(Q, 4, q - 1, m, w3s, 9, rows, A, wt, rows * wt, 0), "cubic_sys_stride_words")
    err(V(Q, 4, q, m, w3s, 9, rows, A, wt - 1, rows * wt, 0), "stride_words")
    err(V(Q, 4, q, m, w3s, 9, rows, A, wt, rows * wt - 1, 0), "sys_stride_words")

    S = L.gf2bv_solve_xl4_cubic_guess_words
    guess_errors(lambda nl, g, nf, a0, na: S(Q, m, w3, nl, g, nf, a0, na, 0, 0, hs))
    err(S(Q, m, w3, n, Gp, f, 0, 8, 0, 0, None), "null")
    err(S(None, m, w3, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(S(Q, m, w3 - 1, n, Gp, f, 0, 8, 0, 0, hs), "cubic_stride_words")
    err(S(Q, m, w3, n, Gp, f, 0, 8, 3, 0, hs), "Invalid mode")
    err(S(Q, 0, 9000, 147, Gp, f, 0, 8, 0, 0, hs), "LDS")
    many = np.arange(20, dtype=np.int32)               # n' = 40: 102090 quartic columns a system, 2^20 systems
    err(S(Q, 0, 564, 60, many.ctypes.data, 20, 0, 2 ** 20, 0, 0, (ctypes.c_void_p * 2 ** 20)()), "all assignments")

    T = L.gf2bv_solve_xl4_cubic_guess_terms
    guess_errors(lambda nl, g, nf, a0, na: T(*P, m, nl, g, nf, a0, na, 0, 0, hs))
    err(T(*P, m, n, Gp, f, 0, 8, 0, 0, None), "null")
    for k in range(8):
        err(T(*swap(k, None), m, n, Gp, f, 0, 8, 0, 0, hs), "null")
    err(T(*P, -1, n, Gp, f, 0, 8, 0, 0, hs), "rows_live")
    err(T(*P, m, n, Gp, f, 0, 8, 5, 0, hs), "Invalid mode")
    for k in (1, 4):
        start, dec = terms[k].copy(), terms[k].copy()
        start[0] = 1
        dec[3] = dec[2] - 1
        err(T(*swap(k, start.ctypes.data), m, n, Gp, f, 0, 8, 0, 0, hs), "start at 0")
        err(T(*swap(k, dec.ctypes.data), m, n, Gp, f, 0, 8, 0, 0, hs), "must not decrease")
    assert not any(hs)                                 # nothing was made

    C = L.gf2bv_xl4_cubic_guess_chunk_device
    chunk = ctypes.c_int64(7)
    err(C(m, n, f, 0, None), "null")
    err(C(m, n, 12, 0, ctypes.byref(chunk)), "out of range")
    assert chunk.value == 0

    # the bindings and the extension: library errors as ValueError, shapes checked before the library sees them
    with pytest.raises(ValueError, match="repeated"):
        hip.cubic_specialise_words(cubic[:m], n, [1, 1])
    with pytest.raises(ValueError, match="cubic_stride_words"):
        hip.cubic_specialise_words(cubic[:m, :4], n, [1])
    with pytest.raises(ValueError, match="null"):
        hip.cubic_specialise_device(Q, m, w3, n, [1], 0, 2, 0, w3s, m * w3s)
    with pytest.raises(ValueError, match="2-D"):
        hip.solve_xl4_cubic_guess_words(cubic.ravel(), n, [1])
    with pytest.raises(ValueError, match="3-D"):
        hip.xl4_cubic_expand_batch_words(cubic, 9)
    with pytest.raises(ValueError, match="null"):
        hip.xl4_cubic_expand_batch_device(Q, 4, q, m, w3s, 9, rows, 0, wt, rows * wt)
    with pytest.raises(ValueError, match="assignments"):
        hip.solve_xl4_cubic_guess_words(cubic[:m], n, [1, 2], a0=3, na=2)
    with pytest.raises(ValueError, match="off3"):
        hip.solve_xl4_cubic_guess_terms(*terms[:4], terms[4][:-1], *terms[5:], n, [1])
    with pytest.raises(ValueError, match="Invalid mode"):
        hip.solve_xl4_cubic_guess_terms(*terms, n, [1], mode=3)
    X = m4ri_solve_xl4_guess_cubic_packed
    with pytest.raises(ValueError, match="repeated"):
        X(*terms, n, [4, 4], 0, 1, 0)
    with pytest.raises(ValueError, match="nguess"):
        X(*terms, n, list(range(12)), 0, 1, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        X(*terms, n, [4], 0, 1, 5)
    with pytest.raises(ValueError, match="assignments"):
        X(*terms, n, [4], 1, 2, 0)
    with pytest.raises(ValueError, match="n_lin - 1"):
        X(*terms, n, [-1], 0, 1, 0)
    with pytest.raises(ValueError, match="n_lin"):
        X(*terms, 0, [], 0, 1, 0)
    with pytest.raises(TypeError, match="sequence"):
        X(*terms, n, 1, 0, 1, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        X(terms[0], terms[1][:-1].copy(), *terms[2:], n, [4], 0, 1, 0)
    with pytest.raises(ValueError, match="same number"):
        X(*terms[:7], terms[7][:-1].copy(), n, [4], 0, 1, 0)
    with pytest.raises(TypeError):
        X(*terms, n, [4], 0, 1)
    assert X(*terms, n, [4], 1, 0, 0) == []            # no assignment: no device is needed


def test_no_device_no_answer():
    """without a GPU the hybrid entries say so; nothing is computed on the host"""
    if hip.device_count() > 0:
        return
    p = PackedCubicGuessSystem([4])
    (x,) = p.gens()
    zeros = [p.mul_bit(p.mul_bit(x[0], x[1]), x[2]) ^ x[3] ^ 1]
    with pytest.raises((RuntimeError, hip.HipError), match="no HIP device"):
        p.solve_one_xl4_guess(zeros, [x[3]])
    with pytest.raises((RuntimeError, hip.HipError), match="no HIP device"):
        list(p.solve_all_xl4_guess(zeros, [3]))
    with pytest.raises((RuntimeError, hip.HipError), match="no HIP device"):
        p.solve_raw_space_xl4_guess(zeros, [0, 1])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.cubic_specialise_words(np.zeros((1, 1), dtype=np.uint64), 4, [0])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_cubic_expand_batch_words(np.zeros((2, 1, 1), dtype=np.uint64), 3)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.solve_xl4_cubic_guess_words(np.zeros((1, 1), dtype=np.uint64), 4, [0])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.solve_xl4_cubic_guess_terms(*p._terms(zeros), 4, [0])
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.xl4_cubic_guess_chunk(1, 4, 1)
