"""Helpers of the degree-4 XL tests, on top of tests.xl_terms: the same set-based host reference -- an equation is a SET of monomials,
multiplying is a set union with x^2 = x -- carried to degree 4.  The columns are numbered by walking the monomials in the documented
order: degree 3's columns first, then the quadruples (i, j, l, p), p < l < j < i, by i, then j, then l, then p.  Equation e gives the
rows f_e, x_k f_e for k = 0 .. n-1, then x_a x_b f_e for a = 1 .. n-1, b = 0 .. a-1.  Nothing here shares a formula with the kernel."""
import functools

import numpy as np

from oracle import gf2_oracle as O
from tests import xl_terms as X


@functools.lru_cache(maxsize=8)
def monomials(n: int) -> tuple:
    """every monomial of degree 1..4 in column order"""
    return X.monomials(n) + tuple(frozenset([i, j, l, p]) for i in range(n) for j in range(i) for l in range(j) for p in range(l))


@functools.lru_cache(maxsize=8)
def columns(n: int) -> dict:
    """monomial -> column"""
    return {mono: c for c, mono in enumerate(monomials(n))}


def cols4(n: int) -> int:
    return len(monomials(n))


def rows_per_equation(n: int) -> int:
    return 1 + n + n * (n - 1) // 2


def multipliers(n: int) -> list:
    """the multipliers in row order: 1, the unknowns, the pairs {a, b}, b < a, by a then b"""
    return [frozenset()] + [frozenset([k]) for k in range(n)] + [frozenset([a, b]) for a in range(n) for b in range(a)]


def times_set(monos: set, mult: frozenset) -> set:
    """a monomial times a polynomial: every monomial gains the multiplier's unknowns, equal ones cancel in pairs"""
    out = set()
    for mono in monos:
        out ^= {mono | mult}
    return out


def xl4_ints(eqs, n: int) -> list:
    """the degree-4 XL rows of quadratic equation ints, as equation ints over the quartic columns (bit 0 the constant, bit 1 + c
    column c): rows_per_equation(n) rows per equation in multiplier order; nothing is dropped"""
    col, mults = columns(n), multipliers(n)
    out = []
    for e in eqs:
        f = X.quad_monos(e, n)
        out.extend(X.to_int(times_set(f, mult), col) for mult in mults)
    return out


def point_vector(x: int, n: int) -> int:
    """the raw point over the quartic columns (bit c = column c) of the linear part x: every monomial evaluated"""
    raw = 0
    for c, mono in enumerate(monomials(n)):
        if all((x >> i) & 1 for i in mono):
            raw |= 1 << c
    return raw


def column_of(mono: frozenset, n: int) -> int:
    """the column of a monomial of degree 1..4 by the front-end's column functions (gf2bv_amd.linsys), which test_xl4_cpu.py checks
    against the walk of `columns` for n = 1..12: for shapes whose quartic table would not fit a test"""
    from gf2bv_amd.linsys import xl3_pair_col, xl3_triple_col, xl4_quad_col      # noqa: PLC0415
    v = sorted(mono, reverse=True)
    if len(v) == 1:
        return v[0]
    return {2: xl3_pair_col, 3: xl3_triple_col, 4: xl4_quad_col}[len(v)](n, *v)


def xl4_aug(eqs, n: int, rows: int, stride: int, table: bool = True) -> np.ndarray:
    """the degree-4 XL rows of quadratic equation ints as augmented words (column c = bit c, the constant at column cols4), `rows` rows
    of `stride` words, zero behind the live ones.  table=False numbers the columns with column_of instead of the walked table."""
    c4 = n + n * (n - 1) // 2 + n * (n - 1) * (n - 2) // 6 + n * (n - 1) * (n - 2) * (n - 3) // 24
    col = columns(n).__getitem__ if table else (lambda mono: column_of(mono, n))
    mults = multipliers(n)
    out = np.zeros((rows, stride), dtype=np.uint64)
    r = 0
    for e in eqs:
        f = X.quad_monos(e, n) if table else _quad_monos_wide(e, n)
        for mult in mults:
            cs = np.array([col(mono) if mono else c4 for mono in times_set(f, mult)], dtype=np.int64)
            np.bitwise_or.at(out[r], cs >> 6, np.uint64(1) << (cs & 63).astype(np.uint64))
            r += 1
    return out


def _quad_monos_wide(e: int, n: int) -> set:
    """X.quad_monos without the cubic table"""
    low = [frozenset([i]) for i in range(n)] + [frozenset([i, j]) for i in range(n) for j in range(i)]
    assert e >> (len(low) + 1) == 0, "not a quadratic equation int"
    return ({frozenset()} if e & 1 else set()) | {low[c] for c in range(len(low)) if (e >> (1 + c)) & 1}


def quartic_aug(eqs, n: int) -> tuple:
    """(augmented words, rows, columns) of the padded degree-4 XL system of quadratic equation ints: what the solve entries build"""
    c4 = cols4(n)
    rows = max(len(eqs) * rows_per_equation(n), c4)
    return xl4_aug(eqs, n, rows, O.words_for(c4)), rows, c4


__all__ = ["cols4", "column_of", "columns", "monomials", "multipliers", "point_vector", "quartic_aug", "rows_per_equation", "times_set",
           "xl4_aug", "xl4_ints"]
