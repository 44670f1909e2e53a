"""Helpers of the tests of degree-4 XL on cubic equations, on top of tests/cubic_terms.py's set-of-monomials product: a polynomial is
a set of monomials, x_k p is the product of p with the one-monomial polynomial {x_k} (so x^2 = x by the union), and the columns of a
polynomial of degree <= 4 come from the front-end's column functions.  Equation e gives the rows p_e, then x_k p_e for k = 0 .. n-1.
Nothing here knows of runs or windows, or shares a formula with the kernel."""
import numpy as np

from gf2bv_amd.linsys import xl3_pair_col, xl3_triple_col, xl4_cols, xl4_quad_col
from tests.cubic_terms import ONE, poly_mul, poly_of_form, register_outputs, register_step


_BIT = {}                                              # (n, monomial) -> its bit in an equation int, filled as monomials are met


def _bit(n: int, m: frozenset) -> int:
    s = sorted(m, reverse=True)
    assert len(s) <= 4 and all(0 <= g < n for g in s), "degree above 4 or an unknown out of range"
    if len(s) == 0:
        return 1
    if len(s) == 1:
        return 1 << (1 + s[0])
    return 1 << (1 + {2: xl3_pair_col, 3: xl3_triple_col, 4: xl4_quad_col}[len(s)](n, *s))


def poly_int4(p: frozenset, n: int) -> int:
    """a polynomial of degree <= 4 as an equation int over the quartic columns (bit 0 constant, bit 1 + c column c)"""
    e = 0
    for m in p:
        b = _BIT.get((n, m))
        if b is None:
            b = _BIT[n, m] = _bit(n, m)
        e ^= b
    return e


def xl4_cubic_polys(n: int, polys) -> list:
    """for each polynomial p: p, then x_k p for k = 0 .. n-1, as sets of monomials"""
    out = []
    for p in polys:
        out.append(frozenset(p))
        out.extend(poly_mul(p, frozenset([frozenset((k,))])) for k in range(n))
    return out


def xl4_cubic_eqs(n: int, polys) -> list:
    """the same rows as equation ints over the quartic columns: n + 1 per polynomial, nothing dropped"""
    return [poly_int4(p, n) for p in xl4_cubic_polys(n, polys)]


def quartic_aug(eqs, n: int, rows: int, stride: int) -> np.ndarray:
    """equation ints over the quartic columns as `rows` rows of `stride` augmented words (column c = bit c, the constant at column
    cols4), zero rows behind the given ones"""
    cols = xl4_cols(n)
    out = np.zeros((rows, stride), dtype=np.uint64)
    mask = (1 << cols) - 1
    for r, e in enumerate(eqs):
        v = ((e >> 1) & mask) | ((e & 1) << cols)
        out[r] = np.frombuffer(v.to_bytes(8 * stride, "little"), dtype=np.uint64)
    return out


def register_polys(secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """the filtered register's equations z_t(x) ^ z_t(secret) = 0 (tests/cubic_terms.py, register_eqs) as sets of monomials"""
    s = [1 << (1 + g) for g in range(n)]
    polys = []
    for z in register_outputs(secret, n, taps, pos, count):
        f = [poly_of_form(s[p], n) for p in pos]
        p = f[0] ^ poly_mul(f[1], f[2]) ^ poly_mul(poly_mul(f[3], f[4]), f[5])
        polys.append(p ^ frozenset([ONE]) if z else p)
        s = register_step(s, taps)
    return polys


__all__ = ["register_polys", "poly_int4", "quartic_aug", "xl4_cubic_eqs", "xl4_cubic_polys", "xl4_cols"]
