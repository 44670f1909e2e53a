"""Helpers of the degree-3 XL tests: a host reference of the expansion that shares nothing with the kernel's formulas.  An equation
is a SET of monomials (frozensets of unknown indices; the empty set is the constant 1), multiplying by x_k is a set union with
x^2 = x, and the columns are numbered by walking the monomials in the documented order: the unknowns, the pairs (i, j), j < i, by
i then j, the triples (i, j, l), l < j < i, by i then j then l."""
import functools

import numpy as np


@functools.lru_cache(maxsize=8)
def monomials(n: int) -> tuple:
    """every monomial of degree 1..3 in column order"""
    out = [frozenset([i]) for i in range(n)]
    out += [frozenset([i, j]) for i in range(n) for j in range(i)]
    out += [frozenset([i, j, l]) for i in range(n) for j in range(i) for l in range(j)]
    return tuple(out)


@functools.lru_cache(maxsize=8)
def columns(n: int) -> dict:
    """monomial -> column"""
    return {mono: c for c, mono in enumerate(monomials(n))}


def cols3(n: int) -> int:
    return len(monomials(n))


def quad_monos(e: int, n: int) -> set:
    """the monomials of a QuadraticSystem equation int (bit 0 the constant, bit 1 + c column c of the n + C(n,2) quadratic columns)"""
    low = monomials(n)[:n + n * (n - 1) // 2]
    assert e >> (len(low) + 1) == 0, "not a quadratic equation int"
    out = {frozenset()} if e & 1 else set()
    e >>= 1
    while e:
        bit = e & -e
        out.add(low[bit.bit_length() - 1])
        e ^= bit
    return out


def times(monos: set, k: int) -> set:
    """x_k times a polynomial: every monomial gains k, equal ones cancel in pairs"""
    out = set()
    for mono in monos:
        out ^= {mono | {k}}
    return out


def to_int(monos: set, col: dict) -> int:
    e = 0
    for mono in monos:
        e ^= 1 if not mono else 1 << (1 + col[mono])
    return e


def xl3_ints(eqs, n: int) -> list:
    """the degree-3 XL rows of quadratic equation ints, as equation ints over the cubic columns: equation e gives rows
    e(n+1) .. e(n+1) + n, itself and then its product with x_0 .. x_{n-1}; nothing is dropped"""
    col = columns(n)
    out = []
    for e in eqs:
        f = quad_monos(e, n)
        out.append(to_int(f, col))
        out.extend(to_int(times(f, k), col) for k in range(n))
    return out


def point_vector(x: int, n: int) -> int:
    """the raw point over the cubic columns (bit c = column c) of the linear part x: every monomial evaluated"""
    raw = 0
    for c, mono in enumerate(monomials(n)):
        if all((x >> i) & 1 for i in mono):
            raw |= 1 << c
    return raw


def quad_point(x: int, n: int) -> int:
    """the same over the quadratic columns alone"""
    return point_vector(x, n) & ((1 << (n + n * (n - 1) // 2)) - 1)


def planted_dense(rng, n: int, m: int, points) -> list:
    """m random dense quadratic equation ints (QuadraticSystem's layout) that vanish at every point of `points` (linear parts): random
    coefficient vectors from the null space of the points' differences are not needed at these sizes -- draw and keep what fits"""
    cols2 = n + n * (n - 1) // 2
    raws = [quad_point(x, n) for x in points]
    par = lambda v: bin(v).count("1") & 1              # noqa: E731
    out = []
    while len(out) < m:
        a = rng.getrandbits(cols2)
        vals = {par(a & r) for r in raws}
        if len(vals) == 1:
            out.append((a << 1) | vals.pop())
    return out


def quad_aug(eqs, n: int, stride: int = 0) -> np.ndarray:
    """quadratic equation ints as augmented words (column c = bit c, the constant at column n + C(n,2))"""
    cols2 = n + n * (n - 1) // 2
    stride = stride or (cols2 + 1 + 63) // 64
    out = np.zeros((len(eqs), stride), dtype=np.uint64)
    for r, e in enumerate(eqs):
        v = (e >> 1) | ((e & 1) << cols2)
        out[r] = np.frombuffer(v.to_bytes(8 * stride, "little"), dtype=np.uint64)
    return out


__all__ = ["cols3", "columns", "monomials", "planted_dense", "point_vector", "quad_aug", "quad_monos", "quad_point", "times", "to_int",
           "xl3_ints"]
