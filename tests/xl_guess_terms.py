"""Helpers of the hybrid XL tests: a host reference of the substitution of guessed unknowns that shares nothing with the kernel's
formulas.  An equation is a SET of monomials (tests.xl_terms); under an assignment a monomial that contains a guessed unknown set to
0 is dropped, guessed unknowns set to 1 are removed from it, the remaining unknowns are renumbered in increasing index, and equal
monomials cancel in pairs.  On top of it: the CPU-oracle pipeline (substitute -> xl3_ints -> solve_words) and the seeded systems the
CPU and the GPU tests share."""
import functools
import random

import numpy as np

from oracle import gf2_oracle as O
from tests import xl_terms as X


def remaining(n: int, guess) -> list:
    """the unknowns that are not guessed, in increasing index"""
    return [u for u in range(n) if u not in guess]


def substitute(monos: set, n: int, guess, a: int) -> set:
    """the polynomial over the remaining unknowns (renumbered) when unknown guess[t] is bit t of a"""
    value = {g: (a >> t) & 1 for t, g in enumerate(guess)}
    new = {u: k for k, u in enumerate(remaining(n, guess))}
    out = set()
    for mono in monos:
        if any(value.get(u) == 0 for u in mono):
            continue                                   # a factor is 0
        out ^= {frozenset(new[u] for u in mono if u not in value)}
    return out


@functools.lru_cache(maxsize=None)
def quad_columns(n: int) -> dict:
    """monomial of degree 1 or 2 -> column (QuadraticSystem's numbering, walked)"""
    monos = [frozenset([i]) for i in range(n)] + [frozenset([i, j]) for i in range(n) for j in range(i)]
    return {mono: c for c, mono in enumerate(monos)}


def quad_monos(e: int, n: int) -> set:
    """the monomials of a quadratic equation int, without the cubic tables of tests.xl_terms (n goes up to 65 here)"""
    col = quad_columns(n)
    low = sorted(col, key=col.get)
    assert e >> (len(low) + 1) == 0, "not a quadratic equation int"
    return ({frozenset()} if e & 1 else set()) | {low[c] for c in range(len(low)) if (e >> (1 + c)) & 1}


def specialise_ints(eqs, n: int, guess, a: int) -> list:
    """quadratic equation ints over n unknowns -> the equation ints of assignment a over the n - len(guess) remaining ones; every
    equation stays, also one that became 0 or the constant 1"""
    col = quad_columns(n - len(guess))
    return [X.to_int(substitute(quad_monos(e, n), n, guess, a), col) for e in eqs]


def specialised_aug(eqs, n: int, guess, a0: int, na: int, stride: int = 0) -> np.ndarray:
    """[na, m, stride] augmented words: what the specialisation writes for the assignments a0 .. a0 + na - 1"""
    ns = n - len(guess)
    stride = stride or (ns + ns * (ns - 1) // 2 + 1 + 63) // 64
    out = np.zeros((na, len(eqs), stride), dtype=np.uint64)
    for s in range(na):
        if eqs:
            out[s] = X.quad_aug(specialise_ints(eqs, n, guess, a0 + s), ns, stride)
    return out


def evaluate(e: int, x: int, n: int) -> int:
    """a quadratic equation int at the point x"""
    return (bin((e >> 1) & X.quad_point(x, n)).count("1") ^ e) & 1


def scatter(y: int, n: int, guess, a: int) -> int:
    """the point over all n unknowns: the remaining ones from y, the guessed ones from a"""
    x = 0
    for t, g in enumerate(guess):
        x |= ((a >> t) & 1) << g
    for k, u in enumerate(remaining(n, guess)):
        x |= ((y >> k) & 1) << u
    return x


def brute_force(eqs, n: int) -> list:
    """every common zero, increasing"""
    return [x for x in range(1 << n) if not any(evaluate(e, x, n) for e in eqs)]


# -- the CPU-oracle pipeline ------------------------------------------------------------------------------------------------------------
def cubic_aug(eqs, n: int) -> tuple:
    """(augmented words, rows, columns) of the padded degree-3 XL system of quadratic equation ints"""
    cols3 = X.cols3(n)
    ints = X.xl3_ints(eqs, n)
    rows = max(len(ints), cols3)
    return O.eqs_to_aug(ints + [0] * (rows - len(ints)), cols3, O.words_for(cols3)), rows, cols3


def oracle_guess(eqs, n: int, guess, a: int) -> dict:
    """{mode: the CPU oracle's result} for assignment a's system"""
    aug, rows, cols3 = cubic_aug(specialise_ints(eqs, n, guess, a), n - len(guess))
    return {md: O.solve_words(aug, rows, cols3, md) for md in (0, 1)}


def oracle_points(eqs, n: int, guess, max_dimension: int = 16) -> tuple:
    """(points, largest dimension): the consistent points of every assignment's space in assignment order and, within one, in
    AffineSpace order -- what solve_all_xl_guess yields for one block of n unknowns"""
    ns = n - len(guess)
    vectors = {X.point_vector(y, ns): y for y in range(1 << ns)} if ns <= 12 else None
    points, largest = [], -1
    for a in range(1 << len(guess)):
        ints = X.xl3_ints(specialise_ints(eqs, n, guess, a), ns)
        space = O.m4ri_solve(ints + [0] * max(0, X.cols3(ns) - len(ints)), X.cols3(ns), 1)
        if space is None:
            continue
        largest = max(largest, space.dimension)
        assert space.dimension <= max_dimension, (a, space.dimension)
        for raw in space:
            y = raw & ((1 << ns) - 1)
            if (vectors[raw] == y if vectors is not None and raw in vectors else X.point_vector(y, ns) == raw):
                points.append(scatter(y, n, guess, a))
    return points, largest


# -- the seeded systems of the solve and front-end tests: (n, m, guess) -> seed ----------------------------------------------------------
# Random dense equations planted at one point.  Each seed was picked so that test_xl_guess_cpu.py's conditions hold: plain degree-3 XL
# leaves a space above dimension 16, no assignment's space does, and the guessed pipeline's consistent points are exactly the
# brute-force solutions -- so no GPU test that compares with them can pass vacuously.
CASES = {
    (12, 12, (1, 4, 7, 10)): 0,
    (10, 9, (2, 6, 9)): 0,
    (14, 14, (9, 10, 11, 12, 13)): 0,
    (9, 8, (1, 8)): 0,
}


@functools.lru_cache(maxsize=None)
def case_eqs(n: int, m: int, guess: tuple) -> tuple:
    rng = random.Random(1000 * n + 10 * m + CASES[(n, m, guess)])
    return tuple(X.planted_dense(rng, n, m, [rng.getrandbits(n)]))
