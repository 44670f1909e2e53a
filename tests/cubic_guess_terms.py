"""Helpers of the tests of hybrid degree-4 XL on cubic equations, on top of tests/cubic_terms.py and tests/cubic_xl4_terms.py: the
substitution of guessed unknowns on SETS of monomials.  Under an assignment a monomial that contains a guessed unknown set to 0 is
dropped, guessed unknowns set to 1 are stripped from it, the remaining unknowns are renumbered in increasing index, and the results
are XORed together (equal monomials cancel in pairs).  It knows nothing of base rows, per-guess vectors or constants' bits: it shares
no formula with the kernel."""
import functools

import numpy as np

from gf2bv_amd.linsys import xl3_cols, xl4_cols
from oracle import gf2_oracle as O
from tests.cubic_terms import poly_int, to_aug
from tests.cubic_xl4_terms import quartic_aug, register_polys, xl4_cubic_eqs


def remaining(n: int, guess) -> list:
    """the unknowns that are not guessed, in increasing index"""
    return [u for u in range(n) if u not in guess]


def substitute(p, n: int, guess, a: int) -> frozenset:
    """the polynomial over the remaining unknowns (renumbered) when unknown guess[t] is bit t of a"""
    value = {g: (a >> t) & 1 for t, g in enumerate(guess)}
    new = {u: k for k, u in enumerate(remaining(n, guess))}
    out = set()
    for mono in p:
        if any(value.get(u) == 0 for u in mono):
            continue                                   # a factor is 0
        out ^= {frozenset(new[u] for u in mono if u not in value)}
    return frozenset(out)


def specialise_polys(polys, n: int, guess, a: int) -> list:
    """every polynomial under assignment a; all of them stay, also one that became 0 or the constant 1"""
    return [substitute(p, n, guess, a) for p in polys]


def specialised_aug(polys, n: int, guess, a0: int, na: int, stride: int = 0) -> np.ndarray:
    """[na, m, stride] augmented words over the cubic columns of the remaining unknowns: what the specialisation writes for the
    assignments a0 .. a0 + na - 1"""
    ns = n - len(guess)
    cols3 = xl3_cols(ns)
    stride = stride or (cols3 + 1 + 63) // 64
    out = np.zeros((na, len(polys), stride), dtype=np.uint64)
    for s in range(na):
        if polys:
            out[s] = to_aug([poly_int(p, ns) for p in specialise_polys(polys, n, guess, a0 + s)], cols3, stride)
    return out


def scatter(y: int, n: int, guess, a: int) -> int:
    """the point over all n unknowns: the remaining ones from y, the guessed ones from a"""
    x = 0
    for t, g in enumerate(guess):
        x |= ((a >> t) & 1) << g
    for k, u in enumerate(remaining(n, guess)):
        x |= ((y >> k) & 1) << u
    return x


def quartic_ints(polys, n: int, guess, a: int) -> list:
    """assignment a's degree-4 XL rows (p', then x_k p' for every remaining unknown) as equation ints over the quartic columns"""
    return xl4_cubic_eqs(n - len(guess), specialise_polys(polys, n, guess, a))


def oracle_guess(polys, n: int, guess, a: int) -> dict:
    """{mode: the CPU oracle's result} for assignment a's system, padded with zero rows up to its columns"""
    ns = n - len(guess)
    eqs, cols4 = quartic_ints(polys, n, guess, a), xl4_cols(ns)
    rows = max(len(eqs), cols4)
    aug = quartic_aug(eqs, ns, rows, O.words_for(cols4))
    return {md: O.solve_words(aug, rows, cols4, md) for md in (0, 1)}


@functools.lru_cache(maxsize=None)
def register_case(secret: int, n: int, taps: int, pos: tuple, count: int) -> tuple:
    """the filtered register's equations as sets of monomials (made once per case, never changed)"""
    return tuple(register_polys(secret, n, taps, pos, count))


__all__ = ["oracle_guess", "quartic_ints", "register_case", "remaining", "scatter", "specialise_polys", "specialised_aug", "substitute"]
