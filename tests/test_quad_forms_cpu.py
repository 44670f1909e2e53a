"""tests/quad_forms.py, the yardstick of tests/test_gpu_quad_forms.py, checked where no GPU exists: its zero sets that are known
by construction equal a walk over every point, its product of affine forms equals a product of sets of monomials, and its
matrices invert."""
import random

import pytest

from tests import quad_forms as QF

KNOWN = [(1, 1, 0), (2, 2, 0), (5, 3, 1), (10, 6, 2), (11, 6, 2), (16, 12, 2), (20, 12, 3), (22, 13, 4)]


@pytest.mark.parametrize("R,p,s", KNOWN, ids=lambda v: str(v))
def test_known_zero_set_is_the_walk(R, p, s):
    rng = random.Random(1000 + R)
    forms, want = QF.known_zero_case(rng, R, p, s, "shuffled")
    assert len(forms) == p * (p - 1) // 2 + R - p - s
    assert len(want) == len(set(want)) == (p + 1) << s
    assert QF.brute_zeros(forms, R) == want
    assert all(QF.evaluate(f, z, R) == 0 for f in forms for z in want[:8])


def test_known_zero_set_orders_hold_the_same_forms():
    natural, zn = QF.known_zero_case(random.Random(3), 9, 5, 2, "natural")
    shuffled, zs = QF.known_zero_case(random.Random(3), 9, 5, 2, "shuffled")
    assert zn == zs and sorted(natural) == sorted(shuffled) and natural != shuffled
    assert all(f >> 10 for f in natural[:10]) and not any(f >> 10 for f in natural[10:])       # products first, then affine


def _monomials(a: int, R: int) -> set:
    """an affine form as a set of monomials (frozensets of unknowns; the empty one is the constant)"""
    return {frozenset() for _ in range(a & 1)} | {frozenset([k]) for k in range(R) if (a >> (1 + k)) & 1}


def _as_form(monos: set, R: int) -> int:
    f = 0
    for mono in monos:
        v = sorted(mono)
        f |= 1 << (0 if not v else 1 + v[0] if len(v) == 1 else 1 + R + v[1] * (v[1] - 1) // 2 + v[0])
    return f


def test_mul_is_the_product_of_monomial_sets():
    R = 5
    rng = random.Random(5)
    cases = [(0, 0), (1, 1), (1, 0b100110), (0b111111, 0b111111)] + [(rng.getrandbits(R + 1), rng.getrandbits(R + 1)) for _ in range(200)]
    for a, b in cases:
        want = set()
        for x in _monomials(a, R):
            for y in _monomials(b, R):
                want ^= {x | y}                      # z^2 = z: the union of the unknowns; equal monomials cancel
        assert QF.mul(a, b, R) == _as_form(want, R) == QF.mul(b, a, R), (a, b)
        for z in range(1 << R):
            assert QF.evaluate(QF.mul(a, b, R), z, R) == QF.evaluate(a, z, R) & QF.evaluate(b, z, R)


@pytest.mark.parametrize("R", [0, 1, 2, 7, 40, 64, 65])
def test_random_invertible_inverts(R):
    rng = random.Random(50 + R)
    A, Ainv = QF.random_invertible(rng, R)
    assert len(A) == len(Ainv) == R
    for _ in range(20):
        v = rng.getrandbits(R) if R else 0
        assert QF.apply(Ainv, QF.apply(A, v)) == v == QF.apply(A, QF.apply(Ainv, v))
    dm = QF.DenseMap(rng, R)
    y = rng.getrandbits(R) if R else 0
    assert all(QF.evaluate(dm.y(i), dm.z(y), R) == (y >> i) & 1 for i in range(R))


@pytest.mark.parametrize("R", [6, 18, 22])
def test_planted_dense_keeps_its_points(R):
    rng = random.Random(70 + R)
    points = [rng.getrandbits(R) for _ in range(3)]
    forms = QF.planted_dense(rng, R, max(R - 6, 3), points)
    got = QF.brute_zeros(forms, R)
    assert set(points) <= set(got) and got == sorted(got)
    assert all(QF.evaluate(f, z, R) == 0 for f in forms for z in got[:50])
    if R <= 6:
        assert got == [z for z in range(1 << R) if all(QF.evaluate(f, z, R) == 0 for f in forms)]


def test_brute_zeros_edges():
    assert QF.brute_zeros([], 0) == [0] and QF.brute_zeros([0], 0) == [0] and QF.brute_zeros([1], 0) == []
    assert QF.brute_zeros([0, 0], 3) == list(range(8)) and QF.brute_zeros([1], 7) == []
    assert QF.brute_zeros([0b10], 1) == [0] and QF.brute_zeros([0b11], 1) == [1]
