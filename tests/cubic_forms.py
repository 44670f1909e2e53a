"""A host reference for the cubic search kernels that shares no formula with them: cubic forms over GF(2) as plain Python ints,
products through the set-of-monomials multiplication of tests/cubic_terms.py, zero sets that are known by construction, and a
numpy walk for the sizes a walk reaches.

A form over R unknowns z_0 .. z_{R-1} is an equation int in the layout hip.cubic_forms_search takes -- that of a PackedCubicSystem
of R unknowns: bit 0 the constant, bit 1 + k the unknown z_k, bit 1 + xl3_pair_col(R, i, j) the product z_i z_j (j < i), bit
1 + xl3_triple_col(R, i, j, l) the product z_i z_j z_l (l < j < i).  An affine form uses bits 0 .. R only.  Forms add by XOR."""
import numpy as np

from tests.cubic_terms import poly_int, poly_mul, poly_of_form
from tests.quad_forms import apply, random_invertible


def width(R: int) -> int:
    """bits of a form over R unknowns"""
    return 1 + R + R * (R - 1) // 2 + R * (R - 1) * (R - 2) // 6


def _pair_off(R: int) -> int:
    return 1 + R


def _triple_off(R: int) -> int:
    return 1 + R + R * (R - 1) // 2


def mul(forms, R: int) -> int:
    """the product of affine forms (two or three of them) in GF(2)[z] / (z^2 + z), constants included"""
    p = poly_of_form(forms[0], R)
    for f in forms[1:]:
        p = poly_mul(p, poly_of_form(f, R))
    return poly_int(p, R)


def evaluate(f: int, z: int, R: int) -> int:
    """the value of form f at the point z (bit k = z_k)"""
    v = (f & 1) ^ (bin((f >> 1) & z & ((1 << R) - 1)).count("1") & 1)
    for i in range(1, R):
        if not (z >> i) & 1:
            continue
        v ^= bin((f >> (_pair_off(R) + i * (i - 1) // 2)) & ((1 << i) - 1) & z).count("1") & 1
        for j in range(1, i):
            if (z >> j) & 1:
                row = f >> (_triple_off(R) + i * (i - 1) * (i - 2) // 6 + j * (j - 1) // 2)
                v ^= bin(row & ((1 << j) - 1) & z).count("1") & 1
    return v


class DenseMap:
    """y = A z ^ b, a random invertible affine change of the unknowns (tests/quad_forms.py's, with cubic products): forms written
    in y, where their zeros are obvious, become forms that are dense in all R unknowns z and in every degree"""

    def __init__(self, rng, R: int):
        self.R = R
        self.A, self.Ainv = random_invertible(rng, R) if R else ([], [])
        self.b = rng.getrandbits(R) if R else 0

    def y(self, i: int) -> int:
        """the affine form in z that y_i is"""
        return (self.A[i] << 1) | ((self.b >> i) & 1)

    def prod(self, *idx) -> int:
        """y_i y_j (y_k) as a form in z"""
        return mul([self.y(i) for i in idx], self.R)

    def affine(self, const: int, ks) -> int:
        """const ^ XOR of y_k, k in ks, as a form in z"""
        f = const
        for k in ks:
            f ^= self.y(k)
        return f

    def z(self, y: int) -> int:
        return apply(self.Ainv, y ^ self.b)

    def zeros(self, ys) -> list:
        return sorted(self.z(y) for y in ys)


def weight_le2(p: int, s: int = 0) -> list:
    """the points y with at most two of the first p bits set and anything on the next s bits: (1 + p + p(p-1)/2) 2^s of them"""
    heads = [0] + [1 << k for k in range(p)] + [(1 << i) | (1 << j) for i in range(1, p) for j in range(i)]
    return [a | (f << p) for a in heads for f in range(1 << s)]


def known_zero_case(rng, R: int, p: int, s: int, order: str = "shuffled") -> tuple:
    """(forms, sorted zeros) under a fresh DenseMap.  In y: y_i y_j y_k for i < j < k < p; up to three products y_i y_j (1 ^ a) with
    a an affine form that is 1 on the zero set (a = 1 ^ some of the y_k, k >= p + s; they need p >= 2 and such a k), so that terms
    of degree two and three mix before the map already; and y_k for k >= p + s.  The common zeros are the
    (1 + p + p(p-1)/2) 2^s points of weight <= 2 on the first p unknowns, free on the next s, 0 on the rest.
    order: "natural" (triples first, then the mixed products, then the linear forms) or "shuffled" (by rng)."""
    assert 0 <= p and 0 <= s and p + s <= R and order in ("natural", "shuffled")
    dm = DenseMap(rng, R)
    forms = [dm.prod(i, j, k) for k in range(2, p) for j in range(1, k) for i in range(j)]
    high = list(range(p + s, R))
    if p >= 2 and high:
        for _ in range(3):
            i, j = rng.sample(range(p), 2)
            ks = [k for k in high if rng.getrandbits(1)] or [high[0]]
            forms.append(mul([dm.y(i), dm.y(j), dm.affine(0, ks)], R))
    forms += [dm.y(k) for k in high]
    if order == "shuffled":
        rng.shuffle(forms)
    return forms, dm.zeros(weight_le2(p, s))


def brute_zeros(forms, R: int) -> list:
    """every common zero of the forms by a numpy walk over all 2^R points (R <= 20), survivors only after each form"""
    assert R <= 20
    z = np.arange(1 << R, dtype=np.uint64)
    one = np.uint64(1)
    for f in forms:
        acc = np.bitwise_count(z & np.uint64((f >> 1) & ((1 << R) - 1))).astype(np.uint8)
        for i in range(1, R):
            zi = ((z >> np.uint64(i)) & one).astype(np.uint8)
            row = (f >> (_pair_off(R) + i * (i - 1) // 2)) & ((1 << i) - 1)
            if row:
                acc = acc + (np.bitwise_count(z & np.uint64(row)) & zi)
            for j in range(1, i):
                row = (f >> (_triple_off(R) + i * (i - 1) * (i - 2) // 6 + j * (j - 1) // 2)) & ((1 << j) - 1)
                if row:
                    acc = acc + (np.bitwise_count(z & np.uint64(row)) & zi & ((z >> np.uint64(j)) & one).astype(np.uint8))
        z = z[(acc & 1) == (f & 1)]
    return [int(v) for v in z]


def planted_dense(rng, R: int, nforms: int, points) -> list:
    """uniformly random cubic forms that vanish at every one of `points`: a random form is kept when it takes one value on all of
    them, and its constant is flipped when that value is 1"""
    out = []
    while len(out) < nforms:
        f = rng.getrandbits(width(R))
        vals = {evaluate(f, z, R) for z in points}
        if len(vals) == 1:
            out.append(f ^ vals.pop())
    return out
