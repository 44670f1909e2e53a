"""A host reference for the quartic search kernels that shares no formula with them: tests/cubic_forms.py one degree up.  Quartic forms
over GF(2) as plain Python ints, products through the set-of-monomials multiplication (tests/cubic_terms.py's poly_mul, numbered by
tests/cubic_xl4_terms.py's poly_int4), zero sets that are known by construction, and a numpy walk for the sizes a walk reaches.

A form over R unknowns z_0 .. z_{R-1} is an equation int in the layout hip.quartic_forms_search takes -- that of a PackedQuarticSystem
of R unknowns: the cubic layout of tests/cubic_forms.py followed by bit 1 + xl4_quad_col(R, i, j, l, p) for the product z_i z_j z_l z_p
(p < l < j < i).  A cubic form is a quartic form as it stands when R is the same.  Forms add by XOR."""
import numpy as np

from tests import cubic_forms as CF
from tests.cubic_terms import poly_mul, poly_of_form
from tests.cubic_xl4_terms import poly_int4


def width(R: int) -> int:
    """bits of a form over R unknowns"""
    return CF.width(R) + R * (R - 1) * (R - 2) * (R - 3) // 24


def _quad_off(R: int) -> int:
    return CF.width(R)


def mul(forms, R: int) -> int:
    """the product of affine forms (two to four of them) in GF(2)[z] / (z^2 + z), constants included"""
    p = poly_of_form(forms[0], R)
    for f in forms[1:]:
        p = poly_mul(p, poly_of_form(f, R))
    return poly_int4(p, R)


def evaluate(f: int, z: int, R: int) -> int:
    """the value of form f at the point z (bit k = z_k)"""
    v = CF.evaluate(f & ((1 << CF.width(R)) - 1), z, R)
    for i in range(3, R):
        if not (z >> i) & 1:
            continue
        for j in range(2, i):
            if not (z >> j) & 1:
                continue
            for l in range(1, j):
                if (z >> l) & 1:
                    row = f >> (_quad_off(R) + i * (i - 1) * (i - 2) * (i - 3) // 24 + j * (j - 1) * (j - 2) // 6 + l * (l - 1) // 2)
                    v ^= bin(row & ((1 << l) - 1) & z).count("1") & 1
    return v


def _form_of_masks(masks: np.ndarray, R: int) -> int:
    """the form whose monomials are the int masks (members = set bits, at most four): the bit of a monomial with members
    m_0 < m_1 < ... is the start of its degree's block + SUM_t C(m_t, t + 1) -- the layout as the module's docstring states it"""
    m = masks.astype(np.uint64)
    bit = np.array([0, 1, 1 + R, 1 + R + R * (R - 1) // 2, CF.width(R)], dtype=np.int64)[np.bitwise_count(m).astype(np.int64)]
    for t in range(4):
        low = m & (~m + np.uint64(1))                                  # the lowest member left, 0 when none is
        g = np.where(low > 0, np.bitwise_count(low - np.uint64(1)), 0).astype(np.int64)
        c = g                                                          # C(g, t + 1)
        for u in range(1, t + 1):
            c = c * (g - u) // (u + 1)
        bit += np.where(low > 0, c, 0)
        m ^= low
    words = np.zeros((width(R) + 63) // 64, dtype=np.uint64)
    np.bitwise_or.at(words, bit >> 6, np.uint64(1) << (bit & 63).astype(np.uint64))
    return int.from_bytes(words.tobytes(), "little")


class DenseMap(CF.DenseMap):
    """tests/cubic_forms.py's map with products of up to four of the y_i.  The products of a case share factors, and four dense forms
    of R = 30 unknowns multiply to 30 000 monomials, too many for `mul` in a test, so prod keeps the partial products in numpy: a
    polynomial is an array of monomials, a monomial the int mask of its unknowns, multiplying the OR of every pair of masks with equal
    monomials cancelling in pairs -- the same set product (tests/test_quartic_search_cpu.py compares the two)."""

    def __init__(self, rng, R: int):
        super().__init__(rng, R)
        self._partial = {}

    def _masks(self, idx: tuple) -> np.ndarray:
        """the product of the y_i, i in idx, as an array of masks"""
        if idx not in self._partial:
            f = self.y(idx[-1])
            out = np.array([1 << g for g in range(self.R) if (f >> (1 + g)) & 1] + ([0] if f & 1 else []), dtype=np.uint64)
            if len(idx) > 1:
                both, times = np.unique((self._masks(idx[:-1])[:, None] | out[None, :]).ravel(), return_counts=True)
                out = both[times % 2 == 1]
            self._partial[idx] = out
        return self._partial[idx]

    def prod(self, *idx) -> int:
        """y_i y_j (y_k (y_l)) as a form in z"""
        return _form_of_masks(self._masks(tuple(sorted(idx))), self.R)


def weight_le3(p: int, s: int = 0) -> list:
    """the points y with at most three of the first p bits set and anything on the next s bits: (1 + p + C(p,2) + C(p,3)) 2^s of them"""
    heads = [y for y in range(1 << p) if bin(y).count("1") <= 3]
    return [a | (f << p) for a in heads for f in range(1 << s)]


def known_zero_case(rng, R: int, p: int, s: int, order: str = "shuffled") -> tuple:
    """(forms, sorted zeros) under a fresh DenseMap.  In y: y_i y_j y_k y_l for i < j < k < l < p; up to three products of two, three
    and four of the first p unknowns (one of each degree 2, 3 and 4 before the factor) times (1 ^ a) with a an affine form that is
    1 on the zero set (a = 1 ^ some of the y_k, k >= p + s; they need p >= 3 and such a k), so that the degrees mix before the map
    already; and y_k for k >= p + s.  The common zeros are the (1 + p + C(p,2) + C(p,3)) 2^s points of weight <= 3 on the first p
    unknowns, free on the next s, 0 on the rest.  order: "natural" (quadruples first, then the mixed products, then the linear forms)
    or "shuffled" (by rng)."""
    assert 0 <= p and 0 <= s and p + s <= R and order in ("natural", "shuffled")
    dm = DenseMap(rng, R)
    forms = [dm.prod(i, j, k, l) for l in range(3, p) for k in range(2, l) for j in range(1, k) for i in range(j)]
    high = list(range(p + s, R))
    if p >= 3 and high:
        for size in (1, 2, 3):                                      # the product has degree size + 1 with the factor
            idx = rng.sample(range(p), size)
            ks = [k for k in high if rng.getrandbits(1)] or [high[0]]
            forms.append(mul([dm.y(i) for i in idx] + [dm.affine(0, ks)], R))
    forms += [dm.y(k) for k in high]
    if order == "shuffled":
        rng.shuffle(forms)
    return forms, dm.zeros(weight_le3(p, s))


def brute_zeros(forms, R: int) -> list:
    """every common zero of the forms by a numpy walk over all 2^R points (R <= 20), survivors only after each form"""
    assert R <= 20
    z = np.arange(1 << R, dtype=np.uint64)
    one = np.uint64(1)
    bit = lambda i: ((z >> np.uint64(i)) & one).astype(np.uint8)      # noqa: E731
    for f in forms:
        acc = np.bitwise_count(z & np.uint64((f >> 1) & ((1 << R) - 1))).astype(np.uint8)
        for i in range(1, R):
            zi = bit(i)
            row = (f >> (1 + R + i * (i - 1) // 2)) & ((1 << i) - 1)
            if row:
                acc = acc + (np.bitwise_count(z & np.uint64(row)) & zi)
            for j in range(1, i):
                zij = zi & bit(j)
                row = (f >> (1 + R + R * (R - 1) // 2 + i * (i - 1) * (i - 2) // 6 + j * (j - 1) // 2)) & ((1 << j) - 1)
                if row:
                    acc = acc + (np.bitwise_count(z & np.uint64(row)) & zij)
                for l in range(1, j):
                    row = (f >> (_quad_off(R) + i * (i - 1) * (i - 2) * (i - 3) // 24 + j * (j - 1) * (j - 2) // 6 + l * (l - 1) // 2)) \
                        & ((1 << l) - 1)
                    if row:
                        acc = acc + (np.bitwise_count(z & np.uint64(row)) & zij & bit(l))
        z = z[(acc & 1) == (f & 1)]
    return [int(v) for v in z]


def planted_dense(rng, R: int, nforms: int, points) -> list:
    """uniformly random quartic forms that vanish at every one of `points`: a random form is kept when it takes one value on all of
    them, and its constant is flipped when that value is 1"""
    out = []
    while len(out) < nforms:
        f = rng.getrandbits(width(R))
        vals = {evaluate(f, z, R) for z in points}
        if len(vals) == 1:
            out.append(f ^ vals.pop())
    return out
