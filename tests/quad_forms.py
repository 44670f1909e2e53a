"""A host reference for the quadratic search kernels that shares nothing with them: quadratic forms over GF(2) as plain Python
ints, zero sets that are known by construction, and a numpy walk for the sizes a walk reaches.

A form over R unknowns z_0 .. z_{R-1} is an equation int in the layout hip.quad_forms_search takes: bit 0 the constant, bit 1 + k
the unknown z_k, bit 1 + R + i(i-1)/2 + j the product z_i z_j (j < i).  An affine form uses bits 0 .. R only.  Forms add by XOR."""
import numpy as np


def width(R: int) -> int:
    """bits of a form over R unknowns"""
    return 1 + R + R * (R - 1) // 2


def mul(a: int, b: int, R: int) -> int:
    """the product of two affine forms in GF(2)[z] / (z^2 + z), constants included"""
    a0, b0, la, lb = a & 1, b & 1, a >> 1, b >> 1
    out = (a0 & b0) | (((la & lb) ^ (lb if a0 else 0) ^ (la if b0 else 0)) << 1)
    for i in range(1, R):                        # pair (i, j), j < i: a_i b_j ^ a_j b_i
        below = (1 << i) - 1
        row = (lb & below if (la >> i) & 1 else 0) ^ (la & below if (lb >> i) & 1 else 0)
        out ^= row << (1 + R + i * (i - 1) // 2)
    return out


def evaluate(f: int, z: int, R: int) -> int:
    """the value of form f at the point z (bit k = z_k)"""
    v = (f & 1) ^ (bin((f >> 1) & z & ((1 << R) - 1)).count("1") & 1)
    for i in range(1, R):
        if (z >> i) & 1:
            v ^= bin((f >> (1 + R + i * (i - 1) // 2)) & ((1 << i) - 1) & z).count("1") & 1
    return v


def apply(A: list, v: int) -> int:
    """A v for a matrix given as row ints (bit c of row i = A[i][c])"""
    out = 0
    for i, row in enumerate(A):
        out |= (bin(row & v).count("1") & 1) << i
    return out


def random_invertible(rng, R: int) -> tuple:
    """(A, A^-1): a uniformly random invertible R x R matrix over GF(2) and its inverse, rows as ints (Gauss-Jordan on ints)"""
    while True:
        A = [rng.getrandbits(R) for _ in range(R)]
        work = [A[i] | (1 << (R + i)) for i in range(R)]          # [A | I]
        ok = True
        for c in range(R):
            p = next((i for i in range(c, R) if (work[i] >> c) & 1), None)
            if p is None:
                ok = False
                break
            work[c], work[p] = work[p], work[c]
            for i in range(R):
                if i != c and (work[i] >> c) & 1:
                    work[i] ^= work[c]
        if ok:
            return A, [w >> R for w in work]


class DenseMap:
    """y = A z ^ b, a random invertible affine change of the unknowns: forms written in y (where their zeros are obvious)
    become forms that are dense in all R unknowns z, and the zero set goes along as z = A^-1 (y ^ b)"""

    def __init__(self, rng, R: int):
        self.R = R
        self.A, self.Ainv = random_invertible(rng, R)
        self.b = rng.getrandbits(R)

    def y(self, i: int) -> int:
        """the affine form in z that y_i is"""
        return (self.A[i] << 1) | ((self.b >> i) & 1)

    def prod(self, i: int, j: int) -> int:
        """y_i y_j as a form in z"""
        return mul(self.y(i), self.y(j), self.R)

    def z(self, y: int) -> int:
        return apply(self.Ainv, y ^ self.b)

    def zeros(self, ys) -> list:
        return sorted(self.z(y) for y in ys)


def weight_le1(p: int, s: int = 0) -> list:
    """the points y with at most one of the first p bits set and anything on the next s bits: (p + 1) 2^s of them"""
    return [a | (f << p) for a in [0] + [1 << k for k in range(p)] for f in range(1 << s)]


def known_zero_case(rng, R: int, p: int, s: int, order: str = "shuffled") -> tuple:
    """(forms, sorted zeros) under a fresh DenseMap.  In y: y_i y_j for i < j < p, and y_k for k >= p + s; the common zeros are the
    (p + 1) 2^s points of weight <= 1 on the first p unknowns, free on the next s, 0 on the rest.  order: "natural" (the
    products first, pairs in layout order, then the linear forms) or "shuffled" (by rng)."""
    assert 0 <= p and 0 <= s and p + s <= R and order in ("natural", "shuffled")
    dm = DenseMap(rng, R)
    forms = [dm.prod(i, j) for i in range(1, p) for j in range(i)] + [dm.y(k) for k in range(p + s, R)]
    if order == "shuffled":
        rng.shuffle(forms)
    return forms, dm.zeros(weight_le1(p, s))


def brute_zeros(forms, R: int) -> list:
    """every common zero of the forms by a numpy walk over all 2^R points (R <= 22), survivors only after each form"""
    assert R <= 22
    z = np.arange(1 << R, dtype=np.uint64)
    one = np.uint64(1)
    for f in forms:
        acc = np.bitwise_count(z & np.uint64((f >> 1) & ((1 << R) - 1)))
        for i in range(1, R):
            row = (f >> (1 + R + i * (i - 1) // 2)) & ((1 << i) - 1)
            if row:
                acc = acc + (np.bitwise_count(z & np.uint64(row)) & ((z >> np.uint64(i)) & one).astype(np.uint8))
        z = z[(acc & 1) == (f & 1)]
    return [int(v) for v in z]


def planted_dense(rng, R: int, nforms: int, points) -> list:
    """uniformly random forms that vanish at every one of `points`: a random form is kept when it takes one value on all of
    them, and its constant is flipped when that value is 1"""
    out = []
    while len(out) < nforms:
        f = rng.getrandbits(width(R))
        vals = {evaluate(f, z, R) for z in points}
        if len(vals) == 1:
            out.append(f ^ vals.pop())
    return out
