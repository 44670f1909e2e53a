"""Helpers of the packed quadratic front-end's tests: the same random expressions built on QuadraticSystem (tuple-of-int bits,
the yardstick) and on PackedQuadraticSystem (factored, packed words), and the factored arrays expanded on the host with
QuadraticSystem._mul_bit -- one product at a time, on ints -- which is what the device expansion must reproduce bit for bit."""
import numpy as np

from gf2bv_amd import QuadraticSystem
from gf2bv_amd.packed import PackedBitVec, PackedQuadBitVec, PackedQuadraticSystem


def row_ints(rows: np.ndarray) -> list:
    return [int.from_bytes(np.ascontiguousarray(r).tobytes(), "little") for r in rows]


def expand_ints(q: QuadraticSystem, lin, off, ta, tb) -> list:
    """equation ints (bit 0 constant, bit 1 + c column c) of factored rows, via QuadraticSystem._mul_bit"""
    lin, ta, tb = row_ints(lin), row_ints(ta), row_ints(tb)
    low = (1 << (q._lin_size + 1)) - 1
    out = []
    for r, e in enumerate(lin):
        e &= low
        for t in range(int(off[r]), int(off[r + 1])):
            e ^= q._mul_bit(ta[t] & low, tb[t] & low)
        out.append(e)
    return out


def bits_of(v) -> list:
    """the expanded equation ints of a symbolic vector of either front-end"""
    if isinstance(v, PackedQuadBitVec):
        return expand_ints(QuadraticSystem([v._n]), v._lin, v._off, v._ta, v._tb)
    return list(v._bits)                               # BitVec, and PackedBitVec's compatibility property


def random_forms(rng, n: int, count: int, constants: bool) -> np.ndarray:
    """`count` random linear forms over n unknowns as [count, Wl] words (equation-int order), some sparse, some dense"""
    wl = (n + 1 + 63) // 64
    out = np.zeros((count, wl), dtype=np.uint64)
    for k in range(count):
        v = rng.getrandbits(n) if rng.random() < 0.6 else 1 << rng.randrange(n)
        v = (v << 1) | (rng.getrandbits(1) if constants else 0)
        out[k] = np.frombuffer(v.to_bytes(8 * wl, "little"), dtype=np.uint64)
    return out


def random_terms(rng, n: int, rows: int, max_terms: int = 4, constants: bool = True):
    """random factored rows: (lin, term_off, ta, tb); rows with no product, a == b and the same product twice all occur"""
    lin = random_forms(rng, n, rows, constants)
    cnt = [rng.randint(0, max_terms) for _ in range(rows)]
    off = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(cnt, out=off[1:])
    T = int(off[-1])
    ta, tb = random_forms(rng, n, T, constants), random_forms(rng, n, T, constants)
    for r in range(rows):
        t0, t1 = int(off[r]), int(off[r + 1])
        if t1 > t0 and rng.random() < 0.2:
            tb[t0] = ta[t0]                            # a square
        if t1 - t0 >= 2 and rng.random() < 0.2:
            ta[t1 - 1], tb[t1 - 1] = ta[t0], tb[t0]    # the same product twice: cancels
    return lin, off, ta, tb


class Twin:
    """one expression built on both front-ends in step"""

    def __init__(self, sizes):
        self.q, self.p = QuadraticSystem(sizes), PackedQuadraticSystem(sizes)
        self.n = self.q._lin_size
        self.qx = self.q.gens()[0]
        for g in self.q.gens()[1:]:
            self.qx = self.qx.concat(g)
        self.px = self.p.gens()[0]
        for g in self.p.gens()[1:]:
            self.px = self.px.concat(g)

    def linear(self, rng, constant: bool):
        """a random single-bit linear expression: (BitVec, PackedBitVec)"""
        a, b = self.qx[rng.randrange(self.n)], None
        b = self.px[self.qx._bits.index(a._bits[0])]
        for _ in range(rng.randint(0, 3)):
            i = rng.randrange(self.n)
            a, b = a ^ self.qx[i], b ^ self.px[i]
        if constant and rng.random() < 0.5:
            a, b = a ^ 1, b ^ 1
        return a, b

    def bit(self, rng, products: int, constant: bool):
        """a random single-bit quadratic expression with `products` products: (BitVec, PackedQuadBitVec | PackedBitVec)"""
        a, b = self.linear(rng, constant)
        first = None
        for k in range(products):
            u, v = self.linear(rng, constant), self.linear(rng, constant)
            if k == 1 and rng.random() < 0.3:
                u, v = first                           # the same product twice
            elif rng.random() < 0.2:
                v = u                                  # a square
            if k == 0:
                first = (u, v)
            a, b = a ^ self.q.mul_bit(u[0], v[0]), b ^ self.p.mul_bit(u[1], v[1])
        return a, b


def to_aug(eqs, cols: int, stride: int) -> np.ndarray:
    """equation ints -> rows of the augmented-words layout (column c = bit c, the constant at column cols)"""
    out = np.zeros((len(eqs), stride), dtype=np.uint64)
    mask = (1 << cols) - 1
    for r, e in enumerate(eqs):
        v = ((e >> 1) & mask) | ((e & 1) << cols)
        out[r] = np.frombuffer(v.to_bytes(8 * stride, "little"), dtype=np.uint64)
    return out


__all__ = ["PackedBitVec", "Twin", "bits_of", "expand_ints", "random_forms", "random_terms", "row_ints", "to_aug"]
