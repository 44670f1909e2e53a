"""Helpers of the packed cubic front-end's tests.  The yardstick is a set-of-monomials product: a polynomial of
GF(2)[x] / (x_i^2 + x_i) is a set of monomials, a monomial a frozenset of unknown indices (the empty one is the constant 1), a sum the
symmetric difference and a product the XOR of all unions.  It knows nothing of runs, windows or the formulas the kernel and the
package use; the factored arrays expanded with it are what the device expansion must reproduce bit for bit."""
import numpy as np

from gf2bv_amd import hip
from gf2bv_amd.linsys import xl3_cols, xl3_pair_col, xl3_triple_col
from tests.quad_terms import row_ints, to_aug

ONE = frozenset()


def poly_of_form(v: int, n: int) -> frozenset:
    """the affine form of an equation int (bit 0 constant, bit 1 + g unknown g < n; bits above n ignored) as a set of monomials"""
    out = {frozenset((g,)) for g in range(n) if (v >> (1 + g)) & 1}
    if v & 1:
        out.add(ONE)
    return frozenset(out)


def poly_mul(p: frozenset, q: frozenset) -> frozenset:
    out = set()
    for a in p:
        for b in q:
            out ^= {a | b}
    return frozenset(out)


def poly_int(p: frozenset, n: int) -> int:
    """a polynomial of degree <= 3 as an equation int over the cubic columns (bit 0 constant, bit 1 + c column c)"""
    e = 0
    for m in p:
        s = sorted(m, reverse=True)
        if len(s) == 0:
            e ^= 1
        elif len(s) == 1:
            e ^= 1 << (1 + s[0])
        elif len(s) == 2:
            e ^= 1 << (1 + xl3_pair_col(n, *s))
        else:
            assert len(s) == 3, "degree above 3"
            e ^= 1 << (1 + xl3_triple_col(n, *s))
    return e


def poly_value(p: frozenset, x: int) -> int:
    """the polynomial at the point x (bit g = unknown g)"""
    return sum(all((x >> g) & 1 for g in m) for m in p) & 1


def row_polys(n: int, lin, off2, ta, tb, off3, ua, ub, uc) -> list:
    """every factored row as a set of monomials"""
    forms = lambda a: [poly_of_form(v, n) for v in row_ints(a)]            # noqa: E731
    lin, ta, tb, ua, ub, uc = (forms(a) for a in (lin, ta, tb, ua, ub, uc))
    out = []
    for r, p in enumerate(lin):
        for t in range(int(off2[r]), int(off2[r + 1])):
            p = p ^ poly_mul(ta[t], tb[t])
        for u in range(int(off3[r]), int(off3[r + 1])):
            p = p ^ poly_mul(poly_mul(ua[u], ub[u]), uc[u])
        out.append(p)
    return out


def expand_ints(n: int, lin, off2, ta, tb, off3, ua, ub, uc) -> list:
    """equation ints over the cubic columns of factored rows, through the set product"""
    return [poly_int(p, n) for p in row_polys(n, lin, off2, ta, tb, off3, ua, ub, uc)]


def bits_of(v) -> list:
    """the expanded equation ints of a PackedCubicBitVec (or of a PackedBitVec: its own bits)"""
    if hasattr(v, "_ua"):
        return expand_ints(v._n, v._lin, v._off2, v._ta, v._tb, v._off3, v._ua, v._ub, v._uc)
    return list(v._bits)


def random_forms(rng, n: int, count: int, constants: bool) -> np.ndarray:
    """`count` random affine forms over n unknowns as [count, Wl] words: dense ones, forms of a few unknowns, single unknowns"""
    wl = (n + 1 + 63) // 64
    out = np.zeros((count, wl), dtype=np.uint64)
    for k in range(count):
        kind = rng.random()
        if kind < 0.3:
            v = rng.getrandbits(n)
        elif kind < 0.7:
            v = 0
            for _ in range(rng.randint(1, 4)):
                v |= 1 << rng.randrange(n)
        else:
            v = 1 << rng.randrange(n)
        v = (v << 1) | (rng.getrandbits(1) if constants else 0)
        out[k] = np.frombuffer(v.to_bytes(8 * wl, "little"), dtype=np.uint64)
    return out


def random_cubic_terms(rng, n: int, rows: int, max_terms: int = 3, constants: bool = True):
    """random factored rows (lin, off2, ta, tb, off3, ua, ub, uc).  Rows with no term, a == b, a == b == c and the same term twice
    all occur; with three rows or more, row 0 is linear only, row 1 has more quadratic and row 2 more cubic terms than one pass of
    the kernel holds in LDS (the chunk sizes are the library's, hip.cubic_chunks)."""
    tch2, tch3 = hip.cubic_chunks(n)
    lin = random_forms(rng, n, rows, constants)
    cnt2 = [rng.randint(0, max_terms) for _ in range(rows)]
    cnt3 = [rng.randint(0, max_terms) for _ in range(rows)]
    if rows >= 3:
        cnt2[0] = cnt3[0] = 0
        cnt2[1] = tch2 + rng.randint(1, 2)
        cnt3[2] = tch3 + rng.randint(1, 2)
    off2, off3 = np.zeros(rows + 1, dtype=np.int64), np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(cnt2, out=off2[1:])
    np.cumsum(cnt3, out=off3[1:])
    ta, tb = (random_forms(rng, n, int(off2[-1]), constants) for _ in range(2))
    ua, ub, uc = (random_forms(rng, n, int(off3[-1]), constants) for _ in range(3))
    for r in range(rows):
        t0, t1, u0, u1 = int(off2[r]), int(off2[r + 1]), int(off3[r]), int(off3[r + 1])
        if t1 > t0 and rng.random() < 0.3:
            tb[t0] = ta[t0]                            # a square
        if t1 - t0 >= 2 and rng.random() < 0.3:
            ta[t1 - 1], tb[t1 - 1] = ta[t0], tb[t0]    # the same product twice: cancels
        if u1 > u0 and rng.random() < 0.3:
            ub[u0] = ua[u0]                            # a == b
            if rng.random() < 0.5:
                uc[u0] = ua[u0]                        # a == b == c
        if u1 - u0 >= 2 and rng.random() < 0.3:
            ua[u1 - 1], ub[u1 - 1], uc[u1 - 1] = ua[u0], ub[u0], uc[u0]
    return lin, off2, ta, tb, off3, ua, ub, uc


class IntBasis:
    """rows of GF(2) as ints, kept in echelon form by their leading bits: add(v) tells whether v was independent of the rows before"""

    def __init__(self):
        self.rows = {}

    def add(self, v: int) -> bool:
        while v:
            h = v.bit_length()
            if h not in self.rows:
                self.rows[h] = v
                return True
            v ^= self.rows[h]
        return False

    def __len__(self):
        return len(self.rows)


# -- the filtered register of the known-answer table: z = s_p0 ^ s_p1 s_p2 ^ s_p3 s_p4 s_p5 before the step ----------------------------
def register_step(state: list, taps: int) -> list:
    """one step on any representation with ^: out = s_0, s_g <- s_{g+1} with s_{n-1} <- 0, then s_g ^= out where bit g of taps is set"""
    n = len(state)
    out = state[0]
    nxt = state[1:] + [None]
    return [(out if nxt[g] is None else nxt[g] ^ out) if (taps >> g) & 1 else (0 if nxt[g] is None else nxt[g]) for g in range(n)]


def register_outputs(secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """`count` output bits of the register started at `secret` (bit g = s_g)"""
    s = [(secret >> g) & 1 for g in range(n)]
    out = []
    for _ in range(count):
        out.append(s[pos[0]] ^ (s[pos[1]] & s[pos[2]]) ^ (s[pos[3]] & s[pos[4]] & s[pos[5]]))
        s = register_step(s, taps)
    return out


def register_eqs(secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """the equations z_t(x) ^ z_t(secret) = 0 as equation ints over the cubic columns, through the set product (the state bits stay
    linear forms, kept as equation ints)"""
    s = [1 << (1 + g) for g in range(n)]
    eqs = []
    for z in register_outputs(secret, n, taps, pos, count):
        f = [poly_of_form(s[p], n) for p in pos]
        p = f[0] ^ poly_mul(f[1], f[2]) ^ poly_mul(poly_mul(f[3], f[4]), f[5])
        eqs.append(poly_int(p, n) ^ z)
        s = register_step(s, taps)
    return eqs


def register_zeros(system, secret: int, taps: int, pos: tuple, count: int) -> list:
    """the same equations written with PackedCubicSystem.mul_bit, one single-bit vector per output"""
    (x,) = system.gens()
    n = len(x)
    s = [x[g] for g in range(n)]
    zeros = []
    for z in register_outputs(secret, n, taps, pos, count):
        zeros.append(s[pos[0]] ^ system.mul_bit(s[pos[1]], s[pos[2]]) ^ system.mul_bit(system.mul_bit(s[pos[3]], s[pos[4]]), s[pos[5]]) ^ z)
        nxt = s[1:] + [None]
        out = s[0]
        s = [(out if nxt[g] is None else nxt[g] ^ out) if (taps >> g) & 1 else (x[0] ^ x[0] if nxt[g] is None else nxt[g]) for g in range(n)]
    return zeros


REGISTER_12 = dict(n=12, taps=0xE08, pos=(1, 3, 5, 7, 9, 11))
REGISTER_16 = dict(n=16, taps=0xB400, pos=(1, 4, 7, 10, 13, 15))

__all__ = ["IntBasis", "REGISTER_12", "REGISTER_16", "bits_of", "expand_ints", "poly_int", "poly_mul", "poly_of_form", "poly_value", "random_cubic_terms",
           "random_forms", "register_eqs", "register_outputs", "register_zeros", "row_polys", "to_aug", "xl3_cols"]
