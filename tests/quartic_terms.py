"""Helpers of the packed quartic front-end's tests.  Factored rows with products of two, three and four affine forms are expanded on the
host through the set-of-monomials product of tests/cubic_terms.py (poly_mul) and the column functions of tests/cubic_xl4_terms.py
(poly_int4): both are degree-agnostic and share no formula with any kernel.  The filtered register's equations come from a second
method that shares nothing with the set product either: truth tables of the outputs over all 2^n states and a Moebius transform."""
import functools

import numpy as np

from gf2bv_amd import hip
from gf2bv_amd.linsys import xl3_cols, xl4_cols
from tests.cubic_terms import IntBasis, poly_mul, poly_of_form, poly_value, random_forms
from tests.cubic_xl4_terms import poly_int4, quartic_aug
from tests.quad_terms import row_ints

ARITIES = (2, 3, 4)


def split_terms(terms) -> tuple:
    """(lin, [(off, operands) per arity]) of the thirteen arrays lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd"""
    return terms[0], [(terms[1], terms[2:4]), (terms[4], terms[5:8]), (terms[8], terms[9:13])]


def row_polys4(n: int, *terms) -> list:
    """every factored row as a set of monomials"""
    lin, groups = split_terms(terms)
    forms = lambda a: [poly_of_form(v, n) for v in row_ints(a)]            # noqa: E731
    out = forms(lin)
    for off, ops in groups:
        ops = [forms(x) for x in ops]
        for r in range(len(out)):
            for t in range(int(off[r]), int(off[r + 1])):
                prod = ops[0][t]
                for x in ops[1:]:
                    prod = poly_mul(prod, x[t])
                out[r] = out[r] ^ prod
    return out


def expand_ints4(n: int, *terms) -> list:
    """equation ints over the quartic columns of factored rows, through the set product"""
    return [poly_int4(p, n) for p in row_polys4(n, *terms)]


def bits_of4(v) -> list:
    """the expanded equation ints of a PackedQuarticBitVec (or of a PackedBitVec: its own bits)"""
    if hasattr(v, "_va"):
        return expand_ints4(v._n, v._lin, v._off2, v._ta, v._tb, v._off3, v._ua, v._ub, v._uc, v._off4, v._va, v._vb, v._vc, v._vd)
    return list(v._bits)


def _form(n: int, v: int) -> np.ndarray:
    wl = (n + 1 + 63) // 64
    return np.frombuffer(int(v).to_bytes(8 * wl, "little"), dtype=np.uint64).copy()


def build_terms(n: int, rows: list) -> tuple:
    """the thirteen arrays of rows given as (lin, [(a, b), ...], [(a, b, c), ...], [(a, b, c, d), ...]) with every form an equation
    int (bit 0 constant, bit 1 + g unknown g)"""
    wl = (n + 1 + 63) // 64
    out = [np.array([_form(n, r[0]) for r in rows], dtype=np.uint64).reshape(len(rows), wl)]
    for g, arity in enumerate(ARITIES):
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(r[1 + g]) for r in rows], out=off[1:])
        out.append(off)
        for k in range(arity):
            out.append(np.array([_form(n, t[k]) for r in rows for t in r[1 + g]], dtype=np.uint64).reshape(int(off[-1]), wl))
    return tuple(out)


def _ints(rng, n: int, count: int, constants: bool = True) -> list:
    return [int(v) for v in row_ints(random_forms(rng, n, count, constants))]


def _dense(rng, n: int) -> int:
    return (rng.getrandbits(n) | 1 | (1 << (n - 1))) << 1 | rng.getrandbits(1)


def case_rows(rng, n: int) -> list:
    """The rows of the expansion tests, one kind each (see test_gpu_packed_quartic.py): rows without terms of one, two or all
    arities; a fourth operand that is 0, the constant 1, a single unknown and dense (with dense partners, so that the multiplier the
    kernel picks is dense too); two equal quartic terms, which cancel; and one row per arity with one term more than a pass of the
    kernel holds (hip.quartic_chunks).  Constants are allowed everywhere, the zero form and the constant-1 form occur."""
    t2, t3, t4 = hip.quartic_chunks(n)
    term = lambda k: tuple(_ints(rng, n, k))                               # noqa: E731
    terms = lambda k, count: [term(k) for _ in range(count)]               # noqa: E731
    lin = lambda: _ints(rng, n, 1)[0]                                      # noqa: E731
    x = 1 << (1 + rng.randrange(n))
    same = term(4)
    return [
        (lin(), [], [], []),                                               # linear only
        (0, terms(2, t2 + 1), [], []),                                     # quadratic only, one more than a pass; the linear part is the zero form
        (lin(), [], terms(3, t3 + 1), []),                                 # cubic only, one more than a pass
        (lin(), [], [], terms(4, t4 + 1)),                                 # quartic only, one more than a pass
        (1, [], terms(3, 2), terms(4, 1)),                                 # no quadratic term; the linear part is the constant 1
        (lin(), terms(2, 2), [], terms(4, 2)),                             # no cubic term
        (lin(), terms(2, 1), terms(3, 1), []),                             # no quartic term
        (lin(), terms(2, 1), [], [term(3) + (0,)]),                        # a fourth operand that is 0: the term vanishes
        (lin(), [], terms(3, 1), [term(3) + (1,)]),                        # ... that is 1: the term is a b c
        (lin(), [], [], [term(3) + (x,)]),                                 # ... that is a single unknown
        (lin(), [], [], [tuple(_dense(rng, n) for _ in range(4))]),        # ... that is dense, like the other three
        (lin(), terms(2, 1), [], [same, term(4), same]),                   # two equal quartic terms cancel
        (lin(), terms(2, t2 + 2), terms(3, t3 + 1), terms(4, 2 * t4 + 1)),  # several passes of every kind at once
    ]


def random_quartic_terms(rng, n: int, rows: int, max_terms: int = 2, constants: bool = True) -> tuple:
    """random factored rows with up to `max_terms` terms of each arity"""
    out = []
    for _ in range(rows):
        out.append((_ints(rng, n, 1, constants)[0],) + tuple([tuple(_ints(rng, n, k, constants)) for _ in range(rng.randint(0, max_terms))]
                                                              for k in ARITIES))
    return build_terms(n, out)


def plant(n: int, terms: tuple, point: int) -> tuple:
    """the same rows with their constants set so that every one vanishes at `point`; returns (terms, equation ints)"""
    polys = row_polys4(n, *terms)
    lin = terms[0].copy()
    for r, p in enumerate(polys):
        lin[r, 0] ^= np.uint64(poly_value(p, point))
    terms = (lin,) + tuple(terms[1:])
    return terms, expand_ints4(n, *terms)


# -- the filtered register: z = s_p0 ^ s_p1 s_p2 ^ s_p3 s_p4 s_p5 ^ s_p6 s_p7 s_p8 s_p9 before the step of tests/cubic_terms.py ------------
REGISTER4_12 = dict(n=12, taps=0xE08, pos=(1, 3, 5, 7, 9, 11, 0, 2, 6, 10))
REGISTER4_16 = dict(n=16, taps=0xB400, pos=(1, 4, 7, 10, 13, 15, 2, 5, 8, 12))


def _filter(s: list, pos: tuple, mul):
    p = [s[k] for k in pos]
    return p[0], mul(p[1], p[2]), mul(mul(p[3], p[4]), p[5]), mul(mul(p[6], p[7]), mul(p[8], p[9]))


@functools.lru_cache(maxsize=None)
def register4_streams(n: int, taps: int, pos: tuple, count: int) -> np.ndarray:
    """[count, 2^n] output bits of the register from every state, by numpy over all states at once (read-only, shared)"""
    s = [((np.arange(1 << n, dtype=np.uint32) >> g) & 1).astype(np.uint8) for g in range(n)]
    out = []
    for _ in range(count):
        a, b, c, d = _filter(s, pos, lambda u, v: u & v)
        out.append(a ^ b ^ c ^ d)
        first, nxt = s[0], s[1:] + [np.zeros_like(s[0])]
        s = [(nxt[g] ^ first) if (taps >> g) & 1 else nxt[g] for g in range(n)]
    out = np.array(out)
    out.setflags(write=False)
    return out


def register4_brute(secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """every state whose first `count` outputs are the secret's, ascending"""
    streams = register4_streams(n, taps, pos, count)
    return [int(x) for x in np.flatnonzero((streams == streams[:, secret:secret + 1]).all(axis=0))]


@functools.lru_cache(maxsize=None)
def _register4_anf(n: int, taps: int, pos: tuple, count: int) -> tuple:
    """per output the equation int over the quartic columns of z_t as a polynomial of the initial state: the Moebius transform of
    its truth table, coefficient of the monomial with members m at index sum 2^g"""
    anf = register4_streams(n, taps, pos, count).copy()
    for g in range(n):
        a = anf.reshape(count, -1, 2, 1 << g)
        a[:, :, 1, :] ^= a[:, :, 0, :]
    bit = {}
    eqs = []
    for row in anf:
        e = 0
        for m in np.flatnonzero(row):
            m = int(m)
            if m not in bit:
                members = frozenset(g for g in range(n) if (m >> g) & 1)
                assert len(members) <= 4, "the register's outputs are of degree 4 at most"
                bit[m] = poly_int4(frozenset([members]), n)
            e ^= bit[m]
        eqs.append(e)
    return tuple(eqs)


def register4_eqs(secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """the equations z_t(x) ^ z_t(secret) = 0 as equation ints over the quartic columns, by the truth-table method"""
    z = register4_streams(n, taps, pos, count)[:, secret]
    return [e ^ int(b) for e, b in zip(_register4_anf(n, taps, pos, count), z)]


def register4_zeros(system, secret: int, n: int, taps: int, pos: tuple, count: int) -> list:
    """the same equations written with PackedQuarticSystem.mul_bit, one single-bit vector per output; the quartic term is the
    product of two quadratic bits"""
    (x,) = system.gens()
    assert len(x) == n
    s = [x[g] for g in range(n)]
    state = [(secret >> g) & 1 for g in range(n)]
    zeros = []
    for _ in range(count):
        a, b, c, d = _filter(state, pos, lambda u, v: u & v)
        fa, fb, fc, fd = _filter(s, pos, system.mul_bit)
        zeros.append(fa ^ fb ^ fc ^ fd ^ (a ^ b ^ c ^ d))
        state = [(state[g + 1] if g + 1 < n else 0) ^ (state[0] if (taps >> g) & 1 else 0) for g in range(n)]
        nxt, out = s[1:] + [x[0] ^ x[0]], s[0]
        s = [nxt[g] ^ out if (taps >> g) & 1 else nxt[g] for g in range(n)]
    return zeros


__all__ = ["ARITIES", "IntBasis", "REGISTER4_12", "REGISTER4_16", "bits_of4", "build_terms", "case_rows", "expand_ints4", "plant", "poly_int4",
           "quartic_aug", "random_quartic_terms", "register4_brute", "register4_eqs", "register4_streams", "register4_zeros", "row_polys4",
           "split_terms", "xl3_cols", "xl4_cols"]
