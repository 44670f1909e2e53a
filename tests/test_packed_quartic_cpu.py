"""The packed quartic front-end without a GPU: the algebra of PackedQuarticBitVec / PackedQuarticSystem against the set-of-monomials
oracle (tests/quartic_terms.py), the refusals, the argument checks of every new entry, and the rank table of the filtered register,
recomputed from truth tables."""
import ctypes
import pickle
import random

import numpy as np
import pytest

import gf2bv_amd
from gf2bv_amd import (BitVec, PackedCubicSystem, PackedQuadraticSystem, PackedQuarticBitVec, PackedQuarticSystem, hip, search_all_cubic,
                       search_all_xl)
from gf2bv_amd._internal import m4ri_solve_quartic_packed
from gf2bv_amd.linsys import xl3_cols, xl4_cols, xl4_quad_col
from tests.cubic_terms import poly_mul, poly_value
from tests.quartic_terms import (REGISTER4_12, IntBasis, bits_of4, build_terms, case_rows, expand_ints4, poly_int4, random_quartic_terms,
                                 register4_eqs, register4_zeros)

ONE = frozenset([frozenset()])


class Twin4:
    """one expression as a PackedQuarticBitVec (or PackedBitVec) and as a set of monomials, built in step"""

    def __init__(self, sizes):
        self.p = PackedQuarticSystem(sizes)
        self.n = sum(sizes)
        self.x = self.p.gens()[0]
        for g in self.p.gens()[1:]:
            self.x = self.x.concat(g)

    def linear(self, rng, constant: bool = True):
        i = rng.randrange(self.n)
        a, s = self.x[i], frozenset([frozenset((i,))])
        for _ in range(rng.randint(0, 3)):
            i = rng.randrange(self.n)
            a, s = a ^ self.x[i], s ^ frozenset([frozenset((i,))])
        if constant and rng.random() < 0.5:
            a, s = a ^ 1, s ^ ONE
        return a, s

    def mul(self, u, v):
        return self.p.mul_bit(u[0], v[0]), poly_mul(u[1], v[1])

    def of_degree(self, rng, degree: int):
        """a single bit of that structural degree: a sum of two products of `degree` linear forms (built left to right) and a form"""
        a, s = self.linear(rng)
        for _ in range(2 if degree > 1 else 0):
            t = self.linear(rng)
            for _ in range(degree - 1):
                t = self.mul(t, self.linear(rng))
            a, s = a ^ t[0], s ^ t[1]
        return a, s

    def bit(self, rng):
        """a random single bit of degree <= 4 with terms of every arity, the quartic ones built as (a b)(c d), ((a b) c) d and
        a (b (c d)); repeated terms and squares included"""
        a, s = self.of_degree(rng, rng.randint(1, 3))
        for shape in rng.sample(("22", "31", "13"), rng.randint(0, 2)):
            f = [self.linear(rng) for _ in range(4)]
            if rng.random() < 0.2:
                f[1] = f[0]
            if shape == "22":
                t = self.mul(self.mul(f[0], f[1]), self.mul(f[2], f[3]))
            elif shape == "31":
                t = self.mul(self.mul(self.mul(f[0], f[1]), f[2]), f[3])
            else:
                t = self.mul(f[0], self.mul(f[1], self.mul(f[2], f[3])))
            a, s = a ^ t[0], s ^ t[1]
        return a, s


@pytest.mark.parametrize("n", [5, 20, 70])
@pytest.mark.parametrize("da, db", [(1, 1), (2, 1), (3, 1), (2, 2), (1, 3)])
def test_mul_bit_of_every_degree_pair_is_the_set_product(n, da, db):
    rng = random.Random(1000 * n + 10 * da + db)
    tw = Twin4([n] if n == 5 else [n - 3, 3])
    for _ in range(4):
        a, b = tw.of_degree(rng, da), tw.of_degree(rng, db)
        assert (a[0]._degree() if da > 1 else 1, b[0]._degree() if db > 1 else 1) == (da, db)
        got, want = tw.mul(a, b)
        assert isinstance(got, PackedQuarticBitVec) and got._degree() == da + db and len(got) == 1
        assert got._eq_ints() == [poly_int4(want, n)] == bits_of4(got)


@pytest.mark.parametrize("da, db", [(3, 2), (4, 1), (2, 3)])
def test_mul_bit_above_degree_four_is_refused(da, db):
    rng = random.Random(da * 10 + db)
    tw = Twin4([6])
    a, b = tw.of_degree(rng, da)[0], tw.of_degree(rng, db)[0]
    with pytest.raises(TypeError) as e:
        tw.p.mul_bit(a, b)
    assert str(e.value) == f"mul_bit of bits of degree {da} and {db} is of degree {da + db}, above 4"


@pytest.mark.parametrize("n", [5, 20, 70])
def test_algebra_matches_set_oracle(n):
    rng = random.Random(n)
    tw = Twin4([n] if n == 5 else [n - 3, 3])
    bits = [tw.bit(rng) for _ in range(8)]
    want = [poly_int4(s, n) for _, s in bits]
    vec = bits[0][0]
    for a, _ in bits[1:]:
        vec = vec.concat(a)
    assert isinstance(vec, PackedQuarticBitVec) and len(vec) == 8 and vec._eq_ints() == want == bits_of4(vec)
    assert vec[2:7:2]._eq_ints() == want[2:7:2] and vec[-1]._eq_ints() == want[-1:] and vec[::-1]._eq_ints() == want[::-1]
    with pytest.raises(IndexError):
        vec[8]
    assert (vec ^ vec[::-1])._eq_ints() == [a ^ b for a, b in zip(want, want[::-1])]
    assert (vec ^ 0xA5)._eq_ints() == [w ^ ((0xA5 >> k) & 1) for k, w in enumerate(want)] == (0xA5 ^ vec)._eq_ints()
    lin = tw.x[:5].concat(tw.x[1:4])
    assert (vec ^ lin)._eq_ints() == (lin ^ vec)._eq_ints() == [w ^ b for w, b in zip(want, lin._bits)]
    assert lin[:2].concat(vec[:3])._eq_ints() == list(lin._bits[:2]) + want[:3]
    assert vec[:3].concat(lin[:2])._eq_ints() == want[:3] + list(lin._bits[:2])
    with pytest.raises(ValueError, match="different lengths"):
        vec ^ vec[:3]
    # distributivity with a quadratic factor on either side
    a, b, c, d, e = (tw.linear(rng) for _ in range(5))
    ab, cd = tw.mul(a, b), tw.mul(c, d)
    left = tw.p.mul_bit(ab[0] ^ e[0], cd[0])
    right = tw.p.mul_bit(ab[0], cd[0]) ^ tw.p.mul_bit(cd[0], e[0])
    assert left._eq_ints() == right._eq_ints() == [poly_int4(poly_mul(ab[1] ^ e[1], cd[1]), n)]
    # equal products cancel, whatever the order of their operands
    t1 = tw.p.mul_bit(tw.p.mul_bit(a[0], b[0]), tw.p.mul_bit(c[0], d[0]))
    t2 = tw.p.mul_bit(tw.p.mul_bit(tw.p.mul_bit(d[0], a[0]), c[0]), b[0])
    both = t1 ^ t2 ^ e[0]
    assert len(both._va) >= 2 and both._eq_ints() == [poly_int4(e[1], n)]


@pytest.mark.parametrize("n", [5, 20])
def test_evaluate_and_convert_sol_at_veronese_points(n):
    rng = random.Random(100 + n)
    tw = Twin4([n])
    bits = [tw.bit(rng) for _ in range(6)]
    vec = bits[0][0]
    for a, _ in bits[1:]:
        vec = vec.concat(a)
    for _ in range(5):
        x = rng.getrandbits(n)
        raw = tw.p._raw_point(x)
        assert tw.p._xl_products_match(raw, n, 4) and tw.p.convert_sol(raw) == (x,)
        want = sum(poly_value(s, x) << k for k, (_, s) in enumerate(bits))
        assert vec.evaluate(raw) == want == tw.p.evaluate(vec, (x,))
        assert tw.p.evaluate(tw.x, (x,)) == x
    full = tw.p._raw_point((1 << n) - 1)
    assert tw.p.convert_sol(full) == ((1 << n) - 1,)
    assert tw.p.convert_sol(full ^ (1 << xl4_quad_col(n, 4, 3, 1, 0))) is None      # one wrong quadruple coordinate
    assert tw.p.convert_sol(full ^ (1 << (xl4_cols(n) - 1))) is None
    assert tw.p.convert_sol(full ^ (1 << (xl3_cols(n) - 1))) is None                # a triple


def test_refusals():
    p = PackedQuarticSystem([6])
    (x,) = p.gens()
    q2 = p.mul_bit(x[0], x[1])
    q4 = p.mul_bit(q2, p.mul_bit(x[2], x[3]))
    assert isinstance(q2, PackedQuarticBitVec) and q2._degree() == 2 and q4._degree() == 4 and x[0]._rows.shape == (1, 1)
    assert not isinstance(p, PackedCubicSystem) and PackedQuarticBitVec._ARITIES == (2, 3, 4)
    with pytest.raises(ValueError, match="single bits"):
        p.mul_bit(x[:2], x[0])
    with pytest.raises(ValueError, match="different numbers of unknowns"):
        p.mul_bit(PackedQuarticSystem([100]).gens()[0][0], x[0])
    with pytest.raises(TypeError, match="mul_bit needs"):
        p.mul_bit(1, x[0])
    quad = PackedQuadraticSystem([6])
    qq = quad.mul_bit(quad.gens()[0][0], quad.gens()[0][1])
    for f in (lambda: q2 ^ qq, lambda: q2.concat(qq), lambda: p.mul_bit(qq, x[0]), lambda: p._terms([qq])):
        with pytest.raises(TypeError, match="_mul_bit"):
            f()
    with pytest.raises(TypeError):
        qq ^ q2
    cubic = PackedCubicSystem([6])
    cc = cubic.mul_bit(cubic.gens()[0][0], cubic.gens()[0][1])
    for f in (lambda: q2 ^ cc, lambda: q2.concat(cc), lambda: p.mul_bit(cc, x[0]), lambda: p.mul_bit(x[0], cc), lambda: p._terms([x, cc])):
        with pytest.raises(TypeError, match="PackedQuarticBitVec.*PackedCubicBitVec"):
            f()
    for f in (lambda: cc ^ q2, lambda: cc.concat(q2), lambda: cubic.mul_bit(q2, cc), lambda: cubic._terms([q2])):
        with pytest.raises(TypeError):
            f()
    with pytest.raises(TypeError, match="tuple-of-int"):
        q2 ^ BitVec((1,))
    for name in ("__and__", "__or__", "__lshift__", "__rshift__", "rotl", "sum", "zeroext", "dup", "broadcast"):
        with pytest.raises(TypeError, match=f"{name} is not supported on a PackedQuarticBitVec"):
            getattr(q4, name)(1)
    for name in ("factor", "bit_assert", "solve_one_rhs", "solve_raw_one_rhs", "solve_raw_space_rhs", "get_rows"):
        with pytest.raises(TypeError) as e:
            getattr(p, name)([q2])
        assert str(e.value) == f"{name} is not built for a PackedQuarticSystem"
    with pytest.raises(TypeError, match="is not built for a PackedCubicSystem"):   # (the cubic class's own message is unchanged)
        cubic.factor([cc])
    with pytest.raises(TypeError, match="0 or 1"):
        p._terms([6])
    # the searches take what they took before
    with pytest.raises(TypeError, match="search_\\*_cubic needs a PackedCubicSystem"):
        search_all_cubic(p, [])
    with pytest.raises(TypeError, match="search_\\*_xl needs a QuadraticSystem"):
        search_all_xl(p, [])
    # bare 0 / 1 and PackedBitVec rows are accepted (q4 = (0 ^ x0 x1)(0 ^ x2 x3) carries the quadratic term 0 * 0 and the cubic
    # terms x0 x1 * 0 and x2 x3 * 0 beside its quartic one)
    terms = p._terms([0, x[:2], q4 ^ q2, 1])
    assert len(terms) == 13 and terms[0].shape == (5, 1) and terms[0][4, 0] == 1
    assert [list(terms[k]) for k in (1, 4, 8)] == [[0, 0, 0, 0, 2, 2], [0, 0, 0, 0, 2, 2], [0, 0, 0, 0, 1, 1]]
    assert [len(terms[k]) for k in (2, 3, 5, 9, 12)] == [2, 2, 2, 1, 1]
    assert (q4 ^ q2)._eq_ints() == [(1 << (1 + xl4_quad_col(6, 3, 2, 1, 0))) | (1 << (1 + 6))]      # x0 x1 x2 x3 + x1 x0 (pair (1, 0) at column 6)
    assert [len(a) for a in p._terms([])] == [0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]


def test_names_and_pickle_round_trip():
    assert "PackedQuarticSystem" in gf2bv_amd.__all__ and "PackedQuarticBitVec" in gf2bv_amd.__all__
    assert gf2bv_amd.PackedQuarticSystem is PackedQuarticSystem
    p = PackedQuarticSystem([5, 9])
    p2 = pickle.loads(pickle.dumps(p))
    assert p2._sizes == [5, 9] and p2._cols == p._cols == xl4_cols(14) and [len(g) for g in p2.gens()] == [5, 9]
    x, y = p.gens()
    v = (p.mul_bit(p.mul_bit(x[0], y[3]), p.mul_bit(y[4], y[7])) ^ p.mul_bit(p.mul_bit(x[1], x[2]), y[0]) ^ p.mul_bit(x[1], x[2]) ^ y[1]
         ^ 1).concat(p.mul_bit(y[8], y[8]))
    v2 = pickle.loads(pickle.dumps(v))
    assert isinstance(v2, PackedQuarticBitVec) and v2._eq_ints() == v._eq_ints() == bits_of4(v) and v2._n == 14


def test_chunks():
    """positive and non-increasing in n, the LDS they ask for within 160 KiB; beyond about n = 157 two staged cubic rows do not fit"""
    prev = None
    for n in range(1, 158):
        t2, t3, t4 = c = hip.quartic_chunks(n)
        wl, w3 = (n + 1 + 63) // 64, (xl3_cols(n) + 1 + 63) // 64
        assert min(c) >= 1 and ((1 + 2 * t2 + 3 * t3 + 4 * t4) * wl + (1 + t4) * w3) * 8 <= 160 * 1024, (n, c)
        assert prev is None or all(a <= b for a, b in zip(c, prev)), (n, c, prev)
        prev = c
    assert hip.quartic_chunks(4) == hip.quartic_chunks(64) == (8, 8, 4) and hip.quartic_chunks(146) == (8, 8, 1)
    with pytest.raises(ValueError, match="do not fit"):
        hip.quartic_chunks(200)


def test_entries_check_arguments_before_device_use():
    """every GF2BV_ERR_ARG case of the new entries returns 1 with its message on a machine without a GPU too"""
    L = hip.lib()
    n, live = 6, 40                                    # 56 columns
    rows = 57
    terms = random_quartic_terms(random.Random(3), n, live)
    assert all(t[-1] > 0 for t in (terms[1], terms[4], terms[8]))
    aug = np.zeros((rows + 1, 4), dtype=np.uint64)
    P = [a.ctypes.data for a in terms]
    A = aug.ctypes.data
    A += -A % 16
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    def swap(k, v):
        return P[:k] + [v] + P[k + 1:]

    bad = {}
    for k in (1, 4, 8):
        bad[k, "start"], bad[k, "dec"] = terms[k].copy(), terms[k].copy()
        bad[k, "start"][0] = 1
        bad[k, "dec"][20] = bad[k, "dec"][19] - 1
    empty = np.zeros(live + 1, dtype=np.int64)
    for name in ("words", "solve"):
        f = L.gf2bv_quartic_expand_words if name == "words" else L.gf2bv_solve_quartic_terms
        tail = (lambda o=A: (o, 2, 0)) if name == "words" else (lambda o=H: (0, 0, o))
        for k in range(13):
            err(f(*swap(k, None), live, rows, n, *tail()), "null")
        err(f(*P, live, rows, n, *tail(o=None)), "null")
        # operands may be null where their count is 0: the next check is reached
        for at, arity in ((1, 2), (4, 3), (8, 4)):
            args = P[:at] + [empty.ctypes.data] + [None] * arity + P[at + 1 + arity:]
            assert f(*args, live, rows, 0, *tail()) == 1 and b"n_lin" in L.gf2bv_last_error()
        err(f(*P, live, rows, 0, *tail()), "n_lin")
        err(f(*P, live, rows, 500, *tail()), "n_lin")              # cols4 >= 2^31 - 64
        err(f(*P, live, rows, 70000, *tail()), "n_lin")
        err(f(*P, live, rows, 200, *tail()), "do not fit")         # two staged cubic rows are beyond the LDS
        err(f(*P, rows + 1, rows, n, *tail()), "rows_live")
        err(f(*P, -1, rows, n, *tail()), "rows_live")
        for k in (1, 4, 8):
            err(f(*swap(k, bad[k, "start"].ctypes.data), live, rows, n, *tail()), "start at 0")
            err(f(*swap(k, bad[k, "dec"].ctypes.data), live, rows, n, *tail()), "must not decrease")
    err(L.gf2bv_quartic_expand_words(*P, live, rows, n, A, 0, 0), "stride")
    err(L.gf2bv_solve_quartic_terms(*P, live, 55, n, 0, 0, H), "greater than or equal")
    err(L.gf2bv_solve_quartic_terms(*P, live, rows, n, 3, 0, H), "Invalid mode")
    D = L.gf2bv_quartic_expand_device
    for k in range(13):
        err(D(*swap(k, None), live, rows, n, A, 2, 0, None), "null")
    err(D(*P, live, rows, n, None, 2, 0, None), "null")
    err(D(*P, live, rows, 0, A, 2, 0, None), "n_lin")
    err(D(*P, live, rows, 500, A, 2, 0, None), "n_lin")
    err(D(*P, live, rows, 200, A, 2, 0, None), "do not fit")
    err(D(*P, rows + 1, rows, n, A, 2, 0, None), "rows_live")
    err(D(*P, live, rows, n, A, 3, 0, None), "stride")
    err(D(*P, live, rows, n, A, 0, 0, None), "stride")
    err(D(*P, live, rows, n, A + 8, 2, 0, None), "16-byte alignment")
    assert not h.value
    c = [ctypes.c_int32() for _ in range(3)]
    err(L.gf2bv_quartic_chunks(0, *map(ctypes.byref, c)), "n_lin")
    for k in range(3):
        err(L.gf2bv_quartic_chunks(9, *[None if j == k else ctypes.byref(c[j]) for j in range(3)]), "null")
    # the bindings: sizes checked against each other, library errors as ValueError
    with pytest.raises(ValueError, match="off4"):
        hip.quartic_expand_words(*terms[:8], terms[8][:-1], *terms[9:], n)
    with pytest.raises(ValueError, match="off4"):
        hip.solve_quartic_terms(*terms[:12], terms[12][:-1], n)
    with pytest.raises(ValueError, match="off3"):
        hip.quartic_expand_words(*terms[:4], terms[4][:-1], *terms[5:], n)
    with pytest.raises(ValueError, match="greater than or equal"):
        hip.solve_quartic_terms(*terms, n, rows=55)
    with pytest.raises(ValueError, match="stride"):
        hip.quartic_expand_words(*terms, n, stride_words=0)
    with pytest.raises(ValueError, match="null"):
        hip.quartic_expand_device(0, *P[1:], live, rows, n, A, 2)
    M = m4ri_solve_quartic_packed
    with pytest.raises(ValueError, match="whole rows"):
        M(terms[0].tobytes()[:-4], *terms[1:], n, rows, 0)
    for k in (1, 4, 8):
        with pytest.raises(ValueError, match="off2, off3 and off4 must hold one int64 per row"):
            M(*terms[:k], terms[k][:-1].copy(), *terms[k + 1:], n, rows, 0)
        with pytest.raises(ValueError, match="off2, off3 and off4 must start at 0"):
            M(*terms[:k], bad[k, "start"], *terms[k + 1:], n, rows, 0)
        with pytest.raises(ValueError, match="off2, off3 and off4 must not decrease"):
            M(*terms[:k], bad[k, "dec"], *terms[k + 1:], n, rows, 0)
    with pytest.raises(ValueError, match="same number"):
        M(*terms[:12], terms[12][:-1].copy(), n, rows, 0)
    with pytest.raises(ValueError, match="end at the number"):
        M(*terms[:9], *[a[:-1].copy() for a in terms[9:]], n, rows, 0)
    with pytest.raises(ValueError, match="at least the rows of lin"):
        M(*terms, n, live - 1, 0)
    with pytest.raises(ValueError, match="n_lin"):
        M(*terms, 0, rows, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        M(*terms, n, rows, 5)
    with pytest.raises(ValueError, match="greater than or equal"):
        M(*terms, n, 55, 1)
    with pytest.raises(TypeError):
        M(*terms, n, rows)


def test_case_rows_cover_the_cases():
    """the generator of the GPU tests gives what it promises: every kind of row, the chunk exceeded by one for each arity, and
    host expansions of the package and of the set oracle that agree"""
    n = 12
    rows = case_rows(random.Random(1), n)
    terms = build_terms(n, rows)
    t2, t3, t4 = hip.quartic_chunks(n)
    c2, c3, c4 = (np.diff(terms[k]) for k in (1, 4, 8))
    assert (c2[0], c3[0], c4[0]) == (0, 0, 0) and c2[1] == t2 + 1 and c3[2] == t3 + 1 and c4[3] == t4 + 1
    assert any(a == 0 and b and c for a, b, c in zip(c2, c3, c4)) and any(a and b == 0 and c for a, b, c in zip(c2, c3, c4))
    assert any(a and b and c == 0 for a, b, c in zip(c2, c3, c4)) and c2[-1] > t2 and c3[-1] > t3 and c4[-1] > 2 * t4
    fourth = [int(v) for v in terms[12][:, 0]]
    assert 0 in fourth and 1 in fourth and any(bin(v).count("1") == 1 and v > 1 for v in fourth) and any(bin(v).count("1") > 3 for v in fourth)
    ints = expand_ints4(n, *terms)
    assert PackedQuarticBitVec(*terms, n)._eq_ints() == ints
    assert max(e.bit_length() for e in ints) > 1 + xl3_cols(n)            # quadruples are there
    # the row of two equal quartic terms is what it is without them
    r = 11
    assert rows[r][3][0] == rows[r][3][2]
    assert ints[r] == expand_ints4(n, *build_terms(n, [(rows[r][0], rows[r][1], [], [rows[r][3][1]])]))[0]


def test_register_rank_table():
    """n = 12, taps 0xE08, z = s1 ^ s3 s5 ^ s7 s9 s11 ^ s0 s2 s6 s10 over the 793 quartic columns.  The equations come from truth
    tables and a Moebius transform; the ones written with mul_bit are the same ints, by the package's host expansion and by the set
    product.  The first 793 rows are independent."""
    n, secret = 12, 0x52F
    assert xl4_cols(n) == 793
    eqs = register4_eqs(secret, count=800, **REGISTER4_12)
    p = PackedQuarticSystem([n])
    zeros = register4_zeros(p, secret, count=800, **REGISTER4_12)
    vec = zeros[0]
    for z in zeros[1:]:
        vec = vec.concat(z)
    assert vec._eq_ints() == eqs and bits_of4(vec[:64]) == eqs[:64]
    basis, rank = IntBasis(), {}
    for k, e in enumerate(eqs):
        basis.add(e >> 1)
        rank[k + 1] = len(basis)
    assert [rank[k] for k in (700, 780, 781, 793, 800)] == [700, 780, 781, 793, 793]
    point = p._raw_point(secret)
    assert all(bin((e >> 1) & point).count("1") & 1 == e & 1 for e in eqs)      # every equation vanishes at the secret's point
    assert register4_eqs(0x3A1, count=800, **REGISTER4_12)[:793] != eqs[:793]
