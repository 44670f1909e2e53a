"""The packed cubic front-end without a GPU: the algebra of PackedCubicBitVec / PackedCubicSystem against the set-of-monomials oracle
(tests/cubic_terms.py), the refusals, the argument checks of every new entry, and the known answers of the filtered register."""
import ctypes
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

from gf2bv_amd import BitVec, DimensionTooLargeError, PackedCubicBitVec, PackedCubicSystem, PackedQuadraticSystem, hip
from gf2bv_amd import _internal
from gf2bv_amd._internal import m4ri_solve_cubic_packed
from gf2bv_amd.linsys import xl3_cols
from oracle import gf2_oracle as O
from tests.cubic_terms import (REGISTER_12, bits_of, poly_int, poly_mul, poly_of_form, poly_value, random_cubic_terms, register_eqs,
                               register_zeros, row_polys)


class Twin:
    """one expression as a PackedCubicBitVec (or PackedBitVec) and as a set of monomials, built in step"""

    def __init__(self, sizes):
        self.p = PackedCubicSystem(sizes)
        self.n = sum(sizes)
        self.x = self.p.gens()[0]
        for g in self.p.gens()[1:]:
            self.x = self.x.concat(g)

    def linear(self, rng, constant: bool):
        a, s = self.x[rng.randrange(self.n)], None
        s = poly_of_form(a._bits[0], self.n)
        for _ in range(rng.randint(0, 3)):
            i = rng.randrange(self.n)
            a, s = a ^ self.x[i], s ^ frozenset([frozenset((i,))])
        if constant and rng.random() < 0.5:
            a, s = a ^ 1, s ^ frozenset([frozenset()])
        return a, s

    def mul(self, u, v):
        return self.p.mul_bit(u[0], v[0]), poly_mul(u[1], v[1])

    def bit(self, rng, constant: bool):
        """a random single bit of degree <= 3: a linear form, some products of two and some products of three, the latter built in
        either order ((a b) c and a (b c)), squares and repeated terms included"""
        a, s = self.linear(rng, constant)
        for _ in range(rng.randint(0, 2)):
            u, v = self.linear(rng, constant), self.linear(rng, constant)
            if rng.random() < 0.2:
                v = u
            t = self.mul(u, v)
            a, s = a ^ t[0], s ^ t[1]
            if rng.random() < 0.3:
                a, s = a ^ t[0] ^ t[0], s ^ t[1] ^ t[1]
        for _ in range(rng.randint(0, 2)):
            u, v, w = self.linear(rng, constant), self.linear(rng, constant), self.linear(rng, constant)
            if rng.random() < 0.2:
                v = w = u
            t = self.mul(self.mul(u, v), w) if rng.random() < 0.5 else self.mul(u, self.mul(v, w))
            a, s = a ^ t[0], s ^ t[1]
        return a, s


@pytest.mark.parametrize("n", [5, 20, 70])
def test_algebra_matches_set_oracle(n):
    rng = random.Random(n)
    tw = Twin([n] if n == 5 else [n - 3, 3])
    bits = [tw.bit(rng, constant=k % 2 == 0) for k in range(8)]
    want = [poly_int(s, n) for _, s in bits]
    assert [bits_of(a)[0] for a, _ in bits] == want
    # distributivity: (a ^ b) c == a c ^ b c, with a quadratic factor on either side
    for _ in range(6):
        a, b, c, d = (tw.linear(rng, True) for _ in range(4))
        ab = tw.mul(a, b)
        left = tw.p.mul_bit(ab[0] ^ d[0], c[0])
        right = tw.p.mul_bit(ab[0], c[0]) ^ tw.p.mul_bit(c[0], d[0])
        both = poly_int(poly_mul(ab[1] ^ d[1], c[1]), n)
        assert bits_of(left) == bits_of(right) == [both]
    # concat, slicing, indexing, ^ with a vector, a PackedBitVec and a constant
    vec = bits[0][0]
    for a, _ in bits[1:]:
        vec = vec.concat(a)
    assert isinstance(vec, PackedCubicBitVec) and len(vec) == 8 and bits_of(vec) == want
    assert bits_of(vec[2:7:2]) == want[2:7:2] and bits_of(vec[-1]) == want[-1:] and bits_of(vec[::-1]) == want[::-1]
    with pytest.raises(IndexError):
        vec[8]
    assert bits_of(vec ^ vec[::-1]) == [a ^ b for a, b in zip(want, want[::-1])]
    assert bits_of(vec ^ 0xA5) == [w ^ ((0xA5 >> k) & 1) for k, w in enumerate(want)]
    assert bits_of(0xA5 ^ vec) == bits_of(vec ^ 0xA5)
    lin = tw.x[:5].concat(tw.x[1:4])
    assert bits_of(vec ^ lin) == bits_of(lin ^ vec) == [w ^ b for w, b in zip(want, lin._bits)]
    assert bits_of(lin[:2].concat(vec[:3])) == list(lin._bits[:2]) + want[:3]
    assert bits_of(vec[:3].concat(lin[:2])) == want[:3] + list(lin._bits[:2])
    with pytest.raises(ValueError, match="different lengths"):
        vec ^ vec[:3]


@pytest.mark.parametrize("n", [5, 20])
def test_evaluate_at_consistent_points(n):
    rng = random.Random(100 + n)
    tw = Twin([n])
    bits = [tw.bit(rng, constant=True) for _ in range(6)]
    vec = bits[0][0]
    for a, _ in bits[1:]:
        vec = vec.concat(a)
    for _ in range(5):
        x = rng.getrandbits(n)
        raw = tw.p._raw_point(x)
        assert tw.p._xl_products_match(raw, n, 3) and tw.p.convert_sol(raw) == (x,)
        want = sum(poly_value(s, x) << k for k, (_, s) in enumerate(bits))
        assert vec.evaluate(raw) == want == tw.p.evaluate(vec, (x,))
    assert tw.p.convert_sol(tw.p._raw_point(3) ^ (1 << (xl3_cols(n) - 1))) is None


def test_refusals():
    p = PackedCubicSystem([6])
    (x,) = p.gens()
    q2, q3 = p.mul_bit(x[0], x[1]), p.mul_bit(p.mul_bit(x[0], x[1]), x[2])
    assert isinstance(q2, PackedCubicBitVec) and q2._degree() == 2 and q3._degree() == 3 and x[0]._rows.shape == (1, 1)
    with pytest.raises(TypeError, match="degree 4"):
        p.mul_bit(q2, q2)
    with pytest.raises(TypeError, match="degree 4"):
        p.mul_bit(x[3], q3)
    with pytest.raises(TypeError, match="degree 5"):
        p.mul_bit(q3, q2)
    with pytest.raises(ValueError, match="single bits"):
        p.mul_bit(x[:2], x[0])
    with pytest.raises(ValueError, match="different numbers of unknowns"):
        p.mul_bit(PackedCubicSystem([100]).gens()[0][0], x[0])
    with pytest.raises(TypeError, match="mul_bit needs"):
        p.mul_bit(1, x[0])
    quad = PackedQuadraticSystem([6])
    qq = quad.mul_bit(quad.gens()[0][0], quad.gens()[0][1])
    for f in (lambda: q2 ^ qq, lambda: qq ^ q2, lambda: q2.concat(qq), lambda: p.mul_bit(qq, x[0]), lambda: p._terms([qq])):
        with pytest.raises(TypeError, match="_mul_bit"):
            f()
    with pytest.raises(TypeError, match="tuple-of-int"):
        q2 ^ BitVec((1,))
    for name in ("__and__", "__or__", "__lshift__", "__rshift__", "rotl", "sum", "zeroext", "dup", "broadcast"):
        with pytest.raises(TypeError, match=name):
            getattr(q3, name)(1)
    for name in ("factor", "bit_assert", "solve_one_rhs", "solve_raw_space_rhs", "get_rows"):
        with pytest.raises(TypeError, match=name):
            getattr(p, name)([q2])
    with pytest.raises(TypeError, match="0 or 1"):
        p._terms([6])
    # bare 0 / 1 and PackedBitVec rows are accepted (q3 = (0 ^ x0 x1) x2 carries the quadratic term 0 * x2 beside its cubic one)
    lin, off2, ta, tb, off3, ua, ub, uc = p._terms([0, x[:2], q3 ^ q2, 1])
    assert lin.shape == (5, 1) and list(off2) == [0, 0, 0, 0, 2, 2] and list(off3) == [0, 0, 0, 0, 1, 1] and lin[4, 0] == 1
    assert len(ta) == len(tb) == 2 and len(ua) == len(ub) == len(uc) == 1


def test_entries_check_arguments_before_device_use():
    """every GF2BV_ERR_ARG case of the new entries returns 1 with its message on a machine without a GPU too"""
    L = hip.lib()
    n, live = 9, 100                                   # 129 columns
    rows = 130
    terms = random_cubic_terms(random.Random(3), n, live)
    lin, off2, ta, tb, off3, ua, ub, uc = terms
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
    for k in (1, 4):
        bad[k, "start"], bad[k, "dec"] = terms[k].copy(), terms[k].copy()
        bad[k, "start"][0] = 1
        bad[k, "dec"][40] = bad[k, "dec"][39] - 1
    empty = np.zeros(live + 1, dtype=np.int64)
    for name in ("words", "solve"):
        f = L.gf2bv_cubic_expand_words if name == "words" else L.gf2bv_solve_cubic_terms
        tail = (lambda o=A: (o, 4, 0)) if name == "words" else (lambda o=H: (0, 0, o))
        for k in range(8):
            err(f(*swap(k, None), live, rows, n, *tail()), "null")
        err(f(*P, live, rows, n, *tail(o=None)), "null")
        # operands may be null where their count is 0
        assert f(*(P[:1] + [empty.ctypes.data, None, None] + P[4:]), live, rows, 0, *tail()) == 1 and b"n_lin" in L.gf2bv_last_error()
        assert f(*(P[:4] + [empty.ctypes.data, None, None, None]), live, rows, 0, *tail()) == 1 and b"n_lin" in L.gf2bv_last_error()
        err(f(*P, live, rows, 0, *tail()), "n_lin")
        err(f(*P, live, rows, 2400, *tail()), "n_lin")             # cols3 >= 2^31 - 64
        err(f(*P, rows + 1, rows, n, *tail()), "rows_live")
        err(f(*P, -1, rows, n, *tail()), "rows_live")
        for k in (1, 4):
            err(f(*swap(k, bad[k, "start"].ctypes.data), live, rows, n, *tail()), "start at 0")
            err(f(*swap(k, bad[k, "dec"].ctypes.data), live, rows, n, *tail()), "must not decrease")
    err(L.gf2bv_cubic_expand_words(*P, live, rows, n, A, 2, 0), "stride")
    err(L.gf2bv_solve_cubic_terms(*P, live, 128, n, 0, 0, H), "greater than or equal")
    err(L.gf2bv_solve_cubic_terms(*P, live, rows, n, 3, 0, H), "Invalid mode")
    err(L.gf2bv_solve_cubic_terms(*P, live, rows, n, 0, 0, None), "null")
    D = L.gf2bv_cubic_expand_device
    for k in range(8):
        err(D(*swap(k, None), live, rows, n, A, 4, 0, None), "null")
    err(D(*P, live, rows, n, None, 4, 0, None), "null")
    err(D(*P, live, rows, 0, A, 4, 0, None), "n_lin")
    err(D(*P, live, rows, 2400, A, 4, 0, None), "n_lin")
    err(D(*P, rows + 1, rows, n, A, 4, 0, None), "rows_live")
    err(D(*P, live, rows, n, A, 5, 0, None), "stride")
    err(D(*P, live, rows, n, A, 2, 0, None), "stride")
    err(D(*P, live, rows, n, A + 8, 4, 0, None), "16-byte alignment")
    assert not h.value
    q, c = ctypes.c_int32(), ctypes.c_int32()
    err(L.gf2bv_cubic_chunks(0, ctypes.byref(q), ctypes.byref(c)), "n_lin")
    err(L.gf2bv_cubic_chunks(9, None, ctypes.byref(c)), "null")
    # the chunk sizes: 64 KiB hold the linear part and every operand of a pass, at every length of a form (so the entries' own
    # "does not fit the LDS" refusal cannot be reached through n_lin <= 65535: the sizes shrink instead)
    for nn in (1, 9, 64, 12000, 40000, 65535):
        t2, t3 = hip.cubic_chunks(nn)
        assert t2 >= 1 and t3 >= 1 and (1 + 2 * t2 + 3 * t3) * ((nn + 1 + 63) // 64) * 8 <= 65536, (nn, t2, t3)
    assert hip.cubic_chunks(64) == (8, 8)
    # the bindings: sizes checked against each other, library errors as ValueError
    with pytest.raises(ValueError, match="term_off"):
        hip.cubic_expand_words(lin, off2[:-1], ta, tb, off3, ua, ub, uc, n)
    with pytest.raises(ValueError, match="off3"):
        hip.cubic_expand_words(lin, off2, ta, tb, off3[:-1], ua, ub, uc, n)
    with pytest.raises(ValueError, match="off3"):
        hip.solve_cubic_terms(lin, off2, ta, tb, off3, ua, ub[:-1], uc, n)
    with pytest.raises(ValueError, match="greater than or equal"):
        hip.solve_cubic_terms(lin, off2, ta, tb, off3, ua, ub, uc, n, rows=128)
    with pytest.raises(ValueError, match="stride"):
        hip.cubic_expand_words(lin, off2, ta, tb, off3, ua, ub, uc, n, stride_words=2)
    with pytest.raises(ValueError, match="null"):
        hip.cubic_expand_device(0, P[1], P[2], P[3], P[4], P[5], P[6], P[7], live, rows, n, A, 4)
    with pytest.raises(ValueError, match="stride"):
        hip.cubic_expand_device(*P, live, rows, n, A, 3)
    M = m4ri_solve_cubic_packed
    with pytest.raises(ValueError, match="whole rows"):
        M(lin.tobytes()[:-8], off2, ta, tb, off3, ua, ub, uc, 100, rows, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        M(lin, off2[:-1].copy(), ta, tb, off3, ua, ub, uc, n, rows, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        M(lin, off2, ta, tb, off3[:-1].copy(), ua, ub, uc, n, rows, 0)
    with pytest.raises(ValueError, match="same number"):
        M(lin, off2, ta, tb[:-1].copy(), off3, ua, ub, uc, n, rows, 0)
    with pytest.raises(ValueError, match="same number"):
        M(lin, off2, ta, tb, off3, ua, ub, uc[:-1].copy(), n, rows, 0)
    with pytest.raises(ValueError, match="end at the number"):
        M(lin, off2, ta, tb, off3, ua[:-1].copy(), ub[:-1].copy(), uc[:-1].copy(), n, rows, 0)
    with pytest.raises(ValueError, match="must start at 0"):           # (the extension's own check, not the library's)
        M(lin, bad[1, "start"], ta, tb, off3, ua, ub, uc, n, rows, 0)
    with pytest.raises(ValueError, match="must not decrease"):
        M(lin, off2, ta, tb, bad[4, "dec"], ua, ub, uc, n, rows, 0)
    with pytest.raises(ValueError, match="at least the rows of lin"):
        M(lin, off2, ta, tb, off3, ua, ub, uc, n, live - 1, 0)
    with pytest.raises(ValueError, match="n_lin"):
        M(lin, off2, ta, tb, off3, ua, ub, uc, 0, rows, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        M(lin, off2, ta, tb, off3, ua, ub, uc, n, rows, 5)
    with pytest.raises(ValueError, match="greater than or equal"):
        M(lin, off2, ta, tb, off3, ua, ub, uc, n, 128, 1)
    with pytest.raises(TypeError):
        M(lin, off2, ta, tb, off3, ua, ub, uc, n, rows)


# The factored-form parser of the extension, per entry and per group of products: (name, number of buffers, arguments behind them).
# n_lin = 3 (one word a form), two rows, one product per group; rows = the columns, so nothing but the buffers is wrong.
_TERM_ENTRIES = [("m4ri_solve_quad_packed", 4, (3, 6, 0)), ("m4ri_factor_quad_packed", 4, (3, 6, 0)), ("m4ri_solve_rhs_quad_packed", 4, (3, 6, 0, [0])),
                 ("m4ri_solve_many_quad_packed", 4, (np.array([0, 2], dtype=np.int64), 3, 6, 0)),
                 ("m4ri_solve_xl3_quad_packed", 4, (3, 0)), ("m4ri_solve_xl4_quad_packed", 4, (3, 0)),
                 ("m4ri_solve_xl3_guess_quad_packed", 4, (3, [0], 0, 2, 0)), ("m4ri_solve_xl4_guess_quad_packed", 4, (3, [0], 0, 2, 0)),
                 ("m4ri_solve_cubic_packed", 8, (3, 7, 0)), ("m4ri_solve_xl4_cubic_packed", 8, (3, 0))]
_QUAD_WORDS = {"len": "term_off must hold one int64 per row of lin and one more", "start": "term_off must start at 0",
               "order": "term_off must not decrease", "end": "term_off must end at the number of operands in ta",
               "ops": "ta and tb must hold the same number of whole operands",
               "ops and start": "ta and tb must hold the same number of whole operands"}       # (the operands are looked at first)
_CUBIC_WORDS = {"len": "off2 and off3 must hold one int64 per row of lin and one more", "start": "off2 and off3 must start at 0",
                "order": "off2 and off3 must not decrease", "end": "off2 and off3 must end at the number of operands of their products",
                "ops": "the operands of a product must hold the same number of whole forms",
                "ops and start": "off2 and off3 must start at 0"}                               # (the offsets are looked at first)


@pytest.mark.parametrize("entry, nbuf, tail, group", [(e, k, t, g) for e, k, t in _TERM_ENTRIES for g in range(k // 4)])
def test_term_parser_messages_per_entry_and_group(entry, nbuf, tail, group):
    """every refusal of the factored-form parser, word for word, before any device use"""
    f = getattr(_internal, entry)
    one = np.ones((1, 1), dtype=np.uint64)
    off = np.array([0, 1, 1], dtype=np.int64)
    good = [np.zeros((2, 1), dtype=np.uint64), off, one, one] + ([off, one, one, one] if nbuf == 8 else [])
    off_at, last_op = (1, 3) if group == 0 else (4, 7)
    words = _QUAD_WORDS if nbuf == 4 else _CUBIC_WORDS

    def refused(text, **swap):
        bufs = list(good)
        for k, v in swap.items():
            bufs[int(k[1:])] = v
        with pytest.raises(ValueError) as e:
            f(*bufs, *tail)
        assert str(e.value) == text

    two = np.ones((2, 1), dtype=np.uint64)
    refused("lin must hold whole rows of ceil((n_lin + 1) / 64) 64-bit words", b0=good[0].tobytes()[:-4])
    refused(words["len"], **{f"b{off_at}": off[:-1].copy()})
    refused(words["start"], **{f"b{off_at}": np.array([1, 1, 1], dtype=np.int64)})
    refused(words["order"], **{f"b{off_at}": np.array([0, 2, 1], dtype=np.int64)})
    refused(words["end"], **{f"b{off_at}": np.array([0, 1, 2], dtype=np.int64)})
    refused(words["ops"], **{f"b{last_op}": two})
    refused(words["ops and start"], **{f"b{last_op}": two, f"b{off_at}": np.array([1, 1, 1], dtype=np.int64)})


def _same_arrays(got, want):
    assert len(got) == len(want)
    for g, (dtype, values) in zip(got, want):
        w = np.array(values, dtype=dtype).reshape((len(values), 1) if dtype is np.uint64 else (len(values),))
        assert g.dtype == w.dtype and g.shape == w.shape and g.flags.c_contiguous and np.array_equal(g, w), (g, w)


def test_terms_layout_is_the_recorded_one():
    """``_terms`` of both systems on a literal 0, a literal 1, a sliced PackedBitVec, a vector with products and a concat of linear
    and product bits, n = 5: unknown i is bit 1 + i of the one word of a form, the expected arrays written down by hand"""
    U, I = np.uint64, np.int64
    p = PackedQuadraticSystem([5])
    (x,) = p.gens()
    q = p.mul_bit(x[0], x[1]) ^ x[2] ^ 1                                  # 1 + x2 + x0 x1
    w = p.mul_bit(x[3], x[4]) ^ p.mul_bit(x[0], x[2])                      # x3 x4 + x0 x2
    _same_arrays(p._terms([0, 1, x[1:3], q, x[4:5].concat(w)]),
                 [(U, [0, 1, 4, 8, 9, 32, 0]), (I, [0, 0, 0, 0, 0, 1, 1, 3]), (U, [2, 16, 2]), (U, [4, 32, 8])])
    _same_arrays(p._terms([]), [(U, []), (I, [0]), (U, []), (U, [])])
    c = PackedCubicSystem([5])
    (y,) = c.gens()
    q = c.mul_bit(y[0], y[1]) ^ y[2] ^ 1                                  # 1 + x2 + x0 x1
    t = c.mul_bit(c.mul_bit(y[0], y[1]), y[3])                             # (0 + x0 x1) x3 = 0 * x3 + x0 x1 x3
    _same_arrays(c._terms([0, 1, y[1:3], q, y[4:5].concat(t ^ q)]),
                 [(U, [0, 1, 4, 8, 9, 32, 9]), (I, [0, 0, 0, 0, 0, 1, 1, 3]), (U, [2, 0, 2]), (U, [4, 16, 4]),
                  (I, [0, 0, 0, 0, 0, 0, 0, 1]), (U, [2]), (U, [4]), (U, [16])])
    _same_arrays(c._terms([]), [(U, []), (I, [0]), (U, []), (U, []), (I, [0]), (U, []), (U, []), (U, [])])


def test_pickle_round_trip():
    p = PackedCubicSystem([5, 9])
    p2 = pickle.loads(pickle.dumps(p))
    assert p2._sizes == [5, 9] and p2._cols == p._cols == xl3_cols(14) and [len(g) for g in p2.gens()] == [5, 9]
    x, y = p.gens()
    v = (p.mul_bit(p.mul_bit(x[0], y[3]), y[4]) ^ p.mul_bit(x[1], x[2]) ^ y[1] ^ 1).concat(p.mul_bit(y[8], y[8]))
    v2 = pickle.loads(pickle.dumps(v))
    assert isinstance(v2, PackedCubicBitVec) and bits_of(v2) == bits_of(v) and v2._n == 14


def test_import_needs_no_numpy():
    code = ("import sys; sys.modules['numpy'] = None\n"
            "import gf2bv_amd\n"
            "assert 'gf2bv_amd.packed' not in sys.modules\n"
            "assert 'PackedCubicSystem' in gf2bv_amd.__all__ and 'PackedCubicBitVec' in gf2bv_amd.__all__\n"
            "try:\n    gf2bv_amd.PackedCubicSystem\nexcept ImportError:\n    print('lazy')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=hip._HERE + "/..")
    assert out.returncode == 0 and "lazy" in out.stdout, out.stderr


def test_random_terms_cover_the_cases():
    """the generator of the GPU tests gives what it promises: a linear-only row and rows beyond one LDS pass of either kind"""
    n = 64
    lin, off2, ta, tb, off3, ua, ub, uc = random_cubic_terms(random.Random(1), n, 6)
    t2, t3 = hip.cubic_chunks(n)
    c2, c3 = np.diff(off2), np.diff(off3)
    assert c2[0] == c3[0] == 0 and c2[1] > t2 and c3[2] > t3
    polys = row_polys(n, lin, off2, ta, tb, off3, ua, ub, uc)
    assert max(len(m) for m in polys[2]) == 3 and all(len(m) <= 1 for m in polys[0])


@pytest.mark.parametrize("outputs, rank", [(298, 298), (248, 248)])
def test_register_known_answers(outputs, rank):
    """n = 12, taps 0xE08, z = s1 ^ s3 s5 ^ s7 s9 s11: plain linearisation over the 298 cubic columns reaches the rank of the table;
    at full rank the one solution is the secret's point, and the equations written with mul_bit are the oracle's"""
    n, secret = 12, 0xB5D
    eqs = register_eqs(secret, count=outputs, **REGISTER_12)
    cols = xl3_cols(n)
    assert cols == 298
    p = PackedCubicSystem([n])
    zeros = register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], outputs)
    vec = zeros[0]
    for z in zeros[1:]:
        vec = vec.concat(z)
    assert bits_of(vec) == eqs
    padded = eqs + [0] * max(0, cols - len(eqs))
    res = O.solve_words(O.eqs_to_aug(padded, cols), len(padded), cols, 1)
    assert res["status"] == 0 and res["rank"] == rank
    space = O.m4ri_solve(padded, cols, 1)
    assert space.dimension == cols - rank
    if rank == cols:
        assert list(space) == [p._raw_point(secret)] and p.convert_sol(space.origin) == (secret,)
    else:
        assert space.dimension == 50 > 16              # what makes solve_all raise DimensionTooLargeError on the device
        assert issubclass(DimensionTooLargeError, Exception)
