"""The packed quadratic front-end without a GPU: PackedQuadBitVec / PackedQuadraticSystem keep the factored form of exactly the
expressions QuadraticSystem writes out (expanded here, in the test, with QuadraticSystem._mul_bit on ints), refuse what they do not
support, pickle, and the C entries behind them check their arguments before they look for a device."""
import ctypes
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

from gf2bv_amd import BitVec, PackedQuadBitVec, PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd._internal import m4ri_solve_quad_packed
from tests.quad_terms import Twin, bits_of, expand_ints, random_terms

SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 100)


@pytest.mark.parametrize("n", SIZES)
def test_algebra_matches_int_front_end(n):
    rng = random.Random(1000 + n)
    tw = Twin([n])
    for constant in (False, True):
        pairs = [tw.bit(rng, k % 5, constant) for k in range(10)]          # 0 .. 4 products per bit
        for a, b in pairs:
            assert bits_of(b) == bits_of(a)
        qa, pa = pairs[0]
        for a, b in pairs[1:]:                                             # concat: one vector of 10 bits
            qa, pa = qa.concat(a), pa.concat(b)
        assert isinstance(pa, PackedQuadBitVec) or n == 1
        assert len(pa) == len(qa) == 10 and bits_of(pa) == bits_of(qa)
        for key in (slice(2, 7), slice(None, None, 3), slice(8, 2, -2), slice(4, 4), 0, 9, -1):
            assert bits_of(pa[key]) == bits_of(qa[key]), key
        with pytest.raises(IndexError):
            pa[10]
        lin_q, lin_p = tw.qx[:1].dup(10), tw.px[:1].dup(10)               # xor with a linear vector (both sides), ints, itself
        for i in range(1, 10):
            u = tw.linear(rng, constant)
            lin_q, lin_p = lin_q ^ (u[0].zeroext(9) << i), lin_p ^ (u[1].zeroext(9) << i)
        assert bits_of(pa ^ lin_p) == bits_of(lin_p ^ pa) == bits_of(qa ^ lin_q)
        assert bits_of(pa ^ 0x2A5) == bits_of(0x2A5 ^ pa) == bits_of(qa ^ 0x2A5)
        assert bits_of(pa ^ -3) == bits_of(qa ^ -3)
        rev_q, rev_p = qa[::-1], pa[::-1]
        assert bits_of(pa ^ rev_p) == bits_of(qa ^ rev_q)                  # (term lists concatenate; equal products cancel in the expansion)
        assert all(e == 0 for e in bits_of(pa ^ pa))
        # evaluate: at a consistent point, as BitVec.evaluate of the expanded bits
        x = rng.getrandbits(n)
        raw = x
        for i in range(1, n):
            for j in range(i):
                if (x >> i) & (x >> j) & 1:
                    raw |= 1 << (n + i * (i - 1) // 2 + j)
        assert pa.evaluate(raw) == qa.evaluate(raw)
        assert tw.p.evaluate(pa, (x,)) == tw.q.evaluate(qa, (x,))


@pytest.mark.parametrize("n", SIZES)
def test_bit_assert_rows(n):
    rng = random.Random(2000 + n)
    tw = Twin([n])
    cases = [(tw.qx[n // 2], tw.px[n // 2])]                               # a single unknown: the x == a skip
    s = tw.linear(rng, False)
    cases.append((s[0] ^ tw.qx[0] ^ tw.qx[n - 1] ^ tw.qx[n // 3], s[1] ^ tw.px[0] ^ tw.px[n - 1] ^ tw.px[n // 3]))
    for a, b in cases:
        if a._bits[0] in (0, 1):
            continue                                                       # (the sum cancelled: the reference asserts)
        for v in (0, 1):
            want = tw.q.bit_assert(a, v)
            got = tw.p.bit_assert(b, v)
            flat = [e for z in got for e in bits_of(z)]
            assert flat == want, (n, v)
    assert len(tw.p.bit_assert(tw.px[0], 1)[1]) == n - 1


def test_several_generators_and_terms_layout():
    tw = Twin([5, 7])
    assert [len(g) for g in tw.p.gens()] == [5, 7] and tw.p._cols == tw.q._cols == 12 + 66
    x, y = tw.p.gens()
    qx, qy = tw.q.gens()
    zeros_p = [tw.p.mul_bit(x[1], y[6]) ^ x[0] ^ 1, y ^ 0x55, 0, 1, tw.p.mul_bit(x[2], x[2]).concat(x[:2])]
    zeros_q = [tw.q.mul_bit(qx[1], qy[6]) ^ qx[0] ^ 1, qy ^ 0x55, 0, 1, tw.q.mul_bit(qx[2], qx[2]).concat(qx[:2])]
    lin, off, ta, tb = tw.p._terms(zeros_p)
    assert lin.shape == (1 + 7 + 1 + 1 + 3, 1) and list(off) == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    want = [e for z in zeros_q for e in (z._bits if isinstance(z, BitVec) else (z,))]
    assert expand_ints(tw.q, lin, off, ta, tb) == want                     # (nothing dropped: zero rows and "1 = 0" go to the solver)
    for raw in (0b1 | (1 << 5) | (1 << 22), 0b1 | (1 << 5), 1 << 12, 0):        # x0 x5 = pair (5, 0), column 12 + 10
        assert tw.p.convert_sol(raw) == tw.q.convert_sol(raw)
    assert tw.p.convert_sol(0b1 | (1 << 5) | (1 << 22)) == (1, 1)


def test_refusals():
    p = PackedQuadraticSystem([8])
    (x,) = p.gens()
    q = p.mul_bit(x[0], x[1]) ^ x[2]
    v = q.concat(x[:3])
    for name, call in (("__and__", lambda: v & 3), ("__rand__", lambda: 3 & v), ("__or__", lambda: v | 1), ("__lshift__", lambda: v << 1),
                       ("__rshift__", lambda: v >> 1), ("__mod__", lambda: v % 2), ("rotl", lambda: v.rotl(1)), ("rotr", lambda: v.rotr(1)),
                       ("sum", lambda: v.sum()), ("zeroext", lambda: v.zeroext(2)), ("signext", lambda: v.signext(2)),
                       ("broadcast", lambda: v.broadcast(0, 4)), ("dup", lambda: v.dup(2)), ("lshift_ext", lambda: v.lshift_ext(1))):
        with pytest.raises(TypeError, match=name):
            call()
    with pytest.raises(ValueError, match="different lengths"):
        v ^ q
    with pytest.raises(ValueError, match="different lengths"):
        v ^ x
    with pytest.raises(ValueError, match="different lengths"):
        x ^ v
    with pytest.raises(ValueError, match="single bits"):
        p.mul_bit(x, x[0])
    with pytest.raises(ValueError, match="single bit"):
        p.bit_assert(x[:2], 0)
    with pytest.raises(TypeError, match="degree"):
        p.mul_bit(q, x[0])
    with pytest.raises(TypeError, match="needs PackedBitVecs"):
        p.mul_bit(QuadraticSystem([8]).gens()[0][0], x[0])
    with pytest.raises(TypeError, match="tuple-of-int"):
        q ^ QuadraticSystem([8]).gens()[0][:1]
    with pytest.raises(TypeError, match="tuple-of-int"):
        p._terms([QuadraticSystem([8]).gens()[0]])
    with pytest.raises(TypeError, match="0 or 1"):
        p._terms([q, 6])
    with pytest.raises(ValueError, match="different numbers of unknowns"):
        p._terms([PackedQuadraticSystem([100]).gens()[0]])
    with pytest.raises(TypeError, match="no rows on the host"):
        p.get_rows([q])
    with pytest.raises(TypeError, match="AND of two symbolic"):
        x & x


def test_entries_check_arguments_before_device_use():
    """every GF2BV_ERR_ARG case of the three entries returns 1 with its message on a machine without a GPU too"""
    L = hip.lib()
    n, rows = 12, 80                                   # 78 columns
    lin, off, ta, tb = random_terms(random.Random(3), n, 70)
    aug = np.zeros((rows + 1, 2), dtype=np.uint64)
    Lp, Op, Ap, Bp, A = lin.ctypes.data, off.ctypes.data, ta.ctypes.data, tb.ctypes.data, aug.ctypes.data
    A += -A % 16
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    bad0, dec = off.copy(), off.copy()
    bad0[0] = 1
    dec[40] = dec[39] - 1
    for name, tail in (("words", lambda r=rows, s=2, o=A: (o, s, 0)), ("solve", lambda r=rows, m=0, o=H: (m, 0, o))):
        f = getattr(L, "gf2bv_quad_expand_words" if name == "words" else "gf2bv_solve_quad_terms")
        err(f(None, Op, Ap, Bp, 70, rows, n, *tail()), "null")
        err(f(Lp, None, Ap, Bp, 70, rows, n, *tail()), "null")
        err(f(Lp, Op, None, Bp, 70, rows, n, *tail()), "null")
        err(f(Lp, Op, Ap, None, 70, rows, n, *tail()), "null")
        err(f(Lp, Op, Ap, Bp, 70, rows, n, *tail(o=None)), "null")
        err(f(Lp, Op, Ap, Bp, 70, rows, 0, *tail()), "n_lin")
        err(f(Lp, Op, Ap, Bp, 70, rows, 70000, *tail()), "n_lin")
        err(f(Lp, Op, Ap, Bp, 81, rows, n, *tail()), "rows_live")
        err(f(Lp, Op, Ap, Bp, -1, rows, n, *tail()), "rows_live")
        err(f(Lp, bad0.ctypes.data, Ap, Bp, 70, rows, n, *tail()), "start at 0")
        err(f(Lp, dec.ctypes.data, Ap, Bp, 70, rows, n, *tail()), "must not decrease")
    err(L.gf2bv_quad_expand_words(Lp, Op, Ap, Bp, 70, rows, n, A, 1, 0), "stride")
    err(L.gf2bv_solve_quad_terms(Lp, Op, Ap, Bp, 70, 77, n, 0, 0, H), "greater than or equal")
    err(L.gf2bv_solve_quad_terms(Lp, Op, Ap, Bp, 70, rows, n, 3, 0, H), "Invalid mode")
    D = L.gf2bv_quad_expand_device
    err(D(None, Op, Ap, Bp, 70, rows, n, A, 2, 0, None), "null")
    err(D(Lp, None, Ap, Bp, 70, rows, n, A, 2, 0, None), "null")
    err(D(Lp, Op, None, Bp, 70, rows, n, A, 2, 0, None), "null")
    err(D(Lp, Op, Ap, None, 70, rows, n, A, 2, 0, None), "null")
    err(D(Lp, Op, Ap, Bp, 70, rows, n, None, 2, 0, None), "null")
    err(D(Lp, Op, Ap, Bp, 70, rows, 0, A, 2, 0, None), "n_lin")
    err(D(Lp, Op, Ap, Bp, 81, rows, n, A, 2, 0, None), "rows_live")
    err(D(Lp, Op, Ap, Bp, 70, rows, n, A, 3, 0, None), "stride")
    err(D(Lp, Op, Ap, Bp, 70, rows, n, A, 0, 0, None), "stride")
    err(D(Lp, Op, Ap, Bp, 70, rows, n, A + 8, 2, 0, None), "16-byte alignment")
    assert not h.value
    # the bindings: sizes checked against each other, library errors as ValueError
    with pytest.raises(ValueError, match="term_off"):
        hip.quad_expand_words(lin, off[:-1], ta, tb, n)
    with pytest.raises(ValueError, match="term_off"):
        hip.solve_quad_terms(lin, off, ta[:-1], tb[:-1], n)
    with pytest.raises(ValueError, match="greater than or equal"):
        hip.solve_quad_terms(lin, off, ta, tb, n, rows=77)
    with pytest.raises(ValueError, match="whole rows"):
        m4ri_solve_quad_packed(lin.tobytes()[:-8], off, ta, tb, 100, rows, 0)
    with pytest.raises(ValueError, match="one int64 per row"):
        m4ri_solve_quad_packed(lin, off[:-1].copy(), ta, tb, n, rows, 0)
    with pytest.raises(ValueError, match="same number"):
        m4ri_solve_quad_packed(lin, off, ta, tb[:-1].copy(), n, rows, 0)
    with pytest.raises(ValueError, match="end at the number"):
        m4ri_solve_quad_packed(lin, off, ta[:-1].copy(), tb[:-1].copy(), n, rows, 0)
    with pytest.raises(ValueError, match="term_off must start at 0"):         # (the extension's own check, not the library's)
        m4ri_solve_quad_packed(lin, bad0, ta, tb, n, rows, 0)
    with pytest.raises(ValueError, match="term_off must not decrease"):
        m4ri_solve_quad_packed(lin, dec, ta, tb, n, rows, 0)
    with pytest.raises(ValueError, match="at least the rows of lin"):
        m4ri_solve_quad_packed(lin, off, ta, tb, n, 69, 0)
    with pytest.raises(ValueError, match="n_lin"):
        m4ri_solve_quad_packed(lin, off, ta, tb, 0, rows, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        m4ri_solve_quad_packed(lin, off, ta, tb, n, rows, 5)
    with pytest.raises(ValueError, match="greater than or equal"):
        m4ri_solve_quad_packed(lin, off, ta, tb, n, 77, 1)
    with pytest.raises(TypeError):
        m4ri_solve_quad_packed(lin, off, ta, tb, n, rows)


def test_pickle_round_trip():
    p = PackedQuadraticSystem([5, 9])
    p2 = pickle.loads(pickle.dumps(p))
    assert p2._quad_sizes == [5, 9] and p2._cols == p._cols and [len(g) for g in p2.gens()] == [5, 9]
    x, y = p.gens()
    v = (p.mul_bit(x[0], y[3]) ^ y[1] ^ 1).concat(p.mul_bit(y[8], y[8]))
    v2 = pickle.loads(pickle.dumps(v))
    assert isinstance(v2, PackedQuadBitVec) and bits_of(v2) == bits_of(v) and v2._n == 14


def test_import_needs_no_numpy():
    code = ("import sys; sys.modules['numpy'] = None\n"
            "import gf2bv_amd\n"
            "assert 'gf2bv_amd.packed' not in sys.modules\n"
            "gf2bv_amd.QuadraticSystem([4])\n"
            "try:\n    gf2bv_amd.PackedQuadraticSystem\nexcept ImportError:\n    print('lazy')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=hip._HERE + "/..")
    assert out.returncode == 0 and "lazy" in out.stdout, out.stderr
