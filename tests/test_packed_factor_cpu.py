"""Kept factorizations, right-hand sides and batches of the packed front-ends, the host side: the right-hand-side words of the packed
factored objects equal FactoredSystem's on the same expressions built on the int front-end (no factorization is made: handles are
created on first solve), value lists are checked alike, and every new C entry and binding function refuses bad arguments before it
looks for a device, so all of it holds on a machine without a GPU.  (What needs a handle -- an n_lin that does not match it -- is
in tests/test_gpu_packed_factor.py.)"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, PackedLinearSystem, PackedQuadraticSystem, QuadraticSystem, _internal, hip
from gf2bv_amd.factored import FactoredSystem, PackedFactoredSystem, PackedQuadFactoredSystem
from tests.quad_terms import Twin, random_terms

NEW_SYMBOLS = ["gf2bv_factor_quad_terms", "gf2bv_factor_append_quad_terms", "gf2bv_solve_rhs_quad_terms", "gf2bv_solve_batch_quad_terms",
               "gf2bv_quad_expand_batch_words"]
NEW_BINDINGS = ["m4ri_factor_packed", "m4ri_factor_quad_packed", "m4ri_solve_rhs_packed", "m4ri_solve_rhs_quad_packed",
                "m4ri_solve_many_quad_packed"]


def test_new_names_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gf2bv_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gf2bv_[a-z_0-9]+)", dyn))
    L = hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in exported and name in hip.EXPORTS and hasattr(L, name), name
    for name in NEW_BINDINGS:
        assert hasattr(_internal, name), name
    for name in ("factor_quad_terms", "solve_rhs_quad_terms", "solve_batch_quad_terms", "quad_expand_batch_words"):
        assert callable(getattr(hip, name)), name
    assert callable(hip.Factor.append_quad_terms)
    for cls in (PackedLinearSystem, PackedQuadraticSystem):
        for name in ("factor", "solve_raw_one_rhs", "solve_raw_space_rhs", "solve_one_rhs"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("solve_raw_one_many", "solve_raw_space_many", "solve_one_many"):
        assert callable(getattr(PackedQuadraticSystem, name)), name
    for name in ("add", "copy", "close", "__enter__", "__exit__", "rhs_words", "solve_raw_one_rhs", "solve_raw_space_rhs", "solve_one_rhs",
                 "solve_one", "solve_all", "search_one_rhs", "search_one", "search_all"):
        assert callable(getattr(PackedQuadFactoredSystem, name)) and callable(getattr(PackedFactoredSystem, name)), name


# -- rhs_words parity --------------------------------------------------------------------------------------------------------------
def _values(rng, widths, n, negative, wide):
    """n value lists for expressions of these widths (0: an equation int, value 0 / 1)"""
    out = []
    for _ in range(n):
        vals = []
        for w in widths:
            if w == 0:
                vals.append(rng.getrandbits(1))
            else:
                v = rng.getrandbits(w + (70 if wide else 0))
                vals.append(-v if negative and rng.random() < 0.5 else v)
        out.append(vals)
    return out


def _quad_exprs(rng, tw: Twin, count: int):
    """`count` random expressions on both front-ends in step: vectors of several bits with and without products (operands with
    constants among them), plain linear vectors, and the literals 0 / 1.  Returns (int exprs, packed exprs, widths, seen)."""
    qe, pe, widths = [], [], []
    seen = {"products": 0, "constant_operands": 0, "linear": 0, "literal": 0, "wide": 0}
    for _ in range(count):
        kind = rng.random()
        if kind < 0.15:
            v = rng.getrandbits(1)
            qe.append(v)
            pe.append(v)
            widths.append(0)
            seen["literal"] += 1
            continue
        nbits = rng.choice((1, 2, 7, 65, 70))
        seen["wide"] += nbits > 64
        if kind < 0.4:
            a, b = tw.linear(rng, True)
            for _ in range(nbits - 1):
                u = tw.linear(rng, True)
                a, b = a.concat(u[0]), b.concat(u[1])
            seen["linear"] += 1
        else:
            constant = rng.random() < 0.6
            a, b = tw.bit(rng, rng.randint(1, 3), constant)
            for _ in range(nbits - 1):
                u = tw.bit(rng, rng.randint(0, 3), constant)
                a, b = a.concat(u[0]), b.concat(u[1])
            seen["products"] += 1
            seen["constant_operands"] += constant
        qe.append(a)
        pe.append(b)
        widths.append(nbits)
    return qe, pe, widths, seen


@pytest.mark.parametrize("n", [3, 20, 64, 70])
def test_rhs_words_equal_int_front_end_quadratic(n):
    rng = random.Random(5100 + n)
    tw = Twin([n] if n < 20 else [n - 7, 7])
    total = {}
    qe, pe, widths, seen = _quad_exprs(rng, tw, 12)
    fq, fp = FactoredSystem(tw.q, qe), tw.p.factor(pe)
    assert isinstance(fp, PackedQuadFactoredSystem) and fp._quadratic and fq._quadratic
    for round_ in range(3):
        assert fp.rows == fq.rows and fp._nspans == fq._nspans
        for negative, wide in ((False, False), (True, False), (False, True), (True, True)):
            vals = _values(rng, widths, 5, negative, wide)
            got, want = fp.rhs_words(vals), fq.rhs_words(vals)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (n, round_, negative, wide)
        assert fp.rhs_words([]).shape == fq.rhs_words([]).shape
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        qa, pa, wa, seen = _quad_exprs(rng, tw, 5)                          # add: the bookkeeping only (no handle exists yet)
        fq.add(qa)
        fp.add(pa)
        widths = widths + wa
    assert all(total[k] > 0 for k in ("products", "constant_operands", "linear", "literal", "wide")), total
    # fewer rows than columns: the zero rows of the padding sit where FactoredSystem puts them, in front of what is added later
    tw = Twin([9])
    pairs = [tw.bit(rng, 2, True), tw.bit(rng, 0, True), tw.bit(rng, 1, False)]
    qe, pe, widths = [a for a, _ in pairs], [b for _, b in pairs], [1, 1, 1]
    fq, fp = FactoredSystem(tw.q, qe), tw.p.factor(pe)
    assert fp.rows == fq.rows == tw.q._cols
    qa, pa, wa, _ = _quad_exprs(rng, tw, 3)
    fq.add(qa)
    fp.add(pa)
    vals = _values(rng, widths + wa, 4, True, True)
    assert np.array_equal(fp.rhs_words(vals), fq.rhs_words(vals)) and fp.rows == fq.rows > tw.q._cols


def test_bit_assert_rows_in_rhs_words():
    """the guess loop's rows: bit_assert(a, v) -> [a ^ v, the n - 1 products] as two expressions against the int front-end's flat list"""
    rng = random.Random(5200)
    tw = Twin([12])
    base_q, base_p, widths, _ = _quad_exprs(rng, tw, 6)
    fq, fp = FactoredSystem(tw.q, base_q), tw.p.factor(base_p)
    for v in (0, 1):
        a = tw.linear(rng, False)
        gq, gp = tw.q.bit_assert(a[0], v), tw.p.bit_assert(a[1], v)
        cq, cp = fq.copy(), fp.copy()
        cq.add(gq)                                                         # 12 equation ints: 12 values 0 / 1
        cp.add(gp)                                                         # one bit and one vector of 11 bits
        assert type(cp) is PackedQuadFactoredSystem and cp.rows == cq.rows == fq.rows + 12
        bits = [rng.getrandbits(1) for _ in gq]
        tail = sum(b << i for i, b in enumerate(bits[1:]))
        vals = _values(rng, widths, 1, False, False)[0]
        assert np.array_equal(cp.rhs_words([vals + [bits[0], tail]]), cq.rhs_words([vals + bits]))
        assert fp.rows == fq.rows                                          # the originals are as they were


@pytest.mark.parametrize("cols", [5, 64, 130])
def test_rhs_words_equal_int_front_end_linear(cols):
    rng = random.Random(5300 + cols)
    sizes = [cols - 3, 3]
    lin, plin = LinearSystem(sizes), PackedLinearSystem(sizes)
    seen_int = seen_wide = 0

    def exprs(count):
        nonlocal seen_int, seen_wide
        qe, pe, widths = [], [], []
        for _ in range(count):
            if rng.random() < 0.3:
                e = rng.getrandbits(cols + 1)
                qe.append(e)
                pe.append(e)
                widths.append(0)
                seen_int += 1
                continue
            (x, y), (px, py) = lin.gens(), plin.gens()
            k, r = rng.getrandbits(cols - 3), rng.randrange(cols - 3)
            a, b = (x ^ k) ^ x.rotl(r), (px ^ k) ^ px.rotl(r)
            if rng.random() < 0.5:
                a, b = a.concat(y), b.concat(py)
            assert b._bits == a._bits
            qe.append(a)
            pe.append(b)
            widths.append(len(a))
            seen_wide += len(a) > 64
        return qe, pe, widths

    qe, pe, widths = exprs(8)
    fq, fp = lin.factor(qe), plin.factor(pe)
    assert type(fp) is PackedFactoredSystem and not fp._quadratic
    for round_ in range(3):
        assert fp.rows == fq.rows
        for negative, wide in ((False, False), (True, False), (False, True), (True, True)):
            vals = _values(rng, widths, 4, negative, wide)
            assert np.array_equal(fp.rhs_words(vals), fq.rhs_words(vals)), (cols, round_, negative, wide)
        qa, pa, wa = exprs(3)
        fq.add(qa)
        fp.add(pa)
        widths = widths + wa
    assert seen_int and (seen_wide or cols < 70), (seen_int, seen_wide)


# -- value-list errors ---------------------------------------------------------------------------------------------------------------
def test_value_list_errors():
    tw = Twin([6])
    x, px = tw.qx, tw.px
    for fs in (tw.p.factor([px, 1, tw.p.mul_bit(px[0], px[1])]), PackedLinearSystem([6]).factor([PackedLinearSystem([6]).gens()[0], 5, 9])):
        with pytest.raises(ValueError, match="values for 3 expressions"):
            fs.rhs_words([[1, 0]])
        with pytest.raises(ValueError, match="values for 3 expressions"):
            fs.rhs_words([[1, 0, 1], [1, 0, 1, 1]])
        with pytest.raises(ValueError, match="must be 0 or 1"):
            fs.rhs_words([[3, 2, 0]])
        with pytest.raises(ValueError, match="must be 0 or 1"):
            fs.rhs_words([[-3, 1, 0], [1 << 80, -1, 1]])                  # (the chunk-by-chunk path)
        assert fs.rhs_words([[63, 1, 1]]).shape == (1, fs._rw)
    # the one-shot forms build the same right-hand sides: the same errors, before any device is touched
    p, (g,) = PackedLinearSystem([6]), PackedLinearSystem([6]).gens()
    for call in (p.solve_raw_one_rhs, p.solve_raw_space_rhs, p.solve_one_rhs):
        with pytest.raises(ValueError, match="values for 2 expressions"):
            call([g, 5], [[1]])
        with pytest.raises(ValueError, match="must be 0 or 1"):
            call([g, 5], [[1, 2]])
        assert call([g, 5], []) == []
    for call in (tw.p.solve_raw_one_rhs, tw.p.solve_raw_space_rhs, tw.p.solve_one_rhs):
        with pytest.raises(ValueError, match="values for 2 expressions"):
            call([px, 0], [[1, 0, 0]])
        assert call([px, 0], []) == []
    assert tw.p.solve_raw_one_many([]) == [] and tw.p.solve_one_many([]) == []
    with pytest.raises(TypeError):
        tw.p.factor([x])                                                   # a tuple-of-int BitVec
    with pytest.raises(TypeError):
        tw.p.factor([5])                                                   # a bare equation int other than 0 / 1
    with pytest.raises(TypeError):
        PackedLinearSystem([6]).factor([tw.p.mul_bit(px[0], px[1])])
    closed = tw.p.factor([px])
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        closed.solve_one([0])
    with pytest.raises(ValueError, match="closed"):
        closed.add([px])


# -- argument checks of the C entries --------------------------------------------------------------------------------------------------
def test_c_entries_check_arguments_before_device_use():
    """GF2BV_ERR_ARG (1) with a specific message, on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2)"""
    L = hip.lib()
    n = 5
    cols = hip.quad_cols(n)                                                # 15
    rows = cols + 2
    lin, off, ta, tb = random_terms(random.Random(1), n, rows, 2)
    A = [a.ctypes.data for a in (lin, off, ta, tb)]
    rw = (rows + 63) // 64
    rhs = np.zeros((3, rw), dtype=np.uint64)
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)
    out = (ctypes.c_void_p * 4)()
    bad0 = off.copy()
    bad0[0] = 1
    dec = off.copy()
    dec[3] = dec[4] + 1

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    def with_(k, v):
        a = list(A)
        a[k] = v
        return a

    # factor
    err(L.gf2bv_factor_quad_terms(*A, rows, rows, n, 0, 0, None), "null")
    err(L.gf2bv_factor_quad_terms(*with_(0, None), rows, rows, n, 0, 0, H), "null")
    err(L.gf2bv_factor_quad_terms(*with_(1, None), rows, rows, n, 0, 0, H), "null")
    err(L.gf2bv_factor_quad_terms(*with_(2, None), rows, rows, n, 0, 0, H), "null")
    err(L.gf2bv_factor_quad_terms(*with_(1, bad0.ctypes.data), rows, rows, n, 0, 0, H), "start at 0")
    err(L.gf2bv_factor_quad_terms(*with_(1, dec.ctypes.data), rows, rows, n, 0, 0, H), "must not decrease")
    err(L.gf2bv_factor_quad_terms(*A, cols - 1, cols - 1, n, 0, 0, H), "greater than or equal")
    err(L.gf2bv_factor_quad_terms(*A, rows, rows - 1, n, 0, 0, H), "rows_live")
    err(L.gf2bv_factor_quad_terms(*A, rows, rows, 0, 0, 0, H), "n_lin")
    err(L.gf2bv_factor_quad_terms(*A, rows, rows, n, 5, 0, H), "Invalid mode")
    assert not h.value
    # append: a null handle (what needs a handle runs on the GPU)
    err(L.gf2bv_factor_append_quad_terms(None, *A, rows, n), "null")
    # many right-hand sides
    R = rhs.ctypes.data
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows, n, R, 3, rw, 0, 0, None), "null")
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows, n, None, 3, rw, 0, 0, out), "null")
    err(L.gf2bv_solve_rhs_quad_terms(*with_(0, None), rows, rows, n, R, 3, rw, 0, 0, out), "null")
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows, n, R, 0, rw, 0, 0, out), "nrhs")
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows, n, R, 3, 0, 0, 0, out), "rhs_words")
    err(L.gf2bv_solve_rhs_quad_terms(*A, cols - 1, cols - 1, n, R, 3, rw, 0, 0, out), "greater than or equal")
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows - 1, n, R, 3, rw, 0, 0, out), "rows_live")
    err(L.gf2bv_solve_rhs_quad_terms(*with_(1, bad0.ctypes.data), rows, rows, n, R, 3, rw, 0, 0, out), "start at 0")
    err(L.gf2bv_solve_rhs_quad_terms(*with_(1, dec.ctypes.data), rows, rows, n, R, 3, rw, 0, 0, out), "must not decrease")
    err(L.gf2bv_solve_rhs_quad_terms(*A, rows, rows, n, R, 3, rw, 2, 0, out), "Invalid mode")
    # batches: three systems of 5, 0 and 12 of the 17 rows
    sys_off = np.array([0, 5, 5, 17], dtype=np.int64)
    S = sys_off.ctypes.data
    for k in range(4):
        out[k] = 0x1000 + k
    err(L.gf2bv_solve_batch_quad_terms(*A, S, 3, cols, n, 0, 0, None), "null")
    err(L.gf2bv_solve_batch_quad_terms(*A, None, 3, cols, n, 0, 0, out), "null")
    assert not any(out[k] for k in range(3)) and out[3] == 0x1003          # cleared before anything can fail
    err(L.gf2bv_solve_batch_quad_terms(*with_(0, None), S, 3, cols, n, 0, 0, out), "null")
    err(L.gf2bv_solve_batch_quad_terms(*A, S, 3, cols - 1, n, 0, 0, out), "greater than or equal")
    err(L.gf2bv_solve_batch_quad_terms(*A, S, 3, cols, n, 3, 0, out), "Invalid mode")
    for bad, what in (([1, 5, 5, 17], "start at 0"), ([0, 6, 5, 17], "must not decrease"), ([0, 0, 0, 17], "live rows")):
        b = np.array(bad, dtype=np.int64)
        err(L.gf2bv_solve_batch_quad_terms(*A, b.ctypes.data, 3, cols, n, 0, 0, out), what)
    err(L.gf2bv_solve_batch_quad_terms(*with_(1, bad0.ctypes.data), S, 3, cols, n, 0, 0, out), "start at 0")
    err(L.gf2bv_solve_batch_quad_terms(*with_(1, dec.ctypes.data), S, 3, cols, n, 0, 0, out), "must not decrease")
    aug = np.zeros((3, cols, 2), dtype=np.uint64)
    err(L.gf2bv_quad_expand_batch_words(*A, None, 3, cols, n, aug.ctypes.data, 2, 0), "null")
    err(L.gf2bv_quad_expand_batch_words(*A, S, 3, cols, n, None, 2, 0), "null")
    err(L.gf2bv_quad_expand_batch_words(*A, S, 3, cols, n, aug.ctypes.data, 0, 0), "stride")
    err(L.gf2bv_quad_expand_batch_words(*A, S, 3, 11, n, aug.ctypes.data, 2, 0), "live rows")
    # and through hip: ValueError
    with pytest.raises(ValueError):
        hip.factor_quad_terms(lin, off, ta, tb, n, rows=cols - 1)
    with pytest.raises(ValueError):
        hip.solve_rhs_quad_terms(lin, off, ta, tb, n, np.zeros((2, 0), dtype=np.uint64))
    with pytest.raises(ValueError):
        hip.solve_batch_quad_terms(lin, off, ta, tb, [0, 5, 5, 16], n)
    with pytest.raises(ValueError):
        hip.solve_batch_quad_terms(lin, off, ta, tb, [0, 17], n, rows=16)
    if hip.device_count() == 0:
        with pytest.raises(hip.HipError, match="no HIP device"):
            hip.factor_quad_terms(lin, off, ta, tb, n)
        with pytest.raises(hip.HipError, match="no HIP device"):
            hip.solve_batch_quad_terms(lin, off, ta, tb, sys_off, n)


# -- argument checks of the binding functions --------------------------------------------------------------------------------------------
def test_binding_functions_check_arguments_before_the_library_is_called():
    n = 5
    cols = hip.quad_cols(n)
    rows = cols + 2
    lin, off, ta, tb = random_terms(random.Random(2), n, rows, 2)
    bad0 = off.copy()
    bad0[0] = 1
    dec = off.copy()
    dec[3] = dec[4] + 1
    rhs = np.zeros((2, 1), dtype=np.uint64)
    sys_off = np.array([0, 5, 17], dtype=np.int64)
    quad = {
        "m4ri_factor_quad_packed": lambda a, n_=n, r=rows, m=0: _internal.m4ri_factor_quad_packed(*a, n_, r, m),
        "m4ri_solve_rhs_quad_packed": lambda a, n_=n, r=rows, m=0: _internal.m4ri_solve_rhs_quad_packed(*a, n_, r, m, rhs),
        "m4ri_solve_many_quad_packed": lambda a, n_=n, r=rows, m=0: _internal.m4ri_solve_many_quad_packed(*a, sys_off, n_, r, m),
    }
    good = (lin, off, ta, tb)
    for name, call in quad.items():
        with pytest.raises(TypeError):
            call((lin, off, ta, None))                                     # not a buffer
        with pytest.raises((ValueError, BufferError)):
            call((lin[::2], off, ta, tb))                                  # not contiguous
        with pytest.raises(ValueError, match="whole rows"):
            call((lin.ravel()[:-1].view(np.uint8)[:-3], off, ta, tb))
        with pytest.raises(ValueError, match="one int64 per row"):
            call((lin, off[:-1], ta, tb))
        with pytest.raises(ValueError, match="same number"):
            call((lin, off, ta, tb[:-1]))
        with pytest.raises(ValueError, match="start at 0"):
            call((lin, bad0, ta, tb))
        with pytest.raises(ValueError, match="must not decrease"):
            call((lin, dec, ta, tb))
        with pytest.raises(ValueError, match="end at the number of operands"):
            call((lin, off, ta[:-1], tb[:-1]))
        with pytest.raises(ValueError, match="n_lin"):
            call(good, n_=0)
        with pytest.raises(ValueError, match="greater than or equal"):
            call((lin[:10], off[:11], ta[:off[10]], tb[:off[10]]), r=cols - 1)
        with pytest.raises(ValueError, match="Invalid mode"):
            call(good, m=2)
        with pytest.raises(TypeError):
            call(good[:3])
    with pytest.raises(ValueError, match="at least the rows of lin"):
        _internal.m4ri_factor_quad_packed(np.concatenate([lin, lin]), np.concatenate([off, off[1:] + off[-1]]), np.concatenate([ta, ta]),
                                          np.concatenate([tb, tb]), n, rows, 0)
    for bad, what in (([1, 5, 17], "start at 0"), ([0, 6, 5, 17], "must not decrease"), ([0, 5, 16], "end at the rows"),
                      ([0, 0, 17], "rows of every system")):
        with pytest.raises(ValueError, match=what):
            _internal.m4ri_solve_many_quad_packed(lin, off, ta, tb, np.array(bad, dtype=np.int64), n, cols, 0)
    with pytest.raises(TypeError):
        _internal.m4ri_solve_many_quad_packed(lin, off, ta, tb, None, n, cols, 0)
    assert _internal.m4ri_solve_many_quad_packed(lin[:0], off[:1], ta[:0], tb[:0], np.zeros(1, dtype=np.int64), n, cols, 0) == []
    # right-hand sides: a list of ints or a 2-D uint64 array of enough words
    for r, exc in ((np.zeros(3, dtype=np.uint64), TypeError), (np.zeros((2, 1), dtype=np.uint32), TypeError), (3, TypeError),
                   ([1, "x"], TypeError), ([-1], ValueError), (np.zeros((2, 0), dtype=np.uint64), ValueError)):
        with pytest.raises(exc):
            _internal.m4ri_solve_rhs_quad_packed(lin, off, ta, tb, n, rows, 0, r)
    assert _internal.m4ri_solve_rhs_quad_packed(lin, off, ta, tb, n, rows, 0, []) == []
    # the packed linear twins: m4ri_solve_packed's checks
    words = 2
    buf = np.zeros((70, words), dtype=np.uint64)
    for call in (lambda b, r, w, c, m: _internal.m4ri_factor_packed(b, r, w, c, m),
                 lambda b, r, w, c, m: _internal.m4ri_solve_rhs_packed(b, r, w, c, m, np.zeros((1, 2), dtype=np.uint64))):
        with pytest.raises(ValueError, match="greater than or equal"):
            call(buf, 70, words, 71, 0)
        with pytest.raises(ValueError, match="columns must be positive"):
            call(buf, 70, words, 0, 0)
        with pytest.raises(ValueError, match="Invalid mode"):
            call(buf, 70, words, 65, 9)
        with pytest.raises(ValueError, match="rows x words"):
            call(buf, 69, words, 65, 0)
        with pytest.raises(ValueError, match="rows x words"):
            call(buf[:, :1].copy(), 70, 1, 65, 0)                          # one word does not cover 66 bits
        with pytest.raises(TypeError):
            call(None, 70, words, 65, 0)
    with pytest.raises(ValueError, match="ceil"):
        _internal.m4ri_solve_rhs_packed(buf, 70, words, 65, 0, np.zeros((1, 1), dtype=np.uint64))
    with pytest.raises(TypeError):
        _internal.m4ri_factor_packed(buf, 70, words)
    if hip.device_count() == 0:                                            # well-formed calls reach the library, which has no CPU fallback
        with pytest.raises(RuntimeError, match="no HIP device"):
            _internal.m4ri_factor_quad_packed(lin, off, ta, tb, n, rows, 0)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _internal.m4ri_factor_packed(buf, 70, words, 65, 0)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _internal.m4ri_solve_many_quad_packed(lin, off, ta, tb, sys_off, n, cols, 0)
