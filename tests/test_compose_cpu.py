"""Composition without a GPU: the host twin against Python-int arithmetic and against xoshiro256's published jump polynomials, the
refusals of gf2bv_amd.compose (raised before any library call), the exponent's word encoding, the exported names, and the argument
errors of the C entries, which return before a device is looked for."""
import ctypes
import random

import numpy as np
import pytest

import gf2bv_amd
from gf2bv_amd import BitVec, LinearSystem, PackedLinearSystem, PackedQuadraticSystem, compose, hip
from tests import compose_terms as T
from tests.harness_models import Xoshiro256starstar

# xoshiro256starstar.c (Blackman & Vigna, public domain): jump() is 2^128 steps, long_jump() 2^192
JUMP = (0x180ec6d33cfd0aba, 0xd5a61266f0c9392c, 0xa9582618e03fc9aa, 0x39abdc4529b1661c)
LONG_JUMP = (0x76e15d3efefdcbbf, 0xc5004e441c522fb3, 0x77710069854ee241, 0x39109bb02acbe635)


def reference_jump(state, poly) -> list:
    """the reference code's jump loop on a concrete state"""
    gen = Xoshiro256starstar(state)
    acc = [0, 0, 0, 0]
    for word in poly:
        for b in range(64):
            if (word >> b) & 1:
                acc = [x ^ y for x, y in zip(acc, gen.s)]
            gen.step()
    return acc


def xoshiro_step_map():
    """(system, images): one symbolic state transition of xoshiro256 over its 256 state bits"""
    lin = PackedLinearSystem([64] * 4)
    sym = Xoshiro256starstar(lin.gens())
    sym.step()
    return lin, tuple(sym.s)


def _rows(images) -> np.ndarray:
    return np.concatenate([v._rows for v in images])


def _state_int(words) -> int:
    return sum(w << (64 * i) for i, w in enumerate(words))


# -- the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nb, ra", [(1, 1, 3), (3, 5, 4), (7, 2, 9), (63, 64, 5), (64, 63, 5), (70, 130, 6)])
def test_twin_against_python_ints(n, nb, ra):
    rng = random.Random(n * 1000 + nb)
    a = [rng.getrandbits(n + 1) for _ in range(ra)]
    b = [rng.getrandbits(nb + 1) for _ in range(n)]
    got = T.substitute(T.rows_of_ints(a, T.form_words(n)), n, T.rows_of_ints(b, T.form_words(nb)), nb)
    assert T.int_rows(got) == T.substitute_ints(a, n, b)


def test_twin_ignores_bits_above_the_unknowns():
    rng = random.Random(5)
    n, nb = 5, 9
    a = [rng.getrandbits(n + 1) for _ in range(4)]
    b = [rng.getrandbits(nb + 1) for _ in range(n)]
    clean = T.substitute(T.rows_of_ints(a, 1), n, T.rows_of_ints(b, 1), nb)
    dirty = T.substitute(T.rows_of_ints([v | rng.getrandbits(50) << (n + 1) for v in a], 1), n,
                         T.rows_of_ints([v | rng.getrandbits(50) << (nb + 1) for v in b], 1), nb)
    assert np.array_equal(clean, dirty)


def test_twin_powers():
    rng = random.Random(6)
    n = 9
    b = T.rows_of_ints([rng.getrandbits(n + 1) for _ in range(n)], 1)
    assert np.array_equal(T.power(b, n, 0), T.identity(n))
    assert np.array_equal(T.power(b, n, 1), b)
    for k in (2, 3, 5, 12):
        assert np.array_equal(T.power(b, n, k), T.power_loop(b, n, k))
        x = rng.getrandbits(n)
        y = x
        for _ in range(k):
            y = T.evaluate(b, n, y)
        assert T.evaluate(T.power(b, n, k), n, x) == y


@pytest.mark.parametrize("k, poly", [(1 << 128, JUMP), (1 << 192, LONG_JUMP)], ids=["jump", "long_jump"])
def test_twin_power_is_the_published_jump(k, poly):
    _, images = xoshiro_step_map()
    jumped = T.power(_rows(images), 256, k)
    rng = random.Random(k.bit_length())
    for _ in range(3):
        state = [rng.getrandbits(64) for _ in range(4)]
        assert T.evaluate(jumped, 256, _state_int(state)) == _state_int(reference_jump(state, poly))


# -- gf2bv_amd.compose: refusals by name, before the library ----------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*args):
        raise AssertionError("the library was called")
    monkeypatch.setattr(compose, "m4ri_compose_packed", refuse)
    monkeypatch.setattr(compose, "m4ri_power_packed", refuse)


def test_refusals(no_library):
    lin = PackedLinearSystem([8, 8])
    x, y = lin.gens()
    tx, ty = LinearSystem([8, 8]).gens()
    assert isinstance(tx, BitVec)
    with pytest.raises(TypeError, match="tuple-of-int"):
        compose.substitute(tx, (x, y))
    with pytest.raises(TypeError, match="tuple-of-int"):
        compose.substitute(x, (tx, ty))
    with pytest.raises(TypeError, match="tuple-of-int"):
        compose.power((tx, ty), 2)
    quad = PackedQuadraticSystem([8, 8])
    qx, qy = quad.gens()
    prod = quad.mul_bit(qx[0], qy[0])
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.substitute(prod, (qx, qy))
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.substitute(qx, (qx[:7].concat(prod), qy))
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.power((qx[:7].concat(prod), qy), 3)
    wide = PackedLinearSystem([100]).gens()[0]                # two words; 16 unknowns are one
    with pytest.raises(ValueError, match="words wide"):
        compose.substitute(wide, (x, y))
    with pytest.raises(ValueError, match="square"):
        compose.power((wide[:16],), 2)                        # 16 image bits over forms of 100 unknowns
    with pytest.raises(ValueError, match="negative"):
        compose.power((x, y), -1)
    with pytest.raises(ValueError, match="different numbers of unknowns"):
        compose.substitute(x, (x, wide[:8]))


def test_calls_reach_the_library_with_the_stacked_rows(monkeypatch):
    seen = []

    def fake_compose(a, ra, n, b, nb):
        seen.append((a.copy(), ra, n, b.copy(), nb))
        return bytearray(ra * b.shape[1] * 8)

    monkeypatch.setattr(compose, "m4ri_compose_packed", fake_compose)
    lin = PackedLinearSystem([8, 8])
    x, y = lin.gens()
    one = compose.substitute(x ^ y, (y, x))
    assert isinstance(one, gf2bv_amd.PackedBitVec) and len(one) == 8
    two = compose.substitute([x, y[:3]], (y, x))
    assert isinstance(two, tuple) and [len(v) for v in two] == [8, 3]
    a, ra, n, b, nb = seen[1]
    assert (ra, n, nb) == (11, 16, 63) and np.array_equal(a, np.concatenate([x._rows, y._rows[:3]]))
    assert np.array_equal(b, np.concatenate([y._rows, x._rows]))


# -- the exponent ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5, (1 << 64) - 1, 1 << 64, (1 << 64) + 3, 1 << 128, (1 << 192) + (1 << 70) + 9])
def test_exponent_words(k):
    for words in (compose._exponent_words(k), hip.exponent_words(k)):
        assert words.dtype == np.uint64 and len(words) == max(1, (k.bit_length() + 63) // 64)
        assert sum(int(w) << (64 * i) for i, w in enumerate(words)) == k
        assert len(words) == 1 or words[-1] != 0


def test_exponent_refuses_negative():
    with pytest.raises(ValueError):
        hip.exponent_words(-1)


# -- names -------------------------------------------------------------------------------------------------------------------------
def test_exported_names():
    assert "substitute" in gf2bv_amd.__all__ and "power" in gf2bv_amd.__all__
    assert gf2bv_amd.substitute is compose.substitute and gf2bv_amd.power is compose.power
    for name in ("gf2bv_compose_words", "gf2bv_compose_device", "gf2bv_compose_power_words", "gf2bv_compose_power_device",
                 "gf2bv_compose_shape", "gf2bv_compose_last_times"):
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)


def test_compose_shape_is_pure():
    s = hip.compose_shape()
    assert s["slice_bits"] % 64 == 0 and s["slice_bits"] >= 64
    assert s["rows_per_workgroup"] % 64 == 0 and s["tile_words"] == 2
    assert s["lds_bytes"] <= 160 * 1024
    # the MT19937 twist map: at least one workgroup per compute unit of an MI355X
    tiles = -(-T.form_words(19968) // s["tile_words"])
    assert tiles * -(-19969 // s["rows_per_workgroup"]) >= 256


# -- argument errors of the C entries: GF2BV_ERR_ARG (1) with no device looked for ---------------------------------------------------
ARG = 1
BIG = (1 << 31) - 65            # n + 1 = 2^31 - 64


def _w(shape):
    return np.zeros(shape, dtype=np.uint64)


def _rc_words(a, ra, a_stride, n, b, b_stride, nb, out, out_stride):
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    return hip.lib().gf2bv_compose_words(p(a), ra, a_stride, n, p(b), b_stride, nb, p(out), out_stride, 0)


@pytest.mark.parametrize("case", [
    dict(a=None), dict(b=None), dict(out=None), dict(ra=-1), dict(n=0), dict(nb=0), dict(n=BIG), dict(nb=BIG),
    dict(a_stride=1), dict(b_stride=2), dict(out_stride=2),
])
def test_compose_words_argument_errors(case):
    # 70 unknowns in (two words), 130 out (three words)
    args = dict(a=_w((4, 2)), ra=4, a_stride=2, n=70, b=_w((70, 3)), b_stride=3, nb=130, out=_w((4, 3)), out_stride=3)
    args.update(case)
    assert _rc_words(**args) == ARG
    assert hip.lib().gf2bv_last_error()


DEV = 0x7f0000001000            # a 16-byte aligned address that is never read: every case fails its checks first


@pytest.mark.parametrize("case", [
    dict(d_a=0), dict(d_b=0), dict(d_out=0), dict(ra=-1), dict(n=0), dict(nb=0), dict(n=BIG), dict(nb=BIG),
    dict(a_stride=0), dict(b_stride=2), dict(out_stride=2), dict(a_stride=3), dict(b_stride=5), dict(out_stride=5),
    dict(d_a=DEV + 8), dict(d_b=DEV + 8), dict(d_out=DEV + 8),
])
def test_compose_device_argument_errors(case):
    args = dict(d_a=DEV, ra=4, a_stride=2, n=70, d_b=DEV, b_stride=4, nb=130, d_out=DEV, out_stride=4)
    args.update(case)
    rc = hip.lib().gf2bv_compose_device(args["d_a"] or None, args["ra"], args["a_stride"], args["n"], args["d_b"] or None, args["b_stride"],
                                        args["nb"], args["d_out"] or None, args["out_stride"], 0, None)
    assert rc == ARG


@pytest.mark.parametrize("case", [
    dict(b=None), dict(k=None), dict(out=None), dict(n=0), dict(n=BIG), dict(b_stride=1), dict(out_stride=1), dict(knw=0), dict(knw=-1),
])
def test_compose_power_words_argument_errors(case):
    args = dict(b=_w((70, 2)), b_stride=2, n=70, k=np.array([3], dtype=np.uint64), knw=1, out=_w((70, 2)), out_stride=2)
    args.update(case)
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    rc = hip.lib().gf2bv_compose_power_words(p(args["b"]), args["b_stride"], args["n"], p(args["k"]), args["knw"], p(args["out"]),
                                             args["out_stride"], 0)
    assert rc == ARG


@pytest.mark.parametrize("case", [
    dict(d_b=0), dict(k=None), dict(d_out=0), dict(n=0), dict(n=BIG), dict(b_stride=0), dict(b_stride=3), dict(out_stride=3),
    dict(d_b=DEV + 8), dict(d_out=DEV + 8), dict(knw=0),
])
def test_compose_power_device_argument_errors(case):
    args = dict(d_b=DEV, b_stride=2, n=70, k=np.array([3], dtype=np.uint64), knw=1, d_out=DEV, out_stride=2)
    args.update(case)
    k = None if args["k"] is None else args["k"].ctypes.data
    rc = hip.lib().gf2bv_compose_power_device(args["d_b"] or None, args["b_stride"], args["n"], k, args["knw"], args["d_out"] or None,
                                              args["out_stride"], 0, None)
    assert rc == ARG


def test_compose_shape_null():
    assert hip.lib().gf2bv_compose_shape(None) == ARG
    v = (ctypes.c_double * 4)()
    hip.lib().gf2bv_compose_last_times(v)                     # (reads this thread's record: no device)
    assert all(x >= 0 for x in v)
