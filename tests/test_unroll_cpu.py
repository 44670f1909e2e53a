"""Unrolling without a GPU: the host twin (tests/unroll_terms.py) against Python-int arithmetic, the refusals of gf2bv_amd.unroll (raised
before any library call), the exported names, and the argument errors of the two C entries, which return before a device is looked for."""
import os
import random
import re

import numpy as np
import pytest

import gf2bv_amd
from gf2bv_amd import BitVec, LinearSystem, PackedLinearSystem, PackedQuadraticSystem, compose, hip
from tests import compose_terms as T
from tests import unroll_terms as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 63, 64, 70])
def test_twin_against_python_ints(n):
    rng = random.Random(n)
    ra, start, step, count = 3, 2, 3, 4
    a = [rng.getrandbits(n + 1) for _ in range(ra)]
    b = [rng.getrandbits(n + 1) for _ in range(n)]
    w = T.form_words(n)
    got = U.unroll(T.rows_of_ints(a, w), n, T.rows_of_ints(b, w), start, step, count)
    assert got.shape == (count * ra, w)
    cur, want = list(a), []
    for t in range(start + (count - 1) * step + 1):
        if t >= start and (t - start) % step == 0:
            want += cur
        cur = T.substitute_ints(cur, n, b)
    assert T.int_rows(got) == want
    # start = 0, step = 1: item 0 is a itself
    plain = U.unroll(T.rows_of_ints(a, w), n, T.rows_of_ints(b, w), 0, 1, 2)
    assert T.int_rows(plain) == a + T.substitute_ints(a, n, b)


def test_twin_large_exponents_take_the_squaring_path():
    rng = random.Random(3)
    n = 9
    a = T.rows_of_ints([rng.getrandbits(n + 1) for _ in range(2)], 1)
    b = T.rows_of_ints([rng.getrandbits(n + 1) for _ in range(n)], 1)
    big = U.WALK + 5
    got = U.unroll(a, n, b, big, big, 3)
    for i in range(3):
        assert np.array_equal(got[2 * i:2 * i + 2], T.substitute(a, n, T.power_loop(b, n, big * (1 + i)), n))


def test_twin_ignores_bits_above_the_unknowns():
    rng = random.Random(5)
    n = 5
    a = [rng.getrandbits(n + 1) for _ in range(4)]
    b = [rng.getrandbits(n + 1) for _ in range(n)]
    for start in (0, 2):
        clean = U.unroll(T.rows_of_ints(a, 1), n, T.rows_of_ints(b, 1), start, 1, 3)
        dirty = U.unroll(T.rows_of_ints([v | rng.getrandbits(50) << (n + 1) for v in a], 1), n,
                         T.rows_of_ints([v | rng.getrandbits(50) << (n + 1) for v in b], 1), start, 1, 3, stride=2)
        assert np.array_equal(clean[:, 0], dirty[:, 0]) and not dirty[:, 1].any()


@pytest.mark.parametrize("start, step, count, want", [
    (0, 1, 0, 0), (0, 1, 1, 0), (0, 1, 2, 1), (0, 1, 3, 3), (0, 1, 4, 3), (0, 1, 5, 5), (0, 1, 8, 5), (0, 1, 9, 7), (0, 1, 17, 9),
    (5, 1, 5, (4 + 1) + 5), (0, 3, 5, 3 + 5), (7, 2, 5, 2 + (5 + 1) + 5), ((1 << 64) + 3, (1 << 64) + 1, 5, 66 + (67 + 1) + 5),
])
def test_product_formula(start, step, count, want):
    assert U.products(start, step, count) == want


# -- gf2bv_amd.unroll: refusals by name, before the library ---------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*args):
        raise AssertionError("the library was called")
    monkeypatch.setattr(compose, "m4ri_unroll_packed", refuse)
    monkeypatch.setattr(compose, "m4ri_compose_packed", refuse)
    monkeypatch.setattr(compose, "m4ri_power_packed", refuse)


def test_refusals(no_library):
    lin = PackedLinearSystem([8, 8])
    x, y = lin.gens()
    tx, ty = LinearSystem([8, 8]).gens()
    assert isinstance(tx, BitVec)
    with pytest.raises(TypeError, match="tuple-of-int"):
        compose.unroll(tx, (x, y), 3)
    with pytest.raises(TypeError, match="tuple-of-int"):
        compose.unroll(x, (tx, ty), 3)
    quad = PackedQuadraticSystem([8, 8])
    qx, qy = quad.gens()
    prod = quad.mul_bit(qx[0], qy[0])
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.unroll(prod, (qx, qy), 3)
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.unroll([qx, prod], (qx, qy), 3)
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.unroll(qx, (qx[:7].concat(prod), qy), 3)
    wide = PackedLinearSystem([100]).gens()[0]                # two words; 16 unknowns are one
    with pytest.raises(ValueError, match="square"):
        compose.unroll(wide[:16], (wide[:16],), 3)            # 16 image bits over forms of 100 unknowns
    with pytest.raises(ValueError, match="words wide"):
        compose.unroll(wide, (x, y), 3)
    with pytest.raises(ValueError, match="negative"):
        compose.unroll(x, (x, y), -1)
    with pytest.raises(ValueError, match="negative"):
        compose.unroll(x, (x, y), 3, start=-1)
    with pytest.raises(ValueError, match="step"):
        compose.unroll(x, (x, y), 3, step=0)
    with pytest.raises(ValueError, match="step"):
        compose.unroll(x, (x, y), 3, step=-2)
    with pytest.raises(ValueError, match="different numbers of unknowns"):
        compose.unroll(x, (x, wide[:8]), 3)


def test_count_zero_is_empty_without_the_library(no_library):
    x, y = PackedLinearSystem([8, 8]).gens()
    assert compose.unroll(x, (y, x), 0) == []
    assert compose.unroll([x, y[:3]], (y, x), 0, start=5, step=2) == []


def test_substitute_of_a_product_still_raises(no_library):
    quad = PackedQuadraticSystem([8, 8])
    qx, qy = quad.gens()
    with pytest.raises(TypeError, match="substitution into products is not linear"):
        compose.substitute(quad.mul_bit(qx[0], qy[0]), (qx, qy))


def test_calls_reach_the_library_and_items_are_views(monkeypatch):
    seen = []

    def fake_unroll(a, ra, n, b, start, step, count):
        seen.append((a.copy(), ra, n, b.copy(), start.copy(), step.copy(), count))
        return bytearray(np.arange(count * ra * b.shape[1], dtype=np.uint64).tobytes())

    monkeypatch.setattr(compose, "m4ri_unroll_packed", fake_unroll)
    x, y = PackedLinearSystem([8, 8]).gens()
    one = compose.unroll(x ^ y, (y, x), 3)
    assert isinstance(one, list) and len(one) == 3
    assert all(isinstance(v, gf2bv_amd.PackedBitVec) and len(v) == 8 for v in one)
    two = compose.unroll([x, y[:3]], (y, x), 4, start=(1 << 64) + 2, step=5)
    assert len(two) == 4 and all(isinstance(it, tuple) and [len(v) for v in it] == [8, 3] for it in two)
    a, ra, n, b, start, step, count = seen[1]
    assert (ra, n, count) == (11, 16, 4) and np.array_equal(a, np.concatenate([x._rows, y._rows[:3]]))
    assert np.array_equal(b, np.concatenate([y._rows, x._rows]))
    assert start.tolist() == [2, 1] and step.tolist() == [5]
    # time-major, and no copy: every item looks into the one array that came back
    assert two[1][0]._rows[0, 0] == 11 and two[1][1]._rows[0, 0] == 11 + 8 and two[3][1]._rows[2, 0] == 3 * 11 + 10
    whole = two[0][0]._rows.base
    while getattr(whole, "base", None) is not None and isinstance(whole.base, np.ndarray):
        whole = whole.base
    assert all(np.shares_memory(v._rows, whole) for it in two for v in it)
    assert not any(v._rows.flags.owndata for it in two for v in it)


# -- names -------------------------------------------------------------------------------------------------------------------------
NAMES = ("gf2bv_compose_unroll_words", "gf2bv_compose_unroll_device")


def test_exported_names():
    assert "unroll" in gf2bv_amd.__all__
    assert gf2bv_amd.unroll is compose.unroll
    header = open(os.path.join(ROOT, "include", "gf2bv_hip.h")).read()
    for name in NAMES:
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    from gf2bv_amd import _internal
    assert _internal.m4ri_unroll_packed.__doc__


# -- argument errors of the C entries: GF2BV_ERR_ARG (1) with no device looked for ---------------------------------------------------
ARG = 1
BIG = (1 << 31) - 65            # n + 1 = 2^31 - 64
RG = hip.compose_shape()["rows_per_workgroup"]
DEV = 0x7f0000001000            # a 16-byte aligned address that is never read: every case fails its checks first


def _w(shape):
    return np.zeros(shape, dtype=np.uint64)


def _k(*words):
    return np.array(words, dtype=np.uint64)


def _p(x):
    return None if x is None else x.ctypes.data


COMMON = [
    dict(ra=-1), dict(count=-1), dict(n=0), dict(n=BIG), dict(start=None), dict(step=None), dict(snw=0), dict(snw=-1), dict(pnw=0),
    dict(step=_k(0)), dict(step=_k(0, 0), pnw=2),
    # n = 70: one column tile, so the largest block may have fewer than 2^31 row groups
    dict(ra=1, count=(1 << 32) * RG), dict(ra=RG, count=1 << 32), dict(ra=3, count=1 << 62),
]


@pytest.mark.parametrize("case", [dict(a=None), dict(b=None), dict(out=None), dict(a_stride=1), dict(b_stride=1), dict(out_stride=1)] + COMMON)
def test_unroll_words_argument_errors(case):
    args = dict(a=_w((4, 2)), ra=4, a_stride=2, n=70, b=_w((70, 2)), b_stride=2, start=_k(3), snw=1, step=_k(1), pnw=1, count=3,
                out=_w((12, 2)), out_stride=2)
    args.update(case)
    rc = hip.lib().gf2bv_compose_unroll_words(_p(args["a"]), args["ra"], args["a_stride"], args["n"], _p(args["b"]), args["b_stride"],
                                              _p(args["start"]), args["snw"], _p(args["step"]), args["pnw"], args["count"],
                                              _p(args["out"]), args["out_stride"], 0)
    assert rc == ARG
    assert hip.lib().gf2bv_last_error()


@pytest.mark.parametrize("case", [
    dict(d_a=0), dict(d_b=0), dict(d_out=0), dict(a_stride=0), dict(b_stride=0), dict(out_stride=0),
    dict(a_stride=3), dict(b_stride=3), dict(out_stride=3), dict(d_a=DEV + 8), dict(d_b=DEV + 8), dict(d_out=DEV + 8),
] + COMMON)
def test_unroll_device_argument_errors(case):
    args = dict(d_a=DEV, ra=4, a_stride=2, n=70, d_b=DEV, b_stride=2, start=_k(3), snw=1, step=_k(1), pnw=1, count=3, d_out=DEV, out_stride=2)
    args.update(case)
    rc = hip.lib().gf2bv_compose_unroll_device(args["d_a"] or None, args["ra"], args["a_stride"], args["n"], args["d_b"] or None,
                                               args["b_stride"], _p(args["start"]), args["snw"], _p(args["step"]), args["pnw"],
                                               args["count"], args["d_out"] or None, args["out_stride"], 0, None)
    assert rc == ARG
    assert hip.lib().gf2bv_last_error()


def test_hip_wrapper_refuses_negative_start_and_step():
    a, b = _w((2, 2)), _w((70, 2))
    with pytest.raises(ValueError):
        hip.compose_unroll_words(a, 70, b, 3, start=-1)
    with pytest.raises(ValueError):
        hip.compose_unroll_words(a, 70, b, 3, step=-1)
