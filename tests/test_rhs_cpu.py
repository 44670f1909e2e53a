"""Many right-hand sides of one matrix, the host side: the flattening of LinearSystem.*_rhs and the argument checks of
m4ri_solve_rhs / gf2bv_solve_rhs_* (made before any device is touched, so they hold on a machine without a GPU)."""
import ctypes
import random

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, _internal, hip


def _system():
    lin = LinearSystem([8, 5, 3])
    a, b, c = lin.gens()
    exprs = [a ^ (b.zeroext(3) << 1), (a & 0x0F) ^ 0xA5, b[0] ^ c[2] ^ 1, 0, 1, a.rotl(3) ^ (a >> 2), b[1:4] ^ b[0:3],
             c[0] ^ c[0] ^ 1,                               # a BitVec whose only bit is the constant 1
             (a ^ a)]                                        # eight literal zeros
    ints = [1 << 3 | 1, (1 << 9) ^ (1 << 14), 0]              # equation ints: x2 ^ 1, x8 ^ x13, a literal zero
    return lin, exprs + ints


def _values(rng, exprs, n):
    out = []
    for _ in range(n):
        vals = []
        for e in exprs:
            if isinstance(e, int):
                vals.append(rng.getrandbits(1))
            else:
                vals.append(rng.choice([0, rng.getrandbits(len(e)), -rng.getrandbits(len(e) + 3), rng.getrandbits(len(e) + 9)]))
        out.append(vals)
    return out


def test_flattening_rebuilds_every_instance():
    lin, exprs = _system()
    rng = random.Random(11)
    values_list = _values(rng, exprs, 40)
    eqs, rhs = lin._rhs_eqs(exprs, values_list)
    assert len(rhs) == len(values_list)
    for vals, b in zip(values_list, rhs):
        zeros = [e ^ v for e, v in zip(exprs, vals)]
        mine = [(e & ~1) | ((b >> r) & 1) for r, e in enumerate(eqs)]
        assert [e for e in mine if e] == lin.get_eqs(zeros)
        assert b >> len(eqs) == 0


def test_flattening_keeps_zero_rows_and_empty_values():
    lin, exprs = _system()
    eqs, rhs = lin._rhs_eqs(exprs, [])
    assert rhs == [] and len(eqs) == sum(len(e) if not isinstance(e, int) else 1 for e in exprs)
    assert 0 in eqs                                          # zero rows stay: they carry the per-instance "1 = 0"
    assert lin.solve_one_rhs(exprs, []) == [] and lin.solve_raw_space_rhs(exprs, []) == []


def test_flattening_rejects_bad_values():
    lin, exprs = _system()
    good = [0] * len(exprs)
    with pytest.raises(ValueError):
        lin._rhs_eqs(exprs, [good, good[:-1]])
    with pytest.raises(ValueError):
        lin._rhs_eqs(exprs, [good + [0]])
    bad = list(good)
    bad[-2] = 2                                              # an equation int takes 0 or 1 only
    with pytest.raises(ValueError):
        lin.solve_raw_one_rhs(exprs, [good, bad])


def test_binding_checks_arguments_first():
    eqs = [0b11, 0b101, 0b110, 0]
    with pytest.raises(ValueError, match="greater than or equal"):
        _internal.m4ri_solve_rhs(eqs[:2], 3, 0, [1])
    with pytest.raises(ValueError, match="columns must be positive"):
        _internal.m4ri_solve_rhs(eqs, 0, 0, [1])
    with pytest.raises(ValueError, match="Invalid mode"):
        _internal.m4ri_solve_rhs(eqs, 3, 5, [1])
    with pytest.raises(ValueError, match="non-negative"):
        _internal.m4ri_solve_rhs(eqs, 3, 0, [1, -1])
    with pytest.raises(TypeError):
        _internal.m4ri_solve_rhs(eqs, 3, 0, (1,))
    with pytest.raises(TypeError):
        _internal.m4ri_solve_rhs(eqs, 3, 0, [1.0])
    with pytest.raises(TypeError):
        _internal.m4ri_solve_rhs(tuple(eqs), 3, 0, [1])
    assert _internal.m4ri_solve_rhs(eqs, 3, 0, []) == []


def test_abi_checks_arguments_before_device_use():
    """Every bad argument returns GF2BV_ERR_ARG (1), on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2)."""
    L = hip.lib()
    rows, cols = 130, 100
    aug = np.zeros((rows, 2), dtype=np.uint64)
    rhs = np.zeros((4, 3), dtype=np.uint64)
    hs = (ctypes.c_void_p * 4)()
    off = np.zeros(rows + 1, dtype=np.int64)
    dig = np.zeros(4, dtype=np.uint32)
    A, R, O, D = aug.ctypes.data, rhs.ctypes.data, off.ctypes.data, dig.ctypes.data

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    err(L.gf2bv_solve_rhs_words(A, rows, cols, 2, R, 0, 3, 0, 0, hs), "nrhs")
    err(L.gf2bv_solve_rhs_words(A, rows, cols, 2, R, 4, 2, 0, 0, hs), "rhs_words")
    err(L.gf2bv_solve_rhs_words(A, rows, cols, 2, None, 4, 3, 0, 0, hs), "null")
    err(L.gf2bv_solve_rhs_words(None, rows, cols, 2, R, 4, 3, 0, 0, hs), "null")
    err(L.gf2bv_solve_rhs_words(A, rows, cols, 2, R, 4, 3, 0, 0, None), "null")
    err(L.gf2bv_solve_rhs_words(A, rows, cols, 1, R, 4, 3, 0, 0, hs), "stride")
    err(L.gf2bv_solve_rhs_words(A, 99, cols, 2, R, 4, 3, 0, 0, hs), "greater than or equal")
    err(L.gf2bv_solve_rhs_words(A, rows, cols, 2, R, 4, 3, 3, 0, hs), "Invalid mode")
    err(L.gf2bv_solve_rhs_digits(D, O, 30, rows, cols, R, 0, 3, 0, 0, hs), "nrhs")
    err(L.gf2bv_solve_rhs_digits(D, O, 30, rows, cols, R, 4, 1, 0, 0, hs), "rhs_words")
    err(L.gf2bv_solve_rhs_digits(D, None, 30, rows, cols, R, 4, 3, 0, 0, hs), "null")
    err(L.gf2bv_solve_rhs_digits(D, O, 30, rows, cols, None, 4, 3, 0, 0, hs), "null")
    err(L.gf2bv_solve_rhs_digits(D, O, 0, rows, cols, R, 4, 3, 0, 0, hs), "bits_per_digit")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 2, R, 0, 3, 0, 0, None, 0, hs), "nrhs")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 2, R, 4, 2, 0, 0, None, 0, hs), "rhs_words")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 2, None, 4, 3, 0, 0, None, 0, hs), "null")
    err(L.gf2bv_solve_rhs_device(None, rows, cols, 2, R, 4, 3, 0, 0, None, 0, hs), "null")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 3, R, 4, 3, 0, 0, None, 0, hs), "stride")
    err(L.gf2bv_solve_rhs_device(A, rows, 0, 2, R, 4, 3, 0, 0, None, 0, hs), "columns must be positive")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 2, R, 4, 3, 0, 0, None, 0, None), "null")
    err(L.gf2bv_solve_rhs_device(A + 8, rows, cols, 2, R, 4, 3, 0, 0, None, 0, hs), "16-byte alignment")
    err(L.gf2bv_solve_rhs_device(A, rows, cols, 2, R + 4, 4, 3, 0, 0, None, 0, hs), "8-byte alignment")
    err(L.gf2bv_solve_rhs_digits(D, O, 33, rows, cols, R, 4, 3, 0, 0, hs), "bits_per_digit")
    err(L.gf2bv_solve_rhs_digits(D, O, 30, rows, cols, R, 4, 3, 0, 0, None), "null")
    err(L.gf2bv_solve_rhs_digits(D, O, 30, 99, cols, R, 4, 3, 0, 0, hs), "greater than or equal")
    bad_off = off.copy()
    bad_off[0] = 1
    err(L.gf2bv_solve_rhs_digits(D, bad_off.ctypes.data, 30, rows, cols, R, 4, 3, 0, 0, hs), "start at 0")
    bad_off = off.copy()
    bad_off[5:] = 3
    bad_off[9] = 2
    err(L.gf2bv_solve_rhs_digits(D, bad_off.ctypes.data, 30, rows, cols, R, 4, 3, 0, 0, hs), "must not decrease")
    some_off = np.arange(rows + 1, dtype=np.int64)
    err(L.gf2bv_solve_rhs_digits(None, some_off.ctypes.data, 30, rows, cols, R, 4, 3, 0, 0, hs), "null")
