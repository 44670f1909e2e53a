"""A kept factorization, the host side: argument checks of gf2bv_factor_* and m4ri_factor (made before any device is touched, so
they hold on a machine without a GPU), the exported symbols, and FactoredSystem's right-hand-side words."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, QuadraticSystem, _internal, hip
from gf2bv_amd.factored import FactoredSystem

FACTOR_SYMBOLS = ["gf2bv_factor_digits", "gf2bv_factor_words", "gf2bv_factor_device", "gf2bv_factor_solve",
                  "gf2bv_factor_solve_device", "gf2bv_factor_rank", "gf2bv_factor_pivots", "gf2bv_factor_device_bytes",
                  "gf2bv_factor_free"]


def test_factor_symbols_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gf2bv_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gf2bv_[a-z_0-9]+)", dyn))
    for name in FACTOR_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in exported, name
        assert name in hip.EXPORTS, name
    assert "typedef struct gf2bv_factor gf2bv_factor;" in header


def test_abi_checks_arguments_before_device_use():
    """Every bad argument returns GF2BV_ERR_ARG (1), on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2)."""
    L = hip.lib()
    rows, cols = 130, 100
    aug = np.zeros((rows, 2), dtype=np.uint64)
    rhs = np.zeros((4, 3), dtype=np.uint64)
    off = np.zeros(rows + 1, dtype=np.int64)
    dig = np.zeros(4, dtype=np.uint32)
    A, R, O, D = aug.ctypes.data, rhs.ctypes.data, off.ctypes.data, dig.ctypes.data
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)
    hs = (ctypes.c_void_p * 4)()

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    err(L.gf2bv_factor_words(A, rows, cols, 2, 0, 0, None), "null")
    err(L.gf2bv_factor_words(None, rows, cols, 2, 0, 0, H), "null")
    err(L.gf2bv_factor_words(A, rows, cols, 1, 0, 0, H), "stride")
    err(L.gf2bv_factor_words(A, 99, cols, 2, 0, 0, H), "greater than or equal")
    err(L.gf2bv_factor_words(A, rows, cols, 2, 3, 0, H), "Invalid mode")
    err(L.gf2bv_factor_words(A, rows, 0, 2, 0, 0, H), "columns must be positive")
    err(L.gf2bv_factor_digits(D, None, 30, rows, cols, 0, 0, H), "null")
    err(L.gf2bv_factor_digits(D, O, 0, rows, cols, 0, 0, H), "bits_per_digit")
    err(L.gf2bv_factor_digits(D, O, 33, rows, cols, 0, 0, H), "bits_per_digit")
    err(L.gf2bv_factor_digits(D, O, 30, rows, cols, 0, 0, None), "null")
    err(L.gf2bv_factor_digits(D, O, 30, 99, cols, 0, 0, H), "greater than or equal")
    bad_off = off.copy()
    bad_off[0] = 1
    err(L.gf2bv_factor_digits(D, bad_off.ctypes.data, 30, rows, cols, 0, 0, H), "start at 0")
    err(L.gf2bv_factor_device(None, rows, cols, 2, 0, 0, None, H), "null")
    err(L.gf2bv_factor_device(A, rows, cols, 3, 0, 0, None, H), "stride")
    err(L.gf2bv_factor_device(A, rows, cols, 2, 0, 0, None, None), "null")
    err(L.gf2bv_factor_device(A, rows, 0, 2, 0, 0, None, H), "columns must be positive")
    err(L.gf2bv_factor_device(A + 8, rows, cols, 2, 0, 0, None, H), "16-byte alignment")
    err(L.gf2bv_factor_device(A, rows, cols, 2, 3, 0, None, H), "Invalid mode")
    err(L.gf2bv_factor_digits(D, O, 30, rows, cols, 3, 0, H), "Invalid mode")
    err(L.gf2bv_factor_digits(D, O, 30, rows, 0, 0, 0, H), "columns must be positive")
    bad_off[5:] = 3
    bad_off[0] = 0
    bad_off[9] = 2
    err(L.gf2bv_factor_digits(D, bad_off.ctypes.data, 30, rows, cols, 0, 0, H), "must not decrease")
    some_off = np.arange(rows + 1, dtype=np.int64)
    err(L.gf2bv_factor_digits(None, some_off.ctypes.data, 30, rows, cols, 0, 0, H), "null")
    assert not h.value                                          # nothing was made
    err(L.gf2bv_factor_solve(None, R, 4, 3, hs), "null")
    err(L.gf2bv_factor_solve_device(None, R, 4, 3, None, 0, hs), "null")
    assert L.gf2bv_factor_rank(None) == -1
    assert L.gf2bv_factor_device_bytes(None) == -1
    assert L.gf2bv_factor_pivots(None, None) == 1
    L.gf2bv_factor_free(None)                                  # (a no-op)


def test_binding_checks_arguments_first():
    eqs = [0b11, 0b101, 0b110, 0]
    with pytest.raises(ValueError, match="greater than or equal"):
        _internal.m4ri_factor(eqs[:2], 3, 0)
    with pytest.raises(ValueError, match="columns must be positive"):
        _internal.m4ri_factor(eqs, 0, 0)
    with pytest.raises(ValueError, match="Invalid mode"):
        _internal.m4ri_factor(eqs, 3, 5)
    with pytest.raises(TypeError):
        _internal.m4ri_factor(tuple(eqs), 3, 0)
    with pytest.raises(TypeError):
        _internal.m4ri_factor([1.0, 2, 3], 3, 0)
    with pytest.raises(TypeError):
        _internal.m4ri_factor(eqs, 3)
    with pytest.raises(TypeError):
        _internal.Factorization()


def test_python_wrapper_raises_after_close():
    f = hip.Factor(None, 4, 3, 0)                               # a closed handle
    with pytest.raises(ValueError):
        f.solve(np.zeros((1, 1), dtype=np.uint64))
    with pytest.raises(ValueError):
        f.rank
    with pytest.raises(ValueError):
        f.device_bytes
    f.close()                                                   # (closing twice is fine)


def _system():
    lin = LinearSystem([8, 5, 3, 70])
    a, b, c, w = lin.gens()
    exprs = [a ^ (b.zeroext(3) << 1), (a & 0x0F) ^ 0xA5, b[0] ^ c[2] ^ 1, 0, 1, a.rotl(3) ^ (a >> 2), b[1:4] ^ b[0:3],
             c[0] ^ c[0] ^ 1, (a ^ a), w ^ (w >> 9)]
    ints = [1 << 3 | 1, (1 << 9) ^ (1 << 14), 0]
    return lin, exprs + ints


def _values(rng, exprs, n, negative=True, wide=True):
    out = []
    for _ in range(n):
        vals = []
        for e in exprs:
            if isinstance(e, int):
                vals.append(rng.getrandbits(1))
            else:
                choices = [0, rng.getrandbits(len(e))]
                if negative:
                    choices.append(-rng.getrandbits(len(e) + 3))
                if wide:
                    choices.append(rng.getrandbits(len(e) + 9))
                vals.append(rng.choice(choices))
        out.append(vals)
    return out


def _as_ints(words: np.ndarray) -> list:
    return [int.from_bytes(row.tobytes(), "little") for row in words]


@pytest.mark.parametrize("negative,wide", [(False, False), (True, False), (False, True), (True, True)])
def test_rhs_words_equal_rhs_eqs(negative, wide):
    """The numpy words of FactoredSystem against LinearSystem._rhs_eqs' ints: BitVec, int and mixed expressions, values that
    are negative or wider than their expression, expressions wider than 64 bits."""
    lin, exprs = _system()
    rng = random.Random(5 + negative + 2 * wide)
    values_list = _values(rng, exprs, 30, negative, wide)
    fs = FactoredSystem(lin, exprs)
    eqs, rhs = lin._rhs_eqs(exprs, values_list)
    assert fs._eqs[:len(eqs)] == eqs and fs.rows >= lin._cols
    assert _as_ints(fs.rhs_words(values_list)) == rhs


def test_rhs_words_only_bitvecs_and_only_ints():
    lin = LinearSystem([32] * 3)
    x, y, z = lin.gens()
    rng = random.Random(9)
    for exprs in ([x ^ y, y ^ (z << 1), z], [x._bits[i] ^ y._bits[i] for i in range(32)] + [z._bits[0]] * 70):
        values_list = [[rng.getrandbits(len(e)) if not isinstance(e, int) else rng.getrandbits(1) for e in exprs] for _ in range(9)]
        fs = FactoredSystem(lin, exprs)
        assert _as_ints(fs.rhs_words(values_list)) == lin._rhs_eqs(exprs, values_list)[1]
        assert fs.rhs_words([]).shape == (0, (fs.rows + 63) // 64)


def test_rhs_words_reject_bad_values():
    lin, exprs = _system()
    fs = FactoredSystem(lin, exprs)
    good = [0] * len(exprs)
    with pytest.raises(ValueError):
        fs.rhs_words([good, good[:-1]])
    bad = list(good)
    bad[-2] = 2                                                 # an equation int takes 0 or 1 only
    with pytest.raises(ValueError):
        fs.rhs_words([good, bad])
    bad[-2] = -1
    with pytest.raises(ValueError):
        fs.rhs_words([bad])


def test_factored_system_closed_raises():
    lin, exprs = _system()
    with lin.factor(exprs) as fs:                               # (nothing reaches the device before the first solve)
        pass
    with pytest.raises(ValueError):
        fs.solve_raw_one_rhs([[0] * len(exprs)])
    with pytest.raises(ValueError):
        fs.solve_one([0] * len(exprs))
    q = QuadraticSystem([4])
    assert isinstance(q.factor([q.gens()[0]]), FactoredSystem)
