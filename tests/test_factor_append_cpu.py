"""Equations appended to a kept factorization, the host side: the new symbols, the argument checks of gf2bv_factor_append_* and
gf2bv_factor_copy (made before any device is touched, so they hold on a machine without a GPU), and FactoredSystem.add's
right-hand-side bookkeeping (no factorization is made: the handles are created on first solve)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, hip
from gf2bv_amd.factored import FactoredSystem

APPEND_SYMBOLS = ["gf2bv_factor_append_words", "gf2bv_factor_append_digits", "gf2bv_factor_append_device",
                  "gf2bv_factor_rows", "gf2bv_factor_copy"]


def test_append_symbols_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gf2bv_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gf2bv_[a-z_0-9]+)", dyn))
    for name in APPEND_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in exported, name
        assert name in hip.EXPORTS, name


def test_append_abi_checks_arguments_before_device_use():
    """Null handles and pointers return GF2BV_ERR_ARG (1), on a machine without a GPU too; the row count of no handle is -1."""
    L = hip.lib()
    aug = np.zeros((4, 2), dtype=np.uint64)
    off = np.zeros(5, dtype=np.int64)
    dig = np.zeros(4, dtype=np.uint32)
    out = ctypes.c_void_p(0)

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    err(L.gf2bv_factor_append_words(None, aug.ctypes.data, 4, 2), "null")
    err(L.gf2bv_factor_append_words(None, aug.ctypes.data, 0, 2), "null")
    err(L.gf2bv_factor_append_digits(None, dig.ctypes.data, off.ctypes.data, 30, 4), "null")
    err(L.gf2bv_factor_append_digits(None, dig.ctypes.data, None, 30, 4), "null")
    err(L.gf2bv_factor_append_device(None, aug.ctypes.data, 4, 2, None), "null")
    err(L.gf2bv_factor_copy(None, ctypes.byref(out)), "null")
    assert out.value is None
    assert L.gf2bv_factor_rows(None) == -1


def _as_ints(words: np.ndarray) -> list:
    return [int.from_bytes(row.tobytes(), "little") for row in words]


def _values(rng, exprs, n, negative, wide):
    out = []
    for _ in range(n):
        vals = []
        for e in exprs:
            if isinstance(e, int):
                vals.append(rng.getrandbits(1))
            else:
                v = rng.getrandbits(len(e) + (40 if wide else 0))
                vals.append(-v if negative and rng.random() < 0.5 else v)
        out.append(vals)
    return out


def _stacked_words(lin, exprs, values_list, first, pad):
    """The words LinearSystem._rhs_eqs builds for the stacked expressions, with FactoredSystem's `pad` padding rows (constant 0)
    put where they stand: after the `first` rows of the first batch of expressions, before the added ones."""
    _, rhs = lin._rhs_eqs(exprs, values_list)
    out = []
    for r in rhs:
        lo = r & ((1 << first) - 1)
        hi = r >> first
        out.append(lo | (hi << (first + pad)))
    return out


@pytest.mark.parametrize("negative,wide", [(False, False), (True, False), (False, True), (True, True)])
def test_add_rhs_words_equal_rhs_eqs(negative, wide):
    """After add: the words equal those of the concatenated expressions, the padding rows in place (the first batch is
    narrower than the unknowns, so the system was padded)."""
    lin = LinearSystem([32, 32, 7])
    x, y, z = lin.gens()
    first = [x ^ (y & 0xFFFF), z, x._bits[3] ^ z._bits[1]]
    more = [[y, x._bits[0] ^ 1], [(y >> 3) ^ x, z._bits[2], z]]
    rng = random.Random(11 + negative + 2 * wide)
    fs = FactoredSystem(lin, first)
    nfirst = sum(len(e) if not isinstance(e, int) else 1 for e in first)
    assert fs.rows == lin._cols > nfirst
    exprs = list(first)
    for batch in more:
        fs.add(batch)
        exprs += batch
        values_list = _values(rng, exprs, 20, negative, wide)
        assert fs.rows == lin._cols + sum(len(e) if not isinstance(e, int) else 1 for e in exprs) - nfirst
        assert _as_ints(fs.rhs_words(values_list)) == _stacked_words(lin, exprs, values_list, nfirst, lin._cols - nfirst)
        assert fs.rhs_words([]).shape == (0, (fs.rows + 63) // 64)
    # the equations of the added rows follow the padding, in order
    eqs, _ = lin._rhs_eqs(exprs, [])
    assert fs._eqs == eqs[:nfirst] + [0] * (lin._cols - nfirst) + eqs[nfirst:]


def test_add_without_padding_and_empty_add():
    lin = LinearSystem([16, 16])
    x, y = lin.gens()
    exprs = [x ^ y, x, y]                                        # 48 rows >= 32 unknowns: no padding
    fs = FactoredSystem(lin, exprs)
    fs.add([])
    assert fs.rows == 48
    fs.add([x ^ (y << 1), 1 ^ x._bits[5]])
    exprs += [x ^ (y << 1), 1 ^ x._bits[5]]
    rng = random.Random(3)
    values_list = _values(rng, exprs, 12, True, True)
    assert _as_ints(fs.rhs_words(values_list)) == lin._rhs_eqs(exprs, values_list)[1]


def test_add_value_counts_and_closed():
    lin = LinearSystem([32, 32])
    x, y = lin.gens()
    fs = FactoredSystem(lin, [x, y])
    fs.add([x ^ y])
    with pytest.raises(ValueError):
        fs.rhs_words([[0, 0]])                                   # three expressions now
    with pytest.raises(ValueError):
        fs.rhs_words([[0, 0, 0, 0]])
    assert fs.rhs_words([[0, 0, 0]]).shape == (1, 2)
    c = fs.copy()
    c.add([x])
    assert c.rows == 128 and fs.rows == 96                      # the copy's bookkeeping is its own
    with pytest.raises(ValueError):
        fs.rhs_words([[0, 0, 0, 0]])
    fs.close()
    with pytest.raises(ValueError):
        fs.add([x])
    with pytest.raises(ValueError):
        fs.copy()
    c.close()
