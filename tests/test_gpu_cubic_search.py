"""search_all_cubic / search_one_cubic / search_all_xl / search_one_xl end to end on the MI355X.  The ground truth is brute force of
the ORIGINAL equations over all 2^n states on the CPU (n = 12), which shares nothing with the library; where the host walk of
solve_all / solve_all_xl still reaches, the order is compared with it too."""
import functools

import numpy as np
import pytest
import torch

from gf2bv_amd import (DimensionTooLargeError, PackedCubicGuessSystem, PackedCubicSystem, PackedQuadraticSystem, QuadraticSystem, hip,
                       search_all_cubic, search_all_xl, search_one_cubic, search_one_xl)
from gf2bv_amd._internal import _space_from_ints
from gf2bv_amd.linsys import xl3_cols
from tests.cubic_terms import REGISTER_12, register_zeros
from tests.harness_models import GaloisLFSR
from tests.test_gpu_stream_order import cycles      # noqa: F401  (fixture)
from tests.test_gpu_xl import _filter, lfsr_zeros

pytestmark = pytest.mark.gpu

N = 12
COLS = xl3_cols(N)                       # 298

# PackedCubicSystem on the n = 12 register.  Output count -> dimension of the linearised space: 298 minus the rank of the first
# `count` equations, computed on the CPU with tests/cubic_terms.py (register_eqs into an IntBasis); the first 286 equations are
# independent for both secrets, so the dimension is 298 - count.  From 21 outputs on the secret is the only state that fits (brute
# force over the 4096 states); 12 outputs leave several.
CUBIC_COUNTS = {286: 12, 281: 17, 40: 258, 12: 286}
SECRETS = (0x52F, 0x3A1)

# search_all_xl on the filtered Galois register of tests/test_gpu_xl.py at n = 12 (taps 0xE08, filter inputs 1, 3, 5, 7, 9).
# Outputs -> (annihilator equations, dimension of degree-3 XL's space, states that fit): the dimension is 298 minus the rank of the
# XL rows (tests/xl_terms.py, xl3_ints into an IntBasis), the states by brute force, both on the CPU.
LFSR = (N, 0xE08, (1, 3, 5, 7, 9), 0x797)
XL_OUTPUTS = {56: (27, 12, 6), 52: (24, 43, 14), 40: (19, 98, 50)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _register_streams(count: int) -> np.ndarray:
    """[count, 4096] output bits of the cubic register from every state, by numpy over all states at once"""
    taps, pos = REGISTER_12["taps"], REGISTER_12["pos"]
    s = [((np.arange(1 << N, dtype=np.uint32) >> g) & 1).astype(np.uint8) for g in range(N)]
    out = []
    for _ in range(count):
        out.append(s[pos[0]] ^ (s[pos[1]] & s[pos[2]]) ^ (s[pos[3]] & s[pos[4]] & s[pos[5]]))
        first, nxt = s[0], s[1:] + [np.zeros_like(s[0])]
        s = [(nxt[g] ^ first) if (taps >> g) & 1 else nxt[g] for g in range(N)]
    return np.array(out)


def _cubic_brute(secret: int, count: int) -> set:
    streams = _register_streams(300)[:count]
    return {(int(s),) for s in np.nonzero((streams == streams[:, secret:secret + 1]).all(axis=0))[0]}


@functools.lru_cache(maxsize=None)
def _cubic_case(secret: int, count: int) -> tuple:
    c = PackedCubicSystem([N])
    return c, tuple(register_zeros(c, secret, REGISTER_12["taps"], REGISTER_12["pos"], count))


@pytest.mark.parametrize("secret", SECRETS, ids=hex)
@pytest.mark.parametrize("count", [286, 281])
def test_cubic_register_where_the_host_walk_reaches(secret, count):
    """dimension 12 (solve_all's default reach) and 17 (max_dimension raised): the same elements in the same order"""
    c, zeros = _cubic_case(secret, count)
    d = CUBIC_COUNTS[count]
    assert c.solve_raw_space(zeros).dimension == d
    want = list(c.solve_all(zeros, max_dimension=d))
    assert set(want) == _cubic_brute(secret, count) == {(secret,)}
    assert search_all_cubic(c, zeros) == want
    assert search_one_cubic(c, zeros) == want[0]


@pytest.mark.parametrize("secret", SECRETS, ids=hex)
@pytest.mark.parametrize("count", [40, 12])
def test_cubic_register_far_above_the_host_walk(secret, count):
    """dimension 258 and 286: solve_all refuses, the search returns the brute-force set"""
    c, zeros = _cubic_case(secret, count)
    assert c.solve_raw_space(zeros).dimension == CUBIC_COUNTS[count]
    with pytest.raises(DimensionTooLargeError):
        list(c.solve_all(zeros))
    want = _cubic_brute(secret, count)
    assert (secret,) in want and (len(want) == 1) == (count == 40)
    got = search_all_cubic(c, zeros)
    assert len(got) == len(want) and set(got) == want
    assert search_one_cubic(c, zeros) == got[0]
    assert hip.cubic_last_times()["ms_search"] > 0


def test_cubic_guess_subclass_is_accepted():
    c = PackedCubicGuessSystem([N])
    zeros = register_zeros(c, 0x52F, REGISTER_12["taps"], REGISTER_12["pos"], 40)
    assert search_all_cubic(c, zeros) == [(0x52F,)]


# -- degree-3 XL on both quadratic front-ends ---------------------------------------------------------------------------------------------
def _lfsr_brute(outputs: int) -> set:
    n, taps, select, secret = LFSR
    reg, stream = GaloisLFSR(n, taps, secret), []
    for _ in range(outputs):
        reg()
        stream.append(_filter(*[(reg.state >> i) & 1 for i in select]))
    fits = set()
    for s in range(1 << n):
        reg, ok = GaloisLFSR(n, taps, s), True
        for bit in stream:
            reg()
            if bit:
                x0, x1, x2 = [(reg.state >> i) & 1 for i in select[:3]]
                if (x0 & x1) ^ x0 ^ (x1 & x2) ^ x1 ^ x2 ^ 1:
                    ok = False
                    break
        if ok:
            fits.add((s,))
    return fits


@pytest.mark.parametrize("outputs", sorted(XL_OUTPUTS))
def test_xl_search_on_both_front_ends(outputs):
    n, taps, select, secret = LFSR
    neq, dim, nfit = XL_OUTPUTS[outputs]
    want = _lfsr_brute(outputs)
    assert (secret,) in want and len(want) == nfit
    results = []
    for cls in (QuadraticSystem, PackedQuadraticSystem):
        q = cls([n])
        zeros = lfsr_zeros(q, n, taps, select, secret, outputs)
        assert len(zeros) == neq and q.solve_raw_space_xl(zeros).dimension == dim
        got = search_all_xl(q, zeros)
        if dim <= 16:
            assert got == list(q.solve_all_xl(zeros))
        else:
            with pytest.raises(DimensionTooLargeError):
                list(q.solve_all_xl(zeros))
        assert len(got) == nfit and set(got) == want
        assert search_one_xl(q, zeros) == got[0]
        results.append(got)
    assert sorted(results[0]) == sorted(results[1])


# -- the other outcomes --------------------------------------------------------------------------------------------------------------
def test_inconsistent_system_has_no_point():
    c, zeros = _cubic_case(0x52F, 40)
    assert search_all_cubic(c, list(zeros) + [1]) == [] and search_one_cubic(c, list(zeros) + [1]) is None
    q = QuadraticSystem([N])
    zq = lfsr_zeros(q, *LFSR, 40)
    assert search_all_xl(q, zq + [1]) == [] and search_one_xl(q, zq + [1]) is None


def test_more_points_than_max_solutions():
    c, zeros = _cubic_case(0x3A1, 12)
    nfit = len(_cubic_brute(0x3A1, 12))
    assert nfit > 2
    with pytest.raises(ValueError, match=rf"^{nfit} consistent points, more than max_solutions \(2\)$"):
        search_all_cubic(c, zeros, max_solutions=2)
    assert len(search_all_cubic(c, zeros, max_solutions=nfit)) == nfit


def test_search_gives_up_above_max_enum(monkeypatch):
    """a hand-built space: six unit vectors on the linear unknowns, every product coordinate 0: r = r_eff = 6, no affine form"""
    n = 6
    c = PackedCubicSystem([n])
    space = _space_from_ints(xl3_cols(n), 0, tuple(1 << a for a in range(n)))
    monkeypatch.setattr(c, "solve_raw_space", lambda zeros: space)
    with pytest.raises(DimensionTooLargeError, match="the search gave up") as err:
        search_all_cubic(c, [], max_enum=4)
    assert err.value.space is space
    with pytest.raises(DimensionTooLargeError):
        search_one_cubic(c, [], max_enum=5)
    want = [c.convert_sol(s) for s in space if c.convert_sol(s) is not None]
    assert sorted(want) == [(0,), (1,), (2,), (4,), (8,), (16,), (32,)]
    assert search_all_cubic(c, [], max_enum=6) == want


# -- stream order -----------------------------------------------------------------------------------------------------------------------
def test_search_right_after_another_solve(cycles):      # noqa: F811
    """the search runs on the solver's pool stream: issued while the device is still busy with a spin and right after another solve,
    it returns what it returns alone"""
    c, zeros = _cubic_case(0x3A1, 12)
    alone = search_all_cubic(c, zeros)
    torch.cuda._sleep(cycles)
    q = QuadraticSystem([N])
    other = search_all_xl(q, lfsr_zeros(q, *LFSR, 52))
    got = search_all_cubic(c, zeros)
    assert got == alone and len(other) == XL_OUTPUTS[52][2]
