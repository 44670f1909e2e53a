"""search_all_quartic / search_one_quartic / search_all_xl4 / search_one_xl4 end to end on the MI355X.  The ground truth is brute force
of the ORIGINAL equations over all 2^n states on the CPU (n = 12 and 16), which shares nothing with the library; where the host walk
of solve_all / solve_all_xl4 still reaches, the order is compared with it too."""
import functools

import pytest
import torch

from gf2bv_amd import (DimensionTooLargeError, PackedCubicGuessSystem, PackedCubicSystem, PackedQuadraticSystem, PackedQuarticSystem,
                       QuadraticSystem, hip, search_all_quartic, search_all_xl4, search_one_quartic, search_one_xl4)
from gf2bv_amd._internal import _space_from_ints
from gf2bv_amd.linsys import xl4_cols
from tests.cubic_terms import REGISTER_12, register_zeros
from tests.quartic_terms import REGISTER4_12, REGISTER4_16, IntBasis, register4_brute, register4_eqs, register4_zeros
from tests.test_gpu_cubic_search import _cubic_brute, _lfsr_brute
from tests.test_gpu_stream_order import cycles      # noqa: F401  (fixture)
from tests.test_gpu_xl import lfsr_zeros

pytestmark = pytest.mark.gpu

N = 12
COLS = xl4_cols(N)                       # 793

# PackedQuarticSystem on the n = 12 register.  Output count -> dimension of the linearised space: 793 minus the rank of the first
# `count` equations; the first 793 equations are independent for both secrets (test_first_equations_are_independent, on the CPU), so
# the dimension is 793 - count.  From 12 outputs on the secret is the only state that fits; 10 outputs leave 6 states for 0x52F and 4
# for 0x3A1 (brute force over the 4096 states, repeated by the tests).
QUARTIC_COUNTS = {781: 12, 777: 16, 40: 753, 12: 781, 10: 783}
SECRETS = (0x52F, 0x3A1)
FITS_AT_10 = {0x52F: 6, 0x3A1: 4}
# the n = 16 register: states that fit 16 and 14 outputs
SECRETS_16 = (0x52E7, 0x3A09)
FITS_16 = {(0x52E7, 16): 1, (0x52E7, 14): 4, (0x3A09, 16): 1, (0x3A09, 14): 3}

# search_all_xl4 on PackedCubicSystem with the cubic register of tests/cubic_terms.py: outputs -> dimension of degree-4 XL's space
# (793 minus the rank of the equations and their products with every unknown, tests/cubic_xl4_terms.py into an IntBasis, on the CPU)
CUBIC_XL4 = {60: 13, 59: 26, 40: 273}

# search_all_xl4 on the filtered Galois register of tests/test_gpu_xl.py at n = 12 (taps 0xE08, filter inputs 1, 3, 5, 7, 9).
# Outputs -> (annihilator equations, dimension of degree-4 XL's space, states that fit): the dimension is 793 minus the rank of the
# XL rows (tests/xl4_terms.py, xl4_ints into an IntBasis), the states by brute force, both on the CPU.
LFSR = (N, 0xE08, (1, 3, 5, 7, 9), 0x797)
XL4_OUTPUTS = {52: (24, 13, 14), 40: (19, 49, 50)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _quartic_case(secret: int, count: int, n: int = N) -> tuple:
    reg = REGISTER4_12 if n == 12 else REGISTER4_16
    c = PackedQuarticSystem([n])
    return c, tuple(register4_zeros(c, secret, count=count, **reg))


def _brute(secret: int, count: int, n: int = N) -> set:
    return {(s,) for s in register4_brute(secret, count=count, **(REGISTER4_12 if n == 12 else REGISTER4_16))}


@pytest.mark.parametrize("secret", SECRETS, ids=hex)
def test_first_equations_are_independent(secret):
    """what makes the dimension 793 - count (CPU only: the truth-table equations of tests/quartic_terms.py into an IntBasis)"""
    basis = IntBasis()
    assert all(basis.add(e) for e in register4_eqs(secret, count=COLS, **REGISTER4_12))


@pytest.mark.parametrize("secret", SECRETS, ids=hex)
@pytest.mark.parametrize("count", [781, 777])
def test_quartic_register_where_the_host_walk_reaches(secret, count):
    """dimension 12 (solve_all's default reach) and 16 (max_dimension raised): the same elements in the same order"""
    c, zeros = _quartic_case(secret, count)
    d = QUARTIC_COUNTS[count]
    assert c.solve_raw_space(zeros).dimension == d
    want = list(c.solve_all(zeros, max_dimension=d))
    assert set(want) == _brute(secret, count) == {(secret,)}
    assert search_all_quartic(c, zeros) == want
    assert search_one_quartic(c, zeros) == want[0]


@pytest.mark.parametrize("secret", SECRETS, ids=hex)
@pytest.mark.parametrize("count", [40, 12, 10])
def test_quartic_register_far_above_the_host_walk(secret, count):
    """dimension 753, 781 and 783: solve_all refuses, the search returns the brute-force set"""
    c, zeros = _quartic_case(secret, count)
    assert c.solve_raw_space(zeros).dimension == QUARTIC_COUNTS[count]
    with pytest.raises(DimensionTooLargeError):
        list(c.solve_all(zeros))
    want = _brute(secret, count)
    assert (secret,) in want and len(want) == (FITS_AT_10[secret] if count == 10 else 1)
    got = search_all_quartic(c, zeros)
    assert len(got) == len(want) and set(got) == want
    assert search_one_quartic(c, zeros) == got[0]
    assert hip.quartic_last_times()["ms_search"] > 0


@pytest.mark.parametrize("secret", SECRETS_16, ids=hex)
@pytest.mark.parametrize("count", [16, 14])
def test_quartic_register_of_sixteen_unknowns(secret, count):
    """n = 16 (2516 columns) from 16 and from 14 outputs: dimension 2500 and 2502"""
    c, zeros = _quartic_case(secret, count, 16)
    assert c.solve_raw_space(zeros).dimension == xl4_cols(16) - count
    want = _brute(secret, count, 16)
    assert (secret,) in want and len(want) == FITS_16[secret, count]
    got = search_all_quartic(c, zeros)
    assert len(got) == len(want) and set(got) == want
    assert search_one_quartic(c, zeros) == got[0]


# -- degree-4 XL on cubic equations -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cubic_case(count: int, cls=PackedCubicSystem) -> tuple:
    c = cls([N])
    return c, tuple(register_zeros(c, 0x52F, REGISTER_12["taps"], REGISTER_12["pos"], count))


def test_cubic_xl4_where_the_host_walk_reaches():
    c, zeros = _cubic_case(60)
    assert c.solve_raw_space_xl4(zeros).dimension == CUBIC_XL4[60]
    want = list(c.solve_all_xl4(zeros))
    assert set(want) == _cubic_brute(0x52F, 60)
    assert search_all_xl4(c, zeros) == want
    assert search_one_xl4(c, zeros) == want[0]


@pytest.mark.parametrize("count", [59, 40])
def test_cubic_xl4_above_the_host_walk(count):
    c, zeros = _cubic_case(count)
    assert c.solve_raw_space_xl4(zeros).dimension == CUBIC_XL4[count]
    with pytest.raises(DimensionTooLargeError):
        list(c.solve_all_xl4(zeros))
    want = _cubic_brute(0x52F, count)
    got = search_all_xl4(c, zeros)
    assert (0x52F,) in want and len(got) == len(want) and set(got) == want
    assert search_one_xl4(c, zeros) == got[0]


def test_cubic_guess_subclass_is_accepted():
    c, zeros = _cubic_case(40, PackedCubicGuessSystem)
    assert search_all_xl4(c, zeros) == [(0x52F,)]


# -- degree-4 XL on both quadratic front-ends -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", sorted(XL4_OUTPUTS))
def test_xl4_search_on_both_front_ends(outputs):
    n, taps, select, secret = LFSR
    neq, dim, nfit = XL4_OUTPUTS[outputs]
    want = _lfsr_brute(outputs)
    assert (secret,) in want and len(want) == nfit <= 64
    results = []
    for cls in (QuadraticSystem, PackedQuadraticSystem):
        q = cls([n])
        zeros = lfsr_zeros(q, n, taps, select, secret, outputs)
        assert len(zeros) == neq and q.solve_raw_space_xl4(zeros).dimension == dim
        got = search_all_xl4(q, zeros)
        if dim <= 16:
            assert got == list(q.solve_all_xl4(zeros))
        else:
            with pytest.raises(DimensionTooLargeError):
                list(q.solve_all_xl4(zeros))
        assert len(got) == nfit and set(got) == want
        assert search_one_xl4(q, zeros) == got[0]
        results.append(got)
    assert results[0] == results[1]


# -- the other outcomes --------------------------------------------------------------------------------------------------------------
def test_inconsistent_system_has_no_point():
    c, zeros = _quartic_case(0x52F, 40)
    assert search_all_quartic(c, list(zeros) + [1]) == [] and search_one_quartic(c, list(zeros) + [1]) is None
    q = QuadraticSystem([N])
    zq = lfsr_zeros(q, *LFSR, 40)
    assert search_all_xl4(q, zq + [1]) == [] and search_one_xl4(q, zq + [1]) is None


def test_more_points_than_max_solutions():
    c, zeros = _quartic_case(0x52F, 10)
    nfit = FITS_AT_10[0x52F]
    with pytest.raises(ValueError, match=rf"^{nfit} consistent points, more than max_solutions \(2\)$"):
        search_all_quartic(c, zeros, max_solutions=2)
    assert len(search_all_quartic(c, zeros, max_solutions=nfit)) == nfit


def test_search_gives_up_above_max_enum():
    """12 unknowns and 10 outputs: no affine form gets the 12 variables down to 4"""
    c, zeros = _quartic_case(0x3A1, 10)
    with pytest.raises(DimensionTooLargeError, match="the search gave up") as err:
        search_all_quartic(c, zeros, max_enum=4)
    assert err.value.space.dimension == QUARTIC_COUNTS[10]
    with pytest.raises(DimensionTooLargeError):
        search_one_quartic(c, zeros, max_enum=4)


def test_search_gives_up_on_a_hand_built_space(monkeypatch):
    """six unit vectors on the linear unknowns, every product coordinate 0: r = r_eff = 6, no affine form"""
    n = 6
    c = PackedQuarticSystem([n])
    space = _space_from_ints(xl4_cols(n), 0, tuple(1 << a for a in range(n)))
    monkeypatch.setattr(c, "solve_raw_space", lambda zeros: space)
    with pytest.raises(DimensionTooLargeError, match="the search gave up") as err:
        search_all_quartic(c, [], max_enum=5)
    assert err.value.space is space
    want = [c.convert_sol(s) for s in space if c.convert_sol(s) is not None]
    assert sorted(want) == [(0,), (1,), (2,), (4,), (8,), (16,), (32,)]
    assert search_all_quartic(c, [], max_enum=6) == want


# -- stream order -----------------------------------------------------------------------------------------------------------------------
def test_search_right_after_another_solve(cycles):      # noqa: F811
    """the search runs on the solver's pool stream: issued while the device is still busy with a spin and right after another solve,
    it returns what it returns alone"""
    c, zeros = _quartic_case(0x52F, 10)
    alone = search_all_quartic(c, zeros)
    torch.cuda._sleep(cycles)
    q = QuadraticSystem([N])
    other = search_all_xl4(q, lfsr_zeros(q, *LFSR, 52))
    got = search_all_quartic(c, zeros)
    assert got == alone and len(other) == XL4_OUTPUTS[52][2]
