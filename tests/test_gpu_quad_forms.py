"""The three kernels under search_all / search_one -- k_quad_forms, k_quad_search, k_forms_check<2> -- on the MI355X against the
host reference of tests/quad_forms.py (plain ints and numpy; tests/test_quad_forms_cpu.py checks it where no GPU exists).

Every search case calls hip.quad_forms_search and compares (count, zeros) exactly with a zero set that is known by construction
(forms written where their zeros are obvious, then carried through a random invertible affine map, so that they are dense in
every unknown, the lanes' high ones included) or with a numpy walk.  The sizes sit on the launch shapes of quad_search_device:
H = max(0, min(R - 10, 18)) high unknowns fixed per lane, L = R - H low ones walked in Gray order."""
import functools
import random
import time

import numpy as np
import pytest

from gf2bv_amd import hip
from tests import quad_forms as QF

pytestmark = pytest.mark.gpu

MAX_CAND = MAX_POINTS = 1 << 22          # kQuadMaxCand, kQuadMaxPoints of gf2_solver.hip


def _search(forms, R, **kw):
    """(count, zeros, first-pass candidates) of one hip.quad_forms_search call"""
    before = hip.quad_last_times()["candidates"]
    count, got = hip.quad_forms_search(forms, R, **kw)
    return count, got, int(hip.quad_last_times()["candidates"] - before)


def _pad_to(rng, forms, m: int) -> list:
    """the forms and XORs of two of them, m in all: every second XOR right behind two of the first eight forms (where the choice
    of the first 64 independent forms has to skip it), the others at the end.  The common zeros stay what they are."""
    forms = list(forms)
    while len(forms) < m:
        if (m - len(forms)) % 2:
            a, b = rng.sample(range(min(8, len(forms))), 2)
            forms.insert(max(a, b) + 1, forms[a] ^ forms[b])
        else:
            a, b = rng.sample(range(len(forms)), 2)
            forms.append(forms[a] ^ forms[b])
    return forms


# -- a. lane splits -----------------------------------------------------------------------------------------------------------------
# R: (p, s, m).  p (p - 1) / 2 + R - p - s forms from known_zero_case, padded to m where m is given; (p + 1) 2^s zeros.
# H / L / launch: R = 1, 2, 3, 10: H = 0, one live lane; 11: H = 1; 12: H = 2; 16: one wave exactly; 17: 128 lanes; 18: one block
# of 256; 19: two blocks; 27: H = 17; 28: H = 18, L = 10; 29, 30, 33, 36: L = 11, 12, 15, 18 (steps i >= 1024: d1s[k bd + tid], k >= 10).
# Below R = 4 no form leaves 8 zeros: those three cases have the most that one form leaves.
LANE_CASES = {
    1: (0, 0, None), 2: (2, 0, None), 3: (2, 1, None),
    10: (6, 2, None), 11: (6, 2, None), 12: (7, 3, None), 16: (12, 2, None),
    17: (11, 3, 63), 18: (11, 4, 64), 19: (11, 4, 65),
    27: (16, 3, 140), 28: (14, 4, None), 29: (15, 3, None), 30: (13, 4, None), 33: (20, 2, None), 36: (12, 4, None),
}


@functools.lru_cache(maxsize=None)
def _lane_case(R: int) -> tuple:
    p, s, m = LANE_CASES[R]
    rng = random.Random(4000 + R)
    forms, want = QF.known_zero_case(rng, R, p, s, "shuffled")
    if m is not None:
        forms = _pad_to(rng, forms, m)
    return tuple(forms), want


def test_lane_cases_cover_the_form_counts():
    """m = 1, 63, 64, 65 and one value above 128 (k_forms_check<2>: forms over the 64 lanes of a wave), zero sets of 8 .. a few hundred"""
    ms = {R: len(_lane_case(R)[0]) for R in LANE_CASES}
    assert {1, 63, 64, 65} <= set(ms.values()) and max(ms.values()) > 128, ms
    assert all(8 <= len(_lane_case(R)[1]) <= 400 for R in LANE_CASES if R > 3)
    assert [len(_lane_case(R)[1]) for R in (1, 2, 3)] == [1, 3, 6]


@pytest.mark.parametrize("R", sorted(LANE_CASES))
def test_lane_split_known_zero_set(R):
    forms, want = _lane_case(R)
    count, got, _ = _search(list(forms), R)
    assert (count, got) == (len(want), want)


@pytest.mark.parametrize("R", [R for R in sorted(LANE_CASES) if 7 <= R <= 22])
def test_lane_split_dense_planted(R):
    """uniformly random forms, R - 6 of them, through three planted points, against the numpy walk"""
    rng = random.Random(4100 + R)
    forms = QF.planted_dense(rng, R, R - 6, [rng.getrandbits(R) for _ in range(3)])
    want = QF.brute_zeros(forms, R)
    assert len(want) >= 3
    count, got, _ = _search(forms, R)
    assert (count, got) == (len(want), want)


# -- b. the largest search the API takes --------------------------------------------------------------------------------------------
def test_forty_unknowns(capsys):
    """R = 40: H = 18, L = 22, 45 KiB of LDS per block, 2^40 points; 82 forms, 48 zeros"""
    rng = random.Random(4040)
    forms, want = QF.known_zero_case(rng, 40, 11, 2, "shuffled")
    assert len(forms) == 82 and len(want) == 48
    t0 = time.perf_counter()
    count, got, _ = _search(forms, 40)
    with capsys.disabled():
        print(f"\n[quad_forms] R = 40: {time.perf_counter() - t0:.3f} s", flush=True)
    assert (count, got) == (len(want), want)


# -- c. no unknowns, degenerate forms -----------------------------------------------------------------------------------------------
def test_degenerate_forms():
    assert hip.quad_forms_search([], 0) == (1, [0])
    assert hip.quad_forms_search([0], 0) == (1, [0])
    assert hip.quad_forms_search([1], 0) == (0, [])
    assert hip.quad_forms_search([0, 0], 3) == (8, list(range(8)))       # no form is chosen: every point is a candidate
    assert hip.quad_forms_search([1], 7) == (0, [])


def test_seventy_copies_of_one_form_first():
    """the choice of the first 64 independent forms has to walk past 69 repeats"""
    forms, want = _lane_case(12)
    count, got, _ = _search([forms[0]] * 70 + list(forms), 12)
    assert (count, got) == (len(want), want)


# -- d. the candidate cap from both sides -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,fused", [(8, False), (7, True)], ids=["at_the_cap_two_pass", "above_the_cap_fused"])
def test_candidate_cap(nz, fused):
    """R = 30.  In y the first 64 forms are y_k for k in Z = {22 .. 22 + nz - 1}, then products y_k y_l (k in Z, l < 22): 64
    independent forms whose common zeros are the subspace y_Z = 0.  |Z| = 8: exactly 2^22 first-pass candidates, which the list
    still holds (k_forms_check<2> strides them over 8192 waves); |Z| = 7: 2^23, twice what it holds (the fused pass).  The forms behind them leave the 23 points of weight <= 1 on y_0 .. y_21 in both cases."""
    R = 30
    rng = random.Random(4300 + nz)
    dm = QF.DenseMap(rng, R)
    Z = list(range(22, 22 + nz))
    first = [dm.y(k) for k in Z] + [dm.prod(k, l) for k in Z for l in range(22)][:64 - nz]
    later = [dm.prod(i, j) for i in range(1, 22) for j in range(i)] + [dm.y(k) for k in range(22 + nz, R)]
    assert len(first) == 64 and len(later) == 231 + (8 - nz)
    want = dm.zeros(QF.weight_le1(22))
    count, got, candidates = _search(first + later, R)
    assert candidates == 1 << (R - nz)
    assert (candidates > MAX_CAND) == fused
    assert len(want) == 23 and (count, got) == (23, want)


# -- e. the fused pass with coefficients on every unknown ---------------------------------------------------------------------------
def test_fused_pass_dense_32():
    """test_forms_search_too_many_candidates_32 of test_gpu_quad_search.py under a dense map: the products y_i y_j, i < j < 12,
    come first, so about 13 x 2^20 points pass the first 64 forms, and the linear forms y_14 .. y_31 behind them leave 13 x 4"""
    forms, want = QF.known_zero_case(random.Random(4032), 32, 12, 2, "natural")
    count, got, candidates = _search(forms, 32)
    assert candidates > MAX_CAND
    assert len(want) == 52 and (count, got) == (52, want)


# -- f. the point cap ---------------------------------------------------------------------------------------------------------------
def _linear_case(R: int) -> tuple:
    """one non-constant affine form in R unknowns and its 2^(R-1) zeros, ascending (numpy)"""
    f = QF.DenseMap(random.Random(4500 + R), R).y(0)
    assert f >> 1 and f >> (R + 1) == 0
    z = np.arange(1 << R, dtype=np.uint64)
    return f, z[(np.bitwise_count(z & np.uint64(f >> 1)) & 1) == (f & 1)]


def test_point_cap_reached():
    """2^22 zeros: as many as are collected, and all of them come back"""
    f, want = _linear_case(23)
    count, got, candidates = _search([f], 23)
    assert count == len(want) == MAX_POINTS and candidates == MAX_POINTS
    assert np.array_equal(np.array(got, dtype=np.uint64), want)


def test_point_cap_exceeded():
    """2^23 zeros: counted, not collected"""
    f, want = _linear_case(24)
    assert len(want) == 2 * MAX_POINTS
    assert hip.quad_forms_search([f], 24, max_out=0) == (2 * MAX_POINTS, [])
    with pytest.raises(hip.HipError, match=r"^gf2bv_hip error 4: more common zeros than can be collected$"):
        hip.quad_forms_search([f], 24, max_out=16)


# -- k_quad_forms against its host twin ---------------------------------------------------------------------------------------------
def _rank(vecs) -> int:
    piv = {}
    for v in vecs:
        while v:
            h = v.bit_length() - 1
            if h not in piv:
                piv[h] = v
                break
            v ^= piv[h]
    return len(piv)


def _consistent(n: int, x: int) -> int:
    pt = x
    for i in range(1, n):
        for j in range(i):
            if (x >> i) & 1 and (x >> j) & 1:
                pt |= 1 << (n + i * (i - 1) // 2 + j)
    return pt


def _space(rng, n: int, r: int, k: int, consistent: bool) -> tuple:
    """(origin, basis) over n linear and n (n - 1) / 2 product coordinates: r vectors with linear part e_a plus random bits on the
    unknowns >= r and a random product part (projection rank r), k vectors with a random product part only (many bits in every
    K row: supports longer than one), shuffled"""
    S = n * (n - 1) // 2
    high = ((1 << n) - 1) >> r << r
    while True:
        basis = [(1 << a) | (rng.getrandbits(n) & high) | (rng.getrandbits(S) << n) for a in range(r)]
        basis += [rng.getrandbits(S) << n for _ in range(k)]
        if _rank(basis) == r + k:
            break
    rng.shuffle(basis)
    origin = _consistent(n, rng.getrandbits(n)) if consistent else rng.getrandbits(n + S)
    return origin, basis


# (n, r, k): r + 1 bits of an affine form go from one word to two at r = 63 / 64 / 65 and from two to three at 127 / 128 / 129
PLAN_CASES = [(5, 0, 4), (12, 8, 3), (66, 63, 5), (66, 64, 5), (67, 65, 40), (130, 127, 6), (130, 128, 6), (131, 129, 6), (9, 0, 0)]


@pytest.mark.parametrize("consistent", [True, False], ids=["consistent_origin", "arbitrary_origin"])
@pytest.mark.parametrize("n,r,k", PLAN_CASES, ids=lambda v: str(v))
def test_forms_kernel_equals_host_twin(n, r, k, consistent):
    """hip.quad_plan with a device (k_quad_forms: the product matrix in LDS, folded by bit gathers) == without (quad_forms_host:
    a loop over cells), the whole dict.  The twin is a reference only in that the two are written differently; what pins the
    twin itself is the brute force of tests/test_quad_search_cpu.py at n <= 12."""
    rng = random.Random(4600 + 7 * n + r + (100 if consistent else 0))
    origin, basis = _space(rng, n, r, k, consistent)
    host = hip.quad_plan(origin, basis, n)
    assert host["r"] == r
    if r >= 63:
        assert host["r_eff"] == r and len(host["forms"]) > 1000      # (nothing affine to eliminate: the kernel's forms are the plan's)
    assert hip.quad_plan(origin, basis, n, device=0) == host
