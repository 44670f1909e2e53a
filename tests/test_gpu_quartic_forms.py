"""The kernels under search_all_xl4 / search_all_quartic -- k_forms_products<4> (with k_forms_sum), k_quartic_search,
k_forms_check<4> -- on the MI355X against the host reference of tests/quartic_forms.py (set-of-monomials products and numpy;
tests/test_quartic_search_cpu.py checks it where no GPU exists).

Every search case calls hip.quartic_forms_search and compares (count, zeros) exactly with a zero set that is known by construction
(forms written where their zeros are obvious, then carried through a random invertible affine map, so that they are dense in every
unknown and every degree, the lanes' high unknowns included) or with a numpy walk.  The launch shapes of the quartic search:
L = min(R, 12) low unknowns walked in Gray order, H = R - L high ones fixed per lane, one wavefront per workgroup -- so every R is
its own shape: H = 0 with a single live lane up to R = 12, a partial workgroup up to R = 17, whole workgroups from R = 18; from
R = 16 on four high unknowns and more enter the start values with their quartic terms, from R = 19 on bits of the lane index above
the wavefront."""
import functools
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from tests import cubic_forms as CF
from tests import quartic_forms as QF
from tests.test_gpu_quad_forms import _pad_to

pytestmark = pytest.mark.gpu

WALK = 12                                # kQuarticWalk of gf2_solver.hip
MAX_CAND = MAX_POINTS = 1 << 22          # kQuadMaxCand, kQuadMaxPoints of gf2_solver.hip (the quartic search shares them)
R_MAX = 32                               # the largest R of the per-R cases (every R up to WALK + 14 = 26 is a shape of its own).  Measured
#                                          with 64 dense forms: 1.28e10 points/s, 335 ms at R = 32 (profiles/quartic_search_time.txt; the
#                                          case itself takes 0.33 s).  At that rate R = 34 would take 1.3 s and R = 35 2.7 s


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _search(forms, R, **kw):
    """(count, zeros, first-pass candidates) of one hip.quartic_forms_search call"""
    before = hip.quartic_last_times()["candidates"]
    count, got = hip.quartic_forms_search(forms, R, **kw)
    return count, got, int(hip.quartic_last_times()["candidates"] - before)


# -- a. every launch shape ----------------------------------------------------------------------------------------------------------
# R: (p, s, m, order).  C(p,4) quadruples, three mixed products and R - p - s linear forms from known_zero_case, padded to m where m
# is given; (1 + p + C(p,2) + C(p,3)) 2^s zeros.  Below R = 5 the cases have what one form, or none, leaves.
PADDED = {13: 63, 14: 64, 15: 65, 20: 140, 29: 65}


def _shape(R: int) -> tuple:
    if R < 5:
        return {0: (0, 0), 1: (0, 0), 2: (1, 0), 3: (2, 0), 4: (4, 0)}[R] + (None, "natural")
    p = min(R, 5 + R % 3)
    return p, min(R - p, (R // 3) % 3), PADDED.get(R), "natural" if R % 2 else "shuffled"


@functools.lru_cache(maxsize=None)
def _lane_case(R: int) -> tuple:
    p, s, m, order = _shape(R)
    rng = random.Random(6000 + R)
    forms, want = QF.known_zero_case(rng, R, p, s, order)
    if m is not None:
        forms = _pad_to(rng, forms, m)
    return tuple(forms), want


def test_lane_cases_cover_the_form_counts():
    """m = 1, 63, 64, 65 and 140 (k_forms_check<4>: forms over the 64 lanes of a wave), forms in natural and in shuffled order"""
    ms = {R: len(_lane_case(R)[0]) for R in range(R_MAX + 1)}
    assert {1, 63, 64, 65, 140} <= set(ms.values()), ms
    assert [len(_lane_case(R)[1]) for R in (0, 1, 2, 3, 4)] == [1, 1, 2, 4, 15]
    assert all(26 <= len(_lane_case(R)[1]) <= 256 for R in range(5, R_MAX + 1))


@pytest.mark.parametrize("R", range(R_MAX + 1))
def test_lane_split_known_zero_set(R):
    forms, want = _lane_case(R)
    count, got, _ = _search(list(forms), R)
    assert (count, got) == (len(want), want)


@pytest.mark.parametrize("R", sorted({7, WALK - 1, WALK, WALK + 1, WALK + 2, WALK + 5, WALK + 6, WALK + 7}))
def test_lane_split_dense_planted(R):
    """uniformly random quartic forms, R - 5 of them, through three planted points, against the numpy walk"""
    assert R <= 20
    rng = random.Random(6100 + R)
    forms = QF.planted_dense(rng, R, R - 5, [rng.getrandbits(R) for _ in range(3)])
    want = QF.brute_zeros(forms, R)
    assert len(want) >= 3
    count, got, _ = _search(forms, R)
    assert (count, got) == (len(want), want)


# -- c. no unknowns, degenerate forms -----------------------------------------------------------------------------------------------
def test_degenerate_forms():
    assert hip.quartic_forms_search([], 0) == (1, [0])
    assert hip.quartic_forms_search([0], 0) == (1, [0])
    assert hip.quartic_forms_search([1], 0) == (0, [])
    assert hip.quartic_forms_search([0, 0], 3) == (8, list(range(8)))     # no form is chosen: every point is a candidate
    assert hip.quartic_forms_search([1], 7) == (0, [])
    R = 15
    dm = QF.DenseMap(random.Random(6200), R)
    affine = [dm.y(k) for k in range(4, R)]                                # purely affine: the subspace y_4 = .. = y_14 = 0
    assert hip.quartic_forms_search(affine, R) == (16, dm.zeros(range(16)))
    quad = 1 << (QF.width(R) - 1)                                          # the single quadruple z_14 z_13 z_12 z_11
    want = [z for z in range(1 << R) if (z >> 11) != 15]
    assert hip.quartic_forms_search([quad], R) == (len(want), want)


@pytest.mark.parametrize("R", [9, WALK, 16, 21])
def test_purely_cubic_and_purely_quadratic_forms(R):
    """no quadruple anywhere (every d3 update is zero): the cubic reference's known zero set, its forms as they stand (the quartic
    layout continues the cubic one); no triple either: the quadratic reference's"""
    from tests import quad_forms as Q2
    forms, want = CF.known_zero_case(random.Random(6300 + R), R, 6, 2, "shuffled")
    assert all(f >> CF.width(R) == 0 for f in forms) and any(f >> Q2.width(R) for f in forms)
    assert hip.quartic_forms_search(forms, R) == (len(want), want)
    forms, want = Q2.known_zero_case(random.Random(6350 + R), R, 6, 2, "shuffled")
    assert all(f >> Q2.width(R) == 0 for f in forms)
    assert hip.quartic_forms_search(forms, R) == (len(want), want)


def test_seventy_copies_of_one_form_first():
    forms, want = _lane_case(14)
    count, got, _ = _search([forms[0]] * 70 + list(forms), 14)
    assert (count, got) == (len(want), want)


# -- d. the candidate cap from both sides -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,fused", [(8, False), (7, True)], ids=["at_the_cap_two_pass", "above_the_cap_fused"])
def test_candidate_cap(nz, fused):
    """R = 30.  In y the first 64 forms are y_k for k in Z = {22 .. 22 + nz - 1}, then four-fold products y_k y_l y_1 y_0 (k in Z, l in
    2 .. 21): 64 independent forms whose common zeros are the subspace y_Z = 0.  |Z| = 8: exactly 2^22 first-pass candidates, which
    the list still holds (k_forms_check<4>); |Z| = 7: 2^23, twice what it holds (the fused pass).  The forms behind them leave the 64
    points of weight <= 3 on y_0 .. y_6 with y_7 .. y_21 = 0 in both cases."""
    R = 30
    rng = random.Random(6400 + nz)
    dm = QF.DenseMap(rng, R)
    Z = list(range(22, 22 + nz))
    first = [dm.y(k) for k in Z] + [dm.prod(k, l, 1, 0) for k in Z for l in range(2, 22)][:64 - nz]
    later = [dm.prod(i, j, k, l) for l in range(3, 7) for k in range(2, l) for j in range(1, k) for i in range(j)]
    later += [dm.y(k) for k in range(7, 22)] + [dm.y(k) for k in range(22 + nz, R)]
    assert len(first) == 64
    want = dm.zeros(QF.weight_le3(7))
    count, got, candidates = _search(first + later, R)
    assert candidates == 1 << (R - nz)
    assert (candidates > MAX_CAND) == fused
    assert len(want) == 64 and (count, got) == (64, want)


# -- e. the point cap ---------------------------------------------------------------------------------------------------------------
def _linear_case(R: int) -> tuple:
    """one non-constant affine form in R unknowns and its 2^(R-1) zeros, ascending (numpy)"""
    f = QF.DenseMap(random.Random(6500 + R), R).y(0)
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
    assert hip.quartic_forms_search([f], 24, max_out=0) == (2 * MAX_POINTS, [])
    with pytest.raises(hip.HipError, match=r"^gf2bv_hip error 4: more common zeros than can be collected$"):
        hip.quartic_forms_search([f], 24, max_out=16)


# -- k_forms_products<4> / k_forms_sum against their host twin ---------------------------------------------------------------------
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


def _space(rng, n: int, r: int, k: int, kbits: int) -> tuple:
    """(origin, basis) over the degree-4 columns of n unknowns: r vectors with linear part e_a plus random bits on the unknowns >= r
    and a few product bits (projection rank r), k vectors with `kbits` random product bits only (kbits large: every form's support
    is long), shuffled; a random origin"""
    S = hip.quartic_cols(n) - n
    high = ((1 << n) - 1) >> r << r
    sparse = lambda bits: sum(1 << (n + rng.randrange(S)) for _ in range(bits))      # noqa: E731
    while True:
        basis = [(1 << a) | (rng.getrandbits(n) & high) | sparse(6) for a in range(r)]
        basis += [sparse(kbits) if kbits < S else rng.getrandbits(S) << n for _ in range(k)]
        if _rank(basis) == r + k:
            break
    rng.shuffle(basis)
    return rng.getrandbits(n + S), basis


# (n, r, k, kbits).  With e2 = 1 + r + C(r,2), e3 = e2 + C(r,3), e4 = e3 + C(r,4) the first bit behind the pair, the triple and the
# quadruple block of a form over r unknowns: r = 7 has e3 = 64 and r = 15 e3 = 576 (the quadruple block starts a word), r = 9 has
# e4 = 256 (the form ends with a word); no r <= 20 puts e2 on a word boundary -- r = 19 comes next to it (e2 = 191, the triple
# block starts at the last bit of a word).  At r = 10, 11, 16 every boundary lies inside a word (e2 = 56, 67, 137).  Supports of size 1
# (k = 0) and above 64 (dense K rows, k = 70 and 90); n > r in most
PLAN_CASES = [(5, 0, 4, 3), (9, 0, 0, 0), (9, 7, 3, 40), (12, 9, 0, 0), (12, 10, 3, 40), (13, 11, 90, 1 << 30), (16, 16, 0, 0),
              (20, 15, 70, 1 << 30), (20, 19, 3, 30)]


@pytest.mark.parametrize("n,r,k,kbits", PLAN_CASES, ids=lambda v: str(v))
def test_forms_kernels_equal_host_twin(n, r, k, kbits):
    """hip.quartic_plan with a device (k_forms_products<4>: Moebius sums per monomial; k_forms_sum: XOR over the supports) == without
    (the host twin: monomial-by-monomial products), the whole dict.  What pins the twin itself is the brute force of
    tests/test_quartic_search_cpu.py at n <= 8."""
    rng = random.Random(6600 + 7 * n + r + k)
    origin, basis = _space(rng, n, r, k, kbits)
    host = hip.quartic_plan(origin, basis, n)
    assert host["r"] == r
    assert hip.quartic_plan(origin, basis, n, device=0) == host
