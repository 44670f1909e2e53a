"""Degree-4 XL on the MI355X: quadratic rows multiplied by 1, by every unknown and by every pair of unknowns on the device
(k_xl4_expand) and solved there.  The yardsticks are the set-based host expansion of tests.xl4_terms and the CPU oracle on its rows;
every comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl4_cols, xl4_quad_col
from oracle import gf2_oracle as O
from tests import xl4_terms as X4
from tests import xl_terms as X
from tests.quad_terms import expand_ints, random_terms
from tests.test_gpu_stream_order import _delayed_copy, _handle, cycles, stream      # noqa: F401  (fixtures)
from tests.test_gpu_xl import LFSR16, _assert_solution, _factored, _packed_zeros, lfsr_zeros, mode      # noqa: F401  (mode: default / plain)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("mode")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


# -- 1. expansion parity -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_cases(n: int) -> tuple:
    """(quadratic rows, rows, stride, expected words) per shape: computed once, shared by both modes"""
    rng = random.Random(4000 + n)
    q = QuadraticSystem([n])
    wt, per = (xl4_cols(n) + 1 + 63) // 64, X4.rows_per_equation(n)
    cases = []
    for m, pad, stride in ((3, 0, wt + (wt & 1)), (2, 5, wt + 4), (1, 0, wt), (0, 2, wt)):
        eqs = expand_ints(q, *random_terms(rng, n, m, 4))
        rows = m * per + pad
        cases.append((X.quad_aug(eqs, n, (q._cols + 1 + 63) // 64 + (m & 1)), rows, stride, X4.xl4_aug(eqs, n, rows, stride)))
    if n in (12, 20):                                  # every coefficient set: every run of every product row is populated
        eqs = [(1 << (q._cols + 1)) - 1] * 2
        cases.append((X.quad_aug(eqs, n), 2 * per, wt, X4.xl4_aug(eqs, n, 2 * per, wt)))
    return tuple(cases)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 20, 33])
def test_expansion_equals_host_reference(n):
    for quad, rows, stride, want in _parity_cases(n):
        got = hip.xl4_expand_words(quad, n, rows=rows, stride_words=stride)
        assert got.shape == want.shape == (rows, stride)
        assert np.array_equal(got, want), (n, len(quad), rows, stride, np.argwhere(got != want)[:4])      # every word of the stride
    assert hip.xl4_expand_words(quad[:0], n).shape == (0, (xl4_cols(n) + 1 + 63) // 64)
    assert ((xl4_cols(n) + 1 + 63) // 64 == 1) == (n <= 6)      # one output word up to n = 6, two from n = 7


@functools.lru_cache(maxsize=None)
def _wide_case():
    """n = 67, one equation with a quarter of its coefficients set and q(64, 0..63) all set: the quadruple run (66, 65, 64, 0..63) of
    x_66 x_65 f is a window of 64 bits, longer than what is left of any output word.  (The columns come from
    tests.xl4_terms.column_of: the walked table of 816663 monomials is not built, which keeps the reference within seconds.)"""
    n, rng = 67, random.Random(67)
    cols2 = n + n * (n - 1) // 2
    eqs = [(rng.getrandbits(cols2 + 1) & rng.getrandbits(cols2 + 1)) | (((1 << 64) - 1) << (1 + n + 64 * 63 // 2))]
    per, wt = X4.rows_per_equation(n), (xl4_cols(n) + 1 + 63) // 64
    return X.quad_aug(eqs, n), per, wt + (wt & 1), X4.xl4_aug(eqs, n, per, wt + (wt & 1), table=False)


def test_expansion_with_runs_longer_than_a_word():
    n = 67
    quad, rows, stride, want = _wide_case()
    row = int.from_bytes(want[1 + n + 66 * 65 // 2 + 65].tobytes(), "little")      # x_66 x_65 f
    assert (row >> xl4_quad_col(n, 66, 65, 64, 0)) & ((1 << 64) - 1) == (1 << 64) - 1
    got = hip.xl4_expand_words(quad, n, rows=rows, stride_words=stride)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_get_eqs_xl4():
    n, rng = 7, random.Random(74)
    eqs = X.planted_dense(rng, n, 4, [rng.getrandbits(n)]) + [0, 1 << 3]
    want = [e for e in X4.xl4_ints(eqs, n) if e]
    assert QuadraticSystem([n]).get_eqs_xl4(eqs) == [e for e in X4.xl4_ints([e for e in eqs if e], n) if e]
    assert PackedQuadraticSystem([n]).get_eqs_xl4(_packed_zeros(eqs, n)) == want
    assert QuadraticSystem([n]).get_eqs_xl4([]) == PackedQuadraticSystem([n]).get_eqs_xl4([]) == []


# -- 2. solve parity against the CPU oracle on the helper's rows -----------------------------------------------------------------------------
SOLVE_CASES = {(7, 6): 0, (8, 7): 3, (9, 9): 1, (10, 11): 0, (12, 13): 0, (14, 16): 0, (16, 20): 0}      # (n, m): the oracle's dimension


@functools.lru_cache(maxsize=None)
def _solve_case(n: int, m: int):
    rng = random.Random(400 * n + m)
    eqs = X.planted_dense(rng, n, m, [rng.getrandbits(n)])
    aug, rows, cols4 = X4.quartic_aug(eqs, n)
    return eqs, {md: O.solve_words(aug, rows, cols4, md) for md in (0, 1)}


def _check_against_oracle(n: int, m: int):
    eqs, want = _solve_case(n, m)
    terms = _factored(eqs, n)
    stats = None
    for md in (0, 1):
        assert want[md]["status"] == 0
        got = hip.solve_xl4_words(X.quad_aug(eqs, n), n, md)
        stats = got.stats
        _assert_solution(got, want[md], md)
        _assert_solution(hip.solve_xl4_quad_terms(*terms, n, md), want[md], md)
    origin = O.words_to_int(want[1]["origin"])
    basis = tuple(O.words_to_int(b) for b in want[1]["basis"])
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    sq, sp = q.solve_raw_space_xl4(eqs), p.solve_raw_space_xl4(_packed_zeros(eqs, n))
    assert (sq.dimension, sq.origin, sq.basis) == (sp.dimension, sp.origin, sp.basis) == (len(basis), origin, basis)
    assert q.solve_raw_one_xl4(eqs) == p.solve_raw_one_xl4(_packed_zeros(eqs, n)) == O.words_to_int(want[0]["origin"])
    return want[1], stats


@pytest.mark.parametrize("n,m", list(SOLVE_CASES))
def test_solves_equal_oracle(n, m):
    want, stats = _check_against_oracle(n, m)
    assert want["dim"] == SOLVE_CASES[(n, m)]
    if (n, m) == (12, 13):
        assert want["rank"] == 793 and m * X4.rows_per_equation(n) == 1027          # 169 rows, rank 169 of 298 at degree 3
    if (n, m) == (7, 6):
        assert stats["small_path"] == 1
    if (n, m) == (16, 20):
        assert want["rank"] == 2516


def test_blocked_path_sees_a_small_quartic_system(monkeypatch):
    monkeypatch.setenv("GF2BV_SMALL", "0")
    n, m = 10, 11
    want, stats = _check_against_oracle(n, m)
    assert stats["small_path"] == 0 and want["dim"] == 0


# -- 3. several true solutions -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _multi_case(k: int):
    n, m = 10, 13
    rng = random.Random(10000 + k)
    points = rng.sample(range(1 << n), k)
    eqs = X.planted_dense(rng, n, m, points)
    rows = X4.xl4_ints(eqs, n)
    space = O.m4ri_solve(rows + [0] * max(0, xl4_cols(n) - len(rows)), xl4_cols(n), 1)
    vectors = {X4.point_vector(x, n): x for x in points}
    return eqs, points, space.dimension, [(vectors[raw],) for raw in space if raw in vectors]


@pytest.mark.parametrize("k", [2, 3])
def test_several_true_solutions(k):
    n = 10
    eqs, points, dim, want = _multi_case(k)
    assert dim == k - 1 and sorted(want) == sorted((x,) for x in points)      # the affine hull of the points' monomial vectors
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        assert qsys.solve_raw_space_xl4(zeros).dimension == dim
        assert list(qsys.solve_all_xl4(zeros)) == want
        assert qsys.solve_one_xl4(zeros) == want[0]
    if k == 3:
        assert len(want) == 3                          # four points in the space, one of them no monomial vector: the filter's work


# -- 4. the filtered register at 44 outputs: degree 3 needs 140 ----------------------------------------------------------------------------
# the consistent points of the quartic space (dimension 9) in AffineSpace order, from the CPU oracle on tests.xl4_terms' rows
LFSR16_AT_44 = [11000, 23693, 26371, 49696, 50915, 15714, 13289, 28533, 53156, 64669]


@pytest.mark.parametrize("cls", [PackedQuadraticSystem, QuadraticSystem], ids=["packed", "int"])
def test_filtered_lfsr_at_44_outputs(cls):
    n, taps, select, secret, _ = LFSR16
    qsys = cls([n])
    zeros = lfsr_zeros(qsys, n, taps, select, secret, 44)
    assert len(zeros) == 29
    with pytest.raises(DimensionTooLargeError) as err:
        list(qsys.solve_all_xl(zeros))
    assert err.value.space.dimension == 261
    space = qsys.solve_raw_space_xl4(zeros)
    assert space.dimension == 9
    got = list(qsys.solve_all_xl4(zeros))
    assert (secret,) in got and got == [(x,) for x in LFSR16_AT_44]
    assert qsys.solve_one_xl4(zeros) == (LFSR16_AT_44[0],)


# -- 5. stream order -------------------------------------------------------------------------------------------------------------------------
def test_expand_device_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the quadratic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then the expansion and the solve are enqueued there with no synchronisation anywhere."""
    n, m = 12, 8                                       # 632 live rows of rank 596, 793 columns: underdetermined, origins and bases to compare
    cols4 = xl4_cols(n)
    rows, stride = cols4 + 12, hip.padded_stride(cols4)
    new = X.quad_aug(X.planted_dense(random.Random(81), n, m, [0xBEE]), n)
    old = X.quad_aug(X.planted_dense(random.Random(82), n, m, [0x123]), n)
    want, stale = hip.solve_xl4_words(new, n, 1), hip.solve_xl4_words(old, n, 1)
    assert want.status == stale.status == 0 and want.rank == 632 - 8 - 28
    key = lambda s: (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    assert key(want) != key(stale), "the two systems have the same answer"
    to_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()                                   # noqa: E731
    buf, src = to_dev(old), to_dev(new)
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _delayed_copy(stream, cycles, buf, src)
    hip.xl4_expand_device(buf.data_ptr(), m, new.shape[1], n, rows, d_aug.data_ptr(), stride, stream=_handle(stream))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols4, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (solve_xl4_words pads to max(632, 793) rows: zero rows change nothing)


# -- 6. inconsistency, and the empty system -------------------------------------------------------------------------------------------------
def test_one_equals_zero():
    n, rng = 6, random.Random(6)
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    eqs = X.planted_dense(rng, n, 5, [rng.getrandbits(n)])
    (x,) = p.gens()
    one = p.mul_bit(x[0], x[0]) ^ x[0] ^ 1             # x0 x0 = x0: expands to the constant 1 on the device
    for qsys, zeros in ((q, eqs + [1]), (q, [1]), (p, _packed_zeros(eqs, n) + [1]), (p, [1]), (p, _packed_zeros(eqs, n) + [one]), (p, [one])):
        assert qsys.solve_raw_one_xl4(zeros) is None and qsys.solve_raw_space_xl4(zeros) is None
        assert list(qsys.solve_all_xl4(zeros)) == [] and qsys.solve_one_xl4(zeros) is None
    assert hip.solve_xl4_words(X.quad_aug(eqs + [1], n), n, 1).status == hip.STATUS_INCONSISTENT
    for qsys in (q, p):                                # no equation: every point of the quartic space, the consistent ones filtered
        assert qsys.solve_raw_space_xl4([]).dimension == xl4_cols(n)
        assert qsys.solve_raw_one_xl4([]) == 0
        with pytest.raises(DimensionTooLargeError):
            list(qsys.solve_all_xl4([]))
