"""Degree-3 XL on the MI355X: quadratic rows multiplied by 1 and by every unknown on the device (k_xl3_expand) and solved there.
The yardsticks are the set-based host expansion of tests.xl_terms and the CPU oracle on its rows; every comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuadBitVec, PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols
from oracle import gf2_oracle as O
from tests import xl_terms as X
from tests.harness_models import GaloisLFSR
from tests.quad_terms import expand_ints, random_terms
from tests.test_gpu_stream_order import _delayed_copy, _handle, cycles, stream      # noqa: F401  (fixtures)


@pytest.fixture(params=["default", "plain"])
def mode(request, monkeypatch):
    """every test as shipped and with GF2BV_PLAIN=1 (the solves underneath on their plain paths)"""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("mode")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _cubic_aug(eqs, n: int, rows: int, stride: int) -> np.ndarray:
    """the helper's XL rows of quadratic equation ints as augmented words, padded with zero rows"""
    ints = X.xl3_ints(eqs, n)
    return O.eqs_to_aug(ints + [0] * (rows - len(ints)), xl3_cols(n), stride)


def _factored(eqs, n: int):
    """quadratic equation ints as factored arrays: per equation its constant and linear part, and for every i with a pair (i, j) one
    product x_i * (sum of the x_j, j < i) -- the pairs (i, j) and nothing else"""
    wl = (n + 1 + 63) // 64
    form = lambda v: np.frombuffer(int(v).to_bytes(8 * wl, "little"), dtype=np.uint64)      # noqa: E731
    lin, off, ta, tb = [], [0], [], []
    for e in eqs:
        lin.append(form(e & ((1 << (n + 1)) - 1)))
        pairs = e >> (n + 1)
        for i in range(1, n):
            run = (pairs >> (i * (i - 1) // 2)) & ((1 << i) - 1)
            if run:
                ta.append(form(1 << (1 + i)))
                tb.append(form(run << 1))
        off.append(len(ta))
    arr = lambda rows: np.array(rows, dtype=np.uint64).reshape(-1, wl)                        # noqa: E731
    return arr(lin), np.array(off, dtype=np.int64), arr(ta), arr(tb)


def _packed_zeros(eqs, n: int) -> list:
    return [PackedQuadBitVec(*_factored(eqs, n), n)] if eqs else []


# -- 1. expansion parity -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_cases(n: int) -> tuple:
    """(quadratic rows, rows, stride, expected words) per shape: computed once, shared by both modes"""
    rng = random.Random(3000 + n)
    q = QuadraticSystem([n])
    wt = (xl3_cols(n) + 1 + 63) // 64
    cases = []
    for m, pad, stride in ((3, 0, wt + (wt & 1)), (2, 5, wt + 4), (1, 0, wt), (0, 2, wt)):
        if n >= 100:
            m = min(m, 2)                              # (keeps the host reference in seconds)
        eqs = expand_ints(q, *random_terms(rng, n, m, 4))
        rows = m * (n + 1) + pad
        cases.append((X.quad_aug(eqs, n, (q._cols + 1 + 63) // 64 + (m & 1)), rows, stride, _cubic_aug(eqs, n, rows, stride)))
    if n in (12, 65):                                  # every coefficient set: every run of every product row is populated
        eqs = [(1 << (q._cols + 1)) - 1] * 2
        cases.append((X.quad_aug(eqs, n), 2 * (n + 1), wt, _cubic_aug(eqs, n, 2 * (n + 1), wt)))
    return tuple(cases)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 11, 12, 31, 32, 33, 63, 64, 65, 100])
def test_expansion_equals_host_reference(n):
    for quad, rows, stride, want in _parity_cases(n):
        got = hip.xl3_expand_words(quad, n, rows=rows, stride_words=stride)
        assert got.shape == want.shape == (rows, stride)
        assert np.array_equal(got, want), (n, len(quad), rows, stride, np.argwhere(got != want)[:4])      # every word of the stride
    assert hip.xl3_expand_words(quad[:0], n).shape == (0, (xl3_cols(n) + 1 + 63) // 64)


def test_get_eqs_xl():
    n, rng = 7, random.Random(70)
    eqs = X.planted_dense(rng, n, 5, [rng.getrandbits(n)]) + [0, 1 << 3]
    want = [e for e in X.xl3_ints(eqs, n) if e]
    assert QuadraticSystem([n]).get_eqs_xl(eqs) == [e for e in X.xl3_ints([e for e in eqs if e], n) if e]
    assert PackedQuadraticSystem([n]).get_eqs_xl(_packed_zeros(eqs, n)) == want
    assert QuadraticSystem([n]).get_eqs_xl([]) == PackedQuadraticSystem([n]).get_eqs_xl([]) == []


# -- 2. solve parity against the CPU oracle on the helper's rows -----------------------------------------------------------------------------
SOLVE_CASES = [(6, 4), (7, 8), (8, 7), (8, 12), (9, 14), (10, 12), (10, 16), (11, 18), (12, 20), (12, 26), (13, 28), (14, 36)]


@functools.lru_cache(maxsize=None)
def _solve_case(n: int, m: int):
    rng = random.Random(100 * n + m)
    eqs = X.planted_dense(rng, n, m, [rng.getrandbits(n)])
    cols3 = xl3_cols(n)
    rows = max(m * (n + 1), cols3)
    aug = _cubic_aug(eqs, n, rows, O.words_for(cols3))
    return eqs, rows, {md: O.solve_words(aug, rows, cols3, md) for md in (0, 1)}


def _assert_solution(got, want, md):
    assert (got.status, got.rank) == (want["status"], want["rank"])
    assert np.array_equal(got.pivots, want["pivcols"])
    assert np.array_equal(got.origin, want["origin"])
    if md == 1:
        assert got.dimension == want["dim"] and np.array_equal(got.basis, want["basis"])          # the vectors and their order


def _check_against_oracle(n: int, m: int):
    eqs, rows, want = _solve_case(n, m)
    terms = _factored(eqs, n)
    for md in (0, 1):
        assert want[md]["status"] == 0
        _assert_solution(hip.solve_xl3_words(X.quad_aug(eqs, n), n, md), want[md], md)
        _assert_solution(hip.solve_xl3_quad_terms(*terms, n, md), want[md], md)
    origin = O.words_to_int(want[1]["origin"])
    basis = tuple(O.words_to_int(b) for b in want[1]["basis"])
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    sq, sp = q.solve_raw_space_xl(eqs), p.solve_raw_space_xl(_packed_zeros(eqs, n))
    assert (sq.dimension, sq.origin, sq.basis) == (sp.dimension, sp.origin, sp.basis) == (len(basis), origin, basis)
    assert q.solve_raw_one_xl(eqs) == p.solve_raw_one_xl(_packed_zeros(eqs, n)) == O.words_to_int(want[0]["origin"])
    return want[1]


@pytest.mark.parametrize("n,m", SOLVE_CASES)
def test_solves_equal_oracle(n, m):
    want = _check_against_oracle(n, m)
    if (n, m) == (10, 12):
        assert want["dim"] == 43 and m * (n + 1) < xl3_cols(n)                # underdetermined and padded on the device
    if (n, m) in ((12, 26), (14, 36)):
        assert want["dim"] == 0


def test_blocked_path_sees_a_small_cubic_system(monkeypatch):
    monkeypatch.setenv("GF2BV_SMALL", "0")
    n, m = 12, 20
    eqs = _solve_case(n, m)[0]
    assert hip.solve_xl3_words(X.quad_aug(eqs, n), n, 1).stats["small_path"] == 0
    assert _check_against_oracle(n, m)["dim"] == 38


# -- 3. several true solutions -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _multi_case(k: int):
    n, m = 12, 30
    rng = random.Random(12000 + k)
    points = rng.sample(range(1 << n), k)
    eqs = X.planted_dense(rng, n, m, points)
    rows = X.xl3_ints(eqs, n)
    space = O.m4ri_solve(rows + [0] * max(0, xl3_cols(n) - len(rows)), xl3_cols(n), 1)
    vectors = {X.point_vector(x, n): x for x in points}
    return eqs, points, space.dimension, [(vectors[raw],) for raw in space if raw in vectors]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_several_true_solutions(k):
    n = 12
    eqs, points, dim, want = _multi_case(k)
    assert dim == k - 1 and sorted(want) == sorted((x,) for x in points)      # the affine hull of the points' monomial vectors
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        assert qsys.solve_raw_space_xl(zeros).dimension == dim
        assert list(qsys.solve_all_xl(zeros)) == want
        assert qsys.solve_one_xl(zeros) == want[0]
    if k == 3:
        assert dim == 2 and len(want) == 3             # four points in the space, one of them no monomial vector: the filter's work


# -- 4. the blocked path: a planted dense system at n = 24 ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _n24_case():
    """m = 100 equations (the value used; plain linearisation needs 300): unique over the 2324 cubic columns by the oracle"""
    n, m = 24, 100
    rng = random.Random(2400)
    planted = rng.getrandbits(n)
    eqs = X.planted_dense(rng, n, m, [planted])
    rows = X.xl3_ints(eqs, n)
    assert len(rows) == 2500 and xl3_cols(n) == 2324
    res = O.solve_words(O.eqs_to_aug(rows, 2324), len(rows), 2324, 1)
    assert (res["status"], res["rank"]) == (0, 2324)
    return eqs, planted


def test_n24_planted_dense():
    n = 24
    eqs, planted = _n24_case()
    assert hip.solve_xl3_words(X.quad_aug(eqs, n), n, 1).stats["small_path"] == 0
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        with pytest.raises(DimensionTooLargeError) as err:
            list(qsys.solve_all(zeros))
        assert err.value.space.dimension == 300 - 100
        assert list(qsys.solve_all_xl(zeros)) == [(planted,)]
        assert qsys.solve_one_xl(zeros) == (planted,)


# -- 5. filtered LFSRs with too few outputs for plain linearisation ------------------------------------------------------------------------
def _filter(x0, x1, x2, x3, x4):
    return (x0 & x1) ^ (x0 & x1 & x3 & x4) ^ x0 ^ x1 ^ x2


def lfsr_zeros(qsys, n: int, taps: int, select, secret: int, outputs: int) -> list:
    """the annihilator equations of examples/nlfsr_recovery.py for the first `outputs` output bits of a Galois register"""
    reg, stream = GaloisLFSR(n, taps, secret), []
    for _ in range(outputs):
        reg()
        stream.append(_filter(*[(reg.state >> i) & 1 for i in select]))
    sym, zeros = GaloisLFSR(n, taps, qsys.gens()[0]), []
    for bit in stream:
        sym()
        if bit:                                        # g = x0 x1 + x0 + x1 x2 + x1 + x2 + 1 vanishes where the filter gives 1
            x0, x1, x2 = [sym.state[i] for i in select[:3]]
            zeros.append(qsys.mul_bit(x0, x1) ^ x0 ^ qsys.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    return zeros


LFSR16 = (16, 0xB400, (1, 4, 7, 10, 13), random.Random(16).getrandbits(16) | 1, 140)
LFSR32 = (32, 0x80200003, (3, 9, 15, 21, 27), random.Random(1).getrandbits(32) | 1, 360)


@pytest.mark.parametrize("case,cls,neq", [(LFSR16, PackedQuadraticSystem, 136), (LFSR16, QuadraticSystem, 136), (LFSR32, PackedQuadraticSystem, 528)],
                         ids=["n16-packed", "n16-int", "n32-packed"])
def test_filtered_lfsr(case, cls, neq):
    n, taps, select, secret, outputs = case
    qsys = cls([n])
    zeros = lfsr_zeros(qsys, n, taps, select, secret, outputs)
    assert len(zeros) < neq - 32                       # far fewer equations than plain linearisation needs ...
    with pytest.raises(DimensionTooLargeError):        # ... which therefore gives up
        list(qsys.solve_all(zeros))
    assert list(qsys.solve_all_xl(zeros)) == [(secret,)]
    assert qsys.solve_one_xl(zeros) == (secret,)


# -- 6. stream order -------------------------------------------------------------------------------------------------------------------------
def test_expand_device_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the quadratic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then the expansion and the solve are enqueued there with no synchronisation anywhere."""
    n, m = 16, 40                                      # 680 live rows, 696 columns: underdetermined, origins and bases to compare
    cols3 = xl3_cols(n)
    rows, stride = cols3 + 12, hip.padded_stride(cols3)
    new = X.quad_aug(X.planted_dense(random.Random(61), n, m, [0xBEEF]), n)
    old = X.quad_aug(X.planted_dense(random.Random(62), n, m, [0x1234]), n)
    want, stale = hip.solve_xl3_words(new, n, 1), hip.solve_xl3_words(old, n, 1)
    assert want.status == stale.status == 0 and 0 < want.rank < cols3
    key = lambda s: (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    assert key(want) != key(stale), "the two systems have the same answer"
    to_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()                                   # noqa: E731
    buf, src = to_dev(old), to_dev(new)
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _delayed_copy(stream, cycles, buf, src)
    hip.xl3_expand_device(buf.data_ptr(), m, new.shape[1], n, rows, d_aug.data_ptr(), stride, stream=_handle(stream))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols3, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (solve_xl3_words pads to max(680, 696) rows: zero rows change nothing)


# -- 7. inconsistency, and the empty system -------------------------------------------------------------------------------------------------
def test_one_equals_zero():
    n, rng = 6, random.Random(6)
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    eqs = X.planted_dense(rng, n, 5, [rng.getrandbits(n)])
    (x,) = p.gens()
    one = p.mul_bit(x[0], x[0]) ^ x[0] ^ 1             # x0 x0 = x0: expands to the constant 1 on the device
    for qsys, zeros in ((q, eqs + [1]), (q, [1]), (p, _packed_zeros(eqs, n) + [1]), (p, [1]), (p, _packed_zeros(eqs, n) + [one]), (p, [one])):
        assert qsys.solve_raw_one_xl(zeros) is None and qsys.solve_raw_space_xl(zeros) is None
        assert list(qsys.solve_all_xl(zeros)) == [] and qsys.solve_one_xl(zeros) is None
    for qsys in (q, p):                                # no equation: every point of the cubic space, the consistent ones filtered
        assert qsys.solve_raw_space_xl([]).dimension == xl3_cols(n)
        assert qsys.solve_raw_one_xl([]) == 0
        with pytest.raises(DimensionTooLargeError):
            list(qsys.solve_all_xl([]))
