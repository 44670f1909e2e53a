"""Hybrid XL at degree 4 on the MI355X: the specialised rows of every assignment multiplied in one launch (k_xl4_expand_batch) and all
systems solved as lock-step gangs.  The yardsticks are the set-based substitution of tests.xl_guess_terms, the set-based expansion of
tests.xl4_terms and the CPU oracle on their rows; every comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl4_cols
from oracle import gf2_oracle as O
from tests import xl4_terms as X4
from tests import xl_guess_terms as G
from tests import xl_terms as X
from tests.test_gpu_stream_order import _delayed_copy, _handle, cycles, stream      # noqa: F401  (fixtures)
from tests.test_gpu_xl import _assert_solution, _factored, _packed_zeros, mode       # noqa: F401  (mode: the default / plain fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("mode")]

SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _w2(n: int) -> int:
    return (n + n * (n - 1) // 2 + 1 + 63) // 64


def _to_dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


# -- 1. batch expansion parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 2, 5])
def test_batch_expansion_equals_single_expansions(nsys):
    for n, m, pad in ((9, 4, 3), (12, 3, 0), (20, 2, 5)):
        rng = random.Random(100 * nsys + n)
        cols2, per = n + n * (n - 1) // 2, X4.rows_per_equation(n)
        quads = np.stack([X.quad_aug([rng.getrandbits(cols2 + 1) for _ in range(m)], n, _w2(n) + 1) for _ in range(nsys)])
        rows = m * per + pad
        stride = (xl4_cols(n) + 1 + 63) // 64 + (nsys & 1)
        sys_stride = rows * stride + 7
        got = hip.xl4_expand_batch_words(quads, n, rows=rows, stride_words=stride, sys_stride_words=sys_stride)
        assert got.shape == (nsys, sys_stride)
        for s in range(nsys):
            want = hip.xl4_expand_words(quads[s], n, rows=rows, stride_words=stride)
            assert np.array_equal(got[s, :rows * stride].reshape(rows, stride), want), (nsys, n, s)
            assert not got[s, rows * stride:].any()    # (the binding's zeros: the entry writes nothing between the systems)
        tight = hip.xl4_expand_batch_words(quads, n)
        assert np.array_equal(tight.reshape(nsys, m * per, -1), np.stack([hip.xl4_expand_words(q, n) for q in quads]))
    assert hip.xl4_expand_batch_words(np.zeros((0, 2, 1), dtype=np.uint64), 9).shape == (0, 2 * 46 * 4)


def test_batch_expansion_device_reads_each_systems_rows():
    """the device entry with the systems' quadratic rows and their expansions both further apart than they need to be"""
    n, m, nsys, rng = 12, 3, 3, random.Random(12)
    cols2, cols4 = n + n * (n - 1) // 2, xl4_cols(n)
    quads = np.stack([X.quad_aug([rng.getrandbits(cols2 + 1) for _ in range(m)], n, 3) for _ in range(nsys)])
    rows, stride = m * X4.rows_per_equation(n) + 2, (cols4 + 1 + 63) // 64 + 1            # 14 words
    qsys, sys_stride = m * 3 + 5, rows * stride + 4
    src = np.full((nsys, qsys), SENTINEL, dtype=np.uint64)
    src[:, :m * 3] = quads.reshape(nsys, -1)
    d_quad = _to_dev(src)
    out = torch.full((nsys * sys_stride,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.xl4_expand_batch_device(d_quad.data_ptr(), nsys, qsys, m, 3, n, rows, out.data_ptr(), stride, sys_stride)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64).reshape(nsys, sys_stride)
    for s in range(nsys):
        assert np.array_equal(got[s, :rows * stride].reshape(rows, stride), X4.xl4_aug(X4_ints(quads[s], n), n, rows, stride))
    assert (got[:, rows * stride:] == SENTINEL).all()


def X4_ints(quad: np.ndarray, n: int) -> list:
    """augmented quadratic words back to equation ints (bit 0 the constant)"""
    cols2 = n + n * (n - 1) // 2
    out = []
    for row in quad:
        v = int.from_bytes(row.tobytes(), "little")
        out.append(((v & ((1 << cols2) - 1)) << 1) | ((v >> cols2) & 1))
    return out


# -- 2. the two hybrid systems against the oracle per assignment -------------------------------------------------------------------------
# (n, m, guess): the consistent assignments, each of dimension 0; degree-3 hybrid leaves dimension 116 / 103 under every assignment
HYBRID = {(14, 14, (12, 13)): [0], (16, 15, (12, 13, 14, 15)): [0, 8, 10, 14]}


@functools.lru_cache(maxsize=None)
def _hybrid_case(n: int, m: int, guess: tuple) -> tuple:
    rng = random.Random(4400 * n + m)
    planted = rng.getrandbits(n)
    eqs = X.planted_dense(rng, n, m, [planted])
    ns, want = n - len(guess), []
    for a in range(1 << len(guess)):
        aug, rows, cols4 = X4.quartic_aug(G.specialise_ints(eqs, n, guess, a), ns)
        want.append({md: O.solve_words(aug, rows, cols4, md) for md in (0, 1)})
    return eqs, planted, want


def _points(n: int, guess: tuple, want: list) -> list:
    """the oracle's consistent points in assignment order"""
    ns = n - len(guess)
    out = []
    for a, w in enumerate(want):
        if w[1]["status"] == 0:
            assert w[1]["dim"] == 0
            raw = O.words_to_int(w[1]["origin"])
            y = raw & ((1 << ns) - 1)
            if X4.point_vector(y, ns) == raw:
                out.append((G.scatter(y, n, guess, a),))
    return out


@pytest.mark.parametrize("n,m,guess", list(HYBRID))
def test_hybrid_solves_equal_oracle(n, m, guess):
    eqs, planted, want = _hybrid_case(n, m, guess)
    total = 1 << len(guess)
    assert [a for a in range(total) if want[a][1]["status"] == 0] == HYBRID[(n, m, guess)]
    assert all(want[a][1]["dim"] == 0 for a in HYBRID[(n, m, guess)])
    quad, terms = X.quad_aug(eqs, n), _factored(eqs, n)
    for md in (0, 1):
        for got in (hip.solve_xl4_guess_words(quad, n, guess, mode=md), hip.solve_xl4_guess_quad_terms(*terms, n, guess, mode=md)):
            assert len(got) == total
            for a in range(total):
                _assert_solution(got[a], want[a][md], md)
    points = _points(n, guess, want)
    assert (planted,) in points and all(not any(G.evaluate(e, x, n) for e in eqs) for (x,) in points)
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    bits = [p.gens()[0][g] for g in guess]
    for qsys, zeros, gs in ((q, eqs, list(guess)), (p, _packed_zeros(eqs, n), bits)):
        assert list(qsys.solve_all_xl4_guess(zeros, gs)) == points
        assert qsys.solve_one_xl4_guess(zeros, gs) == points[0]
        spaces = qsys.solve_raw_space_xl4_guess(zeros, gs)
        assert [a for a, sp in enumerate(spaces) if sp is not None] == HYBRID[(n, m, guess)]
        ones = qsys.solve_raw_one_xl4_guess(zeros, gs)
        assert [o for o in ones if o is not None] == [sp.origin for sp in spaces if sp is not None]
        for a in HYBRID[(n, m, guess)]:
            assert qsys.convert_sol_xl4_guess(spaces[a].origin, gs, a) in points
    with pytest.raises(DimensionTooLargeError):        # degree-3 hybrid on the same guess is hopeless
        list(q.solve_all_xl_guess(eqs, list(guess)))


def test_assignments_range():
    n, m, guess = 16, 15, (12, 13, 14, 15)
    eqs, _, want = _hybrid_case(n, m, guess)
    quad, terms = X.quad_aug(eqs, n), _factored(eqs, n)
    for first, count in ((7, 4), (10, 1), (13, 3)):
        for md in (0, 1):
            for got in (hip.solve_xl4_guess_words(quad, n, guess, first, count, md), hip.solve_xl4_guess_quad_terms(*terms, n, guess, first, count, md)):
                assert len(got) == count
                for s in range(count):
                    _assert_solution(got[s], want[first + s][md], md)
    assert hip.solve_xl4_guess_words(quad, n, guess, 2, 0) == []
    points = _points(n, guess, want)
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        parts = [sol for a in range(0, 16, 5) for sol in qsys.solve_all_xl4_guess(zeros, guess, assignments=(a, min(5, 16 - a)))]
        assert parts == points
        spaces = qsys.solve_raw_space_xl4_guess(zeros, guess, assignments=(8, 3))
        assert [sp is not None for sp in spaces] == [True, False, True]


def test_no_guess_equals_plain_xl4():
    n, m = 9, 9
    rng = random.Random(400 * n + m)
    eqs = X.planted_dense(rng, n, m, [rng.getrandbits(n)])
    quad, terms = X.quad_aug(eqs, n), _factored(eqs, n)
    key = lambda s: (s.status, s.rank, s.dimension, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    for md in (0, 1):
        want = hip.solve_xl4_words(quad, n, md)
        assert want.status == 0 and want.dimension == 1       # (the oracle's: SOLVE_CASES of test_gpu_xl4.py)
        for got in (hip.solve_xl4_guess_words(quad, n, [], mode=md), hip.solve_xl4_guess_quad_terms(*terms, n, [], mode=md)):
            assert len(got) == 1 and key(got[0]) == key(want)
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        assert list(qsys.solve_all_xl4_guess(zeros, [])) == list(qsys.solve_all_xl4(zeros))


# -- 3. stream order -------------------------------------------------------------------------------------------------------------------------
def test_chain_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the quadratic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then specialisation, batched degree-4 expansion and the gang solve are enqueued there with no synchronisation anywhere."""
    n, m, guess = 12, 7, (1, 4, 7)                     # 8 systems over 9 unknowns: 7 * 46 = 322 live rows, 255 columns
    ns, na = n - len(guess), 8
    cols4 = xl4_cols(ns)
    rows, stride = 322 + 3, hip.padded_stride(cols4)
    ss = _w2(ns) + 1                                   # 2 words a specialised row
    new = X.quad_aug(X.planted_dense(random.Random(91), n, m, [0xABC]), n)
    old = X.quad_aug(X.planted_dense(random.Random(92), n, m, [0x123]), n)
    want, stale = hip.solve_xl4_guess_words(new, n, guess, mode=1), hip.solve_xl4_guess_words(old, n, guess, mode=1)
    key = lambda sols: [(s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist()) for s in sols]     # noqa: E731
    assert any(s.status == 0 for s in want) and key(want) != key(stale), "the two systems have the same answers"
    buf, src = _to_dev(old), _to_dev(new)
    d_spec = torch.zeros(na * m * ss, dtype=torch.int64, device="cuda")
    d_xl = torch.zeros(na * rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _delayed_copy(stream, cycles, buf, src)
    hip.quad_specialise_device(buf.data_ptr(), m, new.shape[1], n, guess, 0, na, d_spec.data_ptr(), ss, m * ss, stream=_handle(stream))
    hip.xl4_expand_batch_device(d_spec.data_ptr(), na, m * ss, m, ss, ns, rows, d_xl.data_ptr(), stride, rows * stride, stream=_handle(stream))
    got = hip.solve_batch_device(d_xl.data_ptr(), na, rows * stride, rows, cols4, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (the solve entry's 322 rows and these 325: zero rows change nothing)
