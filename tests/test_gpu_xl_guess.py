"""Hybrid XL on the MI355X: guessed unknowns substituted into the quadratic rows for many assignments at once (k_quad_specialise), every
assignment's rows multiplied in one launch (k_xl3_expand_batch) and all systems solved as lock-step gangs.  The yardsticks are the
set-based substitution of tests.xl_guess_terms, the set-based expansion of tests.xl_terms and the CPU oracle on their rows; every
comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols
from oracle import gf2_oracle as O
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


# -- 1. specialisation parity ------------------------------------------------------------------------------------------------------------
def _guess_sets(n: int) -> list:
    f = min(3, n - 1)
    sets = [(), tuple(range(f)), tuple(range(n - f, n))]
    if n >= 11:
        sets.append((7, 2, 3, n - 1, 5))               # scattered and adjacent, not sorted
    elif n == 4:
        sets.append((2, 0))
    if n <= 31:                                        # f = n - 1: every unknown but one, from the top down
        sets.append(tuple(u for u in range(n - 1, -1, -1) if u != n // 2))
    return sets


@functools.lru_cache(maxsize=None)
def _specialise_cases(n: int) -> tuple:
    """(equation ints, quad rows, guess, a0, na, stride, expected [na, m, stride]) per case: computed once, shared by both modes"""
    rng = random.Random(7000 + n)
    cols2 = n + n * (n - 1) // 2
    ones = (1 << (cols2 + 1)) - 1                      # every coefficient set: every run is populated
    cases = []
    for k, guess in enumerate(_guess_sets(n)):
        total = 1 << len(guess)
        a0 = total - 7 if total >= 8 else 0            # a0 > 0, na = 7; the last assignment sets every guessed unknown
        ws = _w2(n - len(guess))
        for m, stride in ((3, ws), (1, ws | 1), (0, ws)) if k % 2 == 0 else ((3, (ws + 5) & ~1), (1, ws + 1 - (ws & 1))):
            eqs = [rng.getrandbits(cols2 + 1) for _ in range(m - 1)] + [ones][:m]
            quad = X.quad_aug(eqs, n, _w2(n) + (m & 1))
            cases.append((eqs, quad, guess, a0, total - a0, stride, G.specialised_aug(eqs, n, guess, a0, total - a0, stride)))
    guess = _guess_sets(n)[1]                          # every assignment from 0, a random single row
    eqs = [rng.getrandbits(cols2 + 1)]
    cases.append((eqs, X.quad_aug(eqs, n), guess, 0, 1 << len(guess), 0, G.specialised_aug(eqs, n, guess, 0, 1 << len(guess))))
    return tuple(cases)


@pytest.mark.parametrize("n", [2, 3, 4, 11, 12, 33, 64, 65])
def test_specialisation_equals_host_reference(n):
    strides = set()
    for _, quad, guess, a0, na, stride, want in _specialise_cases(n):
        got = hip.quad_specialise_words(quad, n, guess, a0, na, stride_words=stride or None)
        assert got.shape == want.shape == (na, len(quad), stride or _w2(n - len(guess)))
        assert np.array_equal(got, want), (n, guess, a0, len(quad), stride, np.argwhere(got != want)[:4])      # every word of the stride
        if not guess and len(quad):
            assert np.array_equal(got[0, :, :_w2(n)], quad[:, :_w2(n)])        # no guess: the rows as they were
        strides.add(got.shape[2] & 1)
    assert strides == {0, 1}                           # 16-byte and 8-byte stores


@pytest.mark.parametrize("n", [4, 12, 65])
def test_specialise_device_loose_system_stride(n):
    """the device entry: systems further apart than their rows, the words between them untouched; an even and an odd layout"""
    for eqs, quad, guess, a0, na, _, _ in [c for c in _specialise_cases(n) if len(c[0]) == 3 and c[2]][:2]:
        m, ws = len(quad), _w2(n - len(guess))
        for stride, sys_stride in (((ws + 1) & ~1, m * ((ws + 1) & ~1) + 6), (ws | 1, m * (ws | 1) + 3)):
            want = G.specialised_aug(eqs, n, guess, a0, na, stride)
            d_quad = _to_dev(quad)
            out = torch.full((na * sys_stride,), SENTINEL, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            hip.quad_specialise_device(d_quad.data_ptr(), m, quad.shape[1], n, guess, a0, na, out.data_ptr(), stride, sys_stride)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64).reshape(na, sys_stride)
            assert np.array_equal(got[:, :m * stride].reshape(na, m, stride), want), (n, guess, stride)
            assert (got[:, m * stride:] == SENTINEL).all()


# -- 2. batch expansion parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 2, 5])
def test_batch_expansion_equals_single_expansions(nsys):
    for n, m, pad in ((9, 4, 3), (12, 3, 0), (33, 2, 5)):
        rng = random.Random(100 * nsys + n)
        cols2 = n + n * (n - 1) // 2
        quads = np.stack([X.quad_aug([rng.getrandbits(cols2 + 1) for _ in range(m)], n, _w2(n) + 1) for _ in range(nsys)])
        rows = m * (n + 1) + pad
        stride = (xl3_cols(n) + 1 + 63) // 64 + (nsys & 1)
        sys_stride = rows * stride + 7
        got = hip.xl3_expand_batch_words(quads, n, rows=rows, stride_words=stride, sys_stride_words=sys_stride)
        assert got.shape == (nsys, sys_stride)
        for s in range(nsys):
            want = hip.xl3_expand_words(quads[s], n, rows=rows, stride_words=stride)
            assert np.array_equal(got[s, :rows * stride].reshape(rows, stride), want), (nsys, n, s)
            assert not got[s, rows * stride:].any()    # (the binding's zeros: the entry writes nothing between the systems)
        tight = hip.xl3_expand_batch_words(quads, n)
        assert np.array_equal(tight.reshape(nsys, m * (n + 1), -1), np.stack([hip.xl3_expand_words(q, n) for q in quads]))
    assert hip.xl3_expand_batch_words(np.zeros((0, 2, 1), dtype=np.uint64), 9).shape == (0, 20 * 3)


def test_batch_expansion_device_reads_each_systems_rows():
    """the device entry with the systems' quadratic rows and their expansions both further apart than they need to be"""
    n, m, nsys, rng = 12, 3, 3, random.Random(12)
    cols2, cols3 = n + n * (n - 1) // 2, xl3_cols(n)
    quads = np.stack([X.quad_aug([rng.getrandbits(cols2 + 1) for _ in range(m)], n, 3) for _ in range(nsys)])
    rows, stride = m * (n + 1) + 2, (cols3 + 1 + 63) // 64 + 1            # 6 words
    qsys, sys_stride = m * 3 + 5, rows * stride + 4
    src = np.full((nsys, qsys), SENTINEL, dtype=np.uint64)
    src[:, :m * 3] = quads.reshape(nsys, -1)
    d_quad = _to_dev(src)
    out = torch.full((nsys * sys_stride,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.xl3_expand_batch_device(d_quad.data_ptr(), nsys, qsys, m, 3, n, rows, out.data_ptr(), stride, sys_stride)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64).reshape(nsys, sys_stride)
    for s in range(nsys):
        assert np.array_equal(got[s, :rows * stride].reshape(rows, stride), hip.xl3_expand_words(quads[s], n, rows=rows, stride_words=stride))
    assert (got[:, rows * stride:] == SENTINEL).all()


# -- 3. solve parity against the CPU oracle on the helper's rows ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(n: int, m: int, guess: tuple) -> tuple:
    eqs = list(G.case_eqs(n, m, guess))
    return eqs, [G.oracle_guess(eqs, n, guess, a) for a in range(1 << len(guess))]


@pytest.mark.parametrize("n,m,guess", list(G.CASES))
def test_solves_equal_oracle(n, m, guess):
    eqs, want = _oracle_case(n, m, guess)
    quad, terms = X.quad_aug(eqs, n), _factored(eqs, n)
    total = 1 << len(guess)
    assert any(w[1]["status"] == 0 for w in want)      # the right assignments are among them
    for md in (0, 1):
        for got in (hip.solve_xl3_guess_words(quad, n, guess, mode=md), hip.solve_xl3_guess_quad_terms(*terms, n, guess, mode=md)):
            assert len(got) == total
            for a in range(total):
                _assert_solution(got[a], want[a][md], md)
        a0 = max(total - 5, 1)                         # a range inside
        na = min(3, total - a0)
        for got in (hip.solve_xl3_guess_words(quad, n, guess, a0, na, md), hip.solve_xl3_guess_quad_terms(*terms, n, guess, a0, na, md)):
            assert len(got) == na
            for s in range(na):
                _assert_solution(got[s], want[a0 + s][md], md)
    assert hip.solve_xl3_guess_words(quad, n, guess, 2, 0) == []


def test_no_guess_equals_plain_xl():
    n, m = 9, 8
    eqs = list(G.case_eqs(n, m, (1, 8)))
    quad, terms = X.quad_aug(eqs, n), _factored(eqs, n)
    key = lambda s: (s.status, s.rank, s.dimension, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    for md in (0, 1):
        want = hip.solve_xl3_words(quad, n, md)
        assert want.status == 0 and want.dimension > 16
        for got in (hip.solve_xl3_guess_words(quad, n, [], mode=md), hip.solve_xl3_guess_quad_terms(*terms, n, [], mode=md)):
            assert len(got) == 1 and key(got[0]) == key(want)


# -- 4. the front-ends -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth(n: int, m: int, guess: tuple) -> tuple:
    eqs = list(G.case_eqs(n, m, guess))
    points, _ = G.oracle_points(eqs, n, guess)
    assert sorted(points) == G.brute_force(eqs, n)
    return eqs, points


def _assignment_of(x: int, guess) -> int:
    return sum(((x >> g) & 1) << t for t, g in enumerate(guess))


@pytest.mark.parametrize("n,m,guess", [(12, 12, (1, 4, 7, 10)), (10, 9, (2, 6, 9))])
def test_front_ends(n, m, guess):
    eqs, points = _truth(n, m, guess)
    want = [(x,) for x in points]
    assert len(want) >= 2
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    bits = [p.gens()[0][g] for g in guess]             # the guess as one-bit vectors of the packed system, as ints for the other
    got_q, got_p = list(q.solve_all_xl_guess(eqs, list(guess))), list(p.solve_all_xl_guess(_packed_zeros(eqs, n), bits))
    assert got_q == got_p == want                      # the oracle's order: by assignment, then AffineSpace order
    assert {x for (x,) in got_q} == set(G.brute_force(eqs, n))
    order = [_assignment_of(x, guess) for (x,) in got_q]
    assert order == sorted(order)
    total = 1 << len(guess)
    for qsys, zeros in ((q, eqs), (p, _packed_zeros(eqs, n))):
        with pytest.raises(DimensionTooLargeError) as err:
            list(qsys.solve_all_xl(zeros))
        assert err.value.space.dimension > 16
        assert qsys.solve_one_xl_guess(zeros, guess) == want[0]
        whole = qsys.solve_raw_space_xl_guess(zeros, guess)
        parts = [sp for a in range(0, total, 3) for sp in qsys.solve_raw_space_xl_guess(zeros, guess, assignments=(a, min(3, total - a)))]
        as_key = lambda sp: None if sp is None else (sp.dimension, sp.origin, sp.basis)          # noqa: E731
        assert len(whole) == len(parts) == total and [as_key(sp) for sp in whole] == [as_key(sp) for sp in parts]
        chunked = [sol for a in range(0, total, 3) for sol in qsys.solve_all_xl_guess(zeros, guess, assignments=(a, min(3, total - a)))]
        assert chunked == want
        ones = qsys.solve_raw_one_xl_guess(zeros, guess)
        assert [o is None for o in ones] == [sp is None for sp in whole]
        assert [o for o in ones if o is not None] == [sp.origin for sp in whole if sp is not None]
        for a, sp in enumerate(whole):                 # convert_sol_xl_guess on the raw points is what solve_all_xl_guess yields
            if sp is not None and sp.dimension == 0:
                sol = qsys.convert_sol_xl_guess(sp.origin, guess, a)
                assert sol is None or sol in want


def test_chunks_are_fetched_when_asked_for(monkeypatch):
    n, m, guess = 10, 9, (2, 6, 9)
    eqs, points = _truth(n, m, guess)
    calls = []
    monkeypatch.setattr(hip, "xl3_guess_chunk", lambda *a, **k: calls.append(a) or 3)
    for qsys, zeros in ((QuadraticSystem([n]), eqs), (PackedQuadraticSystem([n]), _packed_zeros(eqs, n))):
        solved = []
        inner = qsys._solve_internal_xl_guess

        def spy(zs, g, md, inner=inner, solved=solved):
            count, run = inner(zs, g, md)
            return count, lambda first, na: solved.append((first, na)) or run(first, na)
        monkeypatch.setattr(qsys, "_solve_internal_xl_guess", spy)
        it = qsys.solve_all_xl_guess(zeros, guess)
        first = next(it)
        assert first == (points[0],)
        assert solved == [(a, min(3, 8 - a)) for a in range(0, 3 * (_assignment_of(points[0], guess) // 3) + 1, 3)]      # nothing beyond its chunk
        assert [first] + list(it) == [(x,) for x in points]
        assert solved == [(0, 3), (3, 3), (6, 2)]
    assert calls and all(c == (m, n, len(guess)) for c in calls)


def test_row_that_becomes_one():
    """x_g = 0 as an equation: the constant 1 under every assignment that sets x_g, which the solver reports inconsistent"""
    n, m, guess = 10, 9, (2, 6, 9)
    eqs, points = _truth(n, m, guess)
    q, p = QuadraticSystem([n]), PackedQuadraticSystem([n])
    g = guess[1]
    keep = [(x,) for x in points if not (x >> g) & 1]
    assert keep and len(keep) < len(points)
    for qsys, zeros in ((q, eqs + [1 << (1 + g)]), (p, _packed_zeros(eqs, n) + [p.gens()[0][g]])):
        spaces = qsys.solve_raw_space_xl_guess(zeros, guess)
        assert all(spaces[a] is None for a in range(8) if (a >> 1) & 1)
        assert any(spaces[a] is not None for a in range(8) if not (a >> 1) & 1)
        assert list(qsys.solve_all_xl_guess(zeros, guess)) == keep
    for got in hip.solve_xl3_guess_words(X.quad_aug(eqs + [1 << (1 + g)], n), n, guess, mode=1)[2::4]:
        assert got.status == hip.STATUS_INCONSISTENT


# -- 5. stream order -------------------------------------------------------------------------------------------------------------------------
def test_chain_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the quadratic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then specialisation, batched expansion and the gang solve are enqueued there with no synchronisation anywhere."""
    n, m, guess = 12, 12, (1, 4, 7)                    # 8 systems over 9 unknowns: 120 live rows, 129 columns
    ns, na = n - len(guess), 8
    cols3 = xl3_cols(ns)
    rows, stride = cols3 + 3, hip.padded_stride(cols3)
    ss = _w2(ns) + 1                                   # 2 words a specialised row
    new = X.quad_aug(X.planted_dense(random.Random(71), n, m, [0xABC]), n)
    old = X.quad_aug(X.planted_dense(random.Random(72), n, m, [0x123]), n)
    want, stale = hip.solve_xl3_guess_words(new, n, guess, mode=1), hip.solve_xl3_guess_words(old, n, guess, mode=1)
    key = lambda sols: [(s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist()) for s in sols]     # noqa: E731
    assert any(s.status == 0 for s in want) and key(want) != key(stale), "the two systems have the same answers"
    buf, src = _to_dev(old), _to_dev(new)
    d_spec = torch.zeros(na * m * ss, dtype=torch.int64, device="cuda")
    d_xl = torch.zeros(na * rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _delayed_copy(stream, cycles, buf, src)
    hip.quad_specialise_device(buf.data_ptr(), m, new.shape[1], n, guess, 0, na, d_spec.data_ptr(), ss, m * ss, stream=_handle(stream))
    hip.xl3_expand_batch_device(d_spec.data_ptr(), na, m * ss, m, ss, ns, rows, d_xl.data_ptr(), stride, rows * stride, stream=_handle(stream))
    got = hip.solve_batch_device(d_xl.data_ptr(), na, rows * stride, rows, cols3, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (the solve entry pads to max(120, 129) rows: zero rows change nothing)
