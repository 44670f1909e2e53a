"""The packed cubic front-end on the MI355X: factored cubic equations expanded over the monomials of degree <= 3 on the device
(k_cubic_expand) and solved there.  The yardstick throughout is the set-of-monomials product of tests/cubic_terms.py; every
comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedCubicSystem, hip, m4ri_solve
from gf2bv_amd._internal import m4ri_solve_cubic_packed
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols
from tests.cubic_terms import (REGISTER_12, IntBasis, expand_ints, poly_int, poly_value, random_cubic_terms, register_eqs, register_zeros, row_polys,
                               to_aug)
from tests.test_gpu_stream_order import _handle, cycles      # noqa: F401  (fixture)
from tests.test_packed_cubic_cpu import Twin

pytestmark = pytest.mark.gpu

LIVE, ROWS = 6, 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def _case(n: int):
    """six factored rows over n unknowns (a linear-only one, one beyond an LDS pass of either kind among them) and the oracle's
    equation ints of them with two zero rows behind: made once, shared, never changed"""
    terms = random_cubic_terms(random.Random(7000 + n), n, LIVE, constants=n % 2 == 1 or n >= 63)
    for a in terms:
        a.setflags(write=False)
    return terms, tuple(expand_ints(n, *terms)) + (0,) * (ROWS - LIVE)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a).view(np.int64).reshape(-1)).cuda()      # (a copy: the shared cases are read-only)


# -- expansion parity: n = 1, 2, 3 have no, no and one triple; 7, 9, 15, 17 put the constant on the last bit of a word or the first of
# -- the next (63, 129, 575, 833 columns); 63, 64, 65 take a form from one word to two
@pytest.mark.parametrize("n", [1, 2, 3, 7, 9, 15, 17, 63, 64, 65])
@pytest.mark.parametrize("how", ["wide", "ones"])
def test_expansion_equals_set_oracle(n, how):
    terms, eqs = _case(n)
    cols = xl3_cols(n)
    wt = (cols + 1 + 63) // 64
    if how == "wide":                                  # a stride wider than needed (odd where wt is even: the entry rounds its own up)
        stride = wt + 3
        got = hip.cubic_expand_words(*terms, n, rows=ROWS, stride_words=stride)
    else:                                              # an output that held ones in every bit
        stride = wt + (wt & 1)
        d = [_dev(a) for a in terms]
        d_aug = torch.full((ROWS * stride,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hip.cubic_expand_device(*[t.data_ptr() for t in d], LIVE, ROWS, n, d_aug.data_ptr(), stride)
        torch.cuda.synchronize()
        got = d_aug.cpu().numpy().view(np.uint64).reshape(ROWS, stride)
    want = to_aug(list(eqs), cols, stride)
    assert got.shape == want.shape == (ROWS, stride)
    assert np.array_equal(got, want), (n, how, np.argwhere(got != want)[:4])      # every word: the bits behind column cols3 and the rows >= rows_live are zero
    assert not got[LIVE:].any()
    if how == "wide":
        assert hip.cubic_expand_words(*random_cubic_terms(random.Random(0), n, 0), n, rows=0).shape == (0, wt)      # no row at all


def test_bad_offsets_on_the_device_give_the_linear_part():
    """offsets the device entry cannot check: a row whose offsets decrease or are negative is its linear part, whichever kind is bad"""
    n = 9
    terms, eqs = _case(n)
    cols, stride = xl3_cols(n), 4
    off2, off3 = terms[1].copy(), terms[4].copy()
    off2[2] = off2[1] - 1                              # row 1: its quadratic offsets decrease
    off3[4], off3[3] = -1, -2                          # row 3 negative; row 2 ends below its start
    d = [_dev(a) for a in (terms[0], off2, terms[2], terms[3], off3, terms[5], terms[6], terms[7])]
    d_aug = torch.full((LIVE * stride,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.cubic_expand_device(*[t.data_ptr() for t in d], LIVE, LIVE, n, d_aug.data_ptr(), stride)
    torch.cuda.synchronize()
    got = d_aug.cpu().numpy().view(np.uint64).reshape(LIVE, stride)
    lin = [int(v) & ((1 << (n + 1)) - 1) for v in terms[0][:, 0]]
    want = to_aug([eqs[0], lin[1], lin[2], lin[3]], cols, stride)
    assert np.array_equal(got[:4], want)


# -- a planted, rank-deficient system over n = 12 (298 columns) -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(n: int, live: int, seed: int, point: int):
    rng = random.Random(seed)
    lin, off2, ta, tb, off3, ua, ub, uc = random_cubic_terms(rng, n, live, max_terms=2)
    for r, p in enumerate(row_polys(n, lin, off2, ta, tb, off3, ua, ub, uc)):
        lin[r, 0] ^= np.uint64(poly_value(p, point))   # every row vanishes at the point
    terms = (lin, off2, ta, tb, off3, ua, ub, uc)
    return terms, tuple(expand_ints(n, *terms))


def _key(s):
    return (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())


def test_expand_device_then_solve_device_on_one_stream(cycles):      # noqa: F811
    """The device inputs first hold zeros; the operands arrive by a delayed copy on a side stream, then the expansion and the solve
    are enqueued there with no synchronisation anywhere.  The answer is solve_words' on the oracle's rows."""
    n, live = 12, 250
    cols = xl3_cols(n)
    rows, stride = cols + 6, hip.padded_stride(cols)
    terms, eqs = _planted(n, live, 11, 0x9A7)
    want = hip.solve_words(to_aug(list(eqs) + [0] * (rows - live), cols, stride), rows, cols, 1)
    assert want.status == 0 and 0 < want.rank < cols
    pack = np.concatenate([terms[k].ravel() for k in (0, 2, 3, 5, 6, 7)])
    src, buf = _dev(pack), torch.zeros(len(pack), dtype=torch.int64, device="cuda")
    d_off2, d_off3 = _dev(terms[1]), _dev(terms[4])
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    ptr, at = [], buf.data_ptr()
    for k in (0, 2, 3, 5, 6, 7):
        ptr.append(at)
        at += terms[k].nbytes
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        buf.copy_(src)
        ev.record(s)
    assert not ev.query(), "the producer finished before the call: the window is not there"
    hip.cubic_expand_device(ptr[0], d_off2.data_ptr(), ptr[1], ptr[2], d_off3.data_ptr(), ptr[3], ptr[4], ptr[5], live, rows, n,
                            d_aug.data_ptr(), stride, stream=_handle(s))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols, stride, 1, stream=_handle(s))
    torch.cuda.synchronize()
    assert _key(got) == _key(want)


# -- m4ri_solve_cubic_packed against m4ri_solve on the oracle's equation ints -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deficient():
    """n = 9 (129 columns): the first 126 independent rows of a planted random system, then 40 rows that are sums of two of them -- a
    factored sum is the terms of both -- so the rank is 126 by construction"""
    n = 9
    pool, pool_eqs = _planted(n, 260, 5, 0x135)
    basis, keep = IntBasis(), []
    for r, e in enumerate(pool_eqs):
        if len(keep) < 126 and basis.add(e >> 1):
            keep.append(r)
    assert len(keep) == 126 and keep[:3] == [0, 1, 2]  # (the linear-only and the multi-pass rows are among them)
    rng = random.Random(6)
    pairs = [rng.sample(keep, 2) for _ in range(40)]
    lin, off2, ta, tb, off3, ua, ub, uc = pool
    groups = [[r] for r in keep] + pairs               # the factored rows each output row is the sum of
    rows = lambda x, off, g: [x[off[r]:off[r + 1]] for r in g]                                    # noqa: E731
    cat = lambda x, off: np.concatenate([np.concatenate(rows(x, off, g)) for g in groups])       # noqa: E731
    new_lin = np.stack([np.bitwise_xor.reduce(lin[g], axis=0) for g in groups])
    o2, o3 = np.zeros(len(groups) + 1, dtype=np.int64), np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([sum(off2[r + 1] - off2[r] for r in g) for g in groups], out=o2[1:])
    np.cumsum([sum(off3[r + 1] - off3[r] for r in g) for g in groups], out=o3[1:])
    eqs = [functools.reduce(lambda a, b: a ^ b, (pool_eqs[r] for r in g)) for g in groups]
    return n, (new_lin, o2, cat(ta, off2), cat(tb, off2), o3, cat(ua, off3), cat(ub, off3), cat(uc, off3)), eqs


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("consistent", [True, False])
def test_solve_cubic_packed_equals_m4ri_solve(mode, consistent):
    n, terms, eqs = _deficient()
    cols = xl3_cols(n)
    assert expand_ints(n, *terms)[126:] == eqs[126:]
    if not consistent:                                 # the literal 1: a row that is the constant alone
        one = np.zeros((1, 1), dtype=np.uint64)
        one[0, 0] = 1
        terms = (np.concatenate([terms[0], one]), np.append(terms[1], terms[1][-1]), terms[2], terms[3], np.append(terms[4], terms[4][-1]),
                 terms[5], terms[6], terms[7])
        eqs = eqs + [1]
    rows = len(eqs)
    assert rows >= cols
    want, got = m4ri_solve(eqs, cols, mode), m4ri_solve_cubic_packed(*terms, n, rows, mode)
    low_want = hip.solve_words(to_aug(eqs, cols, hip.padded_stride(cols)), rows, cols, mode)
    low_got = hip.solve_cubic_terms(*terms, n, rows, mode)
    assert (low_got.status, low_got.rank, low_got.pivots.tolist()) == (low_want.status, low_want.rank, low_want.pivots.tolist())
    if not consistent:
        assert want is None and got is None and low_got.status == hip.STATUS_INCONSISTENT
        return
    assert low_got.rank == 126 and np.array_equal(low_got.origin, low_want.origin) and np.array_equal(low_got.basis, low_want.basis)
    if mode == 0:
        assert isinstance(got, int) and got == want
    else:
        assert got.dimension == want.dimension == 3 and got.origin == want.origin and tuple(got.basis) == tuple(want.basis)      # basis order too


# -- PackedCubicSystem ---------------------------------------------------------------------------------------------------------------
def test_register_full_rank_recovers_the_secret():
    """n = 12, taps 0xE08, z = s1 ^ s3 s5 ^ s7 s9 s11, 298 outputs over 298 columns: rank 298, the one solution is the secret"""
    secret = 0xB5D
    p = PackedCubicSystem([12])
    zeros = register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], 298)
    assert list(p.solve_all(zeros)) == [(secret,)]
    assert p.solve_one(zeros) == (secret,)
    raw = p.solve_raw_one(zeros)
    assert raw == p._raw_point(secret) and p.solve_raw_space(zeros).dimension == 0
    want = [e for e in register_eqs(secret, count=298, **REGISTER_12) if e]
    assert p.get_eqs(zeros) == want and p.get_eqs(zeros + [0]) == want and p.get_eqs([]) == []


def test_register_short_of_rank_raises_dimension_too_large():
    secret = 0xB5D
    p = PackedCubicSystem([12])
    zeros = register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], 248)
    with pytest.raises(DimensionTooLargeError) as e:
        list(p.solve_all(zeros))
    assert e.value.space.dimension == 50


def test_solve_all_is_the_brute_force_zero_set():
    """n = 9: equations written with mul_bit that vanish at a planted point, as many as give rank 123; solve_all returns exactly the common zeros over all
    2^9 points, in the order the AffineSpace gives them"""
    n, secret = 9, 0x0D6
    rng = random.Random(33)
    tw = Twin([4, 5])
    zeros, polys, basis = [], [], IntBasis()
    while len(basis) < xl3_cols(n) - 6:                # rank 123: a space of dimension 6
        a, s = tw.bit(rng, constant=True)
        v = poly_value(s, secret)
        zeros.append(a ^ v)
        polys.append(s ^ frozenset([frozenset()]) if v else s)
        basis.add(poly_int(polys[-1], n) >> 1)
    assert len(zeros) > 62
    zeros = zeros[:60] + [zeros[60].concat(zeros[61])] + zeros[62:] + [0, tw.x[3] ^ tw.x[3]]       # vectors of two bits, 0 and a zero PackedBitVec too
    assert tw.p.get_eqs(zeros) == [e for e in (poly_int(s, n) for s in polys) if e]
    space = tw.p.solve_raw_space(zeros)
    assert space is not None and space.dimension == 6
    masks = [[sum(1 << g for g in m) for m in s] for s in polys]
    brute = {x for x in range(1 << n) if not any(sum((m & x) == m for m in ms) & 1 for ms in masks)}
    assert secret in brute
    got = list(tw.p.solve_all(zeros))
    assert len(got) == len(set(got)) and {a | (b << 4) for a, b in got} == brute
    assert got == [sol for sol in (tw.p.convert_sol(raw) for raw in space) if sol is not None]
    assert tw.p.solve_one(zeros) == got[0]
    assert tw.p.solve_one(zeros + [1]) is None and list(tw.p.solve_all(zeros + [1])) == []
