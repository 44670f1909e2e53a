"""The packed quartic front-end on the MI355X: factored quartic equations expanded over the monomials of degree <= 4 on the device
(k_quartic_expand) and solved there.  The yardsticks are the set-of-monomials product of tests/quartic_terms.py, the CPU oracle on
its equation ints, and the register's own outputs over all states; every comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedQuarticBitVec, PackedQuarticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols, xl4_cols
from oracle import gf2_oracle as O
from tests.quartic_terms import (REGISTER4_12, REGISTER4_16, build_terms, case_rows, expand_ints4, plant, quartic_aug, random_quartic_terms,
                                 register4_brute, register4_eqs, register4_zeros)
from tests.test_gpu_stream_order import _handle, cycles      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 8, 11, 12, 20]                 # no quadruple below 4, a single one at 4, blocks that end inside and at the start of a word
EDGES = [9, 29]                                        # the constant on the last bit of a word (255 columns) and on the first (27840)
PAD = 2                                                # zero rows asked for behind the live ones


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def test_sizes_put_the_blocks_on_both_sides_of_a_word_boundary():
    ends = {n: (n + n * (n - 1) // 2, xl3_cols(n), xl4_cols(n)) for n in SIZES + EDGES}      # cols2, cols3, cols4 = the constant's column
    for k in range(3):
        assert any(ends[n][k] < 64 for n in SIZES) and any(ends[n][k] > 64 for n in SIZES)    # in the first word, and beyond it
    assert ends[3][2] - ends[3][1] == 0 and ends[4][2] - ends[4][1] == 1                      # no quadruple, a single one
    assert ends[11][0] % 64 == 2 and ends[20][1] % 64 == 6                                    # a block that ends just inside a new word
    assert ends[9][2] % 64 == 63 and ends[9][1] % 64 == 1 and ends[29][2] % 64 == 0           # the constant last in a word, first in a word


@functools.lru_cache(maxsize=None)
def _case(n: int):
    """the rows of tests/quartic_terms.case_rows over n unknowns and the oracle's equation ints of them: made once, shared, never
    changed"""
    terms = build_terms(n, case_rows(random.Random(9000 + n), n))
    for a in terms:
        a.setflags(write=False)
    return terms, tuple(expand_ints4(n, *terms))


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a).view(np.int64).reshape(-1)).cuda()      # (a copy: the shared cases are read-only)


@pytest.mark.parametrize("n", SIZES + EDGES)
@pytest.mark.parametrize("how", ["wide", "ones"])
def test_expansion_equals_set_oracle(n, how):
    terms, eqs = _case(n)
    live, rows = len(eqs), len(eqs) + PAD
    wt = (xl4_cols(n) + 1 + 63) // 64
    if how == "wide":                                  # a stride wider than needed (odd where wt is even: the entry rounds its own up)
        stride = wt + 3
        got = hip.quartic_expand_words(*terms, n, rows=rows, stride_words=stride)
    else:                                              # an output that held ones in every bit; rows_live < rows
        stride = wt + (wt & 1)
        d = [_dev(a) for a in terms]
        d_aug = torch.full((rows * stride,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hip.quartic_expand_device(*[t.data_ptr() for t in d], live, rows, n, d_aug.data_ptr(), stride)
        torch.cuda.synchronize()
        got = d_aug.cpu().numpy().view(np.uint64).reshape(rows, stride)
    want = quartic_aug(list(eqs), n, rows, stride)
    assert got.shape == want.shape == (rows, stride)
    assert np.array_equal(got, want), (n, how, np.argwhere(got != want)[:4])      # every word: the bits behind column cols4 and the rows >= rows_live are zero
    assert not got[live:].any()
    if how == "wide":
        assert hip.quartic_expand_words(*build_terms(n, []), n, rows=0).shape == (0, wt)      # no row at all


def _sparse_rows(rng, n: int, rows: int) -> list:
    """rows of one quartic term each (and a quadratic and a cubic one) whose forms have a few unknowns from the top of the range, so
    that the quadruples lie in the long runs"""
    form = lambda: sum(1 << (1 + rng.randrange(n - 12, n)) for _ in range(rng.randint(1, 3))) | rng.getrandbits(1)      # noqa: E731
    return [(form(), [(form(), form())], [(form(), form(), form())], [(form(), form(), form(), form())]) for _ in range(rows)]


@pytest.mark.parametrize("n, rows", [(68, 3), (120, 2)])
def test_expansion_of_long_runs(n, rows):
    """n = 68: quadruple runs longer than a word (866 847 columns).  n = 120: the two staged cubic rows take more than 64 KiB of LDS, the
    size at which the launch raises the kernel's dynamic-LDS limit (8.5 million columns, a megabyte a row)"""
    wl, w3 = (n + 1 + 63) // 64, (xl3_cols(n) + 1 + 63) // 64
    t2, t3, t4 = hip.quartic_chunks(n)
    assert (((1 + 2 * t2 + 3 * t3 + 4 * t4) * wl + (1 + t4) * w3) * 8 > 65536) == (n == 120)
    terms = build_terms(n, _sparse_rows(random.Random(n), n, rows))
    eqs = expand_ints4(n, *terms)
    assert all(e.bit_length() > 1 + xl3_cols(n) for e in eqs)             # quadruples in every row
    got = hip.quartic_expand_words(*terms, n)
    assert np.array_equal(got, quartic_aug(eqs, n, rows, got.shape[1]))


def test_get_eqs_equals_the_helper():
    n = 8
    terms, eqs = _case(n)
    p = PackedQuarticSystem([3, 5])
    x, y = p.gens()
    vec = PackedQuarticBitVec(*terms, n)
    lin = x.concat(y[:2])
    assert p.get_eqs([vec]) == [e for e in eqs if e]
    assert p.get_eqs([0, vec[:4], lin, 1, vec[4:], y[1] ^ y[1]]) == [e for e in list(eqs[:4]) + list(lin._bits) + [1] + list(eqs[4:]) if e]
    assert p.get_eqs([]) == [] and p.get_eqs([0]) == []


# -- solve_raw_space against the CPU oracle on the helper's equation ints ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(n: int, m: int, point: int):
    terms, eqs = plant(n, random_quartic_terms(random.Random(100 * n + m), n, m), point)
    return terms, tuple(eqs)


def _against_oracle(n: int, terms, eqs: list, mode: int):
    cols = xl4_cols(n)
    padded = list(eqs) + [0] * max(0, cols - len(eqs))
    ref = O.solve_words(O.eqs_to_aug(padded, cols), len(padded), cols, 1)
    want = O.m4ri_solve(padded, cols, mode)
    p = PackedQuarticSystem([n])
    zeros = [PackedQuarticBitVec(*terms, n)]
    low = hip.solve_quartic_terms(*terms, n, mode=1)
    assert (low.status, low.rank) == (ref["status"], ref["rank"])
    got = p.solve_raw_space(zeros) if mode else p.solve_raw_one(zeros)
    if want is None:
        assert got is None and low.status == hip.STATUS_INCONSISTENT
    elif mode:
        assert got.dimension == want.dimension == cols - ref["rank"] and got.origin == want.origin and tuple(got.basis) == tuple(want.basis)      # basis order too
    else:
        assert isinstance(got, int) and got == want
    return ref, got


@pytest.mark.parametrize("n, m", [(6, 56 + 8), (8, 162 + 8), (10, 385 + 8)])
def test_solve_raw_space_equals_the_oracle_on_planted_systems(n, m):
    point = 0x2B5 & ((1 << n) - 1)
    terms, eqs = _planted(n, m, point)
    p = PackedQuarticSystem([n])
    ref, space = _against_oracle(n, terms, list(eqs), 1)
    assert ref["status"] == 0 and space.dimension <= 10                   # (56, 162 and 379 of 385: every point can be looked at)
    assert p._raw_point(point) in list(space)
    _against_oracle(n, terms, list(eqs), 0)
    zeros = [PackedQuarticBitVec(*terms, n)]
    assert (point,) in list(p.solve_all(zeros))
    assert p.solve_raw_space(zeros + [1]) is None and p.solve_raw_one(zeros + [1]) is None and list(p.solve_all(zeros + [1])) == []
    assert p.solve_one(zeros + [1]) is None


@pytest.mark.parametrize("mode", [0, 1])
def test_solve_of_an_under_determined_system_equals_the_oracle(mode):
    n, m = 8, 100
    terms, eqs = _planted(n, m, 0x9C)
    ref, _ = _against_oracle(n, terms, list(eqs), mode)
    assert ref["status"] == 0 and ref["rank"] <= m < xl4_cols(n)


# -- the filtered register -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _register(secret: int, count: int):
    p = PackedQuarticSystem([12])
    return p, tuple(register4_zeros(p, secret, count=count, **REGISTER4_12))


@pytest.mark.parametrize("secret", [0x52F, 0x3A1])
def test_register_12(secret):
    """n = 12, taps 0xE08, z = s1 ^ s3 s5 ^ s7 s9 s11 ^ s0 s2 s6 s10, 793 columns"""
    p, zeros = _register(secret, 793)
    zeros = list(zeros)
    space = p.solve_raw_space(zeros)
    assert space.dimension == 0 and p.convert_sol(space.origin) == (secret,) and space.origin == p._raw_point(secret)
    assert p.solve_one(zeros) == (secret,) and list(p.solve_all(zeros)) == [(secret,)]
    assert p.get_eqs(zeros[:100]) == [e for e in register4_eqs(secret, count=100, **REGISTER4_12) if e]
    # 781 outputs: dimension 12, and the consistent points are the states that give the same outputs
    space = p.solve_raw_space(zeros[:781])
    assert space.dimension == 12
    got = list(p.solve_all(zeros[:781]))
    brute = register4_brute(secret, count=781, **REGISTER4_12)
    assert secret in brute and len(got) == len(set(got)) and sorted(got) == [(s,) for s in brute]
    assert got == [sol for sol in (p.convert_sol(raw) for raw in space) if sol is not None]      # AffineSpace order
    with pytest.raises(DimensionTooLargeError) as e:
        list(p.solve_all(zeros[:700]))
    assert e.value.space.dimension == 93


def test_register_16_on_the_blocked_path():
    """n = 16, taps 0xB400, z = s1 ^ s4 s7 ^ s10 s13 s15 ^ s2 s5 s8 s12: 2516 outputs over 2516 columns, beyond the solver's small path"""
    secret = 0x52E7
    p = PackedQuarticSystem([16])
    zeros = register4_zeros(p, secret, count=2516, **REGISTER4_16)
    terms = p._terms(zeros)
    low = hip.solve_quartic_terms(*terms, 16, mode=1)
    assert low.stats["small_path"] == 0 and low.status == 0 and low.rank == 2516
    assert p.solve_one(zeros) == (secret,)


# -- stream order ---------------------------------------------------------------------------------------------------------------------
def _key(s):
    return (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())


def test_expand_device_then_solve_device_on_one_stream(cycles):      # noqa: F811
    """The device inputs first hold zeros; the operands arrive by a delayed copy on a side stream, then the expansion and the solve
    are enqueued there with no synchronisation anywhere.  The answer is solve_words' on the oracle's rows."""
    n, live = 8, 150
    cols = xl4_cols(n)
    rows, stride = cols + 6, hip.padded_stride(cols)
    terms, eqs = _planted(n, live, 0x5A)
    want = hip.solve_words(quartic_aug(list(eqs), n, rows, stride), rows, cols, 1)
    assert want.status == 0 and 0 < want.rank < cols
    ops = [k for k in range(13) if k not in (1, 4, 8)]
    pack = np.concatenate([terms[k].ravel() for k in ops])
    src, buf = _dev(pack), torch.zeros(len(pack), dtype=torch.int64, device="cuda")
    d_off = {k: _dev(terms[k]) for k in (1, 4, 8)}
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    ptr, at = {}, buf.data_ptr()
    for k in ops:
        ptr[k] = at
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
    hip.quartic_expand_device(*[d_off[k].data_ptr() if k in d_off else ptr[k] for k in range(13)], live, rows, n, d_aug.data_ptr(), stride,
                              stream=_handle(s))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols, stride, 1, stream=_handle(s))
    torch.cuda.synchronize()
    assert _key(got) == _key(want)


def test_solve_quartic_terms_right_after_another_solve(cycles):      # noqa: F811
    """the staged solve runs on the solver's pool stream: issued while the device is still busy with a spin and right after another
    solve, it returns what it returns alone"""
    n = 8
    terms, _ = _planted(n, 100, 0x9C)
    other, _ = _planted(n, 162 + 8, 0x2B5 & 0xFF)
    alone = hip.solve_quartic_terms(*terms, n, mode=1)
    torch.cuda._sleep(cycles)
    first = hip.solve_quartic_terms(*other, n, mode=1)
    got = hip.solve_quartic_terms(*terms, n, mode=1)
    assert _key(got) == _key(alone) and _key(first) != _key(alone)
