"""Degree-4 XL on cubic equations on the MI355X: cubic rows multiplied by 1 and by every unknown on the device (k_xl4_cubic_expand)
and solved there.  The yardsticks are the set-of-monomials product of tests/cubic_xl4_terms.py and the CPU oracle on its rows; every
comparison is bit-exact."""
import functools
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import PackedCubicSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError, xl3_cols, xl4_cols
from oracle import gf2_oracle as O
from tests.cubic_terms import (ONE, REGISTER_12, REGISTER_16, expand_ints, poly_int, poly_value, random_cubic_terms, register_zeros, row_polys,
                               to_aug)
from tests.cubic_xl4_terms import quartic_aug, register_polys, xl4_cubic_eqs
from tests.known_answer import assert_same
from tests.test_gpu_stream_order import DELAY_MS, _handle, cycles, stream      # noqa: F401  (fixtures)
from tests.test_packed_cubic_cpu import Twin

pytestmark = pytest.mark.gpu

M = lambda *v: frozenset(v)                            # noqa: E731  (a monomial)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).cuda()      # (a copy: the shared cases are read-only)
    torch.cuda.synchronize()
    return t


def _expand_device(src: np.ndarray, n: int, rows: int, stride: int) -> np.ndarray:
    """gf2bv_xl4_cubic_expand_device into a buffer that held ones in every bit"""
    d_src = _dev(src)
    d_aug = torch.full((rows * stride,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.xl4_cubic_expand_device(d_src.data_ptr(), len(src), src.shape[1], n, rows, d_aug.data_ptr(), stride)
    torch.cuda.synchronize()
    return d_aug.cpu().numpy().view(np.uint64).reshape(rows, stride)


# -- 1. expansion parity -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_case(n: int):
    """(cubic source rows, rows, stride, expected words): three random factored rows and one with every coefficient set, three zero
    rows behind, both strides wider than needed; made once, never changed"""
    polys = row_polys(n, *random_cubic_terms(random.Random(9000 + n), n, 3))
    polys.append(frozenset([ONE] + [M(i) for i in range(n)] + [M(i, j) for i in range(n) for j in range(i)]
                           + [M(i, j, l) for i in range(n) for j in range(i) for l in range(j)]))
    cols3, wt = xl3_cols(n), (xl4_cols(n) + 1 + 63) // 64
    src = to_aug([poly_int(p, n) for p in polys], cols3, (cols3 + 1 + 63) // 64 + 1)
    rows, stride = len(polys) * (n + 1) + 3, wt + 2 + (wt & 1)
    want = quartic_aug(xl4_cubic_eqs(n, polys), n, rows, stride)
    src.setflags(write=False)
    want.setflags(write=False)
    return src, rows, stride, want


# n < 4 has no quadruple block, n < 3 no triple block; 11 .. 13 and 33 put the block boundaries inside words
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 20, 33])
def test_expansion_equals_set_oracle(n):
    src, rows, stride, want = _parity_case(n)
    words = hip.xl4_cubic_expand_words(src, n, rows=rows, stride_words=stride)
    dev = _expand_device(src, n, rows, stride)
    assert words.shape == dev.shape == want.shape == (rows, stride)
    assert np.array_equal(dev, want), (n, np.argwhere(dev != want)[:4])          # every word up to the stride, the ones overwritten
    assert np.array_equal(words, dev)
    assert not dev[-3:].any() and dev[:-3].any()
    assert hip.xl4_cubic_expand_words(src[:0], n).shape == (0, (xl4_cols(n) + 1 + 63) // 64)


@pytest.mark.parametrize("n", [7, 9, 12])              # the constant on bit 63 of a word (nothing behind it there), on bit 1, on bit 42
def test_bits_behind_the_constant_are_ignored(n):
    src, rows, stride, want = _parity_case(n)
    cols3 = xl3_cols(n)
    junk = np.array(src)
    for c in range(cols3 + 1, 64 * junk.shape[1]):
        junk[:, c >> 6] |= np.uint64(1 << (c & 63))
    assert not np.array_equal(junk, src)
    assert np.array_equal(hip.xl4_cubic_expand_words(junk, n, rows=rows, stride_words=stride), want)
    assert np.array_equal(_expand_device(junk, n, rows, stride), want)


@functools.lru_cache(maxsize=None)
def _wide_case():
    """n = 70, one row of about 40 chosen monomials and three whole runs of the triple block -- (69, 68, 0..67), (69, 67, 0..66) and
    (68, 67, 0..66), each longer than a word and with members l >= 65 -- so the windows of the quadruple block for k = i, k = j and
    k = l span two source words, and so do the triple block's own"""
    n = 70
    rng = random.Random(70)
    monos = {ONE, M(69), M(3), M(64), M(69, 68), M(66, 65), M(65, 1), M(40, 7), M(67, 66, 65), M(69, 66, 65), M(68, 66, 0), M(5, 3, 1), M(2, 1, 0),
             M(66, 30, 2)}
    for _ in range(26):
        monos.add(frozenset(rng.sample(range(n), rng.choice([1, 2, 3]))))
    few = len(monos)
    monos |= {M(69, 68, l) for l in range(68)} | {M(69, 67, l) for l in range(67)} | {M(68, 67, l) for l in range(67)}
    assert 38 <= few <= 40 and M(69, 68, 67) in monos and M(69, 68, 65) in monos
    p = frozenset(monos)
    cols3, wt = xl3_cols(n), (xl4_cols(n) + 1 + 63) // 64
    src = to_aug([poly_int(p, n)], cols3, (cols3 + 1 + 63) // 64)
    rows, stride = n + 2, wt + (wt & 1)
    return src, rows, stride, quartic_aug(xl4_cubic_eqs(n, [p]), n, rows, stride)


def test_runs_longer_than_a_word():
    n = 70
    src, rows, stride, want = _wide_case()
    got = hip.xl4_cubic_expand_words(src, n, rows=rows, stride_words=stride)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not got[-1].any()


# -- 2. get_eqs_xl4 ------------------------------------------------------------------------------------------------------------------------
def test_get_eqs_xl4_equals_the_helper():
    """n = 9, a mixed list: PackedBitVec rows, the literals 0 and 1, and a bit with more quadratic and more cubic terms than one pass
    of k_cubic_expand holds"""
    n = 9
    rng = random.Random(99)
    tw = Twin([4, 5])
    bits = [tw.bit(rng, constant=True) for _ in range(5)]
    big, big_poly = tw.bit(rng, constant=True)
    while min(len(big._ta), len(big._ua)) <= max(hip.cubic_chunks(n)) * 2:      # several passes' worth of either kind
        a, s = tw.bit(rng, constant=False)
        big, big_poly = big ^ a, big_poly ^ s
    zeros = [bits[0][0], tw.x[:2], 0, bits[1][0].concat(bits[2][0]), 1, big, bits[3][0], tw.x[3] ^ tw.x[3], bits[4][0]]
    polys = [bits[0][1], frozenset([M(0)]), frozenset([M(1)]), frozenset(), bits[1][1], bits[2][1], frozenset([ONE]), big_poly, bits[3][1], frozenset(),
             bits[4][1]]
    off2, off3 = tw.p._terms(zeros)[1], tw.p._terms(zeros)[4]
    assert np.diff(off2).max() > 2 * hip.cubic_chunks(n)[0] and np.diff(off3).max() > 2 * hip.cubic_chunks(n)[1]
    want = [e for e in xl4_cubic_eqs(n, polys) if e]
    assert len(want) < len(polys) * (n + 1)            # (the zero rows are dropped)
    assert tw.p.get_eqs_xl4(zeros) == want
    assert tw.p.get_eqs_xl4([]) == [] and tw.p.get_eqs_xl4([0]) == []


# -- 3. solves against the CPU oracle on the helper's rows ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve_case(n: int, m: int, consistent: bool):
    """m planted random factored rows over n unknowns (with the equation 1 behind them where the case is inconsistent), the cubic rows
    of them, and the oracle's answers in both modes on the helper's rows padded to the quartic columns"""
    rng = random.Random(100 * n + m)
    point = rng.getrandbits(n) | 2
    lin, off2, ta, tb, off3, ua, ub, uc = random_cubic_terms(rng, n, m, max_terms=2)
    for r, p in enumerate(row_polys(n, lin, off2, ta, tb, off3, ua, ub, uc)):
        lin[r, 0] ^= np.uint64(poly_value(p, point))   # every row vanishes at the point
    if not consistent:
        one = np.zeros((1, lin.shape[1]), dtype=np.uint64)
        one[0, 0] = 1
        lin, off2, off3 = np.concatenate([lin, one]), np.append(off2, off2[-1]), np.append(off3, off3[-1])
    terms = (lin, off2, ta, tb, off3, ua, ub, uc)
    cols3, cols4 = xl3_cols(n), xl4_cols(n)
    cubic = to_aug(expand_ints(n, *terms), cols3, (cols3 + 1 + 63) // 64)
    eqs = xl4_cubic_eqs(n, row_polys(n, *terms))
    rows = max(len(eqs), cols4)
    aug = quartic_aug(eqs, n, rows, O.words_for(cols4))
    return terms, cubic, {md: O.solve_words(aug, rows, cols4, md) for md in (0, 1)}


# n = 8: 162 columns, 9 rows an equation; n = 10: 385 columns, 11 rows an equation
@pytest.mark.parametrize("n, m, kind", [(8, 24, "over"), (8, 14, "deficient"), (8, 24, "inconsistent"),
                                        (10, 42, "over"), (10, 30, "deficient"), (10, 42, "inconsistent")])
@pytest.mark.parametrize("mode", [0, 1])
def test_solves_equal_the_cpu_oracle(n, m, kind, mode):
    terms, cubic, want = _solve_case(n, m, kind != "inconsistent")
    w = want[mode]
    if kind == "inconsistent":
        assert w["status"] != 0
    else:
        assert w["status"] == 0 and 0 < w["rank"] < xl4_cols(n)                   # (sparse rows: short of full rank in either case)
        assert (len(cubic) * (n + 1) > xl4_cols(n)) == (kind == "over")          # more live rows than columns, or fewer
    assert_same(hip.solve_xl4_cubic_terms(*terms, n, mode), w, mode)
    assert_same(hip.solve_xl4_cubic_words(cubic, n, mode), w, mode)


# -- 4. the filtered register ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secret", [0x52F, 0x3A1])
def test_register_known_answers(secret):
    """n = 12, taps 0xE08, z = s1 ^ s3 s5 ^ s7 s9 s11 over 793 quartic columns: dimension 0 at 62 outputs, 13 at 60 (the one consistent
    point is still the secret), 26 at 59; plain linearisation of the 62 outputs over the 298 cubic columns is far from its rank"""
    p = PackedCubicSystem([12])
    zeros = register_zeros(p, secret, REGISTER_12["taps"], REGISTER_12["pos"], 62)
    assert list(p.solve_all_xl4(zeros)) == [(secret,)] and p.solve_one_xl4(zeros) == (secret,)
    space = p.solve_raw_space_xl4(zeros)
    assert space.dimension == 0 and p.convert_sol_xl4(space.origin) == (secret,) and p.solve_raw_one_xl4(zeros) == space.origin
    assert p.solve_raw_space_xl4(zeros[:60]).dimension == 13
    assert list(p.solve_all_xl4(zeros[:60])) == [(secret,)]
    with pytest.raises(DimensionTooLargeError) as e:
        list(p.solve_all_xl4(zeros[:59]))
    assert e.value.space.dimension == 26
    with pytest.raises(DimensionTooLargeError) as e:
        list(p.solve_all(zeros))
    assert e.value.space.dimension == 298 - 62
    assert list(p.solve_all_xl4(zeros + [1])) == [] and p.solve_one_xl4(zeros + [1]) is None


def test_register_16_on_the_blocked_path():
    """n = 16, taps 0xB400, z = s1 ^ s4 s7 ^ s10 s13 s15, 149 outputs: 2533 rows over 2516 columns, which the solver's blocked path
    takes; rank and pivots are the oracle's on the helper's rows and the one solution is the secret"""
    n, secret, outputs = 16, 0x52E7, 149
    cols4 = xl4_cols(n)
    assert cols4 == 2516
    eqs = xl4_cubic_eqs(n, register_polys(secret, count=outputs, **REGISTER_16))
    assert len(eqs) == 2533
    want = O.solve_words(quartic_aug(eqs, n, len(eqs), O.words_for(cols4)), len(eqs), cols4, 1)
    assert want["status"] == 0 and want["rank"] == cols4
    p = PackedCubicSystem([n])
    zeros = register_zeros(p, secret, REGISTER_16["taps"], REGISTER_16["pos"], outputs)
    assert_same(hip.solve_xl4_cubic_terms(*p._terms(zeros), n, 1), want, 1)
    assert list(p.solve_all_xl4(zeros)) == [(secret,)]


# -- 5. stream order -------------------------------------------------------------------------------------------------------------------------
def test_expand_device_reads_what_the_stream_produced(stream, cycles):      # noqa: F811
    """The device buffer first holds the cubic rows of a DIFFERENT system; the right ones arrive by a delayed copy on the caller's
    stream, then the expansion and the solve are enqueued there with no synchronisation anywhere."""
    n, m = 12, 40                                      # 520 live rows, 793 columns: underdetermined, origins and bases to compare
    cols4 = xl4_cols(n)
    rows, stride = cols4 + 12, hip.padded_stride(cols4)
    new, old = _solve_case(n, m, True)[1], _solve_case(n, m + 1, True)[1][:m]
    want, stale = hip.solve_xl4_cubic_words(new, n, 1), hip.solve_xl4_cubic_words(old, n, 1)
    assert want.status == stale.status == 0 and 0 < want.rank < cols4
    key = lambda s: (s.status, s.rank, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())     # noqa: E731
    assert key(want) != key(stale), "the two systems have the same answer"
    buf, src = _dev(old), _dev(new)
    d_aug = torch.zeros(rows * stride, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):                    # a spin of DELAY_MS, then the producer
        torch.cuda._sleep(cycles)
        buf.copy_(src)
        ev.record(stream)
    assert DELAY_MS >= 50 and not ev.query(), "the producer finished before the call: the window is not there"
    hip.xl4_cubic_expand_device(buf.data_ptr(), m, new.shape[1], n, rows, d_aug.data_ptr(), stride, stream=_handle(stream))
    got = hip.solve_device(d_aug.data_ptr(), rows, cols4, stride, 1, stream=_handle(stream))
    assert key(got) == key(want)                       # (solve_xl4_cubic_words pads to max(520, 793) rows: zero rows change nothing)


# -- 6. solve_all_xl4 against brute force ---------------------------------------------------------------------------------------------------
def test_solve_all_xl4_is_the_brute_force_zero_set():
    """n = 10: 45 equations that are sums of products of two and of three affine forms, each product vanishing at five chosen points;
    the quartic space has a small dimension and solve_all_xl4 returns exactly the common zeros over all 2^10 points (the five and
    whatever else there is), in the order the AffineSpace gives them"""
    n = 10
    rng = random.Random(41)
    tw = Twin([4, 6])
    chosen = rng.sample(range(1 << n), 5)
    zeros, polys = [], []
    while len(zeros) < 45:
        a, s = None, frozenset()
        for _ in range(rng.randint(1, 2)):
            while True:
                f = [tw.linear(rng, True) for _ in range(rng.choice([2, 3, 3]))]
                t = tw.mul(f[0], f[1])
                if len(f) == 3:
                    t = tw.mul(t, f[2])
                if all(poly_value(t[1], x) == 0 for x in chosen):
                    break
            a, s = (t[0] if a is None else a ^ t[0]), s ^ t[1]
        zeros.append(a)
        polys.append(s)
    masks = [[sum(1 << g for g in m) for m in s] for s in polys]
    brute = {x for x in range(1 << n) if not any(sum((m & x) == m for m in ms) & 1 for ms in masks)}
    assert set(chosen) <= brute and len(brute) >= 5
    space = tw.p.solve_raw_space_xl4(zeros)
    assert space is not None and len(brute) - 1 <= space.dimension <= 16
    got = list(tw.p.solve_all_xl4(zeros))
    assert len(got) == len(set(got)) and {a | (b << 4) for a, b in got} == brute
    assert got == [sol for sol in (tw.p.convert_sol_xl4(raw) for raw in space) if sol is not None]
    assert tw.p.solve_one_xl4(zeros) == got[0]
    assert tw.p.solve_one_xl4(zeros + [1]) is None and list(tw.p.solve_all_xl4(zeros + [1])) == []
