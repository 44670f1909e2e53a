"""The one-launch small solve (k_small_solve), pass by pass: every built system of tests/small_cases.py through the three single-system
entries and both modes against the CPU oracle (status, rank, pivots, origin, basis and its order) AND gf2bv_stats::small_passes /
small_pass_kinds, which say which branches the passes took -- exact for the panel-confined cases, contained for the mixed ones
(tests/test_small_cases_cpu.py checks every premise without a GPU).  Then what no built system is needed for: the eligibility
boundary of every row width the entries can reach (1..13 words: rows >= cols rules out 14-16, see the CPU file), the largest result
buffers, every kind of digit width on both loaders, and the zero-copy / staged-copy input forced both ways."""
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import small_cases as SC
from tests.systems import random_system
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    """name -> (case, aug, {mode: the oracle's answer}): computed once, never changed"""
    out = {}
    for name, case in SC.cases().items():
        aug = case.aug()
        aug.setflags(write=False)
        out[name] = (case, aug, {mode: O.solve_words(aug, case.rows, case.cols, mode) for mode in (0, 1)})
    return out


def other_searches_idle(st):
    return (not any(v for k, v in st.items() if k.startswith("general_")) and st["fast_blocks"] == 0 and st["sparse_blocks"] == [0, 0, 0])


def on_device(aug, cols):
    stride = hip.padded_stride(cols)
    wide = np.zeros((aug.shape[0], stride), dtype=np.uint64)
    wide[:, :aug.shape[1]] = aug
    buf = hip.DeviceBuffer(wide.nbytes)
    buf.upload(wide)
    return buf, stride


@pytest.mark.parametrize("name", SC.NAMES)
def test_built_case_takes_its_passes(name, built, monkeypatch):
    case, aug, want = built[name]
    rows, cols = case.rows, case.cols
    buf, stride = on_device(aug, cols)
    dig, off = SC.digits(case.eqs(), 30)
    for small in ("1", "0"):
        monkeypatch.setenv("GF2BV_SMALL", small)
        for mode in (0, 1):
            got = {"words": hip.solve_words(aug, rows, cols, mode), "device": hip.solve_device(buf.ptr, rows, cols, stride, mode),
                   "digits": hip.solve_digits(dig, off, 30, rows, cols, mode)}
            for entry, g in got.items():
                st = g.stats
                print(f"{name} small {small} mode {mode} {entry}: small_passes {st['small_passes']} small_pass_kinds {st['small_pass_kinds']}"
                      f" (designed {case.passes} / {case.kinds}, {'exact' if case.exact else 'contained'}) rank {g.rank}")
                assert_same(g, want[mode], mode)
                if small == "1":
                    assert st["small_path"] == 1 and other_searches_idle(st), st
                    assert case.holds(st["small_passes"], st["small_pass_kinds"]), (entry, mode, st["small_passes"], st["small_pass_kinds"])
                else:
                    assert st["small_path"] == 0 and st["small_passes"] == 0 and st["small_pass_kinds"] == 0, st
    buf.free()


def dense(rng, rows, cols, cap):
    eqs = random_system(rng, rows, cols, .5, cap, True, 0)
    rng.shuffle(eqs)
    return eqs, O.eqs_to_aug(eqs, cols)


@pytest.mark.parametrize("wt", range(1, 14))
def test_eligibility_boundary_of_every_row_width(wt):
    """(rows + 512) x (wt | 1) <= 18432, rows <= 4096: the largest eligible row count at the width's largest column count takes the one
    launch, one row more the blocked path -- the shapes come from the formula, written out here.  Dense random systems, every
    other width with a rank cap.  (14-16 words: refused for rows < cols, tests/test_small_cases_cpu.py; for the same reason 1023 against
    1024 columns decides nothing -- 1023 columns need 1023 rows, and 16 words admit 572.)"""
    cols = 64 * wt - 1
    rows = min(4096, 18432 // (wt | 1) - 512)
    assert rows >= cols
    rng = random.Random(700 + wt)
    for r, path in ((rows, 1), (rows + 1, 0)):
        eqs, aug = dense(rng, r, cols, cols - 37 if wt % 2 else None)
        for mode in (0, 1):
            got = hip.solve_words(aug, r, cols, mode)
            assert got.stats["small_path"] == path, (r, cols, got.stats)
            assert (got.stats["small_passes"] >= 1) == (path == 1) and (got.stats["small_pass_kinds"] != 0) == (path == 1)
            assert_same(got, O.solve_words(aug, r, cols, mode), mode)


def test_read_out_at_the_largest_result():
    """the widest system's largest results: all-zero 831 x 831 in mode 1 -- 831 kernel vectors of 13 words, 90 KB, more than the first
    allocation of the pinned result buffer -- and 905 x 831 of rank 500: 331 kernel vectors with bits in all 13 panels"""
    rows = cols = 831
    aug = np.zeros((rows, SC.words_of(cols)), dtype=np.uint64)
    got = hip.solve_words(aug, rows, cols, 1)
    assert got.stats["small_path"] == 1 and got.stats["small_passes"] == 0 and got.stats["small_pass_kinds"] == 0
    assert got.status == 0 and got.rank == 0 and got.dimension == cols and got.origin_int() == 0
    assert got.basis_ints() == tuple(1 << i for i in range(cols))
    rows = 905
    eqs, aug = dense(random.Random(77), rows, cols, 500)
    for mode in (0, 1):
        want = O.solve_words(aug, rows, cols, mode)
        got = hip.solve_words(aug, rows, cols, mode)
        assert got.stats["small_path"] == 1 and want["rank"] == 500
        assert_same(got, want, mode)
    assert got.dimension == 331 and all(int(np.bitwise_or.reduce(got.basis[:, w])) for w in range(13))


DIGIT_SHAPES = [(66, 65, None, "1"), (300, 200, 150, "1"), (905, 831, 700, "1"), (200, 129, 77, "0")]


@pytest.fixture(scope="module")
def digit_systems():
    """shape -> (clean equations, the same with bits above cols + 1 on every third row, aug, the oracle's answers); a tenth of the rows
    are 0: no digits at all"""
    out = {}
    for rows, cols, cap, small in DIGIT_SHAPES:
        rng = random.Random(rows * 1000 + cols)
        eqs = random_system(rng, rows, cols, .5, cap, True, rows // 10)
        rng.shuffle(eqs)
        noisy = [v | (rng.getrandbits(45) << (cols + 1)) if i % 3 == 0 and v else v for i, v in enumerate(eqs)]
        aug = O.eqs_to_aug(eqs, cols)
        out[rows, cols] = (eqs, noisy, aug, {mode: O.solve_words(aug, rows, cols, mode) for mode in (0, 1)})
    return out


@pytest.mark.parametrize("bpd", [1, 7, 15, 21, 22, 31])
@pytest.mark.parametrize("shape", DIGIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-small{s[3]}")
def test_digit_widths_on_both_loaders(shape, bpd, digit_systems, monkeypatch):
    """1-32 bits per digit are accepted; 15 is CPython's other build and takes the tail loop of the small loader (a word needs more
    than four digits below 21 bits).  GF2BV_SMALL=0: the blocked path's k_pack_digits sees the same digits."""
    rows, cols, _, small = shape
    eqs, noisy, aug, want = digit_systems[rows, cols]
    monkeypatch.setenv("GF2BV_SMALL", small)
    dig, off = SC.digits(noisy, bpd)
    assert any(off[r + 1] == off[r] for r in range(rows)) and int(off[-1]) * bpd > rows * (cols + 1) // 2
    for mode in (0, 1):
        got = hip.solve_digits(dig, off, bpd, rows, cols, mode)
        words = hip.solve_words(aug, rows, cols, mode)
        assert got.stats["small_path"] == words.stats["small_path"] == int(small)
        assert_same(got, want[mode], mode)
        assert_same(words, want[mode], mode)
        assert np.array_equal(got.origin, words.origin) and np.array_equal(got.basis, words.basis)


@pytest.mark.parametrize("zc", ["0", "1"])
def test_zero_copy_and_staged_input_forced_both_ways(zc, monkeypatch):
    """GF2BV_SMALL_ZC: unset, inputs up to 32 KiB are read over the link and larger ones copied first; forced, both sizes go either way"""
    monkeypatch.setenv("GF2BV_SMALL_ZC", zc)
    for rows, cols, cap in ((66, 65, None), (4096, 100, 70)):
        rng = random.Random(rows + int(zc))
        eqs, aug = dense(rng, rows, cols, cap)
        assert (aug.nbytes <= 32 << 10) == (rows == 66)
        dig, off = SC.digits(eqs, 30)
        for mode in (0, 1):
            want = O.solve_words(aug, rows, cols, mode)
            for got in (hip.solve_words(aug, rows, cols, mode), hip.solve_digits(dig, off, 30, rows, cols, mode)):
                assert got.stats["small_path"] == 1 and got.stats["small_passes"] >= 1
                assert_same(got, want, mode)
