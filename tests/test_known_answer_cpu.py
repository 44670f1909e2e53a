"""tests/known_answer.py checked before anything trusts it: its answers against the CPU oracle on the numpy-edited matrix, its mirror
of the two-level plan against hand-worked values, and its comparison against deliberately wrong answers."""
import random

import numpy as np
import pytest

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import known_answer as KA

B = KA.BLOCK_COLS


def _random_edits(rng, rows, cols, seed, nfree):
    """nfree free columns, about half of them XOR columns over untouched columns to their left, some folded first."""
    planted = O.planted_solution(cols, seed)
    free = sorted(rng.sample(range(1, cols), nfree))
    spec = []
    for c in free:
        if KA.planted_bit(planted, c):
            spec.append(KA.fold_col(c))
        pool = [s for s in range(c) if s not in free]
        if pool and rng.random() < .5:
            spec.append(KA.col_xor(c, rng.sample(pool, min(len(pool), rng.randint(1, 5)))))
        else:
            spec.append(KA.zero_col(c))
    return spec


def _case(kind, rows, cols, seed):
    rng = random.Random(f"{kind}-{rows}-{cols}-{seed}")
    planted = O.planted_solution(cols, seed)
    nb = (cols + B - 1) // B
    if kind == "full_rank":
        return []
    if kind == "zero_cols":                      # planted bit 0: no RHS change at all
        return [KA.zero_col(c) for c in KA.place_free_columns(rows, cols, seed, rng.sample(range(cols), 6))]
    if kind == "xor_cols":
        free = KA.place_free_columns(rows, cols, seed, sorted(rng.sample(range(cols // 2, cols), 4)))
        return [KA.col_xor(c, rng.sample([s for s in range(c) if s not in free], 3)) for c in free]
    if kind == "col0_last":
        return KA.free_columns(planted, [0, cols - 1])
    if kind == "block":                          # a whole block with no pivot, and the short last block besides
        b = rng.randrange(nb - 1)
        return KA.free_columns(planted, range(b * B, (b + 1) * B)) + KA.free_columns(planted, [(nb - 1) * B])
    if kind == "last_block":
        return KA.free_columns(planted, range((nb - 1) * B, cols))
    if kind == "rows":                           # zero rows, copies (a copy of a copy), free columns
        spec = _random_edits(rng, rows, cols, seed, 5)
        return spec + [KA.zero_row(rng.randrange(rows)) for _ in range(10)] + [KA.copy_row(3, 10), KA.copy_row(10, rows - 1),
                                                                                KA.copy_row(rng.randrange(rows), 4)]
    if kind == "head":                           # dead and duplicated head rows
        return [KA.zero_row(0), KA.zero_row(1)] + [KA.copy_row(100, j) for j in range(2, 6)] + _random_edits(rng, rows, cols, seed, 3)
    if kind == "inconsistent":                   # a copy with its RHS flipped
        return _random_edits(rng, rows, cols, seed, 4) + [KA.copy_row(rows - 1, 7), KA.flip_rhs(7)]
    if kind == "inconsistent_zero_row":          # 0 = 1
        return [KA.zero_row(rows // 2), KA.flip_rhs(rows // 2)]
    if kind == "flip_undone":                    # flipped twice, and a flipped row overwritten: consistent again
        return [KA.flip_rhs(5), KA.flip_rhs(5), KA.flip_rhs(9), KA.copy_row(12, 9), KA.flip_rhs(20), KA.zero_row(20)]
    if kind == "mixed":
        return _random_edits(rng, rows, cols, seed, rng.randint(8, 40)) + [KA.zero_row(rng.randrange(rows)) for _ in range(5)]
    raise ValueError(kind)


# (kind, rows, cols, seed): ragged and aligned column counts from 300 to 3000; rows >= cols + 64 + the rows an edit destroys
CASES = [
    ("full_rank", 364, 300, 1), ("full_rank", 1100, 1024, 2),
    ("zero_cols", 400, 300, 3), ("zero_cols", 1350, 1280, 4), ("zero_cols", 3100, 2999, 5),
    ("xor_cols", 600, 511, 6), ("xor_cols", 2200, 2048, 7), ("xor_cols", 3080, 3000, 8),
    ("col0_last", 400, 320, 9), ("col0_last", 1200, 1087, 10), ("col0_last", 2200, 2111, 11),
    ("block", 900, 768, 12), ("block", 1500, 1333, 13), ("block", 2700, 2560, 14),
    ("last_block", 1100, 1000, 15), ("last_block", 2200, 2049, 16),
    ("rows", 500, 300, 17), ("rows", 1400, 1300, 18), ("rows", 2700, 2600, 19),
    ("head", 800, 700, 20), ("head", 2200, 2100, 21),
    ("inconsistent", 720, 640, 22), ("inconsistent", 1900, 1801, 23), ("inconsistent_zero_row", 1200, 1100, 24),
    ("flip_undone", 1200, 1100, 25),
    ("mixed", 500, 400, 26), ("mixed", 1100, 999, 27), ("mixed", 1700, 1536, 28), ("mixed", 2600, 2500, 29),
    ("mixed", 3100, 3000, 30),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{k}-{r}x{c}" for k, r, c, _ in CASES])
def test_known_answer_equals_the_oracle(case):
    kind, rows, cols, seed = case
    spec = _case(kind, rows, cols, seed)
    aug = KA.apply_numpy(O.gen_synthetic(rows, cols, seed), cols, spec)
    want = KA.known_answer(rows, cols, seed, spec)
    assert want["status"] == (1 if kind.startswith("inconsistent") else 0)
    for mode in (0, 1):
        KA.assert_same(O.solve_words(aug, rows, cols, mode), want, mode)


def test_cases_cover_every_edit():
    ops, cols_hit = set(), set()
    for kind, rows, cols, seed in CASES:
        spec = _case(kind, rows, cols, seed)
        ops.update(op[0] for op in spec)
        cols_hit.update(("first" if op[1] == 0 else "last") for op in spec if op[0] == "zero_col" and op[1] in (0, cols - 1))
    assert ops == {"zero_col", "col_xor", "fold_col", "zero_row", "copy_row", "flip_rhs"} and cols_hit == {"first", "last"}


def test_planted_vector_and_placement():
    for cols, seed in ((300, 1), (1087, 31), (131072, 13)):
        planted = O.planted_solution(cols, seed)
        assert np.array_equal(planted, hip.planted_solution(cols, seed))
        got = KA.place_free_columns(cols + 64, cols, seed, [0, cols // 2, cols // 2, cols - 1])
        assert len(set(got)) == 4 and not any(KA.planted_bit(planted, c) for c in got)
        for w, c in zip([0, cols // 2, cols // 2, cols - 1], got):
            between = range(min(w, c), max(w, c))
            assert sum(1 for x in between if not KA.planted_bit(planted, x) and x not in got) <= 1     # nothing nearer was free
    with pytest.raises(AssertionError):
        KA.known_answer(400, 300, 1, [KA.zero_col(KA.place_free_columns(400, 300, 1, [10])[0])] * 2)      # a column twice
    one = next(c for c in range(300) if KA.planted_bit(O.planted_solution(300, 1), c))
    with pytest.raises(AssertionError):
        KA.known_answer(400, 300, 1, [KA.zero_col(one)])                        # solution bit 1, not folded
    with pytest.raises(AssertionError):
        KA.known_answer(400, 300, 1, [KA.col_xor(5, [6])])                     # a source right of the column
    with pytest.raises(AssertionError):
        KA.known_answer(364, 300, 1, [KA.zero_row(0)])                         # fewer than cols + 64 random rows left


def test_plan_two_level_mirror():
    # (rows, cols) -> (K, bend, nblocks).  wt = ceil((cols + 1) / 64) words, 4 panels of 64 columns per block; K = 12 from
    # rows * wt * 8 >= 3 GiB; bend = the last K-multiple m with (rows - 256 m) * (wt - 4 m) * 8 >= 512 MiB.
    assert KA.plan_two_level(66000, 65600) == (0, 0, 257)         # m = 8: 63952 * 994 * 8 = 508.6 MB < 536.9 MB
    assert KA.plan_two_level(65536, 65536) == (0, 0, 256)         # 63488 * 993 * 8 = 504.4 MB
    assert KA.plan_two_level(98704, 98267) == (8, 128, 384)       # m = 128: 65936 * 1024 * 8 = 540.0 MB; m = 136: 507.0 MB
    assert KA.plan_two_level(98304, 98304) == (8, 128, 384)       # 65536 * 1025 * 8 = 537.4 MB
    assert KA.plan_two_level(131472, 131072) == (8, 256, 512)     # 2.155 GB < 3 GiB; m = 256: 65936 * 1025 * 8 = 540.7 MB
    assert KA.plan_two_level(131072, 131072) == (8, 256, 512)
    assert KA.plan_two_level(197008, 196607) == (12, 504, 768)    # 4.84 GB; m = 504: 67984 * 1056 * 8 = 574.3 MB; m = 516: 523.4 MB
    assert KA.plan_two_level(262144, 262144) == (12, 768, 1024)   # m = 768: 65536 * 1025 * 8 = 537.4 MB
    assert KA.plan_two_level(327680, 327680) == (12, 1020, 1280)  # m = 1020: 66560 * 1041 * 8 = 554.3 MB; m = 1032: 504.4 MB
    assert KA.plan_two_level(32968, 32755) == (0, 0, 128)
    # K switches at 3 GiB: 181500 x 181500 holds 181500 * 2837 * 8 = 4.12 GB -> 12; 160000 x 160000: 160000 * 2501 * 8 = 3.20 GB < 3.22
    assert KA.plan_two_level(160000, 160000)[0] == 8 and KA.plan_two_level(181500, 181500)[0] == 12
    # no outer panel ends at the last block: 20M x 6144 (15.5 GB, 24 blocks, far above 0.5 GiB everywhere) stops at 12, one
    # more block and the second panel fits
    assert KA.plan_two_level(20000000, 6144) == (12, 12, 24)
    assert KA.plan_two_level(20000000, 6400) == (12, 24, 25)


def _perturbed(want, what):
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    b = got["basis"]
    if what == "status":
        got["status"] ^= 1
    elif what == "rank":
        got["rank"] -= 1
        got["pivcols"] = got["pivcols"][:-1]
    elif what == "pivots":
        got["pivcols"][3] += 1
    elif what == "origin":
        p = int(got["pivcols"][0])
        got["origin"][p >> 6] ^= np.uint64(1 << (p & 63))
    elif what == "dimension":
        got["dim"] += 1
    elif what == "basis_swap":
        b[[0, 1]] = b[[1, 0]]
    elif what == "basis_mix":                     # v_f ^ v_g for a free column g < f: still in the kernel, still top bit f
        b[2] ^= b[0]
    return got


@pytest.mark.parametrize("what,caught_by", [("status", "status"), ("rank", "rank"), ("pivots", "pivots"), ("origin", "origin"),
                                            ("dimension", "dimension"), ("basis_swap", "basis"), ("basis_mix", "basis")])
def test_a_wrong_answer_does_not_pass(what, caught_by):
    """Each assertion class of assert_same is needed: the oracle's answer, perturbed in one field, fails against the known answer at
    that field's own assertion (the ones before it pass)."""
    rows, cols, seed = 1100, 1000, 3
    planted = O.planted_solution(cols, seed)
    spec = KA.free_columns(planted, [200, 300, 640]) + KA.free_columns(planted, [900])[:-1] + [KA.col_xor(900, [10, 199, 641])]
    aug = KA.apply_numpy(O.gen_synthetic(rows, cols, seed), cols, spec)
    want = KA.known_answer(rows, cols, seed, spec)
    got = O.solve_words(aug, rows, cols, 1)
    KA.assert_same(got, want, 1)
    with pytest.raises(AssertionError, match=caught_by):
        KA.assert_same(_perturbed(got, what), want, 1)
