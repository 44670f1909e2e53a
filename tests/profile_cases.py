"""Column rank profiles with holes (helpers and the case table only, no tests here).

Every rank-deficient system of tests/systems.random_system(rank_cap=...) has its pivots in columns 0 .. cap-1: pivot r of a panel sits
at column bit r, and a pivot's rank index differs from its column by a constant.  The systems here put MANY free columns between pivot
columns -- inside words, panels, blocks and back-substitution groups -- and make every one of them a dense combination of the unedited
columns to its left (tests/known_answer.col_xor with a source set of about half of them), so that every entry of U in a free column and
every kernel vector is dense.  The whole answer still follows from the edits (tests/known_answer.known_answer): nothing is solved here.

    dense_profile(rows, cols, seed, free)   the spec
    apply_fast(aug, cols, spec)             the spec applied with one matrix product (equal to KA.apply_numpy word for word); `aug` may be
                                            a range of rows of the system
    case(name)                              a built, cached case: shape, spec, free set, matrix and known answer
    append_pair()                           a handle A and rows B whose stack has fewer holes than A
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple

import numpy as np

from oracle import gf2_oracle as O
from tests import known_answer as KA

PANEL = 64
B = KA.BLOCK_COLS
COLUMN_OPS = ("zero_col", "col_xor", "fold_col")


def dense_profile(rows: int, cols: int, seed: int, free, density: float = .5, rng: random.Random | None = None) -> list:
    """Spec that frees exactly the columns `free` of O.gen_synthetic(rows, cols, seed): column c becomes the XOR of S_c, a seeded
    random subset (each column with probability `density`) of the never-edited columns below c; column 0, and a column whose draw is
    empty, becomes zero.  A column whose planted bit is 1 is folded into the RHS first.  (`rows` does not enter.)"""
    rng = rng or random.Random(f"dense_profile-{cols}-{seed}")
    planted = O.planted_solution(cols, seed)
    free = sorted(set(int(c) for c in free))
    assert free == [] or (0 <= free[0] and free[-1] < cols)
    is_free = set(free)
    spec = []
    for c in free:
        if KA.planted_bit(planted, c):
            spec.append(KA.fold_col(c))
        sources = [s for s in range(c) if s not in is_free and rng.random() < density]
        spec.append(KA.col_xor(c, sources) if sources else KA.zero_col(c))
    return spec


def unpack_bits(words: np.ndarray, nbits: int) -> np.ndarray:
    """rows x words uint64 -> rows x nbits 0/1 (uint8), bit c of a row = column c"""
    by = np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :nbits]


def pack_bits(bits: np.ndarray, words: int) -> np.ndarray:
    padded = np.zeros((bits.shape[0], words * 64), dtype=np.uint8)
    padded[:, :bits.shape[1]] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(bits.shape[0], words)


def apply_fast(aug: np.ndarray, cols: int, spec) -> np.ndarray:
    """KA.apply_numpy for specs of many large col_xor: the column edits of `spec` as ONE product over GF(2) -- the rows unpacked to 0/1,
    the free columns set to (A[:, sources] @ S) & 1, the folded columns added to the RHS, packed again -- and the row edits, which
    commute with them, through KA.apply_numpy afterwards.  Column edits act on each row alone, so `aug` may be any range of rows of a
    system (then `spec` holds no row edit).  Returns a new array.  (float32 sums of at most `cols` ones are exact: cols < 2^24.)"""
    assert cols < 1 << 24
    stride = aug.shape[1]
    bits = unpack_bits(aug, cols + 1)
    orig = bits.astype(np.float32)
    edits = [op for op in spec if op[0] in ("zero_col", "col_xor")]
    folds = [op[1] for op in spec if op[0] == "fold_col"]
    if edits:
        S = np.zeros((cols, len(edits)), dtype=np.float32)
        for t, op in enumerate(edits):
            if op[0] == "col_xor":
                S[list(op[2]), t] = 1
        bits[:, [op[1] for op in edits]] = (orig[:, :cols] @ S).astype(np.int64) & 1
    if folds:
        bits[:, cols] ^= (orig[:, folds].sum(axis=1).astype(np.int64) & 1).astype(np.uint8)
    out = np.zeros_like(aug)
    out[:, :O.words_for(cols)] = pack_bits(bits, O.words_for(cols))
    assert stride >= O.words_for(cols)
    return KA.apply_numpy(out, cols, [op for op in spec if op[0] not in COLUMN_OPS])


def panel_masks(pivcols, cols: int) -> list:
    """per panel of 64 columns, the pivots as a 64-bit mask (bit b = column 64 * panel + b is a pivot)"""
    masks = [0] * ((cols + PANEL - 1) // PANEL)
    for c in np.asarray(pivcols).tolist():
        masks[c >> 6] |= 1 << (c & 63)
    return masks


def full_mask(panel: int, cols: int) -> int:
    return (1 << min(PANEL, cols - panel * PANEL)) - 1


# -- the case table ---------------------------------------------------------------------------------------------------------------------------
def _spread(n: int, cols: int) -> list:
    """n columns at equal distances over all panels, none at bit 0 or 63 of its word next to another one: single holes inside words"""
    return [5 + (i * (cols - 12)) // (n - 1) for i in range(n)]


def _last_word(cols: int) -> list:
    return sorted({0, (cols - 1) // PANEL * PANEL, cols - 2, cols - 1})


_SMALL = list(range(PANEL, 2 * PANEL, 3)) + [PANEL - 1, 2 * PANEL]          # every 3rd column of panel 1, bit 63 of panel 0, bit 0 of panel 2
_FIFTH_2500 = list(range(300, 2500, 5))
_FIFTH_1300 = list(range(300, 1300, 5))
_INCONSISTENT = [KA.copy_row(50, 3), KA.flip_rhs(3)]

# name -> (rows, cols, seed, free columns, row edits behind the column edits)
TABLE = {
    "alternate": (1500, 1300, 101, list(range(B + 1, 2 * B, 2)), []),                       # every odd column of block 1
    "edges": (1500, 1300, 102, list(range(513, 576)) + list(range(576, 639)) + [640, 767], []),  # block 2: pivots bit 0 / bit 63 / all but bit 0 / all but bit 63
    "panel_free": (1500, 1300, 103, list(range(6 * PANEL, 7 * PANEL)), []),
    "block_free": (2700, 2500, 104, list(range(4 * B, 5 * B)), []),
    "every_5th": (2700, 2500, 105, _FIFTH_2500, []),
    # both sides of the boundary between the back-substitution groups of 16 panels (column 1024), bit 0 of panel 15, bit 63 of panel 16
    # and five single holes in panels 2, 5, 7, 9 and 12
    "group_edge": (1500, 1300, 106, list(range(1010, 1031)) + [960, 1087] + [150, 333, 470, 615, 800], []),
    **{f"dim_{n}": (1500, 1300, 110 + n, _spread(n, 1300), []) for n in (7, 8, 9, 63, 64, 65)},
    **{f"last_word_{c}": (c + 200, c, 200 + c % 64, _last_word(c), []) for c in (1217, 1279, 1280)},
    "small_300x200": (300, 200, 301, _SMALL, []),
    "small_905x831": (905, 831, 302, _SMALL + [830], []),
    "inconsistent": (2700, 2500, 105, _FIFTH_2500, _INCONSISTENT),
    "inconsistent_1300": (1500, 1300, 107, _FIFTH_1300, _INCONSISTENT),                    # (the gang's member: `inconsistent` at the gang's shape)
}
NAMES = [n for n in TABLE if n != "inconsistent_1300"]          # the single-system legs
GANG = ("alternate", "edges", "panel_free", "group_edge", "inconsistent_1300")
DIMS = {f"dim_{n}": n for n in (7, 8, 9, 63, 64, 65)}

# what each case is named for: name -> {panel: pivot mask}; every panel that is not listed is full
ALL = (1 << 64) - 1
MASKS = {
    "alternate": {p: 0x5555555555555555 for p in (4, 5, 6, 7)},
    "edges": {8: 1, 9: 1 << 63, 10: ALL & ~1, 11: ALL & ~(1 << 63)},
    "panel_free": {6: 0},
    "block_free": {p: 0 for p in (16, 17, 18, 19)},
}

Case = namedtuple("Case", "name rows cols seed free spec aug want")


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    """The built case (once per process): `aug` is rows x words_for(cols) and read-only, `want` the known answer."""
    rows, cols, seed, free, row_edits = TABLE[name]
    spec = dense_profile(rows, cols, seed, free) + list(row_edits)
    aug = apply_fast(O.gen_synthetic(rows, cols, seed), cols, spec)
    aug.setflags(write=False)
    want = KA.known_answer(rows, cols, seed, spec)
    assert want["dim"] == len(set(free)) and want["status"] == (1 if row_edits else 0)
    return Case(name, rows, cols, seed, sorted(set(free)), spec, aug, want)


# -- the append pair --------------------------------------------------------------------------------------------------------------------------
Pair = namedtuple("Pair", "rows_a rows cols seed free1 free2 a b stacked want")


@functools.lru_cache(maxsize=None)
def append_pair(rows_a: int = 1100) -> Pair:
    """On the shape and free set F1 of `alternate`: A = the first rows_a rows under F1's spec, B = the rows behind them with the
    fold_col of all of F1 but the col_xor of F2 only (20 columns of F1, the same source sets).  In B the columns of F1 - F2 are random,
    so the stack [A; B] has free set F2, A's origin (the planted vector, zero at all of F1) and F2's kernel vectors: `want`, the known
    answer of the spec B was built with."""
    rows, cols, seed, free1, _ = TABLE["alternate"]
    spec1 = dense_profile(rows, cols, seed, free1)
    free2 = set(random.Random("append_pair").sample(sorted(free1), 20))
    spec2 = [op for op in spec1 if op[0] == "fold_col" or op[1] in free2]
    raw = O.gen_synthetic(rows, cols, seed)
    a, b = apply_fast(raw[:rows_a], cols, spec1), apply_fast(raw[rows_a:], cols, spec2)
    stacked = np.vstack([a, b])
    for x in (a, b, stacked):
        x.setflags(write=False)
    return Pair(rows_a, rows, cols, seed, sorted(free1), sorted(free2), a, b, stacked, KA.known_answer(rows, cols, seed, spec2))


# -- right-hand sides ------------------------------------------------------------------------------------------------------------------------
NRHS = (1, 9, 65)                     # either side of GF2_BSV = 8 and of GF2_BS_MAXRHS = 64
BAD_RHS = (1, 8)                      # the two inconsistent ones: in the calls with 9 and with 65 right-hand sides


@functools.lru_cache(maxsize=None)
def rhs_bits(name: str, nrhs: int = max(NRHS)) -> np.ndarray:
    """nrhs x rows 0/1: b = A x for random x; numbers BAD_RHS with the bit of one row flipped (the systems have at least 200 rows more
    than rank, each a combination of the others: the flipped bit contradicts them; tests/test_profile_cases_cpu.py has the oracle confirm it)"""
    c = case(name)
    rng = np.random.default_rng(c.seed)
    A = unpack_bits(c.aug, c.cols).astype(np.float32)
    x = rng.integers(0, 2, size=(c.cols, nrhs)).astype(np.float32)
    bits = ((A @ x).astype(np.int64) & 1).astype(np.uint8).T.copy()
    for j in BAD_RHS:
        bits[j, 11 * (j + 1)] ^= 1
    bits.setflags(write=False)
    return bits


def with_rhs(aug: np.ndarray, cols: int, b: np.ndarray) -> np.ndarray:
    a = aug.copy()
    w, bit = cols // 64, np.uint64(cols % 64)
    a[:, w] = (a[:, w] & ~(np.uint64(1) << bit)) | (b.astype(np.uint64) << bit)
    return a


def rhs_words(bits: np.ndarray) -> np.ndarray:
    """nrhs x rows 0/1 -> nrhs x ceil(rows / 64) uint64, bit r of row j = bits[j, r]"""
    return pack_bits(bits, (bits.shape[1] + 63) // 64)


@functools.lru_cache(maxsize=None)
def rhs_oracle(name: str) -> tuple:
    """the CPU oracle's mode-1 answer for every right-hand side of rhs_bits(name) (mode 0 compares a part of it)"""
    c = case(name)
    return tuple(O.solve_words(with_rhs(c.aug, c.cols, b), c.rows, c.cols, 1) for b in rhs_bits(name))
