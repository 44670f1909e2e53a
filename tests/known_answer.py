"""Systems whose answer is known without a re-solve, at any size (helpers only, no tests here).

Start from a tall synthetic system (rows >= cols + 64: the columns nobody edits are independent with probability 1 - 2^-64) and
edit it so that the whole answer follows from the edits:

* ``zero_col(c)``           column c becomes zero: a free column, kernel vector e_c;
* ``col_xor(c, sources)``   column c becomes the XOR of the columns ``sources`` (all < c, never edited): a free column, kernel
                            vector e_c + sum e_s;
* ``fold_col(c)``           XOR column c into the RHS column: the solutions move by e_c.  Only needed to free a column whose
                            planted bit is 1 (before its edit), e.g. a whole block;
* ``zero_row(j)``, ``copy_row(i, j)`` (row i over row j, RHS included): never change the answer while enough random rows remain;
* ``flip_rhs(j)``           the system becomes inconsistent (every row agrees with the planted vector except this one).

The answer: pivots = every column except the edited ones, rank = cols - #free, origin = the planted vector (k_synth /
planted_solution) with the folded bits flipped -- zero at every free column, so the origin the contract asks for -- and the basis
in the order of the transposition replay (S4).  The same spec is applied by numpy to a host matrix and by torch to a device one.
"""
from __future__ import annotations

import numpy as np

from oracle import gf2_oracle as O

BLOCK_COLS = 256            # columns per block: GF2_GMAX = 4 panels of 64


def zero_col(c):
    return ("zero_col", int(c))


def col_xor(c, sources):
    return ("col_xor", int(c), tuple(int(s) for s in sources))


def fold_col(c):
    return ("fold_col", int(c))


def zero_row(j):
    return ("zero_row", int(j))


def copy_row(i, j):
    return ("copy_row", int(i), int(j))


def flip_rhs(j):
    return ("flip_rhs", int(j))


def planted_bit(planted: np.ndarray, c: int) -> int:
    return (int(planted[c >> 6]) >> (c & 63)) & 1


def free_columns(planted: np.ndarray, columns) -> list:
    """Spec that zeroes exactly `columns`, folding first every one whose planted bit is 1."""
    spec = []
    for c in columns:
        if planted_bit(planted, c):
            spec.append(fold_col(c))
        spec.append(zero_col(c))
    return spec


def place_free_columns(rows: int, cols: int, seed: int, wanted) -> list:
    """Each wanted position moved to the nearest column whose planted bit is 0 (the lower one on a tie), no column twice: columns
    that can be zeroed or overwritten without touching the RHS.  (`rows` does not enter: the planted vector depends on cols.)"""
    planted = O.planted_solution(cols, seed)
    taken, out = set(), []
    for w in wanted:
        for d in range(cols):
            hit = next((c for c in (w - d, w + d) if 0 <= c < cols and c not in taken and not planted_bit(planted, c)), None)
            if hit is not None:
                break
        else:
            raise ValueError(f"no column with planted bit 0 near {w}")
        taken.add(hit)
        out.append(hit)
    return out


def plan_two_level(rows: int, cols: int):
    """Python mirror of plan_two_level in gf2bv_amd/csrc/gf2_solver.hip (the natural plan of a single system on one GPU: no
    GF2BV_TWO_LEVEL / GF2BV_TWO_LEVEL_MIN_MIB).  G = 4 panels per block; K = GF2_KMAX = 12 blocks per outer panel when the matrix
    holds 3 GiB or more, 8 below; outer panels end before the first one after which less than 0.5 GiB remains right of and below
    it, and never at the last block.  Returns (K, bend, nblocks): blocks [0, bend) run in outer panels of K, (0, 0, nblocks) when
    the plan is one-level.  Gangs (nsys > 1) are always one-level."""
    G, kmax = 4, 12
    wt = (cols + 1 + 63) // 64
    nblocks = ((cols + 63) // 64 + G - 1) // G
    K = kmax if rows * wt * 8 >= 3 << 30 else 8
    bend, b0 = 0, 0
    while b0 + K < nblocks:
        rows_left, words_left = rows - (b0 + K) * 64 * G, wt - (b0 + K) * G
        if (b0 + K) * 64 * G > cols or rows_left <= 0 or words_left <= 0:
            break
        if rows_left * words_left * 8 < 1 << 29:
            break
        bend = b0 + K
        b0 += K
    return (K, bend, nblocks) if bend else (0, 0, nblocks)


def _check_spec(rows: int, cols: int, spec):
    edited, sources, lost_rows = {}, set(), set()
    for op in spec:
        kind = op[0]
        if kind in ("zero_col", "col_xor", "fold_col"):
            c = op[1]
            assert 0 <= c < cols, op
            assert c not in edited, f"column {c} edited before {op}"
            if kind == "fold_col":
                continue
            if kind == "col_xor":
                assert op[2] and all(0 <= s < c and s not in edited for s in op[2]), op
                sources.update(op[2])
            edited[c] = op
        else:
            assert all(0 <= j < rows for j in op[1:]), op
            if kind in ("zero_row", "copy_row"):
                lost_rows.add(op[-1])
    assert not sources & set(edited), "a source column is edited"
    assert rows - len(lost_rows) >= cols + 64, "too few random rows left for the untouched columns to be independent"
    return edited


def known_answer(rows: int, cols: int, seed: int, spec) -> dict:
    """The answer to O.gen_synthetic(rows, cols, seed) edited by `spec`, in the keys and shapes of O.solve_words (what assert_same
    compares).  Nothing here solves anything."""
    edited = _check_spec(rows, cols, spec)
    origin = O.planted_solution(cols, seed).copy()
    rhs_off = {}
    for op in spec:
        kind = op[0]
        if kind == "fold_col":
            origin[op[1] >> 6] ^= np.uint64(1 << (op[1] & 63))
        elif kind in ("zero_col", "col_xor"):
            assert not planted_bit(origin, op[1]), f"column {op[1]} has solution bit 1 when it is edited: fold it first"
        elif kind == "zero_row":
            rhs_off.pop(op[1], None)
        elif kind == "copy_row":
            if rhs_off.get(op[1]):
                rhs_off[op[2]] = 1
            else:
                rhs_off.pop(op[2], None)
        elif kind == "flip_rhs":
            rhs_off[op[1]] = rhs_off.get(op[1], 0) ^ 1
    status = 1 if any(rhs_off.values()) else 0
    free = sorted(edited)
    piv = np.setdiff1d(np.arange(cols, dtype=np.int32), np.array(free, dtype=np.int32)).astype(np.int32)
    rank = len(piv)
    order = list(range(cols))                        # S4: the free columns in the order of the transposition replay
    for i, c in enumerate(piv.tolist()):
        order[i], order[c] = order[c], order[i]
    cw = (cols + 63) // 64
    basis = np.zeros((cols - rank, cw), dtype=np.uint64)
    for t, f in enumerate(order[rank:]):
        op = edited[f]
        for c in (f,) + (op[2] if op[0] == "col_xor" else ()):
            basis[t, c >> 6] ^= np.uint64(1 << (c & 63))
    return {"status": status, "rank": rank, "dim": cols - rank, "pivcols": piv, "origin": origin, "basis": basis}


def _fields(got):
    if isinstance(got, dict):
        return got["status"], got["rank"], got["dim"], np.asarray(got["pivcols"])[: got["rank"]], got["origin"], got["basis"]
    return got.status, got.rank, got.dimension, got.pivots, got.origin, got.basis


def assert_same(got, want: dict, mode: int):
    """Every field the contract fixes: status, rank and pivots always; origin when solvable; dimension and the basis IN ORDER in
    mode 1.  `got` is a hip.Solution or an O.solve_words dict."""
    status, rank, dim, piv, origin, basis = _fields(got)
    assert status == want["status"], f"status {status} != {want['status']}"
    assert rank == want["rank"], f"rank {rank} != {want['rank']}"
    assert np.array_equal(piv, want["pivcols"]), "pivots differ"
    if want["status"] == 0:
        assert np.array_equal(origin, want["origin"]), "origin differs"
        if mode == 1:
            assert dim == want["dim"], f"dimension {dim} != {want['dim']}"
            assert np.array_equal(np.asarray(basis).reshape(-1, want["basis"].shape[1]), want["basis"]), "basis differs"


def apply_numpy(aug: np.ndarray, cols: int, spec) -> np.ndarray:
    """Apply `spec` in place to a host uint64 matrix (rows x stride words, bit c of a row = column c, bit `cols` = RHS)."""
    rw, rb = cols >> 6, np.uint64(cols & 63)
    one = np.uint64(1)

    def col(c):
        return (aug[:, c >> 6] >> np.uint64(c & 63)) & one

    for op in spec:
        kind = op[0]
        if kind == "zero_col":
            aug[:, op[1] >> 6] &= ~np.uint64(1 << (op[1] & 63))
        elif kind == "col_xor":
            c = op[1]
            bit = np.zeros(aug.shape[0], dtype=np.uint64)
            for s in op[2]:
                bit ^= col(s)
            aug[:, c >> 6] = (aug[:, c >> 6] & ~np.uint64(1 << (c & 63))) | (bit << np.uint64(c & 63))
        elif kind == "fold_col":
            aug[:, rw] ^= col(op[1]) << rb
        elif kind == "zero_row":
            aug[op[1], :] = 0
        elif kind == "copy_row":
            aug[op[2], :] = aug[op[1], :]
        elif kind == "flip_rhs":
            aug[op[1], rw] ^= np.uint64(1 << (cols & 63))
        else:
            raise ValueError(op)
    return aug


def _mask(k: int) -> int:
    """1 << k as the int64 bit pattern torch stores (bit 63 wraps to the negative)."""
    v = 1 << k
    return v - (1 << 64) if k == 63 else v


def apply_torch(t, cols: int, spec):
    """Apply `spec` in place to a device int64 tensor (rows x stride words, same layout as apply_numpy)."""
    rw, rm = cols >> 6, _mask(cols & 63)

    def col(c):
        return (t[:, c >> 6] >> (c & 63)) & 1       # (arithmetic shift: the & 1 keeps bit 63 right)

    for op in spec:
        kind = op[0]
        if kind == "zero_col":
            t[:, op[1] >> 6] &= ~_mask(op[1] & 63)
        elif kind == "col_xor":
            c = op[1]
            bit = col(op[2][0])
            for s in op[2][1:]:
                bit ^= col(s)
            t[:, c >> 6] = (t[:, c >> 6] & ~_mask(c & 63)) | (bit * _mask(c & 63))
        elif kind == "fold_col":
            t[:, rw] ^= col(op[1]) * rm
        elif kind == "zero_row":
            t[op[1]] = 0
        elif kind == "copy_row":
            t[op[2]] = t[op[1]]
        elif kind == "flip_rhs":
            t[op[1], rw] ^= rm
        else:
            raise ValueError(op)
    return t
