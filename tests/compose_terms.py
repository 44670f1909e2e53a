"""Host twin of the composition entries (gf2bv_compose_*), written from their meaning with numpy: unpack the bits of a form, XOR-reduce
the rows of B~ they select.  No table, no tile, no slice: nothing is shared with k_compose.  Forms are uint64 rows in the
equation-int order (bit 0 the constant, bit 1 + g unknown g); ``images`` has one row per unknown."""
from __future__ import annotations

import numpy as np


def form_words(unknowns: int) -> int:
    return (unknowns + 1 + 63) // 64


def bits_of(rows: np.ndarray, nbits: int) -> np.ndarray:
    """[r, W] uint64 -> [r, nbits] uint8 of 0 / 1, bit k of a row at column k"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return np.unpackbits(rows.view(np.uint8).reshape(len(rows), -1), axis=1, bitorder="little")[:, :nbits]


def words_of(bits: np.ndarray, words: int) -> np.ndarray:
    """[r, nbits] of 0 / 1 -> [r, words] uint64"""
    full = np.zeros((len(bits), 64 * words), dtype=np.uint8)
    full[:, :bits.shape[1]] = bits
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(len(bits), words)


def with_unit(images: np.ndarray, nb: int) -> np.ndarray:
    """B~ as bits: [n + 1, nb + 1], row 0 the unit form, row 1 + g the image of unknown g cut to its nb + 1 bits"""
    b = bits_of(images, nb + 1)
    unit = np.zeros((1, nb + 1), dtype=np.uint8)
    unit[0, 0] = 1
    return np.concatenate([unit, b])


def substitute(a: np.ndarray, n: int, images: np.ndarray, nb: int, stride: int | None = None) -> np.ndarray:
    """the forms `a` over n unknowns with the n `images` over nb unknowns substituted: [len(a), stride] uint64"""
    assert len(images) == n
    sel = bits_of(a, n + 1)                                 # bits above n are ignored
    bt = with_unit(images, nb)
    out = np.zeros((len(a), nb + 1), dtype=np.uint8)
    for r in range(len(a)):
        picked = bt[sel[r].astype(bool)]
        if len(picked):
            out[r] = np.bitwise_xor.reduce(picked, axis=0)
    return words_of(out, form_words(nb) if stride is None else stride)


def identity(n: int) -> np.ndarray:
    """image g = unknown g"""
    bits = np.zeros((n, n + 1), dtype=np.uint8)
    bits[np.arange(n), 1 + np.arange(n)] = 1
    return words_of(bits, form_words(n))


def power_loop(images: np.ndarray, n: int, k: int) -> np.ndarray:
    """`images` substituted into itself k times, one substitution after the other"""
    cur = identity(n)
    for _ in range(k):
        cur = substitute(cur, n, images, n)
    return cur


def power(images: np.ndarray, n: int, k: int) -> np.ndarray:
    """the same for any k, by the twin's own squaring (least significant bit first: not the library's order)"""
    result, sq = identity(n), substitute(identity(n), n, images, n)
    while k:
        if k & 1:
            result = substitute(result, n, sq, n)
        k >>= 1
        if k:
            sq = substitute(sq, n, sq, n)
    return result


def evaluate(images: np.ndarray, n: int, x: int) -> int:
    """the map at the point x (bit g = unknown g): bit g of the result = image g at x"""
    point = bits_of(np.frombuffer((((x & ((1 << n) - 1)) << 1) | 1).to_bytes(8 * form_words(n), "little"), dtype=np.uint64)[None, :], n + 1)[0]
    par = (bits_of(images, n + 1) & point[None, :]).sum(axis=1) & 1
    return int(sum(int(b) << g for g, b in enumerate(par)))


def int_rows(rows: np.ndarray) -> list:
    """the rows as Python ints (equation ints)"""
    return [int.from_bytes(np.ascontiguousarray(r).tobytes(), "little") for r in rows]


def rows_of_ints(values, words: int) -> np.ndarray:
    return np.array([np.frombuffer(int(v).to_bytes(8 * words, "little"), dtype=np.uint64) for v in values], dtype=np.uint64).reshape(len(values), words)


def substitute_ints(a: list, n: int, images: list) -> list:
    """Python-int arithmetic, bit by bit: the check of the twin itself"""
    out = []
    for f in a:
        acc = f & 1
        for g in range(n):
            if (f >> (1 + g)) & 1:
                acc ^= images[g]
        out.append(acc)
    return out
