"""Substitution and iteration of affine maps on the GPU: ``substitute`` and ``power``.

A model stepped symbolically gives the bits of its next state as ``PackedBitVec``s over the unknowns of a ``PackedLinearSystem``:
an affine MAP, one image row per unknown.  ``substitute(exprs, images)`` replaces every unknown of ``exprs`` by its image -- one
GF(2) matrix product on the device (k_compose) -- and ``power(images, k)`` substitutes a self-map into itself k times by
square-and-multiply there, for k that nobody can step through: outputs observed far apart, a generator that was jumped between
captures, "the state after k steps".  The result is again PackedBitVecs, so it goes into ``solve_one`` like any stepped state.

Functions, not methods: the public names of the system classes are fixed.  Linear (affine) forms only; one device.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from ._internal import m4ri_compose_packed, m4ri_power_packed, m4ri_unroll_packed
from .bitvec import BitVec
from .packed import PackedBitVec, _TermsBitVec


def _exponent_words(k) -> np.ndarray:
    """k as little-endian uint64 words, at least one: what the library's power entries read"""
    k = int(k)
    if k < 0:
        raise ValueError("the exponent of power must not be negative")
    nw = max(1, (k.bit_length() + 63) // 64)
    return np.frombuffer(k.to_bytes(8 * nw, "little"), dtype=np.uint64).copy()


def _rows_of(v, what: str) -> np.ndarray:
    if isinstance(v, _TermsBitVec):
        raise TypeError(f"{what}: substitution into products is not linear (a {type(v).__name__} carries products)")
    if isinstance(v, PackedBitVec):
        return v._rows
    if isinstance(v, BitVec):
        raise TypeError(f"{what}: a tuple-of-int BitVec cannot be substituted, use the PackedBitVecs of a PackedLinearSystem")
    raise TypeError(f"{what}: PackedBitVec expected, not {type(v).__name__}")


def _image_rows(images: Sequence) -> tuple:
    """(widths, the n image rows as one [n, Wb] array)"""
    if isinstance(images, BitVec) or isinstance(images, _TermsBitVec):
        images = (images,)
    parts = [_rows_of(v, "images") for v in images]
    if not parts or not sum(len(p) for p in parts):
        raise ValueError("images must hold at least one bit")
    if len({p.shape[1] for p in parts}) != 1:
        raise ValueError("images: Cannot mix bitvecs over different numbers of unknowns")
    return [len(p) for p in parts], np.ascontiguousarray(np.concatenate(parts))


def _split(rows: np.ndarray, widths: Sequence[int]) -> tuple:
    out, at = [], 0
    for w in widths:
        out.append(PackedBitVec(rows[at:at + w]))
        at += w
    return tuple(out)


def substitute(exprs, images: Sequence, device=None):
    """``exprs`` (a PackedBitVec or a sequence of them, over n unknowns) with unknown g replaced by the g-th bit of ``images`` (a
    sequence of PackedBitVecs whose lengths add up to n, one per generator, as a model's next state comes).  Returns the same
    structure -- one vector in, one out; a sequence in, a tuple out -- over the unknowns of ``images``."""
    single = isinstance(exprs, (BitVec, _TermsBitVec))
    eparts = [_rows_of(v, "exprs") for v in ((exprs,) if single else exprs)]
    _, b = _image_rows(images)
    n, wb = len(b), b.shape[1]
    wa = (n + 1 + 63) // 64
    for p in eparts:
        if p.shape[1] != wa:
            raise ValueError(f"exprs are {p.shape[1]} words wide, forms over the {n} unknowns that images replace are {wa}")
    ewidths = [len(p) for p in eparts]
    a = np.ascontiguousarray(np.concatenate(eparts)) if eparts else np.zeros((0, wa), dtype=np.uint64)
    # (the images' own width: the largest number of unknowns their words can hold -- bits past the system's last unknown are zero)
    nb = 64 * wb - 1
    args = (a, len(a), n, b, nb) + (() if device is None else (device,))
    rows = np.frombuffer(m4ri_compose_packed(*args), dtype=np.uint64).reshape(len(a), wb)
    out = _split(rows, ewidths)
    return out[0] if single else out


def power(images: Sequence, k: int, device=None) -> tuple:
    """The self-map ``images`` (n bits over n unknowns) substituted into itself k times: ``power(images, 0)`` is the identity map,
    ``power(images, 1)`` is ``images``.  k is any non-negative int.  Returns a tuple of PackedBitVecs with the widths of ``images``."""
    widths, b = _image_rows(images)
    n = len(b)
    if b.shape[1] != (n + 1 + 63) // 64:
        raise ValueError(f"power needs a square map: {n} image bits are over forms of {b.shape[1]} words, not of {(n + 1 + 63) // 64}")
    kw = _exponent_words(k)
    args = (b, n, kw) + (() if device is None else (device,))
    rows = np.frombuffer(m4ri_power_packed(*args), dtype=np.uint64).reshape(n, b.shape[1])
    return _split(rows, widths)


def unroll(exprs, images: Sequence, count: int, *, start: int = 0, step: int = 1, device=None) -> list:
    """The bits ``exprs`` (a PackedBitVec or a sequence of them, over the n unknowns of the self-map ``images``) watched while the model
    steps: a list of ``count`` items, item i = ``substitute(exprs, power(images, start + i * step))`` with the structure of ``exprs`` -- the
    whole "step the symbolic model, read the taps" loop as ceil(log2 count) doublings on the device.  The items are views into one array."""
    single = isinstance(exprs, (BitVec, _TermsBitVec))
    eparts = [_rows_of(v, "exprs") for v in ((exprs,) if single else exprs)]
    _, b = _image_rows(images)
    n, w = len(b), b.shape[1]
    if w != (n + 1 + 63) // 64:
        raise ValueError(f"unroll needs a square map: {n} image bits are over forms of {w} words, not of {(n + 1 + 63) // 64}")
    for p in eparts:
        if p.shape[1] != w:
            raise ValueError(f"exprs are {p.shape[1]} words wide, forms over the {n} unknowns that images replace are {w}")
    count, start, step = int(count), int(start), int(step)
    if count < 0 or start < 0:
        raise ValueError("count and start of unroll must not be negative")
    if step < 1:
        raise ValueError("step of unroll must be at least 1")
    if count == 0:
        return []
    ewidths = [len(p) for p in eparts]
    a = np.ascontiguousarray(np.concatenate(eparts)) if eparts else np.zeros((0, w), dtype=np.uint64)
    args = (a, len(a), n, b, _exponent_words(start), _exponent_words(step), count) + (() if device is None else (device,))
    rows = np.frombuffer(m4ri_unroll_packed(*args), dtype=np.uint64).reshape(count, len(a), w)
    items = [_split(rows[i], ewidths) for i in range(count)]
    return [it[0] for it in items] if single else items
