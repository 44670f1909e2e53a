"""FactoredSystem: one coefficient matrix factored once, instances solved against it later (no counterpart in the reference).

``LinearSystem.factor(exprs)`` / ``QuadraticSystem.factor(exprs)`` flatten the expressions once and factor their coefficient
matrix on the GPU (``_internal.m4ri_factor`` -> ``gf2bv_factor_digits``).  An instance is a list of observed values, one per
expression; each method equals the matching ``LinearSystem`` method on ``[e ^ v for e, v in zip(exprs, values)]``.  The
right-hand-side words of a batch are built with numpy from spans kept as arrays: bit r of instance i = the constant term of
equation r xor the bit of values[i][k] that equation r of expression k stands for.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from ._internal import m4ri_factor
from .bitvec import BitVec


class FactoredSystem:
    def __init__(self, system, exprs, device=None):
        from .linsys import QuadraticSystem          # noqa: PLC0415  (linsys imports this module lazily)
        self._system = system
        self._quadratic = isinstance(system, QuadraticSystem)
        self._device = device
        eqs: list = []
        span_at, span_width = [], []                 # per expression: first row, width (0: an equation int, value 0 / 1)
        for e in exprs:
            span_at.append(len(eqs))
            if isinstance(e, BitVec):
                span_width.append(len(e._bits))
                eqs.extend(e._bits)
            else:
                span_width.append(0)
                eqs.append(e)
        self._nspans = len(span_at)
        if len(eqs) < system._cols:                  # the boundary wants rows >= cols (zero rows, constant 0 in every instance)
            eqs.extend([0] * (system._cols - len(eqs)))
        self._eqs = eqs
        self.rows = len(eqs)
        self._rw = (self.rows + 63) // 64
        self._width = np.array(span_width, dtype=np.int64)
        # every row that belongs to an expression: which 64-bit chunk of which value it reads, and which bit of it
        row_span = np.repeat(np.arange(self._nspans), np.maximum(self._width, 1))
        offs = np.arange(len(row_span)) - np.repeat(np.array(span_at, dtype=np.int64), np.maximum(self._width, 1))
        self._nchunks = np.maximum(1, (self._width + 63) // 64)
        first_chunk = np.concatenate(([0], np.cumsum(self._nchunks)[:-1])).astype(np.int64)
        self._row_col = first_chunk[row_span] + offs // 64        # column of the chunk matrix built per call
        self._row_bit = (offs % 64).astype(np.uint64)
        self._nexpr_rows = len(row_span)
        consts = np.zeros(self._rw * 64, dtype=np.uint8)
        consts[:len(eqs)] = [e & 1 for e in eqs]
        self._consts = np.packbits(consts, bitorder="little").view(np.uint64)
        self._handles = {}

    # -- right-hand sides ------------------------------------------------------------------------------------------------
    def _chunks(self, values_list: Sequence[Sequence[int]]) -> np.ndarray:
        """[n, total chunks] uint64: chunk c of expression k = bits 64c .. 64c + 63 of the low `width` bits of |value|
        (BitVec.__xor__ with an int: to_bits of |v|); an equation int takes its value (0 / 1) as is."""
        n = len(values_list)
        for vals in values_list:
            if len(vals) != self._nspans:
                raise ValueError(f"{len(vals)} values for {self._nspans} expressions")
        if n == 0:
            return np.zeros((0, int(self._nchunks.sum())), dtype=np.uint64)
        simple = bool((self._width <= 64).all())
        V = None
        if simple:
            try:
                V = np.array(values_list, dtype=np.uint64).reshape(n, self._nspans)
            except (OverflowError, ValueError, TypeError):
                V = None
        if V is None:                                # negative or wider than 64 bits: chunk by chunk through Python ints
            cols = []
            for k in range(self._nspans):
                w = int(self._width[k])
                for c in range(int(self._nchunks[k])):
                    col = []
                    for vals in values_list:
                        v = int(vals[k])
                        if w == 0:
                            if v not in (0, 1):
                                raise ValueError("the value of an equation int must be 0 or 1")
                            col.append(v)
                        else:
                            col.append(((abs(v) & ((1 << w) - 1)) >> (64 * c)) & 0xFFFFFFFFFFFFFFFF)
                    cols.append(np.array(col, dtype=np.uint64))
            return np.stack(cols, axis=1)
        ints = self._width == 0
        if ints.any() and (V[:, ints] > 1).any():
            raise ValueError("the value of an equation int must be 0 or 1")
        w = np.where(ints, 1, self._width).astype(np.uint64)
        mask = np.where(w >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << (w % np.uint64(64))) - np.uint64(1))
        return V & mask

    def rhs_words(self, values_list: Sequence[Sequence[int]]) -> np.ndarray:
        """[n, ceil(rows / 64)] uint64: bit r of row i = the constant term of equation r in instance i."""
        C = self._chunks(values_list)
        n = C.shape[0]
        bits = np.zeros((n, self._rw * 64), dtype=np.uint8)
        if self._nexpr_rows:
            bits[:, :self._nexpr_rows] = ((C[:, self._row_col] >> self._row_bit) & np.uint64(1)).astype(np.uint8)
        out = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, self._rw)
        return out ^ self._consts

    # -- the factorization (one per mode, made on first use) -----------------------------------------------------------
    def _handle(self, mode: int):
        h = self._handles.get(mode)
        if h is None:
            if self._handles.get("closed"):
                raise ValueError("the factored system is closed")
            args = (self._eqs, self._system._cols, mode) + (() if self._device is None else (self._device,))
            h = self._handles[mode] = m4ri_factor(*args)
        return h

    def _solve(self, values_list, mode: int) -> list:
        if self._handles.get("closed"):
            raise ValueError("the factored system is closed")
        rhs = self.rhs_words(values_list)
        if rhs.shape[0] == 0:
            return []
        return self._handle(mode).solve(rhs)

    def close(self) -> None:
        for mode in (0, 1):
            h = self._handles.pop(mode, None)
            if h is not None:
                h.close()
        self._handles["closed"] = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- LinearSystem's methods, per instance ----------------------------------------------------------------------------
    def solve_raw_one_rhs(self, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve(values_list, 0)

    def solve_raw_space_rhs(self, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve(values_list, 1)

    def solve_one_rhs(self, values_list: Sequence[Sequence[int]], *, max_dimension: int = 16) -> list:
        if not self._quadratic:
            return [None if raw is None else self._system.convert_sol(raw) for raw in self._solve(values_list, 0)]
        from .linsys import DimensionTooLargeError   # noqa: PLC0415
        out = []
        for space in self._solve(values_list, 1):     # QuadraticSystem.solve_one_rhs: the first element that passes convert_sol
            sol = None
            if space is not None:
                if space.dimension > max_dimension:
                    raise DimensionTooLargeError(
                        f"Solution space (dim {space.dimension}) is too large, try increase max_dimension "
                        f"({max_dimension}) if you want (there will be 2**dim solutions)",
                        space=space,
                    )
                for raw in space:
                    sol = self._system.convert_sol(raw)
                    if sol is not None:
                        break
            out.append(sol)
        return out

    def solve_one(self, values: Sequence[int]):
        return self.solve_one_rhs([values])[0]

    def solve_all(self, values: Sequence[int], *, max_dimension: int = 16):
        from .linsys import DimensionTooLargeError   # noqa: PLC0415
        space = self._solve([values], 1)[0]
        if space is None:
            return
        if space.dimension > max_dimension:
            raise DimensionTooLargeError(
                f"Solution space (dim {space.dimension}) is too large, try increase max_dimension "
                f"({max_dimension}) if you want (there will be 2**dim solutions)",
                space=space,
            )
        for raw in space:
            sol = self._system.convert_sol(raw)
            if sol is not None:
                yield sol
