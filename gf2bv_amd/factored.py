"""FactoredSystem: one coefficient matrix factored once, instances solved against it later (no counterpart in the reference).

``LinearSystem.factor(exprs)`` / ``QuadraticSystem.factor(exprs)`` flatten the expressions once and factor their coefficient
matrix on the GPU (``_internal.m4ri_factor`` -> ``gf2bv_factor_digits``).  An instance is a list of observed values, one per
expression; each method equals the matching ``LinearSystem`` method on ``[e ^ v for e, v in zip(exprs, values)]``.  The
right-hand-side words of a batch are built with numpy from spans kept as arrays: bit r of instance i = the constant term of
equation r xor the bit of values[i][k] that equation r of expression k stands for.  ``add(exprs)`` appends expressions to the
factorizations already made; ``copy()`` makes an independent system (a guess tried on the copy leaves the original as it was).
``PackedLinearSystem.factor`` / ``PackedQuadraticSystem.factor`` give the subclasses at the end of this file: the same object with the
rows kept as arrays (packed words, or the factored form of quadratic equations, which the device expands).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from ._internal import (m4ri_factor, m4ri_factor_packed, m4ri_factor_quad_packed, m4ri_solve_rhs_packed,
                        m4ri_solve_rhs_quad_packed)
from .bitvec import BitVec


class FactoredSystem:
    def __init__(self, system, exprs, device=None):
        from .linsys import _QuadraticPoints         # noqa: PLC0415  (linsys imports this module lazily)
        self._system = system
        self._quadratic = isinstance(system, _QuadraticPoints)       # (QuadraticSystem and the packed front-end's twin of it)
        self._device = device
        self._init_rows()
        self._nspans = 0
        self._width = np.zeros(0, dtype=np.int64)        # per expression: width (0: an equation int, value 0 / 1)
        self._nchunks = np.zeros(0, dtype=np.int64)      # per expression: 64-bit chunks of its value
        self._expr_rows = np.zeros(0, dtype=np.int64)    # every row that belongs to an expression: its index,
        self._row_col = np.zeros(0, dtype=np.int64)      # which column of the chunk matrix built per call it reads,
        self._row_bit = np.zeros(0, dtype=np.uint64)     # and which bit of it
        self._extend(exprs)
        self._pad(system._cols)                      # the boundary wants rows >= cols (zero rows, constant 0 in every instance)
        self._set_rows()
        self._handles = {}

    # -- how the rows are kept: equation ints here, arrays in the packed front-end's subclasses below ------------------------
    def _init_rows(self) -> None:
        self._eqs: list = []

    def _pad(self, cols: int) -> None:
        if len(self._eqs) < cols:
            self._eqs.extend([0] * (cols - len(self._eqs)))

    def _extend(self, exprs) -> list:
        """The span bookkeeping of `exprs`, whose rows follow every current row; returns their equations."""
        new: list = []
        widths = []
        for e in exprs:
            if isinstance(e, BitVec):
                widths.append(len(e._bits))
                new.extend(e._bits)
            else:
                widths.append(0)
                new.append(e)
        self._add_spans(len(self._eqs), widths)
        self._eqs.extend(new)
        return new

    def _add_spans(self, base: int, widths: list) -> None:
        """expressions of these widths (0: an equation int, one row) whose rows start at row `base`"""
        width = np.array(widths, dtype=np.int64)
        reps = np.maximum(width, 1)
        at = np.cumsum(reps) - reps                  # first row of each expression, from `base`
        nchunks = np.maximum(1, (width + 63) // 64)
        first_chunk = int(self._nchunks.sum()) + np.concatenate(([0], np.cumsum(nchunks)[:-1])).astype(np.int64)
        row_span = np.repeat(np.arange(len(widths), dtype=np.int64), reps)
        offs = np.arange(len(row_span), dtype=np.int64) - np.repeat(at, reps)
        self._expr_rows = np.concatenate((self._expr_rows, base + np.arange(len(row_span), dtype=np.int64)))
        self._row_col = np.concatenate((self._row_col, first_chunk[row_span] + offs // 64))
        self._row_bit = np.concatenate((self._row_bit, (offs % 64).astype(np.uint64)))
        self._width = np.concatenate((self._width, width))
        self._nchunks = np.concatenate((self._nchunks, nchunks))
        self._nspans += len(widths)

    def _snapshot(self) -> dict:
        """the state an `add` that fails goes back to, and a copy starts from"""
        saved = dict(self.__dict__)
        saved["_eqs"] = list(self._eqs)
        return saved

    def _factor(self, mode: int):
        args = (self._eqs, self._system._cols, mode) + (() if self._device is None else (self._device,))
        return m4ri_factor(*args)

    def _append_to(self, h, new) -> None:
        h.append(new)

    def _set_rows(self) -> None:
        self.rows = len(self._eqs)
        self._rw = (self.rows + 63) // 64
        consts = np.zeros(self._rw * 64, dtype=np.uint8)
        consts[:self.rows] = [e & 1 for e in self._eqs]
        self._consts = np.packbits(consts, bitorder="little").view(np.uint64)

    def _check_open(self) -> None:
        if self._handles.get("closed"):
            raise ValueError("the factored system is closed")

    # -- new equations -----------------------------------------------------------------------------------------------------
    def add(self, exprs) -> None:
        """Append expressions (BitVec or equation int) after every current row; later instances take one value per expression,
        the earlier expressions' first.  Every factorization already made takes the new rows in (gf2bv_factor_append_*: the
        cost of the new rows, not of a new factorization); one made later factors the whole row list."""
        self._check_open()
        saved = self._snapshot()
        before = self.rows
        new = self._extend(exprs)
        self._set_rows()
        if self.rows == before:
            return
        done = []
        try:
            for mode in (0, 1):
                h = self._handles.get(mode)
                if h is not None:
                    self._append_to(h, new)
                    done.append(mode)
        except BaseException:
            handles = self._handles
            self.__dict__.clear()
            self.__dict__.update(saved)
            for mode in (0, 1):
                h = handles.get(mode)
                # those that hold the new rows, and one a failed append left unusable (rank -1), are made again from the old
                # row list on next use
                if h is not None and (mode in done or h.rank < 0):
                    handles.pop(mode).close()
            self._handles = handles
            raise

    def copy(self) -> "FactoredSystem":
        """An independent FactoredSystem: the factorizations made so far copied on the device, the bookkeeping on the host."""
        self._check_open()
        c = object.__new__(type(self))
        c.__dict__.update(self._snapshot())
        c._handles = {}
        try:
            for mode in (0, 1):
                h = self._handles.get(mode)
                if h is not None:
                    c._handles[mode] = h.copy()
        except BaseException:
            c.close()
            raise
        return c

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
        if len(self._expr_rows):
            bits[:, self._expr_rows] = ((C[:, self._row_col] >> self._row_bit) & np.uint64(1)).astype(np.uint8)
        out = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, self._rw)
        return out ^ self._consts

    # -- the factorization (one per mode, made on first use) -----------------------------------------------------------
    def _handle(self, mode: int):
        h = self._handles.get(mode)
        if h is None:
            self._check_open()
            h = self._handles[mode] = self._factor(mode)
        return h

    def _solve(self, values_list, mode: int) -> list:
        self._check_open()
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

    # -- QuadraticSystem.search_*, per instance (quadratic systems only) ------------------------------------------------------
    def _searchable(self) -> None:
        if not self._quadratic:
            raise TypeError("search_* needs a QuadraticSystem's factorization")

    def search_one_rhs(self, values_list: Sequence[Sequence[int]], *, max_enum: int = 32) -> list:
        """QuadraticSystem.search_one for every instance, the spaces from one factorization"""
        self._searchable()
        out = []
        for space in self._solve(values_list, 1):
            if space is None:
                out.append(None)
            else:
                sols = self._system._search_space(space, max_enum, 1, first=True)
                out.append(sols[0] if sols else None)
        return out

    def search_one(self, values: Sequence[int], *, max_enum: int = 32):
        return self.search_one_rhs([values], max_enum=max_enum)[0]

    def search_all(self, values: Sequence[int], *, max_enum: int = 32, max_solutions: int = 65536) -> list:
        self._searchable()
        space = self._solve([values], 1)[0]
        if space is None:
            return []
        return self._system._search_space(space, max_enum, max_solutions)


# ---- the packed front-ends' factored systems -------------------------------------------------------------------------------------
# The same object with the rows kept as the arrays the packed front-ends build (gf2bv_amd/packed.py) instead of equation ints: the
# span bookkeeping, the right-hand sides and every solve method are FactoredSystem's; what differs is where the rows come from,
# how their constants are read and which entry of `_internal` takes them.  The arrays are never written after they are made
# (appending concatenates), so a snapshot or a copy shares them.
class PackedFactoredSystem(FactoredSystem):
    """``PackedLinearSystem.factor``: the rows as one [rows, W] uint64 array in the bit order of the equation ints."""

    def _init_rows(self) -> None:
        self._rows = np.zeros((0, self._system._words), dtype=np.uint64)

    def _pad(self, cols: int) -> None:
        if len(self._rows) < cols:
            self._rows = np.concatenate((self._rows, np.zeros((cols - len(self._rows), self._rows.shape[1]), dtype=np.uint64)))

    def _extend(self, exprs) -> np.ndarray:
        widths, new = self._system._flat_rows(exprs)
        self._add_spans(len(self._rows), widths)
        self._rows = np.concatenate((self._rows, new))
        return new

    def _set_rows(self) -> None:
        self.rows = len(self._rows)
        self._rw = (self.rows + 63) // 64
        consts = np.zeros(self._rw * 64, dtype=np.uint8)
        consts[:self.rows] = self._rows[:, 0] & np.uint64(1)
        self._consts = np.packbits(consts, bitorder="little").view(np.uint64)

    def _snapshot(self) -> dict:
        return dict(self.__dict__)

    def _dev(self) -> tuple:
        return () if self._device is None else (self._device,)

    def _factor(self, mode: int):
        rows = np.ascontiguousarray(self._rows)
        return m4ri_factor_packed(rows, len(rows), rows.shape[1], self._system._cols, mode, *self._dev())

    def _append_to(self, h, new) -> None:
        h.append(np.ascontiguousarray(new))

    def _solve_once(self, rhs: np.ndarray, mode: int) -> list:
        """one elimination for these right-hand sides, nothing kept (the packed twin of m4ri_solve_rhs)"""
        rows = np.ascontiguousarray(self._rows)
        return m4ri_solve_rhs_packed(rows, len(rows), rows.shape[1], self._system._cols, mode, rhs, *self._dev())


class PackedQuadFactoredSystem(PackedFactoredSystem):
    """``PackedQuadraticSystem.factor``: the rows kept FACTORED -- lin [rows, Wl], the products per row and their operands
    ta / tb [T, Wl] (gf2bv_hip.h, "quadratic expansion") -- and expanded on the device, when a factorization is made and when rows
    are appended to one.  No row of the linearised matrix exists on the host."""

    def _init_rows(self) -> None:
        none = np.zeros((0, self._system._words), dtype=np.uint64)
        self._lin, self._ta, self._tb = none, none, none
        self._cnt = np.zeros(0, dtype=np.int64)           # products per row

    def _pad(self, cols: int) -> None:
        pad = cols - len(self._lin)
        if pad > 0:
            self._lin = np.concatenate((self._lin, np.zeros((pad, self._lin.shape[1]), dtype=np.uint64)))
            self._cnt = np.concatenate((self._cnt, np.zeros(pad, dtype=np.int64)))

    def _extend(self, exprs) -> tuple:
        exprs = list(exprs)
        lin, off, ta, tb = self._system._terms(exprs)
        widths = [0 if isinstance(e, int) else len(e) for e in exprs]
        self._add_spans(len(self._lin), widths)
        self._lin = np.concatenate((self._lin, lin))
        self._cnt = np.concatenate((self._cnt, np.diff(off)))
        self._ta, self._tb = np.concatenate((self._ta, ta)), np.concatenate((self._tb, tb))
        return lin, off, ta, tb

    def _set_rows(self) -> None:
        self.rows = len(self._lin)
        self._rw = (self.rows + 63) // 64
        # the constant of a factored row: bit 0 of its linear part xor bit 0 of a & b over its products (what _mul_bit leaves there)
        c = self._lin[:, 0] & np.uint64(1)
        if len(self._ta):
            np.bitwise_xor.at(c, np.repeat(np.arange(self.rows), self._cnt), self._ta[:, 0] & self._tb[:, 0] & np.uint64(1))
        consts = np.zeros(self._rw * 64, dtype=np.uint8)
        consts[:self.rows] = c
        self._consts = np.packbits(consts, bitorder="little").view(np.uint64)

    def _arrays(self) -> tuple:
        off = np.zeros(self.rows + 1, dtype=np.int64)
        np.cumsum(self._cnt, out=off[1:])
        return tuple(np.ascontiguousarray(a) for a in (self._lin, off, self._ta, self._tb))

    def _factor(self, mode: int):
        return m4ri_factor_quad_packed(*self._arrays(), self._system._lin_size, self.rows, mode, *self._dev())

    def _append_to(self, h, new) -> None:
        h.append_quad(*(np.ascontiguousarray(a) for a in new), self._system._lin_size)

    def _solve_once(self, rhs: np.ndarray, mode: int) -> list:
        return m4ri_solve_rhs_quad_packed(*self._arrays(), self._system._lin_size, self.rows, mode, rhs, *self._dev())
