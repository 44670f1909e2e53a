"""Packed symbolic front-end: BitVec algebra on bit matrices instead of tuples of Python ints.

The reference represents a symbolic bit as a Python int (bit 0 = constant term, bit k = coefficient of unknown
k-1) and a BitVec as a tuple of such ints (gf2bv/__init__.py:21-134); every XOR of two 32-bit BitVecs over 19968
unknowns then touches 32 ints of 2.5 KB one by one through the interpreter (or the C helpers of
gf2bv/_internal.c:504-676), and the finished ``zeros`` are handed over as a list of ~20000 PyLongs that
``m4ri_solve`` reads bit by bit.  For the MT19937 recovery of examples/mt.py the front-end costs seconds, the solve
tens of milliseconds.

Here a ``PackedBitVec`` of n bits is ONE numpy array ``[n, W]`` of little-endian 64-bit words, W = ceil((cols+1)/64),
row i = symbolic bit i in the SAME bit order as the reference's ints.  XOR / shift / rotate / mask are whole-array
numpy operations; ``PackedLinearSystem`` stacks the rows of the ``zeros`` and gives the buffer straight to
``_internal.m4ri_solve_packed`` -- the device pack kernel reads it as 32-bit digits -- so no PyLong list exists at any
point.  Same surface and semantics as ``BitVec`` / ``LinearSystem`` (it IS a BitVec: the PRNG models in
tests.harness_models run on it unchanged); ``get_eqs`` still returns the reference's list of ints for callers that want it.
"""
from __future__ import annotations

import operator
from math import comb
from typing import Iterable, Optional, Sequence

import numpy as np

from ._internal import (m4ri_solve_cubic_packed, m4ri_solve_many_quad_packed, m4ri_solve_packed, m4ri_solve_quad_packed,
                        m4ri_solve_quartic_packed, m4ri_solve_xl3_guess_quad_packed, m4ri_solve_xl3_quad_packed, m4ri_solve_xl4_guess_cubic_packed,
                        m4ri_solve_xl4_guess_quad_packed, m4ri_solve_xl4_cubic_packed, m4ri_solve_xl4_quad_packed)
from .bitvec import BitVec
from .linsys import _ProductColumns, _QuadraticPoints, _SolveSurface, _XlGuess, _eqs_from_words, _raw_value, _space_points, xl3_cols, xl4_cols


def _const_bits(n: int, value: int) -> np.ndarray:
    """low n bits of the MAGNITUDE of value, LSB first, as uint64 0/1 -- to_bits of the reference walks the digits of
    |a| (gf2bv/_internal.c:504-531), so a negative constant contributes abs(value), not its two's complement"""
    value = abs(int(value)) & ((1 << n) - 1)
    return np.array([(value >> i) & 1 for i in range(n)], dtype=np.uint64)


def _popcount64(a: np.ndarray) -> np.ndarray:
    if hasattr(np, "bitwise_count"):                   # numpy >= 2.0
        return np.bitwise_count(a)
    b = a.view(np.uint8).reshape(a.shape + (8,))       # numpy 1.x: per-byte table
    return _POP8[b].sum(axis=-1)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)


class PackedBitVec(BitVec):
    __slots__ = ("_rows",)

    def __init__(self, rows: np.ndarray):
        self._rows = rows                              # [nbits, W] uint64, treated as immutable

    # compatibility with code that reads the reference's representation
    @property
    def _bits(self) -> tuple:
        return tuple(int.from_bytes(r.tobytes(), "little") for r in self._rows)

    def _zero_rows(self, n: int) -> np.ndarray:
        return np.zeros((n, self._rows.shape[1]), dtype=np.uint64)

    def _coerce(self, other) -> np.ndarray:
        if isinstance(other, PackedBitVec):
            if other._rows.shape != self._rows.shape:
                raise ValueError("Cannot mix bitvecs of different lengths")
            return other._rows
        if isinstance(other, BitVec):
            raise TypeError("cannot mix packed and tuple-of-int BitVecs")
        rhs = self._zero_rows(len(self))
        rhs[:, 0] = _const_bits(len(self), other)      # a constant only has the affine bit
        return rhs

    # -- container protocol (reference :29-37) ------------------------------------------------
    def __len__(self):
        return self._rows.shape[0]

    def __getitem__(self, key):
        if isinstance(key, slice):
            return PackedBitVec(self._rows[key])
        i = operator.index(key)
        n = self._rows.shape[0]
        if not -n <= i < n:                            # (also what ends `for b in bv`: BitVec has no __iter__)
            raise IndexError("PackedBitVec index out of range")
        i %= n
        return PackedBitVec(self._rows[i:i + 1])

    # -- xor (reference :39-49) ----------------------------------------------------------------
    def __xor__(self, other):
        if isinstance(other, _TermsBitVec):
            return NotImplemented                      # (its __rxor__ takes over: the sum is quadratic or cubic)
        return PackedBitVec(self._rows ^ self._coerce(other))

    __rxor__ = __xor__
    __pow__ = __xor__

    # -- shifts / rotations (reference :51-62, :104-108) -----------------------------------------
    def __rshift__(self, n: int):
        if n == 0:
            return self
        return PackedBitVec(np.concatenate([self._rows[n:], self._zero_rows(n)]))      # (n > len grows it, as bits[n:] + (0,) * n does)

    def __lshift__(self, n: int):
        if n == 0:
            return self
        return PackedBitVec(np.concatenate([self._zero_rows(n), self._rows[:-n]]))

    def lshift_ext(self, n: int):
        return PackedBitVec(np.concatenate([self._zero_rows(n), self._rows]))

    def rotr(self, n: int):
        return PackedBitVec(np.roll(self._rows, -n, axis=0))

    def rotl(self, n: int):
        return PackedBitVec(np.roll(self._rows, n, axis=0))

    # -- masks (reference :64-102) -----------------------------------------------------------------
    def __and__(self, mask: int):
        if isinstance(mask, BitVec):
            raise TypeError("AND of two symbolic vectors is not linear (use QuadraticSystem)")
        sel = _const_bits(len(self), mask)
        if sel.all():
            return self
        return PackedBitVec(self._rows * sel[:, None])

    __rand__ = __and__

    def __or__(self, mask):
        if not isinstance(mask, BitVec):
            sel = _const_bits(len(self), mask)
            out = self._rows * (np.uint64(1) - sel)[:, None]
            out[:, 0] |= sel                           # selected bits become the constant 1
            return PackedBitVec(out)
        if not isinstance(mask, PackedBitVec):
            raise TypeError("cannot mix packed and tuple-of-int BitVecs")
        short, long_ = (self, mask) if len(self) <= len(mask) else (mask, self)
        merged = long_._rows.copy()
        one = np.zeros(self._rows.shape[1], dtype=np.uint64)
        one[0] = 1
        for i in range(len(short)):
            x, y = short._rows[i], long_._rows[i]
            xc = not x[1:].any() and x[0] <= 1         # a constant 0 / 1
            yc = not y[1:].any() and y[0] <= 1
            if not xc and not yc:
                raise ValueError("Cannot compute logical or using bitvecs with non-zero bits")
            if (xc and x[0] == 1) or (yc and y[0] == 1):
                merged[i] = one
            elif xc:                                   # x == 0
                merged[i] = y
            else:
                merged[i] = x
        return PackedBitVec(merged)

    __ror__ = __or__

    def __mod__(self, n: int):
        if n & (n - 1):
            raise ValueError("modulo non-power-of-2 is not a linear operation")
        return self & (n - 1)

    # -- reductions / reshaping (reference :110-126) ---------------------------------------------
    def sum(self):
        return PackedBitVec(np.bitwise_xor.reduce(self._rows, axis=0, keepdims=True))

    def zeroext(self, n: int):
        return PackedBitVec(np.concatenate([self._rows, self._zero_rows(n)]))

    def signext(self, n: int):
        return PackedBitVec(np.concatenate([self._rows, np.repeat(self._rows[-1:], n, axis=0)]))

    def broadcast(self, i: int, n: int):
        return PackedBitVec(np.repeat(self._rows[i:i + 1] if i != -1 else self._rows[-1:], n, axis=0))

    def dup(self, n: int):
        return PackedBitVec(np.tile(self._rows, (n, 1)))

    def concat(self, other: "PackedBitVec"):
        if isinstance(other, _TermsBitVec):            # (linear bits in front of bits that carry products)
            return other._from_rows(self._rows, other._n).concat(other)
        return PackedBitVec(np.concatenate([self._rows, other._rows]))

    # -- evaluation (reference :128-134) -----------------------------------------------------------
    def evaluate(self, s: int) -> int:
        W = self._rows.shape[1]
        point = np.frombuffer((((s << 1) | 1) & ((1 << (64 * W)) - 1)).to_bytes(8 * W, "little"), dtype=np.uint64)
        par = _popcount64(self._rows & point[None, :]).sum(axis=1) & 1
        return int(sum(int(b) << i for i, b in enumerate(par)))


class PackedLinearSystem(_SolveSurface):
    """LinearSystem (gf2bv/__init__.py:137-287) on PackedBitVecs: same methods, same results, no list of ints on the
    way to the solver (what follows the boundary call is LinearSystem's own code, _SolveSurface)."""

    def __init__(self, sizes: Iterable[int]):
        self._sizes = list(sizes)
        self._cols = sum(self._sizes)
        self._words = (self._cols + 1 + 63) // 64
        gens, at = [], 1                               # unknown g is bit g + 1 of an equation
        for width in self._sizes:
            rows = np.zeros((width, self._words), dtype=np.uint64)
            pos = np.arange(at, at + width)
            rows[np.arange(width), pos >> 6] = np.uint64(1) << (pos & 63).astype(np.uint64)
            gens.append(PackedBitVec(rows))
            at += width
        self._vars = tuple(gens)

    def gens(self):
        return self._vars

    def __reduce__(self):
        return (self.__class__, (self._sizes,))

    # -- zeros -> one [n, W] array (the packed twin of get_eqs, reference :214-227) ------------------
    def get_rows(self, zeros: Sequence) -> np.ndarray:
        """the stacked non-zero rows of ``zeros`` as a fresh [n, W] array (the solve methods use the shared buffer of
        ``_stack_rows`` instead and never keep it)"""
        return self._stack_rows(zeros).copy()

    def _stack_rows(self, zeros: Sequence) -> np.ndarray:
        parts = []
        for z in zeros:
            if isinstance(z, PackedBitVec):
                parts.append(z._rows)
            elif isinstance(z, BitVec):
                raise TypeError("cannot mix packed and tuple-of-int BitVecs")
            else:                                      # a bare equation int
                r = np.frombuffer((int(z) & ((1 << (64 * self._words)) - 1)).to_bytes(8 * self._words, "little"),
                                  dtype=np.uint64)
                parts.append(r[None, :])
        n = sum(len(x) for x in parts)
        # (stacked into a buffer that is kept between calls: a fresh 50 MB allocation is paid for in page faults, several
        # times the copy itself.  The returned array is a view of it, valid until the next call: internal use only.)
        buf = getattr(self, "_rowbuf", None)
        if buf is None or len(buf) < n:
            buf = self._rowbuf = np.empty((max(n, 1), self._words), dtype=np.uint64)
        rows = np.concatenate(parts, out=buf[:n]) if parts else buf[:0]
        nz = np.bitwise_or.reduce(rows, axis=1) != 0   # literal zeros carry no information
        return rows if nz.all() else rows[nz]          # (the usual case costs no second copy of the ~50 MB of an MT19937 system)

    def get_eqs(self, zeros: Sequence) -> list:
        """the reference's list of equation ints (for callers that want it; the solve methods do not build it)"""
        return [int.from_bytes(r.tobytes(), "little") for r in self._stack_rows(zeros)]

    # -- boundary call (reference :229-240) ------------------------------------------------------------
    def _solve_internal(self, zeros: Sequence, mode: int):
        rows = self._stack_rows(zeros)
        cand = np.flatnonzero(rows[:, 0] == 1) if len(rows) else ()                # the equation "1 = 0": word 0 is 1 ...
        if len(cand) and (~rows[cand, 1:].any(axis=1)).any():                        # ... and nothing else is set
            return None
        if len(rows) < self._cols:                     # the boundary wants rows >= cols
            rows = np.concatenate([rows, np.zeros((self._cols - len(rows), self._words), dtype=np.uint64)])
        rows = np.ascontiguousarray(rows)
        return m4ri_solve_packed(rows, rows.shape[0], self._words, self._cols, mode)

    # -- many right-hand sides of one matrix, and the matrix factored once (LinearSystem's, no counterpart in the reference) ------
    def _flat_rows(self, exprs: Sequence):
        """(widths, rows) of `exprs` for a factored system: per expression its width (0: an equation int), and every row in
        order as one [n, W] array.  Unlike ``_stack_rows`` no row is dropped: a right-hand side has a bit for each."""
        parts, widths = [np.zeros((0, self._words), dtype=np.uint64)], []
        for e in exprs:
            if isinstance(e, PackedBitVec):
                if e._rows.shape[1] != self._words:
                    raise ValueError("Cannot mix bitvecs over different numbers of unknowns")
                parts.append(e._rows)
                widths.append(len(e))
            elif isinstance(e, (BitVec, PackedQuadBitVec)):
                raise TypeError("a packed linear system takes PackedBitVecs and equation ints")
            else:                                      # a bare equation int
                r = np.frombuffer((int(e) & ((1 << (64 * self._words)) - 1)).to_bytes(8 * self._words, "little"), dtype=np.uint64)
                parts.append(r[None, :])
                widths.append(0)
        return widths, np.concatenate(parts)

    def factor(self, exprs: Sequence, device=None):
        """``LinearSystem.factor`` on packed expressions (PackedBitVec or equation int): the same FactoredSystem surface and the
        same answers, the rows handed over as one array."""
        from .factored import PackedFactoredSystem     # noqa: PLC0415
        return PackedFactoredSystem(self, exprs, device)

    def _solve_internal_rhs(self, exprs: Sequence, values_list: Sequence[Sequence[int]], mode: int) -> list:
        fs = self.factor(exprs)                        # (the bookkeeping of the right-hand sides only: nothing is factored or kept)
        rhs = fs.rhs_words(values_list)
        if not len(rhs):
            return []
        return fs._solve_once(rhs, mode)

    def solve_raw_one_rhs(self, exprs: Sequence, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve_internal_rhs(exprs, values_list, 0)

    def solve_raw_space_rhs(self, exprs: Sequence, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve_internal_rhs(exprs, values_list, 1)

    def solve_one_rhs(self, exprs: Sequence, values_list: Sequence[Sequence[int]]) -> list:
        return [None if raw is None else self.convert_sol(raw) for raw in self._solve_internal_rhs(exprs, values_list, 0)]


# ---- systems kept factored: one vector of bits that carry products --------------------------------------------------------------
# QuadraticSystem.mul_bit writes the linearised row of a product on the host, n(n-1)/2 bits beyond the n + 1 of its operands: at
# n = 256 that is 10 ms per product and a 32896-column system cannot be written down in an hour.  Here a symbolic bit stays what the
# caller wrote: a linear form over the n + 1 bits plus lists of products of such forms.  The rows of the linearised matrix come into
# being on the device (k_quad_expand / k_cubic_expand, through m4ri_solve_quad_packed / m4ri_solve_cubic_packed / hip.*_expand_words),
# where the solver reads them.  PackedQuadBitVec (products of two forms) and PackedCubicBitVec (of two and of three) are one
# vector over groups of products, _TermsBitVec.
def _take_terms(group: tuple, idx: np.ndarray):
    """the products (offsets, operand arrays) of the bits idx[0], idx[1], ... of a group"""
    off, ops = group
    cnt = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(cnt, out=new[1:])
    src = np.repeat(off[idx] - new[:-1], cnt) + np.arange(new[-1])         # operand row of every kept product
    return new, tuple([x[src] for x in ops])


def _xor_terms(a: tuple, b: tuple):
    """bit i of the sum owns the products of a[i], then those of b[i]"""
    (off_a, ops_a), (off_b, ops_b) = a, b
    bits = np.arange(len(off_a) - 1)
    owner = np.concatenate([np.repeat(bits, np.diff(off_a)), np.repeat(bits, np.diff(off_b))])
    order = np.argsort(owner, kind="stable")
    return off_a + off_b, tuple([np.concatenate(xy)[order] for xy in zip(ops_a, ops_b)])


def _cat_terms(a: tuple, b: tuple):
    """the bits of b behind those of a"""
    (off_a, ops_a), (off_b, ops_b) = a, b
    return np.concatenate([off_a, off_b[1:] + off_a[-1]]), tuple([np.concatenate(xy) for xy in zip(ops_a, ops_b)])


def _refuse(name: str):
    def method(self, *args, **kwargs):
        raise TypeError(f"{name} is not supported on a {type(self).__name__} (bits that carry products): only ^, indexing and concat are")
    method.__name__ = name
    return method


def _part(group: int, operand: Optional[int] = None) -> property:
    """a group's offsets, or one of its operand arrays, under the name the class documents"""
    if operand is None:
        return property(lambda self: self._groups[group][0])
    return property(lambda self: self._groups[group][1][operand])


class _TermsBitVec:
    """k symbolic bits, each a linear form (a row of ``_lin``, Wl = ceil((n + 1) / 64) words in the order of ``PackedBitVec``) plus
    products of linear forms, kept as one group ``(off, ops)`` per arity of ``_ARITIES``: bit i owns the rows ``off[i] .. off[i + 1]``
    of every operand array of ``ops``.  Equal products are not cancelled here, they cancel when the rows are expanded.  What a
    product's value is, and what may be mixed with what (``_coerce``), is the subclass's."""
    __slots__ = ("_lin", "_groups", "_n")
    _ARITIES: tuple = ()

    def _new(self, lin: np.ndarray, groups: tuple):
        v = object.__new__(type(self))
        v._lin, v._groups, v._n = lin, groups, self._n                     # [k, Wl] uint64, ([k + 1] int64, [T, Wl] x arity) per group: immutable
        return v

    @classmethod
    def _from_rows(cls, rows: np.ndarray, n: int):
        """linear bits (the rows of a PackedBitVec) over n unknowns as a vector of this kind"""
        v = object.__new__(cls)
        none, off = rows[:0], np.zeros(len(rows) + 1, dtype=np.int64)
        v._lin, v._groups, v._n = rows, tuple([(off, (none,) * arity) for arity in cls._ARITIES]), n
        return v

    def __len__(self):
        return self._lin.shape[0]

    def _take(self, idx: np.ndarray):
        """the bits idx[0], idx[1], ... as a new vector"""
        return self._new(self._lin[idx], tuple([_take_terms(g, idx) for g in self._groups]))

    def __getitem__(self, key):
        n = len(self)
        if isinstance(key, slice):
            return self._take(np.arange(n)[key])
        i = operator.index(key)
        if not -n <= i < n:
            raise IndexError(f"{type(self).__name__} index out of range")
        return self._take(np.array([i % n]))

    def __xor__(self, other):
        if isinstance(other, PackedBitVec) and other._rows.shape == self._lin.shape:
            return self._new(self._lin ^ other._rows, self._groups)      # (no products to merge, no vector to make of the rows)
        if isinstance(other, (_TermsBitVec, BitVec)):
            other = self._coerce(other, "^")
            if other is NotImplemented:
                return other
            if other._lin.shape[0] != self._lin.shape[0]:
                raise ValueError("Cannot mix bitvecs of different lengths")
            return self._new(self._lin ^ other._lin, tuple(map(_xor_terms, self._groups, other._groups)))
        lin = self._lin.copy()
        lin[:, 0] ^= _const_bits(len(self), other)      # a constant only has the affine bit
        return self._new(lin, self._groups)

    __rxor__ = __xor__
    __pow__ = __xor__

    def concat(self, other):
        other = self._coerce(other, "concat")
        return self._new(np.concatenate([self._lin, other._lin]), tuple(map(_cat_terms, self._groups, other._groups)))


for _name in ("__and__", "__rand__", "__or__", "__ror__", "__lshift__", "__rshift__", "__mod__", "__invert__", "lshift_ext", "rotl", "rotr",
              "sum", "zeroext", "signext", "broadcast", "dup"):
    setattr(_TermsBitVec, _name, _refuse(_name))
del _name


# The quadratic class's products are QuadraticSystem._mul_bit's, which drops the constant x linear cross terms; the cubic class's are
# the EXACT products of GF(2)[x] / (x_i^2 + x_i), constants included.  That is why the two kinds of vector do not mix.
_QUAD_MIX = ("a PackedQuadBitVec cannot be mixed with a PackedCubicBitVec: the quadratic class's products follow the reference's "
             "_mul_bit (no constant x linear cross terms), this class's are the exact products")


class PackedQuadBitVec(_TermsBitVec):
    """``_TermsBitVec`` with products of two linear forms: bit i owns the operand rows ``_off[i] .. _off[i + 1]`` of ``_ta`` /
    ``_tb``.  The value of a product is ``QuadraticSystem._mul_bit`` of its operands."""
    __slots__ = ()
    _ARITIES = (2,)
    _off, _ta, _tb = _part(0), _part(0, 0), _part(0, 1)

    def __init__(self, lin: np.ndarray, off: np.ndarray, ta: np.ndarray, tb: np.ndarray, n: int):
        self._lin, self._groups = lin, ((off, (ta, tb)),)                  # [k, Wl] uint64, [k + 1] int64, [T, Wl], [T, Wl]: immutable
        self._n = n                                    # unknowns of the system (Wl alone leaves 64 candidates)

    def _coerce(self, other, what: str):
        # (the texts are the ones each operator has always had: under ^ a form of another width is "of different lengths", and concat
        # names the kinds it takes where ^ names the one it does not)
        if not isinstance(other, PackedQuadBitVec):
            if what == "^" and isinstance(other, PackedCubicBitVec):
                return NotImplemented                  # (its __rxor__ says why the two do not mix)
            if not isinstance(other, PackedBitVec):
                raise TypeError("cannot mix packed and tuple-of-int BitVecs" if what == "^" else "concat needs a PackedQuadBitVec or a PackedBitVec")
            other = self._from_rows(other._rows, self._n)
        if other._lin.shape[1] != self._lin.shape[1]:
            raise ValueError("Cannot mix bitvecs of different lengths" if what == "^" else "Cannot mix bitvecs over different numbers of unknowns")
        return other

    def evaluate(self, s: int) -> int:
        """Value under the raw point ``s`` of the LINEARISED unknowns (bit j = unknown j, the products behind the n linear ones),
        as BitVec.evaluate gives it for the expanded bits; on the host, a product at a time."""
        n = self._n
        low = ((s << 1) | 1) & ((1 << (n + 1)) - 1)
        runs = [(s >> (n + i * (i - 1) // 2)) & ((1 << i) - 1) for i in range(n)]          # the products (i, 0 .. i-1) at s
        ints = lambda rows: [int.from_bytes(r.tobytes(), "little") for r in rows]            # noqa: E731
        lin, ta, tb = ints(self._lin), ints(self._ta), ints(self._tb)
        par = lambda v: bin(v).count("1") & 1                                                 # noqa: E731
        value = 0
        for k in range(len(self)):
            bit = par(lin[k] & low)
            for t in range(self._off[k], self._off[k + 1]):
                a, b = ta[t], tb[t]
                bit ^= par(a & b & low)
                for i in range(n):
                    if (a >> (1 + i)) & 1:
                        bit ^= par((b >> 1) & runs[i])
                    if (b >> (1 + i)) & 1:
                        bit ^= par((a >> 1) & runs[i])
            value |= bit << k
        return value


def _zeros_terms(zeros: Sequence, cls, kind: str, words: int) -> tuple:
    """(lin [R, Wl], then per group of ``cls`` its offsets [R + 1] and its operand arrays) of all the bits of ``zeros``, in order, for a
    system of that kind.  No row is dropped: whether a factored row is the literal 0 or the equation "1 = 0" is only known once it is
    expanded, and the solver needs neither decided -- an all-zero row changes no pivot, origin or basis, and a row that is exactly
    the constant 1 makes it report the system inconsistent (LinearSystem._rhs_eqs relies on the same two facts)."""
    none = np.zeros((0, words), dtype=np.uint64)
    one_row = np.zeros(1, dtype=np.int64)
    lins, vecs, terms = [none], [], []                 # per entry its rows; its groups, or (linear rows) a count of no products per row
    for z in zeros:
        if isinstance(z, cls):
            lin = z._lin
            vecs.append(z._groups)
            terms.append(z._groups)
        elif isinstance(z, PackedBitVec):              # (no vector is made of linear rows)
            lin = z._rows
            terms.append(np.zeros(len(lin), dtype=np.int64))
        elif isinstance(z, BitVec):
            raise TypeError("cannot mix packed and tuple-of-int BitVecs")
        elif isinstance(z, int) and z in (0, 1):       # the literal 0, or the equation "1 = 0"
            lin = np.zeros((1, words), dtype=np.uint64)
            lin[0, 0] = z
            terms.append(one_row)
        elif isinstance(z, PackedQuadBitVec):          # (given to a cubic system)
            raise TypeError(_QUAD_MIX)
        else:
            raise TypeError(f"a bare equation of a packed {kind} system is 0 or 1: build the others from gens() and mul_bit")
        if lin.shape[1] != words:
            raise ValueError("Cannot mix bitvecs over different numbers of unknowns")
        lins.append(lin)
    lin = np.concatenate(lins)
    out = [lin]
    for g, arity in enumerate(cls._ARITIES):
        off = np.zeros(len(lin) + 1, dtype=np.int64)
        if not vecs:
            cnt = terms
        elif len(vecs) == len(terms):                  # (the usual cases, all linear and all products, without a test per entry)
            cnt = [np.diff(v[g][0]) for v in vecs]
        else:
            cnt = [np.diff(t[g][0]) if type(t) is tuple else t for t in terms]
        if cnt:
            np.cumsum(np.concatenate(cnt), out=off[1:])
        out.append(off)
        out.extend(np.concatenate([none] + [v[g][1][k] for v in vecs]) for k in range(arity))
    return tuple(out)


class PackedQuadraticSystem(_QuadraticPoints, PackedLinearSystem):
    """QuadraticSystem (gf2bv/__init__.py:290-408) with the equations kept factored: same methods, same results, and no row of the
    linearised matrix -- n + n(n-1)/2 columns -- on the host.  ``gens()`` are PackedBitVecs over the n + 1 bits of the unknowns
    themselves, so everything linear (the LFSR / PRNG models of tests.harness_models) runs on them as on a PackedLinearSystem's;
    ``mul_bit`` / ``bit_assert`` give PackedQuadBitVecs; the solve methods hand the factored arrays to the device, which expands
    and solves them.  ``convert_sol``, ``solve_one``, ``solve_one_rhs`` and the searches are QuadraticSystem's own (_QuadraticPoints); ``factor``,
    ``solve_*_rhs`` and ``solve_*_many`` hand over the factored arrays as well."""

    def __init__(self, sizes: Iterable[int]):
        sizes = list(sizes)
        n = sum(sizes)
        self._quad_sizes = sizes
        self._lin_size = n
        self._quad_size = n * (n - 1) // 2
        self._sizes = sizes + [self._quad_size]        # (what _convert_sol splits a raw solution into)
        self._cols = n + self._quad_size
        self._words = (n + 1 + 63) // 64               # words of a linear form: the generators have no product coordinates
        self._vars = PackedLinearSystem(sizes).gens()

    def __reduce__(self):
        return (self.__class__, (self._quad_sizes,))

    def _single(self, a, what: str) -> np.ndarray:
        if isinstance(a, PackedQuadBitVec):
            raise TypeError(f"{what} of a bit that carries products is of degree above 2")
        if not isinstance(a, PackedBitVec):
            raise TypeError(f"{what} needs PackedBitVecs of this system")
        if len(a) != 1:
            raise ValueError("The inputs should be single bits" if what == "mul_bit" else "The input should be a single bit")
        if a._rows.shape[1] != self._words:
            raise ValueError("Cannot mix bitvecs over different numbers of unknowns")
        return a._rows

    def mul_bit(self, a: PackedBitVec, b: PackedBitVec) -> PackedQuadBitVec:
        ra, rb = self._single(a, "mul_bit"), self._single(b, "mul_bit")
        return PackedQuadBitVec(np.zeros((1, self._words), dtype=np.uint64), np.array([0, 1], dtype=np.int64), ra, rb, self._lin_size)

    def bit_assert(self, a: PackedBitVec, v: int) -> list:
        """QuadraticSystem.bit_assert: "bit a equals v" and its product with every unknown x other than a itself, a * x = v * x --
        the same rows in the same order, as [a ^ v, one PackedQuadBitVec of the products]"""
        ra = self._single(a, "bit_assert")
        assert v in (0, 1), "Invalid bit"
        assert ra[0, 1:].any() or ra[0, 0] > 1, "a should not be a constant"
        assert not (a._bits[0] >> (self._lin_size + 1)), "Not a linear term"
        x = np.concatenate([g._rows for g in self._vars])                  # unknown i: bit 1 + i alone
        x = x[(x != ra).any(axis=1)]                                       # (the reference skips x == a)
        lin = x if v else np.zeros_like(x)
        return [a ^ v, PackedQuadBitVec(lin, np.arange(len(x) + 1, dtype=np.int64), np.repeat(ra, len(x), axis=0), x, self._lin_size)]

    # -- zeros -> the factored arrays the device expands --------------------------------------------------------------------------
    def _terms(self, zeros: Sequence):
        """(lin [R, Wl], term_off [R + 1], ta, tb) of all the bits of ``zeros``, in order; no row is dropped (_zeros_terms)"""
        return _zeros_terms(zeros, PackedQuadBitVec, "quadratic", self._words)

    def _stack_rows(self, zeros: Sequence):
        raise TypeError("a packed quadratic system has no rows on the host: use get_eqs, or hip.quad_expand_words on the factored arrays")

    def get_eqs(self, zeros: Sequence) -> list:
        """the reference's list of equation ints over the linearised unknowns, expanded on the device (needs the GPU)"""
        from . import hip                              # noqa: PLC0415  (ctypes binding, first use only)
        lin, off, ta, tb = self._terms(zeros)
        if not len(lin):
            return []
        return _eqs_from_words(hip.quad_expand_words(lin, off, ta, tb, self._lin_size), self._cols)

    # -- boundary call ---------------------------------------------------------------------------------------------------------------
    def _solve_internal(self, zeros: Sequence, mode: int):
        lin, off, ta, tb = self._terms(zeros)
        return m4ri_solve_quad_packed(lin, off, ta, tb, self._lin_size, max(len(lin), self._cols), mode)      # (the boundary wants rows >= cols)

    # -- degree-3 XL: the factored arrays go down, the device expands, multiplies and pads them (nothing is decided on the host) ----
    def _solve_internal_xl(self, zeros: Sequence, mode: int, degree: int = 3):
        lin, off, ta, tb = self._terms(zeros)
        return (m4ri_solve_xl4_quad_packed if degree == 4 else m4ri_solve_xl3_quad_packed)(lin, off, ta, tb, self._lin_size, mode)

    def _solve_internal_xl_guess(self, zeros: Sequence, guess: list, mode: int):
        return self._stage_xl_guess(zeros, guess, mode, 3)

    def _solve_internal_xl4_guess(self, zeros: Sequence, guess: list, mode: int):
        return self._stage_xl_guess(zeros, guess, mode, 4)

    def _stage_xl_guess(self, zeros: Sequence, guess: list, mode: int, degree: int):
        lin, off, ta, tb = self._terms(zeros)
        solve = m4ri_solve_xl4_guess_quad_packed if degree == 4 else m4ri_solve_xl3_guess_quad_packed
        return len(lin), lambda first, count: solve(lin, off, ta, tb, self._lin_size, guess, first, count, mode)

    def get_eqs_xl(self, zeros: Sequence) -> list:
        """the equations and their products with every unknown as equation ints over the cubic columns (needs the GPU)"""
        return self._get_eqs_xl(zeros, 3)

    def _get_eqs_xl(self, zeros: Sequence, degree: int) -> list:
        from . import hip                              # noqa: PLC0415
        lin, off, ta, tb = self._terms(zeros)
        if not len(lin):
            return []
        return self._xl_eqs(hip.quad_expand_words(lin, off, ta, tb, self._lin_size), degree)

    def get_eqs_xl4(self, zeros: Sequence) -> list:
        """the equations and their products with every unknown and every pair of unknowns as equation ints over the quartic columns"""
        return self._get_eqs_xl(zeros, 4)

    # -- a kept factorization, many right-hand sides, batches: QuadraticSystem's methods on the factored arrays --------------------
    # (solve_*_rhs are PackedLinearSystem's through ``factor``; solve_one_rhs is QuadraticSystem's own, _QuadraticPoints)
    def _flat_rows(self, exprs: Sequence):
        raise TypeError("a packed quadratic system has no rows on the host")

    def factor(self, exprs: Sequence, device=None):
        """``QuadraticSystem.factor`` on packed expressions (PackedBitVec, PackedQuadBitVec, the literals 0 / 1): the same
        FactoredSystem surface -- ``add(q.bit_assert(a, v))`` on a ``copy()`` included -- with every row expanded on the device."""
        from .factored import PackedQuadFactoredSystem     # noqa: PLC0415
        return PackedQuadFactoredSystem(self, exprs, device)

    def _solve_internal_many(self, zeros_list: Sequence[Sequence], mode: int) -> list:
        """independent systems as ONE concatenated term set: one upload, one expansion launch, lock-step gangs"""
        terms = [self._terms(z) for z in zeros_list]
        if not terms:
            return []
        sys_off = np.zeros(len(terms) + 1, dtype=np.int64)
        np.cumsum([len(t[0]) for t in terms], out=sys_off[1:])
        lin = np.concatenate([t[0] for t in terms])
        off = np.zeros(len(lin) + 1, dtype=np.int64)
        np.cumsum(np.concatenate([np.diff(t[1]) for t in terms]), out=off[1:])
        ta, tb = np.concatenate([t[2] for t in terms]), np.concatenate([t[3] for t in terms])
        rows = max(self._cols, int(np.diff(sys_off).max()))               # (the boundary wants rows >= cols; zero rows come from the device)
        return m4ri_solve_many_quad_packed(lin, off, ta, tb, sys_off, self._lin_size, rows, mode)

    def solve_raw_one_many(self, zeros_list: Sequence[Sequence]) -> list:
        return self._solve_internal_many(zeros_list, 0)

    def solve_raw_space_many(self, zeros_list: Sequence[Sequence]) -> list:
        return self._solve_internal_many(zeros_list, 1)

    def solve_one_many(self, zeros_list: Sequence[Sequence]) -> list:
        return [None if raw is None else self.convert_sol(raw) for raw in self._solve_internal_many(zeros_list, 0)]


# ---- cubic and quartic systems kept factored ------------------------------------------------------------------------------------------
# One and two degrees up: a symbolic bit is a linear form plus products of two, of three and (quartic) of four affine forms, and the rows
# over the n + C(n,2) + C(n,3) columns of degree-3 XL, or those and the C(n,4) of degree-4 XL, come into being on the device
# (k_cubic_expand / k_quartic_expand, through m4ri_solve_cubic_packed / m4ri_solve_quartic_packed / hip.*_expand_words).  The columns
# of degree <= 3 are the same in both layouts, so a product of two or of three forms is the same equation int in both.  Each kind is
# one vector class and one system class over a shared base (_ExactBitVec, _ExactSystem); the two kinds are siblings and do not mix.
def _exact_product_int(forms: tuple, n: int) -> int:
    """the exact product of two or three affine forms (equation ints over n unknowns) as an equation int over the cubic columns:
    bit 0 the constant, bit 1 + c column c of xl3_cols(n), put together from runs of consecutive columns"""
    low = (1 << n) - 1
    a, b = forms[0], forms[1]
    a0, b0, A, B = a & 1, b & 1, (a >> 1) & low, (b >> 1) & low
    l = (A & B) ^ (B if a0 else 0) ^ (A if b0 else 0)                      # the linear part of a b
    k0 = a0 & b0
    pair0, tri0 = 1 + n, 1 + n + n * (n - 1) // 2
    if len(forms) == 2:
        e = k0 | (l << 1)
        for i in range(1, n):
            run = ((B if (A >> i) & 1 else 0) ^ (A if (B >> i) & 1 else 0)) & ((1 << i) - 1)
            e |= run << (pair0 + i * (i - 1) // 2)
        return e
    c = forms[2]
    c0, C = c & 1, (c >> 1) & low
    e = (k0 & c0) | (((C if k0 else 0) ^ (l if c0 else 0) ^ (l & C)) << 1)
    for i in range(1, n):
        ai, bi, ci, li = (A >> i) & 1, (B >> i) & 1, (C >> i) & 1, (l >> i) & 1
        q = (B if ai else 0) ^ (A if bi else 0)                            # pairs (i, .) of a b
        run = (q & (C ^ (low if c0 ^ ci else 0))) ^ (C if li else 0) ^ (l if ci else 0)
        e |= (run & ((1 << i) - 1)) << (pair0 + i * (i - 1) // 2)
        if not (ai | bi | ci):
            continue                                   # (every mask below has a factor from i)
        for j in range(1, i):
            aj, bj, cj = (A >> j) & 1, (B >> j) & 1, (C >> j) & 1
            run = (C if (ai & bj) ^ (aj & bi) else 0) ^ (B if (ai & cj) ^ (aj & ci) else 0) ^ (A if (bi & cj) ^ (bj & ci) else 0)
            e |= (run & ((1 << j) - 1)) << (tri0 + i * (i - 1) * (i - 2) // 6 + j * (j - 1) // 2)
    return e


def _monomial_bit(members: tuple, n: int) -> int:
    """the bit, in an equation int over the quartic columns, of the monomial of these unknowns (descending, four at most): the
    unknowns, then per degree the combinatorial number C(i,k) + C(j,k-1) + ... of its members"""
    k = len(members)
    if k < 2:
        return 1 + members[0] if k else 0
    return 1 + n + sum(comb(n, d) for d in range(2, k)) + sum(comb(g, k - t) for t, g in enumerate(members))


def _monomial_of_bit(bit: int, n: int) -> tuple:
    """the inverse of ``_monomial_bit``"""
    c = bit - 1
    if c < n:
        return (c,) if c >= 0 else ()
    c -= n
    k = 2
    while c >= comb(n, k):
        c -= comb(n, k)
        k += 1
    members = []
    for d in range(k, 0, -1):
        g = d - 1
        while comb(g + 1, d) <= c:
            g += 1
        members.append(g)
        c -= comb(g, d)
    return tuple(members)


def _exact_product4_int(forms: tuple, n: int) -> int:
    """the exact product of four affine forms as an equation int over the quartic columns: ``_exact_product_int`` of three of them,
    multiplied a monomial at a time by the constant and by every unknown of the fourth (x^2 = x: the union of the members)"""
    forms = sorted(forms, key=lambda v: bin(v).count("1"))                 # (the lightest one multiplies, as on the device)
    d, cubic = forms[0], _exact_product_int(tuple(forms[1:]), n)
    factors = ([()] if d & 1 else []) + [(g,) for g in range(n) if (d >> (1 + g)) & 1]
    e = 0
    while cubic:
        low = cubic & -cubic
        cubic ^= low
        m = _monomial_of_bit(low.bit_length() - 1, n)
        for x in factors:
            e ^= 1 << _monomial_bit(tuple(sorted(set(m + x), reverse=True)), n)
    return e


_CUBIC_MIX = ("a PackedQuarticBitVec cannot be mixed with a PackedCubicBitVec: the two kinds carry different groups of products and are "
              "not promoted; write the bits of one system with that system's mul_bit")


class _ExactBitVec(_TermsBitVec):
    """``_TermsBitVec`` whose products are the exact products in GF(2)[x] / (x_i^2 + x_i), of as many affine forms as ``_ARITIES`` says;
    ``_cols(n)``: the columns its bits expand over; ``_REFUSED``: the other kinds of vector, each with the text it is refused with."""
    __slots__ = ()
    _REFUSED: tuple = ()
    _PRODUCT = {2: _exact_product_int, 3: _exact_product_int, 4: _exact_product4_int}

    def _degree(self) -> int:
        """structural: the highest arity the bits have terms of, 1 with none"""
        return next((arity for arity, (_, ops) in zip(self._ARITIES[::-1], self._groups[::-1]) if len(ops[0])), 1)

    def _coerce(self, other, what: str):
        if not isinstance(other, type(self)):
            for cls, text in self._REFUSED:
                if isinstance(other, cls):
                    raise TypeError(text)
            if not isinstance(other, PackedBitVec):
                if isinstance(other, BitVec):
                    raise TypeError("cannot mix packed and tuple-of-int BitVecs")
                raise TypeError(f"{what} needs a {type(self).__name__} or a PackedBitVec")
            other = self._from_rows(other._rows, self._n)
        if other._lin.shape[1] != self._lin.shape[1] or other._n != self._n:
            raise ValueError("Cannot mix bitvecs over different numbers of unknowns")
        return other

    def _eq_ints(self) -> list:
        """every bit as an equation int over the columns of its kind, expanded on the host a product at a time"""
        n = self._n
        ints = lambda rows: [int.from_bytes(r.tobytes(), "little") & ((1 << (n + 1)) - 1) for r in rows]      # noqa: E731
        out = ints(self._lin)
        for arity, (off, ops) in zip(self._ARITIES, self._groups):
            forms = list(zip(*[ints(x) for x in ops]))
            for k in range(len(out)):
                for t in range(off[k], off[k + 1]):
                    out[k] ^= self._PRODUCT[arity](forms[t], n)
        return out

    def evaluate(self, s: int) -> int:
        """Value under the raw point ``s`` over the columns of its kind (bit c = column c: the n unknowns, their pairs, their triples
        and, quartic, their quadruples), as BitVec.evaluate gives it for the expanded bits; on the host."""
        point = ((s << 1) | 1) & ((1 << (self._cols(self._n) + 1)) - 1)
        return sum((bin(e & point).count("1") & 1) << k for k, e in enumerate(self._eq_ints()))


class PackedCubicBitVec(_ExactBitVec):
    """``_ExactBitVec`` with products of two affine forms (bit i owns the operand rows ``_off2[i] .. _off2[i + 1]`` of ``_ta`` /
    ``_tb``) and products of three (``_off3``, ``_ua`` / ``_ub`` / ``_uc``)."""
    __slots__ = ()
    _ARITIES = (2, 3)
    _cols = staticmethod(xl3_cols)
    _REFUSED = ((PackedQuadBitVec, _QUAD_MIX),)
    _off2, _ta, _tb = _part(0), _part(0, 0), _part(0, 1)
    _off3, _ua, _ub, _uc = _part(1), _part(1, 0), _part(1, 1), _part(1, 2)

    def __init__(self, lin, off2, ta, tb, off3, ua, ub, uc, n: int):
        # [k, Wl] uint64, then [k + 1] int64, [T2, Wl] x 2 and [k + 1] int64, [T3, Wl] x 3: immutable
        self._lin, self._groups = lin, ((off2, (ta, tb)), (off3, (ua, ub, uc)))
        self._n = n                                    # unknowns of the system


class PackedQuarticBitVec(_ExactBitVec):
    """``_ExactBitVec`` with products of two affine forms (``_off2``, ``_ta`` / ``_tb``), of three (``_off3``, ``_ua`` / ``_ub`` /
    ``_uc``) and of four (``_off4``, ``_va`` / ``_vb`` / ``_vc`` / ``_vd``)."""
    __slots__ = ()
    _ARITIES = (2, 3, 4)
    _cols = staticmethod(xl4_cols)
    _REFUSED = ((PackedQuadBitVec, _QUAD_MIX), (PackedCubicBitVec, _CUBIC_MIX))
    _off2, _ta, _tb = _part(0), _part(0, 0), _part(0, 1)
    _off3, _ua, _ub, _uc = _part(1), _part(1, 0), _part(1, 1), _part(1, 2)
    _off4, _va, _vb, _vc, _vd = _part(2), _part(2, 0), _part(2, 1), _part(2, 2), _part(2, 3)

    def __init__(self, lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd, n: int):
        # [k, Wl] uint64, then per arity [k + 1] int64 and [T, Wl] per operand: immutable
        self._lin, self._groups = lin, ((off2, (ta, tb)), (off3, (ua, ub, uc)), (off4, (va, vb, vc, vd)))
        self._n = n                                    # unknowns of the system


def _refuse_system(name: str):
    def method(self, *args, **kwargs):
        raise TypeError(f"{name} is not built for a Packed{self._KIND.capitalize()}System")
    method.__name__ = name
    return method


class _ExactSystem(_ProductColumns, PackedLinearSystem):
    """Equations up to the degree of ``_VEC`` (its highest arity) written directly and kept factored: ``gens()`` are PackedLinearSystem's
    PackedBitVecs, ``mul_bit`` multiplies single bits up to that degree (exact products), and the solve methods hand the factored
    arrays to the device (``_SOLVE``), which expands them over ``_VEC._cols`` columns and solves.  ``solve_all`` keeps the points of the
    linearised space whose product coordinates are the products of their linear bits.  ``_KIND``: "cubic" / "quartic"."""

    def __init__(self, sizes: Iterable[int]):
        super().__init__(sizes)
        self._lin_size = sum(self._sizes)
        self._cols = self._VEC._cols(self._lin_size)   # (``_words`` stays the words of a linear form: the generators have no product coordinates)

    def _single(self, a):
        for cls, text in self._VEC._REFUSED:
            if isinstance(a, cls):
                raise TypeError(text)
        if not isinstance(a, (PackedBitVec, self._VEC)):
            raise TypeError(f"mul_bit needs PackedBitVecs or {self._VEC.__name__}s of this system")
        if len(a) != 1:
            raise ValueError("The inputs should be single bits")
        rows = a._rows if isinstance(a, PackedBitVec) else a._lin
        if rows.shape[1] != self._words:
            raise ValueError("Cannot mix bitvecs over different numbers of unknowns")
        return self._VEC._from_rows(rows, self._lin_size) if isinstance(a, PackedBitVec) else a

    def mul_bit(self, a, b):
        """the exact product of two single bits whose degrees (structural: the highest arity a bit has terms of) add up to the
        system's at most.  By distributivity lin_a lin_b is one quadratic term, a product of either bit times the other's linear form
        one term of the next arity (the form appended as one more operand), and two products of two forms one quartic term."""
        a, b = self._single(a), self._single(b)
        da, db, degree = a._degree(), b._degree(), self._VEC._ARITIES[-1]
        if da + db > degree:
            raise TypeError(f"mul_bit of bits of degree {da} and {db} is of degree {da + db}, above {degree}")
        a2, b2 = a._groups[0][1], b._groups[0][1]      # (a term of a's and one of b's whose arities add up to more than the degree cannot both exist)
        by = lambda ops, form: ops + (np.repeat(form, len(ops[0]), axis=0),)                      # noqa: E731
        cat = lambda *groups: [np.concatenate(xs) for xs in zip(*groups)]                          # noqa: E731
        groups = [[a._lin, b._lin], cat(by(a2, b._lin), by(b2, a._lin))]
        if degree == 4:
            a3, b3 = a._groups[1][1], b._groups[1][1]
            ia, ib = np.repeat(np.arange(len(a2[0])), len(b2[0])), np.tile(np.arange(len(b2[0])), len(a2[0]))      # every pair of quadratic terms
            groups.append(cat(by(a3, b._lin), by(b3, a._lin), (a2[0][ia], a2[1][ia], b2[0][ib], b2[1][ib])))
        parts = [x for ops in groups for x in (np.array([0, len(ops[0])], dtype=np.int64), *ops)]
        return self._VEC(np.zeros((1, self._words), dtype=np.uint64), *parts, self._lin_size)

    # -- zeros -> the factored arrays the device expands ----------------------------------------------------------------------------
    def _terms(self, zeros: Sequence):
        """(lin, then per arity its offsets and its operand arrays: off2, ta, tb, off3, ua, ub, uc ...) of all the bits of ``zeros``, in
        order; no row is dropped (_zeros_terms)"""
        return _zeros_terms(zeros, self._VEC, self._KIND, self._words)

    def get_eqs(self, zeros: Sequence) -> list:
        """equation ints over the system's columns, expanded on the device (needs the GPU); zero rows are dropped"""
        from . import hip                              # noqa: PLC0415  (ctypes binding, first use only)
        terms = self._terms(zeros)
        if not len(terms[0]):
            return []
        return _eqs_from_words(getattr(hip, f"{self._KIND}_expand_words")(*terms, self._lin_size), self._cols)

    # -- boundary call ---------------------------------------------------------------------------------------------------------------
    def _solve_internal(self, zeros: Sequence, mode: int):
        terms = self._terms(zeros)
        return self._SOLVE(*terms, self._lin_size, max(len(terms[0]), self._cols), mode)      # (the boundary wants rows >= cols)

    def convert_sol(self, s: int) -> Optional[tuple]:
        """the values of the generators at a raw point over the system's columns whose product coordinates are the products of its
        linear bits, None for any other point"""
        n = self._lin_size
        if not self._xl_products_match(s, n, self._VEC._ARITIES[-1]):
            return None
        return self._convert_sol(s & ((1 << n) - 1))

    def solve_one(self, zeros: Sequence):
        # the particular solution of the linearised system need not be consistent: take the first one that is
        for sol in self.solve_all(zeros):
            return sol
        return None

    def _raw_point(self, lin: int) -> int:
        """the raw point over the system's columns whose linear part is ``lin``"""
        n = self._lin_size
        pi, pj, ti, tj, tl = self._xl_index(n)
        x = np.array([(lin >> i) & 1 for i in range(n)], dtype=np.uint8)
        bits = [x, x[pi] & x[pj], x[ti] & x[tj] & x[tl]]
        if self._VEC._ARITIES[-1] == 4:
            qi, qj, ql, qp = self._xl4_index(n)
            bits.append(x[qi] & x[qj] & x[ql] & x[qp])
        return int.from_bytes(np.packbits(np.concatenate(bits), bitorder="little").tobytes(), "little")

    def evaluate(self, bv, sol: tuple) -> int:
        raw = _raw_value(sol, self._sizes)
        return bv.evaluate(self._raw_point(raw) if isinstance(bv, self._VEC) else raw)


for _name in ("get_rows", "_stack_rows", "_flat_rows", "factor", "bit_assert", "_solve_internal_rhs", "solve_raw_one_rhs", "solve_raw_space_rhs",
              "solve_one_rhs"):
    setattr(_ExactSystem, _name, _refuse_system(_name))
del _name


class PackedCubicSystem(_ExactSystem):
    """``_ExactSystem`` of degree 3, over the n + C(n,2) + C(n,3) columns of degree-3 XL.  The ``*_xl4`` methods are degree-4 XL: the
    device multiplies every expanded equation by 1 and by each unknown too and solves over the n + C(n,2) + C(n,3) + C(n,4) monomials
    of degree <= 4, which takes about C(n,3) / 4 equations where plain linearisation takes about C(n,3).  Its hybrid form, which
    guesses unknowns, is PackedCubicGuessSystem's."""
    _VEC, _KIND, _SOLVE = PackedCubicBitVec, "cubic", staticmethod(m4ri_solve_cubic_packed)

    # -- degree-4 XL: the factored arrays go down, the device expands, multiplies by 1 and by every unknown, pads and solves ----------
    def _solve_internal_xl4(self, zeros: Sequence, mode: int):
        return m4ri_solve_xl4_cubic_packed(*self._terms(zeros), self._lin_size, mode)

    def solve_raw_one_xl4(self, zeros: Sequence):
        return self._solve_internal_xl4(zeros, 0)

    def solve_raw_space_xl4(self, zeros: Sequence):
        return self._solve_internal_xl4(zeros, 1)

    def convert_sol_xl4(self, s: int) -> Optional[tuple]:
        """convert_sol over the quartic columns: the quadruple coordinates are checked too"""
        n = self._lin_size
        if not self._xl_products_match(s, n, 4):
            return None
        return self._convert_sol(s & ((1 << n) - 1))

    def solve_all_xl4(self, zeros: Sequence, *, max_dimension: int = 16):
        """solve_all through degree-4 XL: the consistent points of the quartic system's solution space, in AffineSpace order"""
        yield from _space_points(self.solve_raw_space_xl4(zeros), max_dimension, self.convert_sol_xl4)

    def solve_one_xl4(self, zeros: Sequence):
        for sol in self.solve_all_xl4(zeros):
            return sol
        return None

    def get_eqs_xl4(self, zeros: Sequence) -> list:
        """the equations and their products with every unknown as equation ints over the quartic columns, expanded and multiplied on
        the device (needs the GPU); zero rows are dropped"""
        from . import hip                              # noqa: PLC0415
        terms = self._terms(zeros)
        if not len(terms[0]):
            return []
        return _eqs_from_words(hip.xl4_cubic_expand_words(hip.cubic_expand_words(*terms, self._lin_size), self._lin_size), xl4_cols(self._lin_size))


class PackedCubicGuessSystem(_XlGuess, PackedCubicSystem):
    """A PackedCubicSystem with the hybrid form of degree-4 XL.  The ``*_xl4_guess`` methods have the meaning and the guess parsing of
    the quadratic classes' (_XlGuess): f unknowns are fixed in all 2^f ways, the device substitutes them into the expanded cubic rows
    and solves every assignment's degree-4 XL system in the other n - f unknowns (about cols4(n - f) / (n - f + 1) equations) as one
    batch, a chunk of assignments at a time (hip.xl4_cubic_guess_chunk).  Everything else is PackedCubicSystem's, whose set of public
    names is fixed; the bits of either class work with the other."""

    def _solve_internal_xl4_guess(self, zeros: Sequence, guess: list, mode: int):
        terms = self._terms(zeros)
        return len(terms[0]), lambda first, count: m4ri_solve_xl4_guess_cubic_packed(*terms, self._lin_size, guess, first, count, mode)

    def _xl_guess_chunk(self, degree: int):
        from . import hip                              # noqa: PLC0415  (ctypes binding, first use only)
        return hip.xl4_cubic_guess_chunk

    def _guess_sol(self, full: int) -> tuple:
        return self._convert_sol(full)                 # (this class has no block of product unknowns behind the generators')


class PackedQuarticSystem(_ExactSystem):
    """``_ExactSystem`` of degree 4, over the n + C(n,2) + C(n,3) + C(n,4) columns of degree-4 XL.  Not a PackedCubicSystem: its columns
    differ, and the searches over cubic spaces take anything that is one."""
    _VEC, _KIND, _SOLVE = PackedQuarticBitVec, "quartic", staticmethod(m4ri_solve_quartic_packed)

    def _terms(self, zeros: Sequence):
        if any(isinstance(z, PackedCubicBitVec) for z in zeros):
            raise TypeError(_CUBIC_MIX)
        return super()._terms(zeros)
