"""LinearSystem: the solve front-end that feeds the MI355X solver.

Re-statement (own code) of gf2bv/__init__.py:137-287 of maple3142/gf2bv: same public
surface (``gens``, ``get_eqs``, ``solve_one``, ``solve_all``, ``solve_raw_*``,
``evaluate``, ``convert_sol``, pickling) and the same conventions -- but
``_internal.m4ri_solve`` is the HIP path in libgf2bv_hip.so, not M4RI.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Union

from ._internal import (AffineSpace, QuadSearchGaveUp, eqs_to_sage_mat_helper, m4ri_solve, m4ri_solve_many, m4ri_solve_rhs, m4ri_solve_xl3, m4ri_solve_xl3_guess,
                        m4ri_solve_xl4, m4ri_solve_xl4_guess, mul_bit_quad)
from .bitvec import BitVec

Zeros = Sequence[Union[BitVec, int]]


class DimensionTooLargeError(Exception):
    """Raised by solve_all when the solution space has more than 2**max_dimension points."""

    def __init__(self, message: str, space: AffineSpace):
        super().__init__(message)
        self.space = space


def _refuse_large(space: AffineSpace, max_dimension: int) -> None:
    if space.dimension > max_dimension:
        raise DimensionTooLargeError(
            f"Solution space (dim {space.dimension}) is too large, try increase max_dimension "
            f"({max_dimension}) if you want (there will be 2**dim solutions)",
            space=space,
        )


def _space_points(space: Optional[AffineSpace], max_dimension: int, convert):
    """the points of a solution space (None: no solution) that `convert` keeps, in AffineSpace order"""
    if space is None:
        return
    _refuse_large(space, max_dimension)
    for raw in space:
        sol = convert(raw)
        if sol is not None:
            yield sol


def _raw_value(sol: tuple, sizes: Sequence[int]) -> int:
    """per-variable ints -> the raw int they are the parts of"""
    raw, shift = 0, 0
    for value, width in zip(sol, sizes):
        raw |= value << shift
        shift += width
    return raw


def _eqs_from_words(rows, cols: int) -> list:
    """device rows of the augmented-words layout (column c at bit c, the constant at column `cols`) -> equation ints (bit 0 the
    constant, bit 1 + c column c), zeros dropped"""
    mask = (1 << cols) - 1
    eqs = []
    for r in rows:
        v = int.from_bytes(r.tobytes(), "little")
        eqs.append(((v & mask) << 1) | (v >> cols))
    return [e for e in eqs if e]                       # literal zeros carry no information


class _SolveSurface:
    """What follows the boundary call, shared by ``LinearSystem`` and the packed front-end's ``PackedLinearSystem``: raw solutions
    to per-variable ints and back.  Needs ``_sizes`` and ``_solve_internal(zeros, mode)`` of the class it is mixed into."""

    # -- raw int -> per-variable ints (reference :242-251) ----------------------------------------------
    def _convert_sol(self, s: int) -> tuple:
        parts = []
        for width in self._sizes:
            parts.append(s & ((1 << width) - 1))
            s >>= width
        assert s == 0, "Invalid solution"
        return tuple(parts)

    def convert_sol(self, s: int) -> Optional[tuple]:
        return self._convert_sol(s)

    def solve_raw_one(self, zeros: Zeros):
        return self._solve_internal(zeros, 0)

    def solve_raw_space(self, zeros: Zeros):
        return self._solve_internal(zeros, 1)

    def solve_all(self, zeros: Zeros, *, max_dimension: int = 16):
        yield from _space_points(self.solve_raw_space(zeros), max_dimension, self.convert_sol)

    def solve_one(self, zeros: Zeros):
        raw = self._solve_internal(zeros, 0)
        return None if raw is None else self.convert_sol(raw)

    def evaluate(self, bv: BitVec, sol: tuple) -> int:
        return bv.evaluate(_raw_value(sol, self._sizes))


class LinearSystem(_SolveSurface):
    def __init__(self, sizes: Iterable[int]):
        self._sizes = list(sizes)
        self._cols = sum(self._sizes)
        # bit 0 of an equation int is the constant term; unknown g is bit g+1
        self._basis = [1 << i for i in range(self._cols + 1)]
        gens, at = [], 1
        for width in self._sizes:
            gens.append(BitVec(tuple(self._basis[at:at + width])))
            at += width
        self._vars = tuple(gens)

    def gens(self):
        return self._vars

    def __reduce__(self):
        return (self.__class__, (self._sizes,))

    # -- zeros -> equation ints (reference :214-227) ------------------------------------------------
    def get_eqs(self, zeros: Zeros) -> list:
        flat: list = []
        for z in zeros:
            if isinstance(z, BitVec):
                flat.extend(z._bits)
            else:
                flat.append(z)
        return [e for e in flat if e]          # literal zeros carry no information

    # -- Sage export (reference :167-212) --------------------------------------------------------------------
    def get_sage_mat_slow(self, zeros: Zeros, *, tqdm=lambda x, desc: x):
        """(A, b) over GF(2) with A x = b, as Sage objects -- needs Sage at call time (reference :167-192)."""
        from sage.all import GF, matrix, vector          # noqa: PLC0415  (optional dependency, as in the reference)
        eqs = self.get_eqs(zeros)
        F2 = GF(2)
        b = vector(F2, [e & 1 for e in eqs])
        A = matrix(F2, len(eqs), self._cols)
        for i, e in enumerate(tqdm(eqs, desc="Converting equations")):
            e >>= 1
            while e:
                low = e & -e
                A[i, low.bit_length() - 1] = 1
                e ^= low
        return A, b

    def get_sage_mat(self, zeros: Zeros):
        """(A, b) as Sage objects, the fast way (reference :194-212): the coefficient matrix travels as a two-colour PNG
        (`eqs_to_sage_mat_helper`, _internal.c:678-765 -- written without libgd here) into Sage's own unpickler for
        GF(2) matrices; the affine bits come back as a list of bools.  Needs Sage at call time."""
        import struct                                     # noqa: PLC0415

        from sage.all import GF, vector                   # noqa: PLC0415  (optional dependency, as in the reference)
        from sage.matrix.matrix_mod2_dense import unpickle_matrix_mod2_dense_v2      # noqa: PLC0415

        eqs = self.get_eqs(zeros)
        buf, affine = eqs_to_sage_mat_helper(eqs, self._cols)
        b = vector(GF(2), affine)
        signed = struct.unpack(f">{len(buf)}b", buf)      # Sage wants the PNG as signed chars
        return unpickle_matrix_mod2_dense_v2(len(eqs), self._cols, signed, len(signed), False), b

    # -- boundary call (reference :229-240) ------------------------------------------------------------
    def _solve_internal(self, zeros: Zeros, mode: int):
        eqs = self.get_eqs(zeros)
        if 1 in eqs:                            # the equation "1 = 0"
            return None
        if len(eqs) < self._cols:               # the boundary wants rows >= cols
            eqs.extend([0] * (self._cols - len(eqs)))
        return m4ri_solve(eqs, self._cols, mode)

    # -- batches (no counterpart in the reference) ----------------------------------------------------------
    # Independent instances of the same LinearSystem (one zeros list per instance / per output bit) go to
    # the GPU as ONE call: _internal.m4ri_solve_many -> gf2bv_solve_batch_digits, lock-step gangs.
    # Element i of the result is exactly what the single-system method returns for zeros_list[i].
    # `devices`: None = the module's default device (set_default_device / GF2BV_DEVICE, like solve_one), "all" = every visible
    # GPU, an int, or a sequence of device indices (the systems are sharded in contiguous blocks over them inside the library,
    # one host thread per entry, no collective -- gf2bv_solve_batch_digits_multi).
    def _solve_internal_many(self, zeros_list: Sequence[Zeros], mode: int, devices=None) -> list:
        eqs_list = [self.get_eqs(z) for z in zeros_list]
        live = [i for i, eqs in enumerate(eqs_list) if 1 not in eqs]      # "1 = 0" is decided on the host
        rows = max([self._cols] + [len(eqs_list[i]) for i in live])
        for i in live:
            eqs_list[i].extend([0] * (rows - len(eqs_list[i])))
        out: list = [None] * len(eqs_list)
        if live:
            for i, res in zip(live, m4ri_solve_many([eqs_list[i] for i in live], self._cols, mode, devices)):
                out[i] = res
        return out

    def solve_raw_one_many(self, zeros_list: Sequence[Zeros], devices=None) -> list:
        return self._solve_internal_many(zeros_list, 0, devices)

    def solve_raw_space_many(self, zeros_list: Sequence[Zeros], devices=None) -> list:
        return self._solve_internal_many(zeros_list, 1, devices)

    def solve_one_many(self, zeros_list: Sequence[Zeros], devices=None) -> list:
        return [None if raw is None else self.convert_sol(raw)
                for raw in self._solve_internal_many(zeros_list, 0, devices)]

    # -- many right-hand sides of one matrix (no counterpart in the reference) -------------------------------------------
    # Instances that share every coefficient and differ only in constants -- the recovery workloads' outputs enter only as
    # `expr ^ observed` -- go to the GPU as ONE elimination: _internal.m4ri_solve_rhs -> gf2bv_solve_rhs_digits.  Element i of
    # the result is exactly what the single-system method returns for [e ^ v for e, v in zip(exprs, values_list[i])].
    def _rhs_eqs(self, exprs: Zeros, values_list: Sequence[Sequence[int]]):
        """exprs flattened once into equation ints, and one right-hand-side int per instance: bit r = the constant term of
        equation r in that instance (exprs[k] ^ values_list[i][k], as BitVec.__xor__ / int ^ would form it).  Rows whose
        coefficient part is zero are kept: with constant 1 such a row is the equation "1 = 0" and the solver reports exactly
        that instance inconsistent (_solve_internal's `1 in eqs`), with constant 0 it is the literal zero get_eqs drops --
        an all-zero row changes no pivot, origin or basis."""
        eqs: list = []
        spans: list = []                       # per element of exprs: (first row, width) -- width None: an equation int
        for e in exprs:
            if isinstance(e, BitVec):
                spans.append((len(eqs), len(e._bits)))
                eqs.extend(e._bits)
            else:
                spans.append((len(eqs), None))
                eqs.append(e)
        consts = 0
        for r, e in enumerate(eqs):
            if e & 1:
                consts |= 1 << r
        rhs = []
        for vals in values_list:
            vals = list(vals)
            if len(vals) != len(spans):
                raise ValueError(f"{len(vals)} values for {len(spans)} expressions")
            b = consts
            for (at, width), v in zip(spans, vals):
                if width is None:
                    if v not in (0, 1):
                        raise ValueError("the value of an equation int must be 0 or 1")
                    b ^= int(v) << at
                else:
                    b ^= (abs(v) & ((1 << width) - 1)) << at          # (to_bits: the low `width` bits of |v|)
            rhs.append(b)
        return eqs, rhs

    def _solve_internal_rhs(self, exprs: Zeros, values_list: Sequence[Sequence[int]], mode: int) -> list:
        eqs, rhs = self._rhs_eqs(exprs, values_list)
        if not rhs:
            return []
        if len(eqs) < self._cols:               # the boundary wants rows >= cols (zero rows, constant 0 in every instance)
            eqs.extend([0] * (self._cols - len(eqs)))
        return m4ri_solve_rhs(eqs, self._cols, mode, rhs)

    def solve_raw_one_rhs(self, exprs: Zeros, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve_internal_rhs(exprs, values_list, 0)

    def solve_raw_space_rhs(self, exprs: Zeros, values_list: Sequence[Sequence[int]]) -> list:
        return self._solve_internal_rhs(exprs, values_list, 1)

    def solve_one_rhs(self, exprs: Zeros, values_list: Sequence[Sequence[int]]) -> list:
        return [None if raw is None else self.convert_sol(raw) for raw in self._solve_internal_rhs(exprs, values_list, 0)]

    def factor(self, exprs: Zeros, device=None):
        """The coefficient matrix of `exprs` factored once on the GPU: a FactoredSystem whose methods take the observed values
        (one per expression) and equal this system's methods on [e ^ v for e, v in zip(exprs, values)].  Needs numpy."""
        from .factored import FactoredSystem     # noqa: PLC0415  (numpy on first use only)
        return FactoredSystem(self, exprs, device)


# -- the columns of degree-3 XL: the n unknowns, their pairs, their triples -----------------------------------------
def xl3_cols(n: int) -> int:
    return n + n * (n - 1) // 2 + n * (n - 1) * (n - 2) // 6


def xl3_pair_col(n: int, i: int, j: int) -> int:
    """column of x_i x_j, j < i: QuadraticSystem's"""
    assert 0 <= j < i < n
    return n + i * (i - 1) // 2 + j


def xl3_triple_col(n: int, i: int, j: int, l: int) -> int:
    """column of x_i x_j x_l, l < j < i"""
    assert 0 <= l < j < i < n
    return n + n * (n - 1) // 2 + i * (i - 1) * (i - 2) // 6 + j * (j - 1) // 2 + l


# -- degree 4 adds the quadruples behind degree 3's columns ---------------------------------------------------------------------------------
def xl4_cols(n: int) -> int:
    return xl3_cols(n) + n * (n - 1) * (n - 2) * (n - 3) // 24


def xl4_quad_col(n: int, i: int, j: int, l: int, p: int) -> int:
    """column of x_i x_j x_l x_p, p < l < j < i"""
    assert 0 <= p < l < j < i < n
    return xl3_cols(n) + i * (i - 1) * (i - 2) * (i - 3) // 24 + j * (j - 1) * (j - 2) // 6 + l * (l - 1) // 2 + p


class _ProductColumns:
    """The product columns behind the n unknowns -- pairs, triples and (degree 4) quadruples, in the order of xl3_cols / xl4_cols -- as
    index arrays, and the test that a raw point's product coordinates are the products of its linear bits.  For every system whose
    columns are those: the XL methods of the quadratic classes, the packed cubic and quartic systems."""

    def _xl_index(self, n: Optional[int] = None):
        """(bit position of every coordinate's members) index arrays of the pair and the triple columns over n unknowns (default: the
        system's), built once per n"""
        n = self._lin_size if n is None else n
        cache = self.__dict__.setdefault("_xl_index_cache", {})
        idx = cache.get(n)
        if idx is None:
            import numpy as np                         # noqa: PLC0415  (first use only: the package imports without numpy)
            pi, pj = np.tril_indices(n, -1)            # (1,0) (2,0) (2,1) ...: pair (i, j) at i(i-1)/2 + j
            a = np.arange(n)
            ti, tj, tl = np.nonzero((a[:, None, None] > a[None, :, None]) & (a[None, :, None] > a[None, None, :]))      # i, then j, then l
            idx = cache[n] = (pi, pj, ti, tj, tl)
        return idx

    def _xl4_index(self, n: int):
        """the same for the quadruple columns: i, then j, then l, then p"""
        cache = self.__dict__.setdefault("_xl4_index_cache", {})
        idx = cache.get(n)
        if idx is None:
            import numpy as np                         # noqa: PLC0415
            a = np.arange(n)
            idx = cache[n] = np.nonzero((a[:, None, None, None] > a[None, :, None, None]) & (a[None, :, None, None] > a[None, None, :, None])
                                        & (a[None, None, :, None] > a[None, None, None, :]))
        return idx

    def _xl_products_match(self, s: int, n: int, degree: int = 3) -> bool:
        """every pair and triple (degree 4: and quadruple) coordinate of a raw point over the XL columns of n unknowns is the product
        of its linear bits"""
        import numpy as np                             # noqa: PLC0415
        cols3 = xl3_cols(n)
        cols = xl4_cols(n) if degree == 4 else cols3
        assert s >> cols == 0, "Invalid solution"
        bits = np.unpackbits(np.frombuffer(s.to_bytes((cols + 7) // 8, "little"), dtype=np.uint8), bitorder="little")[:cols]
        pi, pj, ti, tj, tl = self._xl_index(n)
        lin, pairs, triples = bits[:n], bits[n:n + len(pi)], bits[n + len(pi):cols3]
        if not (np.array_equal(pairs, lin[pi] & lin[pj]) and np.array_equal(triples, lin[ti] & lin[tj] & lin[tl])):
            return False
        if degree == 4:
            qi, qj, ql, qp = self._xl4_index(n)
            return bool(np.array_equal(bits[cols3:], lin[qi] & lin[qj] & lin[ql] & lin[qp]))
        return True


class _XlGuess:
    """The driver of hybrid XL: the guess parsed, every assignment's system solved a chunk at a time, the raw points scattered back over
    all unknowns; and the ``*_xl4_guess`` methods on top of it.  The class mixed into supplies ``_lin_size``, ``_xl_products_match``
    (_ProductColumns), ``_solve_internal_xl4_guess(zeros, guess, mode)`` (degree 3: ``_solve_internal_xl_guess``) -> None (every
    assignment inconsistent) or (number of equations, run) with run(first, count) the list of raw results of the assignments
    first .. first + count - 1, ``_xl_guess_chunk(degree)`` (the library's chunk function for its systems) and ``_guess_sol(full)`` (its
    solution tuple of a point over all unknowns)."""

    def _parse_guess(self, guess) -> list:
        """the flattened unknown index of every item: an int, or a one-bit BitVec / PackedBitVec that is exactly one unknown"""
        n = self._lin_size
        out = []
        for item in guess:
            if isinstance(item, BitVec):
                bits = item._bits
                v = bits[0] if len(bits) == 1 else 0
                if v < 2 or v & (v - 1) or v.bit_length() - 2 >= n:
                    raise ValueError("a guessed bit must be exactly one unknown")
                idx = v.bit_length() - 2
            elif isinstance(item, int) and not isinstance(item, bool):
                idx = item
            else:
                raise ValueError("a guess is an unknown index or a one-bit BitVec")
            if not 0 <= idx < n:
                raise ValueError(f"guessed unknown {idx} is not in 0..{n - 1}")
            if idx in out:
                raise ValueError(f"unknown {idx} is guessed twice")
            out.append(idx)
        if len(out) > min(n - 1, 30):
            raise ValueError(f"at most min(n - 1, 30) = {min(n - 1, 30)} unknowns can be guessed, not {len(out)}")
        return out

    def _xl_guess_chunks(self, zeros: Zeros, guess, assignments, mode: int, degree: int = 3):
        """(first assignment, raw results) chunk by chunk, the next chunk solved only when it is asked for"""
        g = self._parse_guess(guess)
        first, count = (0, 1 << len(g)) if assignments is None else assignments
        if first < 0 or count < 0 or first + count > 1 << len(g):
            raise ValueError(f"assignments must be a range (first, count) inside 0..{(1 << len(g)) - 1}")
        staged = (self._solve_internal_xl4_guess if degree == 4 else self._solve_internal_xl_guess)(zeros, g, mode)
        if staged is None:
            yield first, [None] * count
            return
        m, run = staged
        chunk = self._xl_guess_chunk(degree)(m, self._lin_size, len(g))
        if chunk < 1:
            raise MemoryError(f"one assignment's degree-{degree} XL system does not fit a quarter of the free device memory")
        end = first + count
        while first < end:
            na = min(chunk, end - first)
            yield first, run(first, na)
            first += na

    def _scatter_guess(self, raw: int, g: list, assignment: int, degree: int = 3) -> Optional[tuple]:
        n = self._lin_size
        ns = n - len(g)
        if not self._xl_products_match(raw, ns, degree):
            return None
        full = 0
        for t, idx in enumerate(g):
            full |= ((assignment >> t) & 1) << idx
        rest = [u for u in range(n) if u not in g]
        for k, u in enumerate(rest):
            full |= ((raw >> k) & 1) << u
        return self._guess_sol(full)

    def _solve_all_xl_guess(self, zeros: Zeros, guess, max_dimension: int, assignments, degree: int):
        g = self._parse_guess(guess)
        for first, spaces in self._xl_guess_chunks(zeros, g, assignments, 1, degree):
            for k, space in enumerate(spaces):
                if space is None:
                    continue
                if space.dimension > max_dimension:
                    raise DimensionTooLargeError(
                        f"Solution space of assignment {first + k} (dim {space.dimension}) is too large, try increase max_dimension "
                        f"({max_dimension}) or guess more unknowns (there will be 2**dim solutions)",
                        space=space,
                    )
                for raw in space:
                    sol = self._scatter_guess(raw, g, first + k, degree)
                    if sol is not None:
                        yield sol

    def solve_raw_one_xl4_guess(self, zeros: Zeros, guess, assignments=None) -> list:
        """solve_raw_one_xl_guess over the quartic columns of the remaining unknowns"""
        return [raw for _, raws in self._xl_guess_chunks(zeros, guess, assignments, 0, 4) for raw in raws]

    def solve_raw_space_xl4_guess(self, zeros: Zeros, guess, assignments=None) -> list:
        """solve_raw_space_xl_guess over the quartic columns of the remaining unknowns"""
        return [raw for _, raws in self._xl_guess_chunks(zeros, guess, assignments, 1, 4) for raw in raws]

    def convert_sol_xl4_guess(self, raw: int, guess, assignment: int) -> Optional[tuple]:
        """convert_sol_xl_guess of a raw point over the quartic columns of the remaining unknowns"""
        return self._scatter_guess(raw, self._parse_guess(guess), assignment, 4)

    def solve_all_xl4_guess(self, zeros: Zeros, guess, *, max_dimension: int = 16, assignments=None):
        """solve_all_xl_guess with every assignment's degree-4 XL system (about (n - f)^2 / 12 equations)"""
        return self._solve_all_xl_guess(zeros, guess, max_dimension, assignments, 4)

    def solve_one_xl4_guess(self, zeros: Zeros, guess, *, max_dimension: int = 16):
        for sol in self.solve_all_xl4_guess(zeros, guess, max_dimension=max_dimension):
            return sol
        return None


class _QuadraticPoints(_ProductColumns, _XlGuess):
    """What a linearised quadratic system does with the solutions of its linear solve, shared by ``QuadraticSystem`` and the packed
    front-end's ``PackedQuadraticSystem``: the points whose product unknowns equal the products of their linear part.  Needs
    ``_lin_size`` / ``_quad_size`` / ``_quad_sizes``, ``_convert_sol`` and ``solve_raw_space`` / ``solve_raw_space_rhs`` / ``solve_all`` of the
    class it is mixed into."""

    def _products_match(self, lin: int, quad: int) -> bool:
        n = self._lin_size
        for i in range(n):
            if (lin >> i) & 1:
                # products with x_i = 1: pairs (i, j) for j < i must repeat the low i bits of lin
                want = lin & ((1 << i) - 1)
            else:
                want = 0
            if quad & ((1 << i) - 1) != want:
                return False
            quad >>= i
        assert quad == 0, "Invalid quadratic part"
        return True

    def convert_sol(self, s: int) -> Optional[tuple]:
        lin = s & ((1 << self._lin_size) - 1)
        quad = s >> self._lin_size
        assert quad >> self._quad_size == 0, "Invalid solution"
        if not self._products_match(lin, quad):
            return None
        return self._convert_sol(lin)[:-1]

    def solve_one(self, zeros: Zeros):
        # the particular solution of the linearised system need not be consistent: take the first one that is
        for sol in self.solve_all(zeros):
            return sol
        return None

    # -- the consistent points on the GPU (no counterpart in the reference) -------------------------------------------------
    # solve_all walks all 2^d points of the linearised space on the host; search_all reduces the space to quadratic forms in
    # r_eff <= r variables (r: the rank of its projection onto the linear unknowns) and finds their common zeros on the device
    # (AffineSpace.quad_search -> gf2bv_quad_search).  Same elements in the same order as solve_all,
    # at any dimension.
    def _search_space(self, space, max_enum: int, max_solutions: int, first: bool = False) -> list:
        try:
            raws = space.quad_search(self._lin_size, max_enum, max_solutions, first)
        except QuadSearchGaveUp as e:
            raise DimensionTooLargeError(f"Solution space (dim {space.dimension}): {e.args[0]}", space=space) from None
        out = []
        for raw in raws:
            sol = self.convert_sol(raw)
            if sol is None:
                raise RuntimeError("quad_search returned an inconsistent point")
            out.append(sol)
        return out

    def search_all(self, zeros: Zeros, *, max_enum: int = 32, max_solutions: int = 65536) -> list:
        """list(solve_all(zeros, max_dimension=d)) without the 2^d walk; DimensionTooLargeError (with .space) when the search
        gives up, ValueError when there are more than max_solutions consistent points."""
        space = self.solve_raw_space(zeros)
        if space is None:
            return []
        return self._search_space(space, max_enum, max_solutions)

    def search_one(self, zeros: Zeros, *, max_enum: int = 32):
        """solve_one(zeros) at any dimension: the first consistent point in iteration order, None if there is none."""
        space = self.solve_raw_space(zeros)
        if space is None:
            return None
        sols = self._search_space(space, max_enum, 1, first=True)
        return sols[0] if sols else None

    def solve_one_rhs(self, exprs: Zeros, values_list: Sequence[Sequence[int]], *, max_dimension: int = 16) -> list:
        """solve_one for every instance (the first element of its solve_all that passes convert_sol, None if there is none),
        from ONE elimination (solve_raw_space_rhs); DimensionTooLargeError as solve_all raises it."""
        out = []
        for space in self.solve_raw_space_rhs(exprs, values_list):
            sol = None
            if space is not None:
                _refuse_large(space, max_dimension)
                for raw in space:
                    sol = self.convert_sol(raw)
                    if sol is not None:
                        break
            out.append(sol)
        return out

    # -- degree-3 XL (no counterpart in the reference) ----------------------------------------------------------
    # Every equation is multiplied by 1 and by each unknown on the device and the system is linearised over the n + C(n,2) + C(n,3)
    # monomials of degree <= 3 (xl3_cols): about n^2 / 6 independent quadratic equations pin the solution down where plain
    # linearisation needs n^2 / 2.  The class mixed into supplies _solve_internal_xl(zeros, mode, degree) and get_eqs_xl(zeros).
    # Degree-4 XL (the *_xl4 methods) multiplies by every pair x_a x_b too and linearises over the monomials of degree <= 4 (xl4_cols): about
    # n^2 / 12 equations.  The multipliers reach the equations' own degree, so f_i f_j = f_j f_i and f_i f_i = f_i: the m(1 + n + C(n,2))
    # rows have rank at most that minus m + C(m,2).  Both degrees run through the same methods underneath, which take the degree.
    @staticmethod
    def _check_degree(degree: int):
        if degree != 3:
            raise ValueError(f"XL is built for degree 3 only (multipliers 1 and x_k), not degree {degree!r}")

    def solve_raw_one_xl(self, zeros: Zeros):
        return self._solve_internal_xl(zeros, 0)

    def solve_raw_one_xl4(self, zeros: Zeros):
        return self._solve_internal_xl(zeros, 0, 4)

    def solve_raw_space_xl4(self, zeros: Zeros):
        return self._solve_internal_xl(zeros, 1, 4)

    def solve_raw_space_xl(self, zeros: Zeros):
        return self._solve_internal_xl(zeros, 1)

    def convert_sol_xl(self, s: int) -> Optional[tuple]:
        """the linear parts of a raw point over the cubic columns when every pair and triple coordinate is the product of its linear
        bits, None otherwise"""
        n = self._lin_size
        if not self._xl_products_match(s, n):
            return None
        return self._convert_sol(s & ((1 << n) - 1))[:-1]

    def convert_sol_xl4(self, s: int) -> Optional[tuple]:
        """convert_sol_xl over the quartic columns: the quadruple coordinates are checked too"""
        n = self._lin_size
        if not self._xl_products_match(s, n, 4):
            return None
        return self._convert_sol(s & ((1 << n) - 1))[:-1]

    def solve_all_xl(self, zeros: Zeros, *, degree: int = 3, max_dimension: int = 16):
        """solve_all through degree-3 XL: the consistent points of the cubic system's solution space, in AffineSpace order"""
        self._check_degree(degree)
        return self._solve_all_xl(zeros, max_dimension, 3)

    def solve_all_xl4(self, zeros: Zeros, *, max_dimension: int = 16):
        """solve_all through degree-4 XL (multipliers 1, x_k and x_a x_b; about n^2 / 12 equations): the consistent points of the
        quartic system's solution space, in AffineSpace order"""
        return self._solve_all_xl(zeros, max_dimension, 4)

    def solve_one_xl4(self, zeros: Zeros):
        for sol in self.solve_all_xl4(zeros):
            return sol
        return None

    def _solve_all_xl(self, zeros: Zeros, max_dimension: int, degree: int):
        convert = self.convert_sol_xl4 if degree == 4 else self.convert_sol_xl
        yield from _space_points(self._solve_internal_xl(zeros, 1, degree), max_dimension, convert)

    def solve_one_xl(self, zeros: Zeros, *, degree: int = 3):
        self._check_degree(degree)
        for sol in self.solve_all_xl(zeros):
            return sol
        return None

    # -- hybrid XL (no counterpart in the reference) -------------------------------------------------------------
    # With fewer equations than degree-3 XL needs, f unknowns are fixed in all 2^f ways: assignment a sets unknown guess[t] to bit t of
    # a and leaves a quadratic system in the other n - f unknowns (renumbered in increasing index), which needs about (n - f)^2 / 6
    # equations.  The device substitutes, multiplies and solves every assignment's system as one batch.  The driver and the degree-4
    # methods are _XlGuess's, which says what the class mixed into supplies.
    def _xl_guess_chunk(self, degree: int):
        """the library's chunk function for this class's systems of that degree"""
        from . import hip                              # noqa: PLC0415  (ctypes binding, first use only)
        return hip.xl4_guess_chunk if degree == 4 else hip.xl3_guess_chunk

    def solve_raw_one_xl_guess(self, zeros: Zeros, guess, assignments=None) -> list:
        """one particular solution (or None) per assignment, over the cubic columns of the remaining unknowns"""
        return [raw for _, raws in self._xl_guess_chunks(zeros, guess, assignments, 0) for raw in raws]

    def solve_raw_space_xl_guess(self, zeros: Zeros, guess, assignments=None) -> list:
        """one AffineSpace (or None) per assignment -- `assignments` = (first, count), default all 2^f -- over the cubic columns of the
        remaining unknowns"""
        return [raw for _, raws in self._xl_guess_chunks(zeros, guess, assignments, 1) for raw in raws]

    def convert_sol_xl_guess(self, raw: int, guess, assignment: int) -> Optional[tuple]:
        """convert_sol_xl of a raw point of assignment `assignment`'s system: the check over the remaining unknowns, then their bits
        and the guessed ones scattered into the solution; None when a product coordinate disagrees"""
        g = self._parse_guess(guess)
        return self._scatter_guess(raw, g, assignment)

    def _guess_sol(self, full: int) -> tuple:
        return self._convert_sol(full)[:-1]            # (without the trailing block of the product unknowns)

    def solve_all_xl_guess(self, zeros: Zeros, guess, *, degree: int = 3, max_dimension: int = 16, assignments=None):
        """the consistent points of every assignment's degree-3 XL system, in assignment order and within an assignment in AffineSpace
        order; the assignments are solved a chunk at a time (hip.xl3_guess_chunk), the next chunk when more is asked for"""
        self._check_degree(degree)
        return self._solve_all_xl_guess(zeros, guess, max_dimension, assignments, 3)

    def solve_one_xl_guess(self, zeros: Zeros, guess, *, degree: int = 3, max_dimension: int = 16):
        for sol in self.solve_all_xl_guess(zeros, guess, degree=degree, max_dimension=max_dimension):
            return sol
        return None

    def _xl_eqs(self, quad, degree: int = 3) -> list:
        """quadratic rows of the augmented-words layout -> the equation ints of their XL rows of that degree (bit 0 the constant,
        bit 1 + c column c), multiplied on the device, zeros dropped"""
        from . import hip                              # noqa: PLC0415  (ctypes binding, first use only)
        if not len(quad):
            return []
        if degree == 4:
            return _eqs_from_words(hip.xl4_expand_words(quad, self._lin_size), xl4_cols(self._lin_size))
        return _eqs_from_words(hip.xl3_expand_words(quad, self._lin_size), xl3_cols(self._lin_size))

    def evaluate(self, bv: BitVec, sol: tuple) -> int:
        return bv.evaluate(_raw_value(sol, self._quad_sizes))


class QuadraticSystem(_QuadraticPoints, LinearSystem):
    """Quadratic equations over GF(2) by linearisation: on top of the n unknowns of ``sizes`` every product
    x_i x_j (j < i) is an unknown of its own, n(n-1)/2 of them after the linear ones, and the linearised system
    goes through the same solve path (e.g. 128 unknowns -> 8256 columns, the NLFSR example).  Solutions whose
    "product" unknowns do not equal the products of their linear part are filtered out by ``convert_sol``.

    Own restatement of gf2bv/__init__.py:290-408 (same surface: ``gens``, ``mul_bit``, ``bit_assert``,
    ``convert_sol``, ``solve_one`` = first of ``solve_all``, ``evaluate``, pickling).  One convention of the
    reference is kept on purpose: ``mul_bit`` combines the constant / linear parts of its operands as
    ``a & b`` (x_i^2 = x_i), i.e. the constant x linear cross terms are not formed -- callers multiply
    bits without constant terms (gf2bv/__init__.py:334-338)."""

    def __init__(self, sizes: Iterable[int]):
        sizes = list(sizes)
        n = sum(sizes)
        pairs = n * (n - 1) // 2
        super().__init__(sizes + [pairs])
        self._quad_sizes = sizes
        self._lin_size = n
        self._quad_size = pairs
        self._const_lin_mask = (1 << (n + 1)) - 1          # constant bit + the n linear unknowns

    def gens(self):
        return super().gens()[:-1]                          # the block of product unknowns is internal

    def __reduce__(self):
        return (self.__class__, (self._quad_sizes,))

    # product of two single-bit expressions, as an equation int over the linearised unknowns
    def _mul_bit(self, a: int, b: int) -> int:
        low = (a & self._const_lin_mask) & b
        # pair (i, j), j < i, sits at bit 1 + n + i(i-1)/2 + j; it is present iff a_i b_j + a_j b_i = 1
        return mul_bit_quad(self._lin_size, a >> 1, b >> 1, low, self._basis)

    def mul_bit(self, a: BitVec, b: BitVec) -> BitVec:
        if len(a) != 1 or len(b) != 1:
            raise ValueError("The inputs should be single bits")
        return BitVec((self._mul_bit(a._bits[0], b._bits[0]),))

    # "bit a equals v" plus everything that follows from it after multiplying by each unknown
    def _bit_assert(self, a: int, v: int) -> list:
        assert v in (0, 1), "Invalid bit"
        assert a not in (0, 1), "a should not be a constant"
        # DEVIATION from the reference, on purpose and documented: gf2bv/__init__.py:349 asserts
        # `a >> self._lin_size == 0`, which rejects every expression that contains the LAST linear unknown (bit
        # lin_size of an equation int: bit 0 is the constant, unknown g is bit g + 1) although it is a linear term;
        # the bound that matches the representation is lin_size + 1.  Every input the reference accepts gives the
        # same zeros here; inputs it rejects by that off-by-one are accepted.
        assert a >> (self._lin_size + 1) == 0, "Not a linear term"
        zeros = [a ^ v]
        for i in range(1, self._lin_size + 1):
            x = self._basis[i]
            if x == a:
                continue
            zeros.append(self._mul_bit(a, x) ^ (x if v else 0))     # a * x = v * x
        return zeros

    def bit_assert(self, a: BitVec, v: int) -> Zeros:
        if len(a) != 1:
            raise ValueError("The input should be a single bit")
        return self._bit_assert(a._bits[0], v)

    # -- degree-3 XL: the equation ints go down as they are, the device multiplies and pads them ------------------------------------------
    def _solve_internal_xl(self, zeros: Zeros, mode: int, degree: int = 3):
        eqs = self.get_eqs(zeros)
        if 1 in eqs:                            # the equation "1 = 0"
            return None
        return (m4ri_solve_xl4 if degree == 4 else m4ri_solve_xl3)(eqs, self._lin_size, mode)

    def _solve_internal_xl_guess(self, zeros: Zeros, guess: list, mode: int):
        return self._stage_xl_guess(zeros, guess, mode, 3)

    def _solve_internal_xl4_guess(self, zeros: Zeros, guess: list, mode: int):
        return self._stage_xl_guess(zeros, guess, mode, 4)

    def _stage_xl_guess(self, zeros: Zeros, guess: list, mode: int, degree: int):
        eqs = self.get_eqs(zeros)
        if 1 in eqs:                            # the equation "1 = 0": under every assignment
            return None
        solve = m4ri_solve_xl4_guess if degree == 4 else m4ri_solve_xl3_guess
        return len(eqs), lambda first, count: solve(eqs, self._lin_size, guess, first, count, mode)

    def get_eqs_xl(self, zeros: Zeros) -> list:
        """the equations and their products with every unknown as equation ints over the cubic columns (needs the GPU and numpy)"""
        return self._get_eqs_xl(zeros, 3)

    def get_eqs_xl4(self, zeros: Zeros) -> list:
        """the equations and their products with every unknown and every pair of unknowns as equation ints over the quartic columns"""
        return self._get_eqs_xl(zeros, 4)

    def _get_eqs_xl(self, zeros: Zeros, degree: int) -> list:
        import numpy as np                             # noqa: PLC0415
        eqs = self.get_eqs(zeros)
        words = (self._cols + 1 + 63) // 64
        mask = (1 << self._cols) - 1
        quad = np.zeros((len(eqs), words), dtype=np.uint64)
        for r, e in enumerate(eqs):
            quad[r] = np.frombuffer((((e >> 1) & mask) | ((e & 1) << self._cols)).to_bytes(8 * words, "little"), dtype=np.uint64)
        return self._xl_eqs(quad, degree)
