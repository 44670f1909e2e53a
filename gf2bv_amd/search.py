"""The consistent points of a solution space over the degree-3 columns, searched on the GPU (no counterpart in the reference).

``solve_all_xl`` of the quadratic front-ends and ``PackedCubicSystem.solve_all`` walk all 2^d points of the linearised space on the
host and refuse above ``max_dimension``.  The functions here reduce the same space to cubic forms in r_eff <= r <= n variables
(r: the rank of its projection onto the n linear unknowns) and find their common zeros on the device
(``AffineSpace.cubic_search`` -> gf2bv_cubic_search): the same elements in the same order, at any dimension.
With n <= max_enum the search never gives up -- it is then the fast exhaustive search of Bouillaguet et al. (CHES 2010) on the
original equations, whatever the linearisation left.  They are functions, not methods: the classes' public names are fixed."""
from __future__ import annotations

import sys
from typing import Sequence

from ._internal import CubicSearchGaveUp, QuarticSearchGaveUp
from .linsys import DimensionTooLargeError, _QuadraticPoints

__all__ = ["search_all_cubic", "search_all_xl", "search_one_cubic", "search_one_xl"]


def _xl_parts(q):
    if not isinstance(q, _QuadraticPoints):
        raise TypeError(f"search_*_xl needs a QuadraticSystem or a PackedQuadraticSystem, not {type(q).__name__}")
    return q.solve_raw_space_xl, q.convert_sol_xl


def _cubic_parts(c):
    packed = sys.modules.get(__package__ + ".packed")      # (not loaded: nothing can be an instance of its classes)
    if packed is None or not isinstance(c, packed.PackedCubicSystem):
        raise TypeError(f"search_*_cubic needs a PackedCubicSystem (or a subclass of it), not {type(c).__name__}")
    return c.solve_raw_space, c.convert_sol


_GAVE_UP = {"cubic": CubicSearchGaveUp, "quartic": QuarticSearchGaveUp}


def _search(parts, system, zeros: Sequence, max_enum: int, max_solutions: int, first: bool, kind: str = "cubic") -> list:
    """the body of every search_* function here and in search4.py; kind: the AffineSpace method, cubic_search or quartic_search"""
    solve, convert = parts(system)
    space = solve(zeros)
    if space is None:
        return []
    try:
        raws = getattr(space, kind + "_search")(system._lin_size, max_enum, max_solutions, first)
    except _GAVE_UP[kind] as e:
        raise DimensionTooLargeError(f"Solution space (dim {space.dimension}): {e.args[0]}", space=space) from None
    out = []
    for raw in raws:
        sol = convert(raw)
        if sol is None:
            raise RuntimeError(f"{kind}_search returned an inconsistent point")
        out.append(sol)
    return out


def search_all_xl(q, zeros: Sequence, *, max_enum: int = 32, max_solutions: int = 65536) -> list:
    """list(q.solve_all_xl(zeros, max_dimension=d)) without the 2^d walk, for a QuadraticSystem or a PackedQuadraticSystem;
    DimensionTooLargeError (with .space) when the search gives up, ValueError when there are more than max_solutions points."""
    return _search(_xl_parts, q, zeros, max_enum, max_solutions, False)


def search_one_xl(q, zeros: Sequence, *, max_enum: int = 32):
    """the first element of search_all_xl, None if there is none"""
    sols = _search(_xl_parts, q, zeros, max_enum, 1, True)
    return sols[0] if sols else None


def search_all_cubic(c, zeros: Sequence, *, max_enum: int = 32, max_solutions: int = 65536) -> list:
    """list(c.solve_all(zeros, max_dimension=d)) without the 2^d walk, for a PackedCubicSystem; exceptions as search_all_xl"""
    return _search(_cubic_parts, c, zeros, max_enum, max_solutions, False)


def search_one_cubic(c, zeros: Sequence, *, max_enum: int = 32):
    """the first element of search_all_cubic, None if there is none"""
    sols = _search(_cubic_parts, c, zeros, max_enum, 1, True)
    return sols[0] if sols else None
