"""The consistent points of a solution space over the degree-4 columns, searched on the GPU (no counterpart in the reference).

``PackedQuarticSystem.solve_all`` and ``solve_all_xl4`` of the quadratic front-ends and of ``PackedCubicSystem`` walk all 2^d points
of the linearised space on the host and refuse above ``max_dimension``.  The functions here are ``search.py``'s one degree up: the
same space is reduced to quartic forms in r_eff <= r <= n variables and their common zeros are found on the device
(``AffineSpace.quartic_search`` -> gf2bv_quartic_search): the same elements in the same order, at any dimension,
and with n <= max_enum the search never gives up.  They are functions, not methods: the classes' public names are fixed."""
from __future__ import annotations

import sys
from typing import Sequence

from .linsys import _QuadraticPoints
from .search import _search

__all__ = ["search_all_quartic", "search_all_xl4", "search_one_quartic", "search_one_xl4"]


def _packed(name: str):
    packed = sys.modules.get(__package__ + ".packed")      # (not loaded: nothing can be an instance of its classes)
    return getattr(packed, name) if packed is not None else ()


def _xl4_parts(system):
    if not isinstance(system, _QuadraticPoints) and not isinstance(system, _packed("PackedCubicSystem")):
        raise TypeError("search_*_xl4 needs a QuadraticSystem, a PackedQuadraticSystem or a PackedCubicSystem (or a subclass of it), "
                        f"not {type(system).__name__}")
    return system.solve_raw_space_xl4, system.convert_sol_xl4


def _quartic_parts(c):
    if not isinstance(c, _packed("PackedQuarticSystem")):
        raise TypeError(f"search_*_quartic needs a PackedQuarticSystem (or a subclass of it), not {type(c).__name__}")
    return c.solve_raw_space, c.convert_sol


def search_all_xl4(system, zeros: Sequence, *, max_enum: int = 32, max_solutions: int = 65536) -> list:
    """list(system.solve_all_xl4(zeros, max_dimension=d)) without the 2^d walk, for a QuadraticSystem, a PackedQuadraticSystem or a
    PackedCubicSystem; DimensionTooLargeError (with .space) when the search gives up, ValueError when there are more than
    max_solutions points."""
    return _search(_xl4_parts, system, zeros, max_enum, max_solutions, False, "quartic")


def search_one_xl4(system, zeros: Sequence, *, max_enum: int = 32):
    """the first element of search_all_xl4, None if there is none"""
    sols = _search(_xl4_parts, system, zeros, max_enum, 1, True, "quartic")
    return sols[0] if sols else None


def search_all_quartic(c, zeros: Sequence, *, max_enum: int = 32, max_solutions: int = 65536) -> list:
    """list(c.solve_all(zeros, max_dimension=d)) without the 2^d walk, for a PackedQuarticSystem; exceptions as search_all_xl4"""
    return _search(_quartic_parts, c, zeros, max_enum, max_solutions, False, "quartic")


def search_one_quartic(c, zeros: Sequence, *, max_enum: int = 32):
    """the first element of search_all_quartic, None if there is none"""
    sols = _search(_quartic_parts, c, zeros, max_enum, 1, True, "quartic")
    return sols[0] if sols else None
