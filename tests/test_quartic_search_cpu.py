"""The reduction behind search_all_xl4 / search_all_quartic, pinned on the host (gf2bv_quartic_plan / gf2bv_quartic_points, no GPU),
the host reference of tests/quartic_forms.py against itself, the argument checks of every gf2bv_quartic_* entry and the front-end's
errors.

For spaces over the degree-4 columns of small systems, the forms the plan returns, walked over all 2^r_eff inputs by the reference,
must stand for exactly the points of the space whose pair, triple and quadruple coordinates are the products of their linear bits, in
the order of the walk over the space."""
import ctypes
import itertools
import random

import numpy as np
import pytest

import gf2bv_amd
from gf2bv_amd import QuadraticSystem, hip, search, search4
from gf2bv_amd._internal import QuarticSearchGaveUp, _space_from_ints
from gf2bv_amd.linsys import xl3_pair_col, xl3_triple_col, xl4_cols, xl4_quad_col
from tests import quartic_forms as QF
from tests.cubic_terms import poly_mul, poly_of_form, poly_value


# -- the reference against itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,p,s", [(0, 0, 0), (1, 0, 1), (3, 3, 0), (4, 4, 0), (5, 4, 1), (7, 5, 1), (9, 5, 0), (11, 6, 2), (14, 7, 2)])
def test_known_zero_sets_equal_the_walk(R, p, s):
    for order in ("natural", "shuffled"):
        forms, want = QF.known_zero_case(random.Random(9000 + R), R, p, s, order)
        assert len(want) == (1 + p + p * (p - 1) // 2 + p * (p - 1) * (p - 2) // 6) << s and len(set(want)) == len(want)
        assert QF.brute_zeros(forms, R) == want
        assert all(QF.evaluate(f, z, R) == 0 for f in forms for z in want[:8])
        assert all(f >> QF.width(R) == 0 for f in forms)


def test_reference_value_against_the_set_of_monomials():
    """evaluate reads the layout; the set of monomials knows nothing of it"""
    rng = random.Random(9100)
    R = 9
    ops = [rng.getrandbits(R + 1) for _ in range(4)]
    p = poly_of_form(ops[0], R)
    for g in ops[1:]:
        p = poly_mul(p, poly_of_form(g, R))
    f = QF.mul(ops, R)
    assert f >> QF.width(R) == 0 and f >> QF.CF.width(R)               # (it has quartic terms)
    for z in range(1 << R):
        assert QF.evaluate(f, z, R) == poly_value(p, z)
    dm = QF.DenseMap(rng, R)                                           # (prod keeps partial products on int masks: the same set product)
    for idx in ((0, 1), (4, 2, 7), (3, 8, 1, 5), (2, 2, 6), (0, 1, 2, 3)):
        assert dm.prod(*idx) == QF.mul([dm.y(i) for i in idx], R)
    pts = [rng.getrandbits(R) for _ in range(3)]
    forms = QF.planted_dense(rng, R, 7, pts)
    assert set(pts) <= set(QF.brute_zeros(forms, R))
    assert QF.weight_le3(5, 1) == sorted(QF.weight_le3(5, 1), key=lambda y: (y & 31, y >> 5)) and len(QF.weight_le3(5, 1)) == 52


# -- gf2bv_quartic_plan / gf2bv_quartic_points ------------------------------------------------------------------------------------------
def _consistent_point(n: int, x: int) -> int:
    pt = x
    bits = [g for g in range(n) if (x >> g) & 1]
    for j, i in itertools.combinations(bits, 2):
        pt |= 1 << xl3_pair_col(n, i, j)
    for l, j, i in itertools.combinations(bits, 3):
        pt |= 1 << xl3_triple_col(n, i, j, l)
    for p, l, j, i in itertools.combinations(bits, 4):
        pt |= 1 << xl4_quad_col(n, i, j, l, p)
    return pt


def _is_consistent(n: int, s: int) -> bool:
    return s == _consistent_point(n, s & ((1 << n) - 1))


def _rank(vecs, mask: int) -> int:
    piv = {}
    for v in vecs:
        v &= mask
        while v:
            h = v.bit_length() - 1
            if h not in piv:
                piv[h] = v
                break
            v ^= piv[h]
    return len(piv)


def _check_space(n: int, origin: int, basis) -> dict:
    """the plan's forms walked by the reference and mapped back give the consistent points of the walk over the space"""
    cols = xl4_cols(n)
    sp = _space_from_ints(cols, origin, tuple(basis))
    brute = sorted(s for s in sp if _is_consistent(n, s))
    plan = hip.quartic_plan(origin, basis, n)
    assert plan["r"] == _rank(basis, (1 << n) - 1)
    re = plan["r_eff"]
    assert 0 <= re <= plan["r"]
    if plan["forms"] != [1]:
        # what the affine elimination leaves: every form has a term of degree two or more and fits the r_eff unknowns
        assert all(f >> (1 + re) and f >> QF.width(re) == 0 for f in plan["forms"])
    else:
        assert re == 0
    zs = QF.brute_zeros(plan["forms"], re)
    pts = hip.quartic_points(origin, basis, n, zs) if zs else []
    assert sorted(pts) == brute
    return plan


def _independent(rng, count: int, width: int, mask: int) -> list:
    out: list = []
    while len(out) < count:
        v = rng.getrandbits(width) & mask
        if _rank(out + [v], (1 << width) - 1) == len(out) + 1:
            out.append(v)
    return out


@pytest.mark.parametrize("seed", range(8))
def test_plan_random_spaces(seed):
    """n = 4..8 (cols4(8) = 162), d = 0..14, origins consistent (planted) and arbitrary"""
    rng = random.Random(9200 + seed)
    for _ in range(6):
        n = rng.randint(4, 8)
        N = xl4_cols(n)
        d = min(rng.randint(0, 14), N)
        origin = _consistent_point(n, rng.getrandbits(n)) if rng.random() < 0.7 else rng.getrandbits(N)
        _check_space(n, origin, _independent(rng, d, N, (1 << N) - 1))


@pytest.mark.parametrize("seed", range(4))
def test_plan_hand_built_shapes(seed):
    """r = 0 (every basis vector in the product coordinates), d - r = 0 with r < n (independent linear parts), and differences of
    consistent points (many consistent points, affine forms to eliminate)"""
    rng = random.Random(9300 + seed)
    for _ in range(3):
        n = rng.randint(4, 8)
        N = xl4_cols(n)
        high = ((1 << N) - 1) ^ ((1 << n) - 1)
        plan = _check_space(n, _consistent_point(n, rng.getrandbits(n)), _independent(rng, rng.randint(0, 10), N, high))
        assert plan["r"] == 0
        d = rng.randint(0, n - 1)
        lin = _independent(rng, d, n, (1 << n) - 1)
        plan = _check_space(n, _consistent_point(n, rng.getrandbits(n)), [v | (rng.getrandbits(N) & high) for v in lin])
        assert plan["r"] == d < n
        pts = [_consistent_point(n, rng.getrandbits(n)) for _ in range(6)]
        basis = []
        for q in pts[1:]:
            if _rank(basis + [q ^ pts[0]], (1 << N) - 1) > len(basis):
                basis.append(q ^ pts[0])
        _check_space(n, pts[0], basis + _independent(rng, 3, N, high)[:max(0, 14 - len(basis))])


def test_plan_affine_forms_cascade_into_a_second_round():
    """x0 = x1 = a, x2 = b, the pair coordinate (1,0) fixed at 1, every other product coordinate at 0.  The first build has the
    affine form a ^ 1 (x1 x0 = a a = a against 1) and a b for (2,0), (2,1) and the triple; a b becomes the affine form b only once
    a = 1 is substituted, so a second round eliminates b and a third build finds nothing left: the one point x = (1, 1, 0)"""
    n = 3
    p10 = 1 << xl3_pair_col(n, 1, 0)
    plan = _check_space(n, p10, [0b011, 0b100])
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (2, 0, [])
    # the same cascade beside two unknowns that stay: x3 = c, x4 = d, whose products with x0 = x1 = 1 follow them and whose products
    # with each other are free coordinates of the space (vectors without a linear part).  Both rounds run, c and d are left
    n = 5
    pair, triple, quad = (lambda *m: 1 << xl3_pair_col(n, *m)), (lambda *m: 1 << xl3_triple_col(n, *m)), 1 << xl4_quad_col(n, 4, 3, 1, 0)
    c = 0b01000 | pair(3, 0) | pair(3, 1) | triple(3, 1, 0)
    d = 0b10000 | pair(4, 0) | pair(4, 1) | triple(4, 1, 0)
    plan = _check_space(n, pair(1, 0), [0b00011, 0b00100, c, d, pair(4, 3), triple(4, 3, 0), triple(4, 3, 1), quad])
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (4, 2, [])


def test_plan_inconsistent_space_is_the_constant_one():
    n = 5
    origin = 1 << xl4_quad_col(n, 4, 3, 1, 0)                      # x4 x3 x1 x0 = 1 with x = 0
    plan = hip.quartic_plan(origin, [], n)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (0, 0, [1])
    # a form that folds to the constant 1: x0 = x1 = c, x1 x0 = c ^ 1, so c c ^ c ^ 1 = 1
    n = 4
    plan = hip.quartic_plan(1 << xl3_pair_col(n, 1, 0), [0b0011 | 1 << xl3_pair_col(n, 1, 0)], n)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (1, 0, [1])
    # the same fold through a quadruple: x0 = x1 = x2 = x3 = c, x3 x2 x1 x0 = c ^ 1
    q = 1 << xl4_quad_col(n, 3, 2, 1, 0)
    plan = _check_space(n, q, [_consistent_point(n, 0b1111)])
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (1, 0, [1])


def test_plan_rank_at_the_cap_and_above():
    """kQuarticMaxRank = 64: one unknown and one basis vector more than 64 are not reduced (r_eff = -1, no forms).  (r = 64 itself
    with n = 64 is over the memory budget at this degree: the next test.)"""
    plan = hip.quartic_plan(0, [1 << a for a in range(65)], 65)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (65, -1, [])
    n = 12                                                         # every product coordinate its own monomial
    plan = hip.quartic_plan(0, [1 << a for a in range(n)], n)
    assert (plan["r"], plan["r_eff"], len(plan["forms"])) == (12, 12, xl4_cols(n) - n)
    assert plan["forms"][0] == 1 << (1 + xl3_pair_col(n, 1, 0)) and plan["forms"][-1] == 1 << (1 + xl4_quad_col(n, 11, 10, 9, 8))


def test_forms_above_the_memory_budget_are_refused_unallocated():
    """n = 64: 679 056 product coordinates; r = 40 makes a form 1596 words, 8 GiB for the products alone: GF2BV_ERR_NOMEM"""
    with pytest.raises(hip.HipError, match="more than 1 GiB"):
        hip.quartic_plan(0, [1 << a for a in range(40)], 64)


# -- argument checks, in front of any device -------------------------------------------------------------------------------------------
def test_every_entry_checks_its_arguments_before_the_device():
    """GF2BV_ERR_ARG (1) with the message of the check, on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2)"""
    L = hip.lib()
    o = np.zeros(8, dtype=np.uint64)
    A = o.ctypes.data
    cnt, lr = ctypes.c_int64(), ctypes.c_int64()
    r, re, m, fw = (ctypes.c_int64() for _ in range(4))
    outs = (ctypes.byref(r), ctypes.byref(re), ctypes.byref(m), ctypes.byref(fw), None, 0)
    pp = ctypes.c_void_p()

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    # the space: 10 unknowns have 385 columns, seven words
    assert xl4_cols(10) == 385
    for space, what in [((None, A, 0, 7, 10), "null"), ((A, None, 2, 7, 10), "null"), ((A, A, -1, 7, 10), "dimension"),
                        ((A, A, 0, 0, 10), "words > 0"), ((A, A, 0, 7, 0), "n_lin must be 1..450"),
                        ((A, A, 0, 7, 451), "n_lin must be 1..450"), ((A, A, 0, 6, 10), "words does not cover")]:
        err(L.gf2bv_quartic_search(*space, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), A), what)
        err(L.gf2bv_quartic_search_alloc(*space, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), ctypes.byref(pp)), what)
        err(L.gf2bv_quartic_plan(*space, *outs), what)
        err(L.gf2bv_quartic_plan_device(*space, 0, *outs), what)
        err(L.gf2bv_quartic_points(*space, A, 1, 1, A), what)
    err(L.gf2bv_quartic_plan(A, A, 0, 6, 10, *outs), "C(n_lin,4) columns")
    ok = (A, A, 0, 7, 10)
    for entry, last in ((L.gf2bv_quartic_search, A), (L.gf2bv_quartic_search_alloc, ctypes.byref(pp))):
        err(entry(*ok, 41, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_enum must be 0..40")
        err(entry(*ok, -1, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_enum must be 0..40")
        err(entry(*ok, 32, -1, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_solutions")
        err(entry(*ok, 32, 4, 0, None, ctypes.byref(lr), last), "null")
        err(entry(*ok, 32, 4, 0, ctypes.byref(cnt), None, last), "null")
        err(entry(*ok, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), None), "null")
    for k in range(4):
        bad = list(outs)
        bad[k] = None
        err(L.gf2bv_quartic_plan(*ok, *bad), "null")
        err(L.gf2bv_quartic_plan_device(*ok, 0, *bad), "null")
    err(L.gf2bv_quartic_points(*ok, None, 1, 1, A), "null")
    err(L.gf2bv_quartic_points(*ok, A, 1, 1, None), "null")
    err(L.gf2bv_quartic_points(*ok, A, -1, 1, A), "null")
    err(L.gf2bv_quartic_points(*ok, A, 1, 0, A), "y_words")
    bad_origin = np.array([1 << xl3_pair_col(3, 1, 0)], dtype=np.uint64)      # x1 x0 = 1 with x = 0: no consistent point
    err(L.gf2bv_quartic_points(bad_origin.ctypes.data, A, 0, 1, 3, A, 1, 1, A), "no forms to map from")
    err(L.gf2bv_quartic_forms_search(None, 1, 3, 0, 4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_quartic_forms_search(A, 1, 3, 0, 4, None, A), "null")
    err(L.gf2bv_quartic_forms_search(A, 1, 3, 0, 4, ctypes.byref(cnt), None), "null")
    err(L.gf2bv_quartic_forms_search(A, -1, 3, 0, 4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_quartic_forms_search(A, 1, 3, 0, -4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_quartic_forms_search(A, 1, -1, 0, 4, ctypes.byref(cnt), A), "r_eff must be 0..40")
    err(L.gf2bv_quartic_forms_search(A, 1, 41, 0, 4, ctypes.byref(cnt), A), "r_eff must be 0..40")
    L.gf2bv_quartic_last_times(None)                              # (a null pointer is ignored)
    assert list(hip.quartic_last_times()) == list(hip.quad_last_times())


# -- the front-end ---------------------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    names = {"search_all_xl4", "search_one_xl4", "search_all_quartic", "search_one_quartic"}
    assert names <= set(gf2bv_amd.__all__) and names == set(search4.__all__)
    assert all(getattr(gf2bv_amd, k) is getattr(search4, k) for k in names)
    assert set(search.__all__) == {"search_all_xl", "search_one_xl", "search_all_cubic", "search_one_cubic"}
    assert search4._search is search._search


def test_front_end_type_errors_name_the_accepted_classes():
    from gf2bv_amd import LinearSystem, PackedCubicGuessSystem, PackedCubicSystem, PackedQuadraticSystem, PackedQuarticSystem
    q, c, v = QuadraticSystem([4]), PackedCubicSystem([4]), PackedQuarticSystem([4])
    for fn in (search4.search_all_xl4, search4.search_one_xl4):
        for bad in (v, LinearSystem([4]), None):
            with pytest.raises(TypeError, match=r"^search_\*_xl4 needs a QuadraticSystem, a PackedQuadraticSystem or a PackedCubicSystem "
                                                r"\(or a subclass of it\), not "):
                fn(bad, [])
    for fn in (search4.search_all_quartic, search4.search_one_quartic):
        for bad in (c, q, PackedQuadraticSystem([4]), PackedCubicGuessSystem([4]), 7):
            with pytest.raises(TypeError, match=r"^search_\*_quartic needs a PackedQuarticSystem \(or a subclass of it\), not "):
                fn(bad, [])
    # the accepted ones get past the check (no equations: the solve entry is what refuses, or a device is missing -- not a TypeError
    # of the check)
    assert search4._xl4_parts(q) and search4._xl4_parts(c) and search4._xl4_parts(PackedQuadraticSystem([4]))
    assert search4._xl4_parts(PackedCubicGuessSystem([4])) and search4._quartic_parts(v)


def test_space_method_value_errors_and_exception_type():
    sp = _space_from_ints(xl4_cols(4), 0, ())
    with pytest.raises(ValueError, match=r"^max_enum must be 0\.\.40$"):
        sp.quartic_search(4, 41)
    with pytest.raises(ValueError, match=r"^max_enum must be 0\.\.40$"):
        sp.quartic_search(4, -1)
    with pytest.raises(ValueError, match=r"^max_solutions must be >= 0$"):
        sp.quartic_search(4, 32, -1)
    with pytest.raises(TypeError, match=r"^quartic_search\(n_lin, max_enum=32, max_solutions=65536, first=False\)$"):
        sp.quartic_search()
    assert issubclass(QuarticSearchGaveUp, RuntimeError)
    e = QuarticSearchGaveUp("message", 7)
    assert e.args == ("message", 7)
