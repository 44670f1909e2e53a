"""The reduction behind search_all_xl / search_all_cubic, pinned on the host (gf2bv_cubic_plan / gf2bv_cubic_points, no GPU), the
host reference of tests/cubic_forms.py against itself, the argument checks of every gf2bv_cubic_* entry and the front-end's errors.

For spaces over the degree-3 columns of small systems, the forms the plan returns, walked over all 2^r_eff inputs by the reference,
must stand for exactly the points of the space whose pair and triple coordinates are the products of their linear bits."""
import ctypes
import itertools
import random

import numpy as np
import pytest

import gf2bv_amd
from gf2bv_amd import QuadraticSystem, hip, search
from gf2bv_amd._internal import CubicSearchGaveUp, _space_from_ints
from gf2bv_amd.linsys import xl3_cols, xl3_pair_col, xl3_triple_col
from oracle import gf2_oracle as O
from tests import cubic_forms as CF
from tests.cubic_terms import poly_int, poly_value


# -- the reference against itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,p,s", [(0, 0, 0), (1, 0, 1), (2, 2, 0), (3, 3, 0), (4, 3, 1), (7, 4, 1), (9, 5, 0), (11, 5, 2), (14, 6, 2)])
def test_known_zero_sets_equal_the_walk(R, p, s):
    for order in ("natural", "shuffled"):
        forms, want = CF.known_zero_case(random.Random(9000 + R), R, p, s, order)
        assert len(want) == (1 + p + p * (p - 1) // 2) << s and len(set(want)) == len(want)
        assert CF.brute_zeros(forms, R) == want
        assert all(CF.evaluate(f, z, R) == 0 for f in forms for z in want[:8])
        assert all(f >> CF.width(R) == 0 for f in forms)


def test_reference_product_and_planted_forms():
    rng = random.Random(9100)
    R = 9
    a, b, c = (rng.getrandbits(R + 1) for _ in range(3))
    f = CF.mul([a, b, c], R)
    for z in range(1 << R):
        lin = lambda g: (g & 1) ^ (bin((g >> 1) & z).count("1") & 1)          # noqa: E731
        assert CF.evaluate(f, z, R) == lin(a) & lin(b) & lin(c)
    pts = [rng.getrandbits(R) for _ in range(3)]
    forms = CF.planted_dense(rng, R, 7, pts)
    assert set(pts) <= set(CF.brute_zeros(forms, R))


# -- gf2bv_cubic_plan / gf2bv_cubic_points ---------------------------------------------------------------------------------------------
def _consistent_point(n: int, x: int) -> int:
    pt = x
    bits = [g for g in range(n) if (x >> g) & 1]
    for j, i in itertools.combinations(bits, 2):
        pt |= 1 << xl3_pair_col(n, i, j)
    for l, j, i in itertools.combinations(bits, 3):
        pt |= 1 << xl3_triple_col(n, i, j, l)
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
    cols = xl3_cols(n)
    sp = _space_from_ints(cols, origin, tuple(basis))
    brute = sorted(s for s in sp if _is_consistent(n, s))
    plan = hip.cubic_plan(origin, basis, n)
    assert plan["r"] == _rank(basis, (1 << n) - 1)
    re = plan["r_eff"]
    assert 0 <= re <= plan["r"]
    if plan["forms"] != [1]:
        # what the affine elimination leaves: every form has a term of degree two or three and fits the r_eff unknowns
        assert all(f >> (1 + re) and f >> CF.width(re) == 0 for f in plan["forms"])
    else:
        assert re == 0
    zs = CF.brute_zeros(plan["forms"], re)
    pts = hip.cubic_points(origin, basis, n, zs) if zs else []
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
    """n = 3..8, d = 0..12, origins consistent (planted) and arbitrary; dense and sparse basis vectors"""
    rng = random.Random(9200 + seed)
    for _ in range(8):
        n = rng.randint(3, 8)
        N = xl3_cols(n)
        d = min(rng.randint(0, 12), N)
        origin = _consistent_point(n, rng.getrandbits(n)) if rng.random() < 0.7 else rng.getrandbits(N)
        _check_space(n, origin, _independent(rng, d, N, (1 << N) - 1))


@pytest.mark.parametrize("seed", range(4))
def test_plan_hand_built_shapes(seed):
    """r = 0 (every basis vector in the product coordinates), d - r = 0 (independent linear parts), and differences of consistent
    points (many consistent points, affine forms to eliminate)"""
    rng = random.Random(9300 + seed)
    for _ in range(4):
        n = rng.randint(4, 8)
        N = xl3_cols(n)
        high = ((1 << N) - 1) ^ ((1 << n) - 1)
        plan = _check_space(n, _consistent_point(n, rng.getrandbits(n)), _independent(rng, rng.randint(0, 10), N, high))
        assert plan["r"] == 0
        d = rng.randint(0, n)
        lin = _independent(rng, d, n, (1 << n) - 1)
        plan = _check_space(n, _consistent_point(n, rng.getrandbits(n)), [v | (rng.getrandbits(N) & high) for v in lin])
        assert plan["r"] == d
        pts = [_consistent_point(n, rng.getrandbits(n)) for _ in range(6)]
        basis = []
        for q in pts[1:]:
            if _rank(basis + [q ^ pts[0]], (1 << N) - 1) > len(basis):
                basis.append(q ^ pts[0])
        _check_space(n, pts[0], basis + _independent(rng, 3, N, high)[:max(0, 12 - len(basis))])


@pytest.mark.parametrize("seed", range(6))
def test_plan_oracle_cubic_systems(seed):
    """spaces of random cubic systems (n = 6..10) with a planted secret, a few equations short of full rank, solved by the CPU oracle"""
    rng = random.Random(9400 + seed)
    n = 6 + seed % 5
    cols = xl3_cols(n)
    secret = rng.getrandbits(n)
    eqs = []
    for _ in range(2 * cols):
        p = frozenset(frozenset(rng.sample(range(n), rng.randint(1, 3))) for _ in range(rng.randint(2, 6)))
        eqs.append(poly_int(p, n) ^ poly_value(p, secret))
    count = cols - rng.randint(2, 11)
    while True:                                                    # (sparse random equations are dependent now and then: take more)
        sp = O.m4ri_solve(eqs[:count] + [0] * max(0, cols - count), cols, 1)
        if sp.dimension <= 14:
            break
        count += 3
    assert sp is not None and 2 <= sp.dimension <= 14
    plan = _check_space(n, sp.origin, sp.basis)
    assert plan["forms"] != [1]


def test_plan_inconsistent_space_is_the_constant_one():
    n = 4
    origin = 1 << xl3_triple_col(n, 3, 2, 0)                      # x3 x2 x0 = 1 with x = 0
    plan = hip.cubic_plan(origin, [], n)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (0, 0, [1])
    # a form that folds to the constant 1: x0 = x1 = c, x1 x0 = c ^ 1, so c c ^ c ^ 1 = 1
    n = 3
    plan = hip.cubic_plan(1 << xl3_pair_col(n, 1, 0), [0b011 | 1 << xl3_pair_col(n, 1, 0)], n)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (1, 0, [1])


def test_plan_rank_at_the_cap_and_above():
    """kCubicMaxRank = 64.  n = 64, basis e_0 .. e_63 with zero product parts: r = r_eff = 64, one form per product coordinate (its
    monomial); one unknown and one basis vector more: r = 65, not reduced (r_eff = -1, no forms)"""
    n = 64
    plan = hip.cubic_plan(0, [1 << a for a in range(n)], n)
    assert (plan["r"], plan["r_eff"], len(plan["forms"])) == (64, 64, xl3_cols(n) - n)
    assert plan["forms"][0] == 1 << (1 + xl3_pair_col(n, 1, 0)) and plan["forms"][-1] == 1 << (1 + xl3_triple_col(n, 63, 62, 61))
    plan = hip.cubic_plan(0, [1 << a for a in range(65)], 65)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (65, -1, [])


# -- argument checks, in front of any device -------------------------------------------------------------------------------------------
def test_every_entry_checks_its_arguments_before_the_device():
    """GF2BV_ERR_ARG (1) with the message of the check, on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2)"""
    L = hip.lib()
    o = np.zeros(4, dtype=np.uint64)
    A = o.ctypes.data
    cnt, lr = ctypes.c_int64(), ctypes.c_int64()
    r, re, m, fw = (ctypes.c_int64() for _ in range(4))
    outs = (ctypes.byref(r), ctypes.byref(re), ctypes.byref(m), ctypes.byref(fw), None, 0)
    pp = ctypes.c_void_p()

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    # the space: 10 unknowns have 175 columns, three words
    for space, what in [((None, A, 0, 3, 10), "null"), ((A, None, 2, 3, 10), "null"), ((A, A, -1, 3, 10), "dimension"),
                        ((A, A, 0, 0, 10), "words > 0"), ((A, A, 0, 3, 0), "n_lin must be 1..2000"),
                        ((A, A, 0, 3, 2001), "n_lin must be 1..2000"), ((A, A, 0, 2, 10), "words does not cover")]:
        err(L.gf2bv_cubic_search(*space, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), A), what)
        err(L.gf2bv_cubic_search_alloc(*space, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), ctypes.byref(pp)), what)
        err(L.gf2bv_cubic_plan(*space, *outs), what)
        err(L.gf2bv_cubic_plan_device(*space, 0, *outs), what)
        err(L.gf2bv_cubic_points(*space, A, 1, 1, A), what)
    ok = (A, A, 0, 3, 10)
    for entry, last in ((L.gf2bv_cubic_search, A), (L.gf2bv_cubic_search_alloc, ctypes.byref(pp))):
        err(entry(*ok, 41, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_enum must be 0..40")
        err(entry(*ok, -1, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_enum must be 0..40")
        err(entry(*ok, 32, -1, 0, ctypes.byref(cnt), ctypes.byref(lr), last), "max_solutions")
        err(entry(*ok, 32, 4, 0, None, ctypes.byref(lr), last), "null")
        err(entry(*ok, 32, 4, 0, ctypes.byref(cnt), None, last), "null")
        err(entry(*ok, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), None), "null")
    for k in range(4):
        bad = list(outs)
        bad[k] = None
        err(L.gf2bv_cubic_plan(*ok, *bad), "null")
        err(L.gf2bv_cubic_plan_device(*ok, 0, *bad), "null")
    err(L.gf2bv_cubic_points(*ok, None, 1, 1, A), "null")
    err(L.gf2bv_cubic_points(*ok, A, 1, 1, None), "null")
    err(L.gf2bv_cubic_points(*ok, A, -1, 1, A), "null")
    err(L.gf2bv_cubic_points(*ok, A, 1, 0, A), "y_words")
    bad_origin = np.array([1 << xl3_pair_col(3, 1, 0)], dtype=np.uint64)      # x1 x0 = 1 with x = 0: no consistent point
    err(L.gf2bv_cubic_points(bad_origin.ctypes.data, A, 0, 1, 3, A, 1, 1, A), "no forms to map from")
    err(L.gf2bv_cubic_forms_search(None, 1, 3, 0, 4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_cubic_forms_search(A, 1, 3, 0, 4, None, A), "null")
    err(L.gf2bv_cubic_forms_search(A, 1, 3, 0, 4, ctypes.byref(cnt), None), "null")
    err(L.gf2bv_cubic_forms_search(A, -1, 3, 0, 4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_cubic_forms_search(A, 1, 3, 0, -4, ctypes.byref(cnt), A), "null")
    err(L.gf2bv_cubic_forms_search(A, 1, -1, 0, 4, ctypes.byref(cnt), A), "r_eff must be 0..40")
    err(L.gf2bv_cubic_forms_search(A, 1, 41, 0, 4, ctypes.byref(cnt), A), "r_eff must be 0..40")
    L.gf2bv_cubic_last_times(None)                                # (a null pointer is ignored)
    assert set(hip.cubic_last_times()) == set(hip.quad_last_times())


def test_forms_above_the_memory_budget_are_refused_unallocated():
    """n = 200: 1 333 300 product coordinates; r = 40 makes a form 168 words, 1.7 GiB for the products alone: GF2BV_ERR_NOMEM"""
    n = 200
    with pytest.raises(hip.HipError, match="more than 1 GiB"):
        hip.cubic_plan(0, [1 << a for a in range(40)], n)


# -- the front-end ---------------------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    names = {"search_all_xl", "search_one_xl", "search_all_cubic", "search_one_cubic"}
    assert names <= set(gf2bv_amd.__all__) and names == set(search.__all__)
    assert all(getattr(gf2bv_amd, k) is getattr(search, k) for k in names)


def test_front_end_type_errors_name_the_accepted_classes():
    from gf2bv_amd import LinearSystem, PackedCubicSystem, PackedQuadraticSystem
    q, c = QuadraticSystem([4]), PackedCubicSystem([4])
    for fn in (search.search_all_xl, search.search_one_xl):
        for bad in (c, LinearSystem([4]), None):
            with pytest.raises(TypeError, match=r"^search_\*_xl needs a QuadraticSystem or a PackedQuadraticSystem, not "):
                fn(bad, [])
    for fn in (search.search_all_cubic, search.search_one_cubic):
        for bad in (q, PackedQuadraticSystem([4]), 7):
            with pytest.raises(TypeError, match=r"^search_\*_cubic needs a PackedCubicSystem \(or a subclass of it\), not "):
                fn(bad, [])


def test_space_method_value_errors_and_exception_type():
    sp = _space_from_ints(xl3_cols(4), 0, ())
    with pytest.raises(ValueError, match=r"^max_enum must be 0\.\.40$"):
        sp.cubic_search(4, 41)
    with pytest.raises(ValueError, match=r"^max_enum must be 0\.\.40$"):
        sp.cubic_search(4, -1)
    with pytest.raises(ValueError, match=r"^max_solutions must be >= 0$"):
        sp.cubic_search(4, 32, -1)
    with pytest.raises(TypeError, match=r"^cubic_search\(n_lin, max_enum=32, max_solutions=65536, first=False\)$"):
        sp.cubic_search()
    assert issubclass(CubicSearchGaveUp, RuntimeError)
    e = CubicSearchGaveUp("message", 7)
    assert e.args == ("message", 7)
