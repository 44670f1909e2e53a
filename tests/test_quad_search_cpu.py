"""The reduction behind QuadraticSystem.search_all, pinned on the host (gf2bv_quad_plan / gf2bv_quad_points, no GPU).

For random spaces over small QuadraticSystems, the forms the plan returns, evaluated over all 2^r_eff inputs, must stand for
exactly the points of the space that pass convert_sol, and r must be the rank of the space's projection onto the linear
unknowns."""
import random

import numpy as np
import pytest

from gf2bv_amd import QuadraticSystem, hip
from gf2bv_amd._internal import _space_from_ints
from oracle import gf2_oracle as O


def _eval_form(f: int, y: int, re: int) -> int:
    v = f & 1
    v ^= bin((f >> 1) & y & ((1 << re) - 1)).count("1") & 1
    for i in range(1, re):
        if (y >> i) & 1:
            row = (f >> (1 + re + i * (i - 1) // 2)) & ((1 << i) - 1)
            v ^= bin(row & y).count("1") & 1
    return v


def _np_rank(vecs, n: int) -> int:
    """rank over GF(2) of the low n bits of vecs, by numpy row reduction"""
    if not vecs:
        return 0
    M = np.array([[(v >> c) & 1 for c in range(n)] for v in vecs], dtype=np.uint8)
    rank = 0
    for c in range(n):
        rows = np.nonzero(M[rank:, c])[0]
        if len(rows) == 0:
            continue
        p = rank + rows[0]
        M[[rank, p]] = M[[p, rank]]
        hit = np.nonzero(M[:, c])[0]
        hit = hit[hit != rank]
        M[hit] ^= M[rank]
        rank += 1
        if rank == len(vecs):
            break
    return rank


def _consistent_point(n: int, x: int) -> int:
    pt = x
    for i in range(1, n):
        for j in range(i):
            if (x >> i) & 1 and (x >> j) & 1:
                pt |= 1 << (n + i * (i - 1) // 2 + j)
    return pt


def _check_space(q: QuadraticSystem, origin: int, basis) -> dict:
    n = q._lin_size
    sp = _space_from_ints(q._cols, origin, tuple(basis))
    brute = sorted(s for s in sp if q.convert_sol(s) is not None)
    plan = hip.quad_plan(origin, basis, n)
    assert plan["r"] == _np_rank(list(basis), n)
    re = plan["r_eff"]
    assert 0 <= re <= plan["r"]
    # what the affine elimination leaves: every form has a product term and uses only the r_eff unknowns -- or the
    # single form 1 (no consistent point)
    width = 1 + re + re * (re - 1) // 2
    if plan["forms"] != [1]:
        assert all(f >> (1 + re) and f >> width == 0 for f in plan["forms"])
    zs = [y for y in range(1 << re) if all(_eval_form(f, y, re) == 0 for f in plan["forms"])]
    pts = hip.quad_points(origin, basis, n, zs) if zs else []
    assert sorted(pts) == brute
    return plan


def _independent(rng, count: int, width: int, mask: int) -> list:
    out: list = []
    while len(out) < count:
        v = rng.getrandbits(width) & mask
        if _np_rank(out + [v], width) == len(out) + 1:
            out.append(v)
    return out


@pytest.mark.parametrize("seed", range(8))
def test_plan_random_spaces(seed):
    """n = 4..12, d = 0..14, origins consistent (planted) and arbitrary"""
    rng = random.Random(100 + seed)
    for _ in range(12):
        n = rng.randint(4, 12)
        q = QuadraticSystem([n])
        N = q._cols
        d = min(rng.randint(0, 14), N)
        origin = _consistent_point(n, rng.getrandbits(n)) if rng.random() < 0.7 else rng.getrandbits(N)
        _check_space(q, origin, _independent(rng, d, N, (1 << N) - 1))


@pytest.mark.parametrize("seed", range(4))
def test_plan_no_linear_directions(seed):
    """d - r = d: every basis vector lies in the product coordinates (r = 0)"""
    rng = random.Random(200 + seed)
    for _ in range(8):
        n = rng.randint(4, 9)
        q = QuadraticSystem([n])
        d = min(rng.randint(0, 10), n * (n - 1) // 2)
        mask = ((1 << q._cols) - 1) ^ ((1 << n) - 1)
        plan = _check_space(q, _consistent_point(n, rng.getrandbits(n)), _independent(rng, d, q._cols, mask))
        assert plan["r"] == 0


@pytest.mark.parametrize("seed", range(4))
def test_plan_no_kernel_directions(seed):
    """d - r = 0: the linear parts of the basis are independent"""
    rng = random.Random(300 + seed)
    for _ in range(8):
        n = rng.randint(4, 12)
        q = QuadraticSystem([n])
        d = rng.randint(0, min(n, 12))
        lin = _independent(rng, d, n, (1 << n) - 1)
        basis = [v | (rng.getrandbits(q._cols) >> n << n) for v in lin]
        plan = _check_space(q, _consistent_point(n, rng.getrandbits(n)), basis)
        assert plan["r"] == d


@pytest.mark.parametrize("seed", range(6))
def test_plan_oracle_quadratic_systems(seed):
    """spaces of random quadratic systems with a planted secret, solved by the CPU oracle"""
    rng = random.Random(400 + seed)
    n = rng.randint(5, 10)
    q = QuadraticSystem([n])
    (x,) = q.gens()
    secret = rng.getrandbits(n)
    pairs = q._quad_size
    neq = rng.randint(max(1, q._cols - 14), q._cols + 4)
    zeros = []
    for _ in range(neq):
        e = 0
        for _ in range(3):
            a, b = x[rng.randrange(n)], x[rng.randrange(n)]
            if a is not b:
                e ^= q.mul_bit(a, b)._bits[0]
        e ^= x[rng.randrange(n)]._bits[0]
        # make the secret a root: the constant term is the value of the rest at the secret
        raw = _consistent_point(n, secret)
        e ^= bin((e >> 1) & raw).count("1") & 1
        zeros.append(e)
    eqs = q.get_eqs(zeros)
    eqs += [0] * max(0, q._cols - len(eqs))
    sp = O.m4ri_solve(eqs, q._cols, 1)
    assert sp is not None and pairs > 0
    _check_space(q, sp.origin, sp.basis)
    assert q.convert_sol(_consistent_point(n, secret)) == (secret,)


def test_plan_inconsistent_space_is_the_constant_one():
    """no consistent point: the single form 1 over r_eff = 0 unknowns"""
    q = QuadraticSystem([4])
    n = 4
    origin = 1 << n                                 # x1 x0 = 1 with x = 0
    plan = hip.quad_plan(origin, [], n)
    assert (plan["r"], plan["r_eff"], plan["forms"]) == (0, 0, [1])
    assert [s for s in _space_from_ints(q._cols, origin, ()) if q.convert_sol(s) is not None] == []


def test_plan_argument_checks():
    with pytest.raises(ValueError):
        hip.quad_plan(0, [], 0)                     # n_lin must be positive
    L = hip.lib()
    import ctypes
    o = np.zeros(1, dtype=np.uint64)
    r, re, m, fw = (ctypes.c_int64() for _ in range(4))
    # words must cover n_lin + n_lin(n_lin-1)/2 columns: 12 linear unknowns need 78 bits
    assert L.gf2bv_quad_plan(o.ctypes.data, o.ctypes.data, 0, 1, 12, ctypes.byref(r), ctypes.byref(re), ctypes.byref(m),
                             ctypes.byref(fw), None, 0) == 1


def test_search_argument_checks_come_before_the_device():
    """gf2bv_quad_search rejects bad arguments with GF2BV_ERR_ARG whether or not a device is visible"""
    import ctypes
    L = hip.lib()
    o = np.zeros(2, dtype=np.uint64)
    cnt, lr = ctypes.c_int64(), ctypes.c_int64()
    out = np.zeros(4, dtype=np.uint64)
    ok = (o.ctypes.data, o.ctypes.data, 0, 2, 10)
    assert L.gf2bv_quad_search(o.ctypes.data, o.ctypes.data, 0, 1, 12, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(*ok, 41, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(*ok, -1, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(*ok, 32, -1, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(*ok, 32, 4, 0, None, ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(*ok, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), None) == 1
    assert L.gf2bv_quad_search(None, o.ctypes.data, 0, 2, 10, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
    assert L.gf2bv_quad_search(o.ctypes.data, None, 3, 2, 10, 32, 4, 0, ctypes.byref(cnt), ctypes.byref(lr), out.ctypes.data) == 1
