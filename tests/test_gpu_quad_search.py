"""QuadraticSystem.search_all / search_one on the MI355X: the consistent points of the linearised space found on the device
(AffineSpace.quad_search -> gf2bv_quad_search), against the host walk of solve_all where that walk is possible, and against the
planted secret beyond it."""
import random

import pytest

from gf2bv_amd import QuadraticSystem, hip
from gf2bv_amd.linsys import DimensionTooLargeError
from tests.harness_models import FibonacciLFSR, GaloisLFSR

@pytest.fixture(params=["default", "plain"])
def mode(request, monkeypatch):
    """every test as shipped and with GF2BV_PLAIN=1 (the solves underneath on their plain paths)"""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900), pytest.mark.usefixtures("mode")]


def _raw(n: int, x: int) -> int:
    """the consistent raw point of linear part x"""
    pt = x
    for i in range(1, n):
        for j in range(i):
            if (x >> i) & 1 and (x >> j) & 1:
                pt |= 1 << (n + i * (i - 1) // 2 + j)
    return pt


def _planted(rng, n: int, neq: int, secrets: int = 1):
    """random quadratic equations in n unknowns that vanish at `secrets` planted points"""
    q = QuadraticSystem([n])
    (x,) = q.gens()
    pts = [rng.getrandbits(n) for _ in range(secrets)]
    raws = [_raw(n, p) for p in pts]
    zeros = []
    while len(zeros) < neq:
        e = x[rng.randrange(n)]
        for _ in range(rng.randint(1, 3)):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b:
                e = e ^ q.mul_bit(x[a], x[b])
        vals = {e.evaluate(r) for r in raws}
        if len(vals) == 1:
            zeros.append(e ^ vals.pop())
    return q, zeros, pts


def test_search_all_equals_solve_all():
    rng = random.Random(7)
    seen_multi = seen_high = seen_relin = 0
    for trial in range(40):
        n = rng.randint(6, 24)
        q = QuadraticSystem([n])
        neq = rng.randint(max(1, q._cols - 16), q._cols + 8)
        q, zeros, _ = _planted(rng, n, neq, secrets=1 + (trial % 3))
        space = q.solve_raw_space(zeros)
        d = space.dimension if space is not None else 0
        if d > 16:
            continue
        want = list(q.solve_all(zeros, max_dimension=d))
        assert q.search_all(zeros) == want, (n, neq, d)
        assert q.search_one(zeros) == q.solve_one(zeros)
        seen_multi += len(want) > 1
        seen_high += d >= 8
        # the same through a relinearisation level (a small max_enum: no direct search at the top), where it gets anywhere
        for max_enum in (2, 1):
            try:
                relin = q.search_all(zeros, max_enum=max_enum)
            except DimensionTooLargeError:
                continue
            assert relin == want, (n, neq, d, max_enum)
            seen_relin += len(want) > 1 and hip.quad_last_times()["levels"] > 1
    assert seen_multi and seen_high and seen_relin


def test_inconsistent_systems():
    q = QuadraticSystem([8])
    (x,) = q.gens()
    zeros = [q.mul_bit(x[0], x[1]) ^ 1, x[0]]       # linearly consistent (d = 34), no consistent point
    assert q.solve_raw_space(zeros) is not None
    assert q.search_all(zeros) == []
    assert q.search_one(zeros) is None
    assert q.search_all([x[0] ^ x[0] ^ 1]) == [] and q.search_one([1]) is None


def test_large_dimension_order():
    """n = 16 with few equations: d well above the host walk's default limit, order = solve_all(max_dimension=d)"""
    rng = random.Random(11)
    q, zeros, pts = _planted(rng, 16, 120, secrets=3)
    space = q.solve_raw_space(zeros)
    assert space.dimension > 16
    got = q.search_all(zeros)
    assert {(p,) for p in pts} <= set(got)
    if space.dimension <= 22:
        assert got == list(q.solve_all(zeros, max_dimension=space.dimension))


def _coefficients(space, raw: int) -> int:
    """c with raw = origin ^ XOR_{k in c} basis[k] (host elimination on the highest bits)"""
    piv = {}                                         # highest bit -> (vector, coefficient mask)
    for k, v in enumerate(space.basis):
        c = 1 << k
        while v:
            h = v.bit_length() - 1
            if h not in piv:
                piv[h] = (v, c)
                break
            v, c = v ^ piv[h][0], c ^ piv[h][1]
        assert v
    v, c = raw ^ space.origin, 0
    while v:
        pv, pc = piv[v.bit_length() - 1]
        v, c = v ^ pv, c ^ pc
    return c


def test_binary_walk_order_above_64():
    """d > 64 (AffineSpaceIteratorSlow, basis[0] the least significant bit): several consistent points, checked against a
    host enumeration of the 2^14 linear assignments and ordered by their coefficients as integers"""
    rng = random.Random(21)
    n = 14
    q, zeros, pts = _planted(rng, n, 30, secrets=4)
    space = q.solve_raw_space(zeros)
    assert space.dimension > 64
    eqs = q.get_eqs(zeros)
    want = []
    for x in range(1 << n):
        raw = _raw(n, x)
        if all(bin((e >> 1) & raw).count("1") & 1 == e & 1 for e in eqs):
            want.append(raw)
    want.sort(key=lambda raw: _coefficients(space, raw))
    got = q.search_all(zeros)
    assert len(want) >= 4 and got == [q.convert_sol(r) for r in want]
    assert q.search_one(zeros) == got[0]


# -- beyond the old limit: the filtered 128-bit LFSR of examples/nlfsr_recovery.py ------------------------------------------------
N_BITS, TAPS = 128, 0xD670201BAC7515352A273372B2A95B23
SELECT = (13, 24, 35, 46, 57)


def _filter(x0, x1, x2, x3, x4):
    return (x0 & x1) ^ (x0 & x1 & x3 & x4) ^ x0 ^ x1 ^ x2


def _nlfsr(kind, seed: int, count: int):
    secret = random.Random(seed).getrandbits(N_BITS)
    reg, stream = kind(N_BITS, TAPS, secret), []
    for _ in range(count):
        reg()
        stream.append(_filter(*[(reg.state >> i) & 1 for i in SELECT]))
    q = QuadraticSystem([65, 63])
    lo, hi = q.gens()
    sym = kind(N_BITS, TAPS, lo.concat(hi))
    zeros = []
    for bit in stream:
        sym()
        if bit:                                       # the annihilator g = x0 x1 + x0 + x1 x2 + x1 + x2 + 1 vanishes
            x0, x1, x2 = [sym.state[i] for i in SELECT[:3]]
            zeros.append(q.mul_bit(x0, x1) ^ x0 ^ q.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    return q, zeros, (secret & ((1 << 65) - 1), secret >> 65)


# (kind, seed, outputs, relinearised): d / r / r_eff of each case are recorded in DESIGN.md section 7
NLFSR_CASES = [
    (GaloisLFSR, 1, 16384, True),       # d = 107, r = r_eff = 107: relinearised (5778 unknowns), then unique
    (GaloisLFSR, 1, 16500, True),       # d = 46, r = r_eff = 46: relinearised
    (FibonacciLFSR, 2, 16320, False),   # d = 19, r = r_eff = 19: the direct search
]


@pytest.mark.parametrize("kind,seed,count,relin", NLFSR_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_nlfsr_beyond_max_dimension(kind, seed, count, relin):
    q, zeros, want = _nlfsr(kind, seed, count)
    with pytest.raises(DimensionTooLargeError):
        q.solve_one(zeros)
    assert q.search_one(zeros) == want
    assert q.search_all(zeros) == [want]
    assert (hip.quad_last_times()["levels"] > 1) == relin


# -- the device search on its own ------------------------------------------------------------------------------------------------
def _eval(f: int, y: int, re: int) -> int:
    v = f & 1
    v ^= bin((f >> 1) & y).count("1") & 1
    for i in range(1, re):
        if (y >> i) & 1:
            v ^= bin(((f >> (1 + re + i * (i - 1) // 2)) & ((1 << i) - 1)) & y).count("1") & 1
    return v


def _form(rng, re: int, density: float = 0.3) -> int:
    f = 0
    for b in range(1 + re + re * (re - 1) // 2):
        if rng.random() < density:
            f |= 1 << b
    return f


def _vanish_at(f: int, y: int, re: int) -> int:
    return f ^ _eval(f, y, re)


def _monomials(re: int, limit=None) -> list:
    """the forms x_i x_j (equation ints over re unknowns), pairs in layout order"""
    out = [1 << (1 + re + i * (i - 1) // 2 + j) for i in range(1, re) for j in range(i)]
    return out[:limit] if limit else out


def _weight_le1(re: int) -> list:
    return [0] + [1 << k for k in range(re)]


def test_forms_search_matches_host_walk_20():
    """r_eff = 20: the complete survivor list equals a host walk.  The forms are the 190 products x_i x_j, repeated: the first
    pass bit-slices the first 64 independent ones (the pairs among x0..x11), which thousands of points pass, and the second
    pass removes all but the common zeros of every form (the 21 points of weight <= 1)"""
    import numpy as np
    re = 20
    forms = _monomials(re) + _monomials(re, 64)
    y = np.arange(1 << re, dtype=np.uint64)
    bits = [((y >> np.uint64(k)) & np.uint64(1)).astype(np.uint8) for k in range(re)]
    alive = np.ones(1 << re, dtype=bool)
    for i in range(1, re):
        for j in range(i):
            alive &= (bits[i] & bits[j]) == 0
    want = [int(v) for v in np.nonzero(alive)[0]]
    before = hip.quad_last_times()["candidates"]
    count, got = hip.quad_forms_search(forms, re)
    candidates = hip.quad_last_times()["candidates"] - before
    assert count == len(want) == 21 and got == want == sorted(_weight_le1(re))
    assert candidates > 1000


def test_forms_search_too_many_candidates_32():
    """r_eff = 32 with the same kind of forms: ~13.6 million points pass the first 64 forms, more than the candidate list
    holds (2^22); the search is repeated with every form tested in the lanes, and still returns exactly the 33 common zeros"""
    re = 32
    before = hip.quad_last_times()["candidates"]
    count, got = hip.quad_forms_search(_monomials(re), re)
    candidates = hip.quad_last_times()["candidates"] - before
    assert candidates > 1 << 22
    assert count == 33 and got == sorted(_weight_le1(re))


def test_forms_search_finds_planted_28():
    rng = random.Random(5)
    re = 28
    point = rng.getrandbits(re)
    forms = [_vanish_at(_form(rng, re, 0.2), point, re) for _ in range(80)]
    count, got = hip.quad_forms_search(forms, re)
    assert point in got and count == len(got)
    assert all(_eval(f, y, re) == 0 for y in got for f in forms)


def test_forms_search_without_forms():
    assert hip.quad_forms_search([], 5) == (32, list(range(32)))


# -- FactoredSystem -------------------------------------------------------------------------------------------------------------
def test_factored_search_one_rhs():
    rng = random.Random(9)
    n = 12
    q = QuadraticSystem([n])
    (x,) = q.gens()
    exprs = []
    for _ in range(q._cols - 10):
        e = x[rng.randrange(n)]
        for _ in range(2):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b:
                e = e ^ q.mul_bit(x[a], x[b])
        exprs.append(e)
    secrets = [rng.getrandbits(n) for _ in range(5)]
    values_list = [[e.evaluate(_raw(n, s)) for e in exprs] for s in secrets]
    values_list.append([v ^ (k == 0) for k, v in enumerate(values_list[0])])
    with q.factor(exprs) as fs:
        got = fs.search_one_rhs(values_list)
        want = [q.search_one([e ^ v for e, v in zip(exprs, vals)]) for vals in values_list]
        assert got == want
        for s, g in zip(secrets, got):
            assert g is not None
        assert fs.search_all(values_list[0]) == q.search_all([e ^ v for e, v in zip(exprs, values_list[0])])
        assert fs.search_one(values_list[1]) == want[1]


# -- errors ---------------------------------------------------------------------------------------------------------------------
def test_gives_up_with_space():
    """nlfsr with 16000 outputs: d = 188, r = 128, and relinearisation makes no progress"""
    q, zeros, _ = _nlfsr(FibonacciLFSR, 2, 16000)
    with pytest.raises(DimensionTooLargeError) as ei:
        q.search_one(zeros)
    assert ei.value.space is not None and ei.value.space.dimension == 188
    assert "rank 128" in str(ei.value)


def test_too_many_solutions():
    q = QuadraticSystem([10])
    (x,) = q.gens()
    zeros = [x[0] ^ x[1]]                               # 2^9 consistent points
    with pytest.raises(ValueError, match="512.*max_solutions \\(100\\)"):
        q.search_all(zeros, max_solutions=100)
    assert len(q.search_all(zeros, max_solutions=512)) == 512
