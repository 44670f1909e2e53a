"""Kept factorizations, right-hand sides and batches of the packed front-ends on the MI355X.  The yardstick throughout is the int
front-end -- LinearSystem / QuadraticSystem / FactoredSystem on the same equations -- and, for the C ABI, gf2bv_solve_rhs_words on
gf2bv_quad_expand_words of the same terms; every comparison is bit-exact."""
import random

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, PackedLinearSystem, PackedQuadraticSystem, QuadraticSystem, hip
from gf2bv_amd.factored import PackedFactoredSystem, PackedQuadFactoredSystem
from tests.harness_models import MT19937
from tests.quad_terms import Twin, expand_ints, random_terms, to_aug
from tests.test_gpu_quad_search import _raw


@pytest.fixture(params=["default", "plain"])
def mode(request, monkeypatch):
    """every test as shipped and with GF2BV_PLAIN=1 (the solves underneath on their plain paths)"""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


# (the timeout: the n = 100 case writes ~10000 products over 5050 columns on the int front-end, twice with the plain run)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900), pytest.mark.usefixtures("mode")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _space(sp):
    return None if sp is None else (sp.dimension, sp.origin, sp.basis)


def _key(s):
    return (s.status, s.rank, s.dimension, s.origin.tolist(), s.basis.tolist(), s.pivots.tolist())


def _vectors(bits_q, bits_p, sizes=(1, 3, 8)):
    """single-bit expressions of both front-ends grouped into vectors of 1, 3, 8, 1, ... bits: (int exprs, packed exprs, groups)"""
    eq, ep, groups, at, k = [], [], [], 0, 0
    while at < len(bits_q):
        w = min(sizes[k % len(sizes)], len(bits_q) - at)
        a, b = bits_q[at], bits_p[at]
        for j in range(at + 1, at + w):
            a, b = a.concat(bits_q[j]), b.concat(bits_p[j])
        eq.append(a)
        ep.append(b)
        groups.append((at, w))
        at, k = at + w, k + 1
    return eq, ep, groups


def _values(groups, bits):
    return [sum(bits[at + j] << j for j in range(w)) for at, w in groups]


def _agree(fp, fq, q, values_list, max_dimension=16):
    """every method of the packed factored object against the int front-end's; returns per instance ((dimension, origin, basis) | None, consistent points)"""
    assert fp.solve_raw_one_rhs(values_list) == fq.solve_raw_one_rhs(values_list)
    sp, sq = fp.solve_raw_space_rhs(values_list), fq.solve_raw_space_rhs(values_list)
    assert [_space(s) for s in sp] == [_space(s) for s in sq]
    assert fp.solve_one_rhs(values_list, max_dimension=max_dimension) == fq.solve_one_rhs(values_list, max_dimension=max_dimension)
    assert fp.search_one_rhs(values_list) == fq.search_one_rhs(values_list)
    out = []
    for vals, s in zip(values_list, sq):
        want = list(fq.solve_all(vals, max_dimension=max_dimension))
        assert list(fp.solve_all(vals, max_dimension=max_dimension)) == want
        assert fp.search_all(vals) == fq.search_all(vals) == want
        assert fp.solve_one(vals) == fq.solve_one(vals) == (want[0] if want else None)
        assert fp.search_one(vals) == (want[0] if want else None)
        out.append((_space(s), want))
    hp, hq = fp._handle(1), fq._handle(1)
    assert hp.rank == hq.rank and hp.pivots == hq.pivots and hp.rows == hq.rows == fp.rows
    return out


def _planted(n: int, seed: int, short: int = 3, dups: int = 3):
    """cols - short random dense quadratic bits that take the same value at two secret points, and `dups` of them once more (rank
    deficiency: their values must agree); on both front-ends in step.  Returns (twin, bits_q, bits_p, secrets)."""
    rng = random.Random(seed)
    tw = Twin([n])
    q, p, x, y = tw.q, tw.p, tw.qx, tw.px
    s1, s2 = _raw(n, rng.getrandbits(n)), _raw(n, rng.getrandbits(n))
    bq, bp = [], []
    while len(bq) < q._cols - short:
        k = rng.randrange(n)
        e, f = x[k], y[k]
        for _ in range(rng.randint(1, 2)):                                 # products of dense forms: about half of all pairs each
            ma, mb = rng.getrandbits(n), rng.getrandbits(n)
            e, f = e ^ q.mul_bit((x & ma).sum(), (x & mb).sum()), f ^ p.mul_bit((y & ma).sum(), (y & mb).sum())
        if e.evaluate(s1) == e.evaluate(s2):
            bq.append(e)
            bp.append(f)
    for k in range(dups):
        bq.append(bq[k])
        bp.append(bp[k])
    return tw, bq, bp, (s1, s2), rng


def _instances(rng, tw, bq, groups, secrets, dups=3):
    """value lists: the first secret's (both secrets are consistent points), a product-inconsistent linearised point's (a
    non-empty space, usually without a consistent point), the first secret's with a duplicate's value flipped (inconsistent), the
    first secret's negated (the same bits), random ones"""
    at = lambda pt: [e.evaluate(pt) for e in bq]                           # noqa: E731
    first = at(secrets[0])
    loose = at(rng.getrandbits(tw.q._cols))
    flipped = list(first)
    flipped[len(bq) - dups] ^= 1
    rand = [rng.getrandbits(1) for _ in bq]
    return [_values(groups, first), _values(groups, loose), _values(groups, flipped), [-v for v in _values(groups, first)],
            _values(groups, rand)]


# -- 1. quadratic factor parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 33, 64, 100])
def test_quadratic_factor_equals_int_front_end(n):
    tw, bq, bp, secrets, rng = _planted(n, 6100 + n)
    eq, ep, groups = _vectors(bq, bp)
    values_list = _instances(rng, tw, bq, groups, secrets)
    with tw.q.factor(eq) as fq, tw.p.factor(ep) as fp:
        assert type(fp) is PackedQuadFactoredSystem
        assert np.array_equal(fp.rhs_words(values_list), fq.rhs_words(values_list))
        seen = _agree(fp, fq, tw.q, values_list)
        assert _agree(fp, fq, tw.q, values_list[::-1]) == seen[::-1]      # any order, any number of calls
    # the one-shot forms: one elimination, nothing kept
    assert [_space(s) for s in tw.p.solve_raw_space_rhs(ep, values_list)] == [s for s, _ in seen]
    assert tw.p.solve_raw_one_rhs(ep, values_list) == tw.q.solve_raw_one_rhs(eq, values_list)
    assert tw.p.solve_one_rhs(ep, values_list) == tw.q.solve_one_rhs(eq, values_list) == [w[0] if w else None for _, w in seen]
    inconsistent = sum(s is None for s, _ in seen)
    several = sum(s is not None and s[0] >= 2 and len(w) > 1 for s, w in seen)
    empty_handed = sum(s is not None and not w for s, w in seen)
    assert inconsistent >= 1 and several >= 1 and empty_handed >= 1, (n, inconsistent, several, empty_handed)


# -- 2. append and copy ----------------------------------------------------------------------------------------------------------------
def test_add_and_copy_equal_fresh_solves():
    n = 20
    tw, bq, bp, secrets, rng = _planted(n, 6200, short=30, dups=2)
    q, p, x, y = tw.q, tw.p, tw.qx, tw.px
    eq, ep, groups = _vectors(bq, bp)
    bits = [e.evaluate(secrets[0]) for e in bq]
    vals = _values(groups, bits)
    grew = same = 0

    def fresh(zeros_q, fp, fq, values, values_q=None):
        """fp / fq on `values` against QuadraticSystem's own solve of the stacked equations"""
        sq = q.solve_raw_space(zeros_q)
        values_q = values if values_q is None else values_q
        assert _space(fp.solve_raw_space_rhs([values])[0]) == _space(fq.solve_raw_space_rhs([values_q])[0]) == _space(sq)
        assert fp.solve_raw_one_rhs([values])[0] == q.solve_raw_one(zeros_q)
        assert fp.search_all(values) == q.search_all(zeros_q)
        assert fp.search_one(values) == q.search_one(zeros_q)
        if sq is not None and sq.dimension <= 16:
            assert list(fp.solve_all(values)) == list(q.solve_all(zeros_q))
            assert fp.solve_one(values) == q.solve_one(zeros_q)
        return sq

    zeros = [e ^ v for e, v in zip(eq, vals)]
    with q.factor(eq) as fq, p.factor(ep) as fp:
        base = fresh(zeros, fp, fq, vals)
        assert base is not None and base.dimension >= 25
        rank0 = fp._handle(1).rank
        # plain rows (a vector of linear bits), product rows, rows that add nothing (one of the base's bits once more)
        steps = [([x[:6] ^ x[7:13]], [y[:6] ^ y[7:13]], [x[:6].evaluate(secrets[0]) ^ x[7:13].evaluate(secrets[0])]),
                 ([q.mul_bit(x[1], x[2]) ^ x[3], q.mul_bit(x[4], x[9]).concat(q.mul_bit(x[5], x[6]) ^ q.mul_bit(x[0], x[19]))],
                  [p.mul_bit(y[1], y[2]) ^ y[3], p.mul_bit(y[4], y[9]).concat(p.mul_bit(y[5], y[6]) ^ p.mul_bit(y[0], y[19]))], None),
                 ([bq[5], bq[9] ^ bq[11]], [bp[5], bp[9] ^ bp[11]], None)]
        for add_q, add_p, v in steps:
            if v is None:
                v = [e.evaluate(secrets[0]) for e in add_q]
            before = fp._handle(1).rank
            fq.add(add_q)
            fp.add(add_p)
            vals = vals + v
            zeros = zeros + [e ^ w for e, w in zip(add_q, v)]
            assert fp.rows == fq.rows and np.array_equal(fp.rhs_words([vals]), fq.rhs_words([vals]))
            fresh(zeros, fp, fq, vals)
            after = fp._handle(1).rank
            grew += after > before
            same += after == before
            assert fp._handle(0).rank == after == fq._handle(1).rank and fp._handle(1).pivots == fq._handle(1).pivots
        # the guess loop: bit_assert(a, v) for both v on copies; the original answers as before
        want_orig = (_space(fp.solve_raw_space_rhs([vals])[0]), fp.search_all(vals))
        for v in (0, 1):
            a = (x[2] ^ x[11], y[2] ^ y[11])
            gq, gp = q.bit_assert(a[0], v), p.bit_assert(a[1], v)
            with fq.copy() as cq, fp.copy() as cp:
                before = cp._handle(1).rank
                cq.add(gq)
                cp.add(gp)
                gv = [0] * len(gq)
                pv = [0, 0]
                assert np.array_equal(cp.rhs_words([vals + pv]), cq.rhs_words([vals + gv]))
                fresh(zeros + list(gq), cp, cq, vals + pv, vals + gv)
                assert _space(cp.solve_raw_space_rhs([vals + pv])[0]) == _space(cq.solve_raw_space_rhs([vals + gv])[0])
                grew += cp._handle(1).rank > before
            assert (_space(fp.solve_raw_space_rhs([vals])[0]), fp.search_all(vals)) == want_orig
        # an add that fails with a bad argument leaves the object answering as before
        other = PackedQuadraticSystem([200]).gens()[0]
        with pytest.raises(ValueError):
            fp.add([other[:2]])
        lin, off, ta, tb = random_terms(rng, n + 1, 3, 2)
        h = fp._handle(1)
        with pytest.raises(ValueError, match="n_lin"):
            h.append_quad(lin, off, ta, tb, n + 1)
        assert h.rows == fp.rows and h.rank == fq._handle(1).rank
        assert (_space(fp.solve_raw_space_rhs([vals])[0]), fp.search_all(vals)) == want_orig
        assert fp._handle(1).rank > rank0
    assert grew >= 1 and same >= 1, (grew, same)
    # the C ABI's own check of the same mistake, through hip
    lin, off, ta, tb = random_terms(rng, 6, hip.quad_cols(6), 2)
    with hip.factor_quad_terms(lin, off, ta, tb, 6, mode=1) as f:
        rank = f.rank
        with pytest.raises(ValueError, match="n_lin does not match"):
            f.append_quad_terms(*random_terms(rng, 7, 2, 2), 7)
        assert f.rank == rank and f.rows == hip.quad_cols(6)


def test_failed_append_rolls_back(monkeypatch):
    """add's rollback with live handles: the append to the mode-0 factorization succeeds, the one to the mode-1 factorization
    fails with a bad argument.  The object then answers as before (the arrays a snapshot shares were not written), the handle
    that holds the new rows is dropped and made again from the old rows on next use, and a later add goes through."""
    n = 14
    tw, bq, bp, secrets, rng = _planted(n, 6250, short=6, dups=2)
    q, p, x, y = tw.q, tw.p, tw.qx, tw.px
    eq, ep, groups = _vectors(bq, bp)
    vals = _values(groups, [e.evaluate(secrets[0]) for e in bq])
    for quadratic in (True, False):
        if quadratic:
            fq, fp = q.factor(eq), p.factor(ep)
            add_q, add_p = [q.mul_bit(x[1], x[2]) ^ x[3], x[4:9]], [p.mul_bit(y[1], y[2]) ^ y[3], y[4:9]]
            values = vals
        else:
            lin, plin = LinearSystem([40]), PackedLinearSystem([40])
            (u,), (w,) = lin.gens(), plin.gens()
            masks = [rng.getrandbits(40) for _ in range(5)]
            fq, fp = lin.factor([(u & m) ^ u.rotl(3) for m in masks[:3]]), plin.factor([(w & m) ^ w.rotl(3) for m in masks[:3]])
            add_q, add_p = [(u & m)[:7] for m in masks[3:]], [(w & m)[:7] for m in masks[3:]]
            values = [rng.getrandbits(40) for _ in range(3)]
        more = [e.evaluate(secrets[0] if quadratic else 0x5A5A5A5A5A) for e in add_q]
        with fq, fp:
            one, space = fp.solve_raw_one_rhs([values]), _space(fp.solve_raw_space_rhs([values])[0])     # both handles exist
            assert one == fq.solve_raw_one_rhs([values]) and space == _space(fq.solve_raw_space_rhs([values])[0])
            before = (fp.rows, fp._nspans, fp._handle(0).rows, fp._handle(1).rank, fp.rhs_words([values]).tolist())
            real, calls = type(fp)._append_to, []

            def failing(self, h, new):
                calls.append(h.mode)
                if len(calls) == 2:
                    raise ValueError("refused")                            # (what a GF2BV_ERR_ARG of the library becomes)
                real(self, h, new)
            with monkeypatch.context() as m:
                m.setattr(type(fp), "_append_to", failing)
                with pytest.raises(ValueError, match="refused"):
                    fp.add(add_p)
            assert calls == [0, 1]
            assert 0 not in fp._handles and fp._handles[1].rows == before[0]           # the handle with the new rows is gone
            assert (fp.rows, fp._nspans, fp._handle(0).rows, fp._handle(1).rank, fp.rhs_words([values]).tolist()) == before
            assert fp.solve_raw_one_rhs([values]) == one and _space(fp.solve_raw_space_rhs([values])[0]) == space
            with pytest.raises(ValueError, match="values for"):
                fp.solve_raw_one_rhs([values + more])
            fq.add(add_q)
            fp.add(add_p)                                                  # and now it goes through, on both handles
            assert fp.rows == fq.rows == before[0] + sum(len(e) for e in add_q)
            assert fp.solve_raw_one_rhs([values + more]) == fq.solve_raw_one_rhs([values + more])
            assert _space(fp.solve_raw_space_rhs([values + more])[0]) == _space(fq.solve_raw_space_rhs([values + more])[0])
            assert fp._handle(0).rank == fp._handle(1).rank == fq._handle(1).rank


# -- 3. linear ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [40, 130, 700])
def test_linear_factor_add_and_rhs(cols):
    rng = random.Random(6300 + cols)
    lin, plin = LinearSystem([cols - 8, 8]), PackedLinearSystem([cols - 8, 8])
    (x, x2), (y, y2) = lin.gens(), plin.gens()
    nx = cols - 8
    eq, ep = [], []
    for k in range(cols // 8 - 2):                                        # fewer independent rows than columns
        m, r = rng.getrandbits(nx), rng.randrange(nx)
        a, b = (x & m) ^ x.rotl(r), (y & m) ^ y.rotl(r)
        if k % 3 == 0:
            a, b = a.sum().concat(x2), b.sum().concat(y2)
        eq.append(a if k % 5 else a[:11])
        ep.append(b if k % 5 else b[:11])
    eq += [eq[0], rng.getrandbits(cols + 1) | 2]                           # a repeated vector (rank deficiency), an equation int
    ep += [ep[0], eq[-1]]
    secret = rng.getrandbits(cols)

    def values(exprs, n, honest):
        out = []
        for i in range(n):
            vals = [e.evaluate(secret) if not isinstance(e, int) else bin(e >> 1 & secret).count("1") & 1 ^ (e & 1) for e in exprs]
            if not honest or i % 2:
                vals = [rng.getrandbits(max(len(e), 1) if not isinstance(e, int) else 1) for e in exprs]
            out.append(vals)
        return out

    seen_none = seen_some = 0
    with lin.factor(eq) as fq, plin.factor(ep) as fp:
        assert type(fp) is PackedFactoredSystem
        exprs_q = list(eq)
        for round_ in range(3):
            neg = [v if isinstance(e, int) else -v for e, v in zip(exprs_q, values(exprs_q, 1, True)[0])]      # (|v|: the same bits)
            vl = values(exprs_q, 4, True) + [neg]
            assert np.array_equal(fp.rhs_words(vl), fq.rhs_words(vl))
            assert fp.solve_raw_one_rhs(vl) == fq.solve_raw_one_rhs(vl)
            sp, sq = fp.solve_raw_space_rhs(vl), fq.solve_raw_space_rhs(vl)
            assert [_space(s) for s in sp] == [_space(s) for s in sq]
            assert fp.solve_one_rhs(vl) == fq.solve_one_rhs(vl)
            assert fp.solve_one(vl[0]) == fq.solve_one(vl[0])
            assert fp._handle(1).rank == fq._handle(1).rank and fp._handle(1).pivots == fq._handle(1).pivots
            seen_none += sum(s is None for s in sq)
            seen_some += sum(s is not None for s in sq)
            with pytest.raises(TypeError):
                fp.search_one(vl[0])
            m = rng.getrandbits(nx)
            add_q, add_p = [(x & m)[:9], x2 ^ (x >> 3)[:8]], [(y & m)[:9], y2 ^ (y >> 3)[:8]]
            fq.add(add_q)
            fp.add(add_p)
            exprs_q += add_q
    ep_all = ep                                                            # the one-shot forms on the first expressions
    vl0 = values(eq, 3, True)
    assert plin.solve_raw_one_rhs(ep_all, vl0) == lin.solve_raw_one_rhs(eq, vl0)
    assert [_space(s) for s in plin.solve_raw_space_rhs(ep_all, vl0)] == [_space(s) for s in lin.solve_raw_space_rhs(eq, vl0)]
    assert plin.solve_one_rhs(ep_all, vl0) == lin.solve_one_rhs(eq, vl0)
    assert seen_none >= 1 and seen_some >= 1, (seen_none, seen_some)


def test_mt19937_known_answer_through_a_kept_factorization():
    """tests/test_gpu_factor.py's scenario on the packed front-end: 624 outputs of 32 bits and the top bit of mt[0] fix the state; a
    factorization of all but the last 8 outputs takes those in by add; several captures share it, and LinearSystem's factored
    system (the int front-end, generation included) gives the same answers"""
    plin, lin = PackedLinearSystem([32] * 624), LinearSystem([32] * 624)
    sym, ref = MT19937(plin.gens()), MT19937(lin.gens())
    exprs = [plin.gens()[0]] + [sym.getrandbits(32) for _ in range(624)]
    exprs_q = [lin.gens()[0]] + [ref.getrandbits(32) for _ in range(624)]
    states, outs = [], []
    for seed in (3142, 1000, 1001):
        r = random.Random(seed)
        states.append(tuple(r.getstate()[1][:-1]))
        outs.append([0x80000000] + [r.getrandbits(32) for _ in range(624)])
    with plin.factor(exprs[:617]) as fs, lin.factor(exprs_q[:617]) as fq:
        short = [o[:617] for o in outs]
        assert np.array_equal(fs.rhs_words(short), fq.rhs_words(short))
        sp, sq = fs.solve_raw_space_rhs(short[:1])[0], fq.solve_raw_space_rhs(short[:1])[0]
        assert _space(sp) == _space(sq) and sp.dimension > 0
        before = fs._handle(1).rank
        fs.add(exprs[617:])
        fq.add(exprs_q[617:])
        assert fs._handle(1).rank == fq._handle(1).rank == 19968 > before and fs._handle(1).pivots == fq._handle(1).pivots
        assert fs.solve_one_rhs(outs) == fq.solve_one_rhs(outs) == states
        assert fs.solve_one(outs[1]) == states[1]
        assert fs.solve_raw_one_rhs(outs) == fq.solve_raw_one_rhs(outs)
    assert plin.solve_one_rhs(exprs, outs[2:]) == states[2:]
    assert plin.solve_one([e ^ o for e, o in zip(exprs, outs[0])]) == states[0]


# -- 4. batches ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gang", [1, 3, 8])
def test_batches_equal_single_solves(gang, monkeypatch):
    monkeypatch.setenv("GF2BV_GANG", str(gang))
    n = 12
    rng = random.Random(6400)
    tw = Twin([n])
    p, y, cols = tw.p, tw.px, tw.p._cols
    systems = []
    for k in range(11):
        neq = (cols - 9, cols + 5, cols, cols - 1, cols + 17)[k % 5]      # live rows differ; several have fewer rows than columns
        secret = _raw(n, rng.getrandbits(n))
        zs = []
        for _ in range(neq):
            _, f = tw.bit(rng, rng.randint(0, 3), False)
            zs.append(f ^ f.evaluate(secret))
        systems.append(zs)
    systems[4] = systems[4] + [p.mul_bit(y[0], y[0]) ^ y[0] ^ 1]          # expands to the constant 1: inconsistent
    systems[7] = [systems[7][0] ^ systems[7][0]] + systems[7]             # a row that expands to 0
    systems[9] = []                                                        # no rows at all: every row is padding
    want_space = [p.solve_raw_space(z) for z in systems]
    got_space = p.solve_raw_space_many(systems)
    assert [_space(s) for s in got_space] == [_space(s) for s in want_space]
    assert p.solve_raw_one_many(systems) == [p.solve_raw_one(z) for z in systems]
    ones = p.solve_one_many(systems)
    assert ones == [None if r is None else p.convert_sol(r) for r in (p.solve_raw_one(z) for z in systems)]
    assert sum(s is None for s in want_space) == 1 and want_space[4] is None
    assert sum(len(z) < cols for z in systems) >= 3 and want_space[9].dimension == cols
    assert p.solve_raw_space_many(systems[:1])[0].origin == want_space[0].origin and p.solve_raw_space_many([]) == []


# -- 5. the batched expansion alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 64, 65, 128])
def test_batched_expansion_equals_int_front_end(n):
    rng = random.Random(6500 + n)
    q = QuadraticSystem([n])
    wt = (q._cols + 1 + 63) // 64
    lives = [5, 0, 9, 1, 3]
    many = 0
    for rows, stride in ((9, wt), (12, wt + 3), (10, wt + (wt & 1))):
        parts = [random_terms(rng, n, live, 11 if k == 2 else 4) for k, live in enumerate(lives)]       # (11: beyond one pass's 8)
        many += max(int(np.diff(t[1]).max(initial=0)) for t in parts) > 8
        lin = np.concatenate([t[0] for t in parts])
        cnt = np.concatenate([np.diff(t[1]) for t in parts])
        off = np.zeros(len(lin) + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        ta, tb = np.concatenate([t[2] for t in parts]), np.concatenate([t[3] for t in parts])
        sys_off = np.concatenate(([0], np.cumsum(lives))).astype(np.int64)
        got = hip.quad_expand_batch_words(lin, off, ta, tb, sys_off, n, rows, stride_words=stride)
        assert got.shape == (len(lives), rows, stride)
        for s, (t, live) in enumerate(zip(parts, lives)):
            want = to_aug(expand_ints(q, *t) + [0] * (rows - live), q._cols, stride)
            assert np.array_equal(got[s], want), (n, s, rows, stride, np.argwhere(got[s] != want)[:4])   # padding rows, bits behind cols
    assert many >= 1


# -- 6. C ABI identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kmode", [(9, 0), (9, 1), (46, 1)])
def test_factor_quad_terms_is_solve_rhs_words_of_the_expansion(n, kmode):
    rng = random.Random(6600 + n + kmode)
    cols = hip.quad_cols(n)
    live, rows = cols - 7, cols + 3
    terms = random_terms(rng, n, live, 3)
    aug = hip.quad_expand_words(*terms, n, rows=rows)
    rw = (rows + 63) // 64

    def rhs_for(a, count):
        """right-hand sides: planted (A x for random x), and random ones"""
        nrows = a.shape[0]
        out = np.zeros((count, (nrows + 63) // 64), dtype=np.uint64)
        ints = [int.from_bytes(r.tobytes(), "little") & ((1 << cols) - 1) for r in a]
        for j in range(count):
            xs = rng.getrandbits(cols)
            bits = [bin(v & xs).count("1") & 1 for v in ints] if j % 2 == 0 else [rng.getrandbits(1) for _ in ints]
            out[j] = np.frombuffer(sum(b << i for i, b in enumerate(bits)).to_bytes(out.shape[1] * 8, "little"), dtype=np.uint64)
        return out

    with hip.factor_quad_terms(*terms, n, rows=rows, mode=kmode) as f:
        rhs = rhs_for(aug, 5)
        assert rhs.shape[1] == rw
        want = hip.solve_rhs_words(aug, rows, cols, rhs, kmode)
        assert [_key(s) for s in f.solve(rhs)] == [_key(s) for s in want]
        assert [_key(s) for s in hip.solve_rhs_quad_terms(*terms, n, rhs, rows=rows, mode=kmode)] == [_key(s) for s in want]
        assert f.rank == want[0].rank and np.array_equal(f.pivots, want[0].pivots)
        assert {s.status for s in want} == {0, 1}
        more = random_terms(rng, n, 11, 3)
        f.append_quad_terms(*more, n)
        stacked = np.vstack([aug, hip.quad_expand_words(*more, n)])
        assert f.rows == rows + 11
        rhs = rhs_for(stacked, 5)
        want = hip.solve_rhs_words(stacked, rows + 11, cols, rhs, kmode)
        assert [_key(s) for s in f.solve(rhs)] == [_key(s) for s in want]
        assert f.rank == want[0].rank and np.array_equal(f.pivots, want[0].pivots)


# -- 7. rows that expand to 0 and to the constant 1 ---------------------------------------------------------------------------------------
def test_rows_that_expand_to_zero_or_one_in_factor_add_and_batch():
    n = 6
    tw = Twin([n])
    q, p, x, y = tw.q, tw.p, tw.qx, tw.px
    nothing_p, nothing_q = p.mul_bit(y[0], y[1]) ^ p.mul_bit(y[1], y[0]), q.mul_bit(x[0], x[1]) ^ q.mul_bit(x[1], x[0])
    one_p, one_q = p.mul_bit(y[0], y[0]) ^ y[0] ^ 1, q.mul_bit(x[0], x[0]) ^ x[0] ^ 1
    assert nothing_q._bits == (0,) and one_q._bits == (1,)
    eq, ep = [x[2] ^ x[3], nothing_q, one_q, 0], [y[2] ^ y[3], nothing_p, one_p, 0]
    # value bits: the row "1" is consistent exactly when its value is 1, the rows "0" exactly when theirs is 0
    vl = [[0, 0, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 1, 1], [1, 0, 1, 0]]
    dead = [False, False, True, True, True, False]
    with q.factor(eq) as fq, p.factor(ep) as fp:
        assert np.array_equal(fp.rhs_words(vl), fq.rhs_words(vl))
        sp, sq = fp.solve_raw_space_rhs(vl), fq.solve_raw_space_rhs(vl)
        assert [_space(s) for s in sp] == [_space(s) for s in sq] and [s is None for s in sp] == dead
        assert [r is None for r in fp.solve_raw_one_rhs(vl)] == dead
        fq.add([one_q, x[1], nothing_q])
        fp.add([one_p, y[1], nothing_p])
        vl2 = [v + t for v, t in zip(vl, ([1, 0, 0], [1, 1, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]))]
        dead2 = [False, False, True, True, True, True]
        sp, sq = fp.solve_raw_space_rhs(vl2), fq.solve_raw_space_rhs(vl2)
        assert [_space(s) for s in sp] == [_space(s) for s in sq] and [s is None for s in sp] == dead2
        assert fp.search_all(vl2[0]) == fq.search_all(vl2[0]) and len(fp.search_all(vl2[0])) == 1 << (n - 2)
    assert [_space(s) for s in p.solve_raw_space_rhs(ep, vl)] == [_space(s) for s in q.solve_raw_space_rhs(eq, vl)]
    batch = [[nothing_p], [one_p, y[0]], [y[0], nothing_p, 0], [nothing_p, 1], []]
    got = p.solve_raw_space_many(batch)
    assert [s is None for s in got] == [False, True, False, True, False]
    assert [_space(s) for s in got] == [_space(p.solve_raw_space(z)) for z in batch]
    assert got[0].dimension == got[4].dimension == p._cols
