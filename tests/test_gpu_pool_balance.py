"""Every entry gives back to the pool what it took: hip.pool_in_use (buffers, streams and events handed out and not yet returned) reads
the same after an entry as before it, once what the entry returned is gone -- on success, for an inconsistent system (a result, not
an error), and for a call that is refused.  A kept handle raises the numbers by what it owns until it is closed.

One thread, except the last test: while another thread is inside the library the numbers are a snapshot of its work."""
import functools
import gc
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import compose_terms as CT
from tests import cubic_forms as CF
from tests import quad_forms as QF
from tests import quartic_forms as Q4F
from tests import thread_jobs as J
from tests import threads as T
from tests.cubic_terms import random_cubic_terms
from tests.quad_terms import random_terms
from tests.quartic_terms import random_quartic_terms
from tests.small_cases import digits
from tests.systems import random_system
from tests.test_gpu_compose import dense, invertible_affine
from tests.test_gpu_quad_search import _planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def in_use(collect: bool = False) -> dict:
    """the numbers now; collect: after whatever Python still owns by a reference cycle is gone (results and handles are freed when their
    last reference goes; a full collection costs more than most cases here, so it runs once per case)"""
    if collect:
        gc.collect()
    return hip.pool_in_use(0)


def balanced(call, refused=None):
    """`call` leaves the numbers as they were once its result is gone; so does `refused`, which must raise ValueError (GF2BV_ERR_ARG)"""
    before = in_use(collect=True)
    out = call()
    del out
    assert in_use() == before
    if refused is not None:
        with pytest.raises(ValueError):
            refused()
        assert in_use() == before


# -- single solves ------------------------------------------------------------------------------------------------------------------------
# 64 x 64: the one-launch path (the input read from pinned host memory, or copied to a pool buffer first); 200 x 130 with GF2BV_SMALL=0:
# the blocked path
SHAPES = {"small": (64, 64, {}), "small_copied": (64, 64, {"GF2BV_SMALL_ZC": "0"}), "blocked": (200, 130, {"GF2BV_SMALL": "0"})}


def _system(rows: int, cols: int, consistent: bool = True) -> list:
    eqs = random_system(random.Random(100 * rows + cols), rows, cols, .5, cols - 7, True, 0)
    if not consistent:
        eqs[-1] = eqs[0] ^ 1                           # the first equation again, with the other constant
    return eqs


def _solve(form: str, eqs: list, rows: int, cols: int, mode: int, device: int = 0):
    if form == "words":
        return hip.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, mode, device)
    if form == "digits":
        return hip.solve_digits(*digits(eqs, 30), 30, rows, cols, mode, device)
    stride = hip.padded_stride(cols)
    buf = hip.DeviceBuffer(rows * stride * 8)
    try:
        buf.upload(O.eqs_to_aug(eqs, cols, stride))
        return hip.solve_device(buf.ptr, rows, cols, stride, mode, device)
    finally:
        buf.free()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", ["words", "digits", "device"])
def test_single_solves(monkeypatch, form, shape, mode):
    rows, cols, env = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eqs = _system(rows, cols)
    want = O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, mode)

    def call():
        sol = _solve(form, eqs, rows, cols, mode)
        assert sol.stats["small_path"] == (shape != "blocked") and (sol.status, sol.rank) == (want["status"], want["rank"])
        return sol
    balanced(call, lambda: _solve(form, eqs, rows, cols, 3))
    balanced(call, lambda: _solve(form, eqs, rows, cols, mode, device=99))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", ["words", "digits", "device"])
def test_an_inconsistent_system_is_a_result(monkeypatch, form, shape):
    rows, cols, env = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eqs = _system(rows, cols, consistent=False)
    assert O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, 1)["status"] != 0

    def call():
        sol = _solve(form, eqs, rows, cols, 1)
        assert not sol.solved
    balanced(call)


# -- batches: 5 systems in gangs of 2 -- three gangs, the last one ragged, on two host threads -----------------------------------------------
@pytest.mark.parametrize("form", ["device", "digits"])
def test_batches(monkeypatch, form):
    monkeypatch.setenv("GF2BV_SMALL", "0")
    monkeypatch.setenv("GF2BV_GANG", "2")
    nsys, rows, cols = 5, 96, 64
    rng = random.Random(5)
    systems = [random_system(rng, rows, cols, .5, cap) for cap in (None, 40, 1, 63, 20)]
    want = [O.solve_words(O.eqs_to_aug(e, cols), rows, cols, 1)["rank"] for e in systems]
    if form == "digits":
        dig, off = digits([e for s in systems for e in s], 30)
        solve = lambda mode=1, device=0: hip.solve_batch_digits(dig, off, 30, nsys, rows, cols, mode, device)      # noqa: E731
    else:
        augs = np.stack([O.eqs_to_aug(e, cols, 2) for e in systems])
        solve = lambda mode=1, device=0: hip.solve_batch_words(augs, rows, cols, mode, device)                     # noqa: E731

    def call():
        sols = solve()
        assert [s.rank for s in sols] == want and sols[0].stats["gang_systems"] == 2
    balanced(call, lambda: solve(mode=3))


# -- many right-hand sides -----------------------------------------------------------------------------------------------------------------
RHS = (130, 100, 3)


def _rhs_case():
    rows, cols, nrhs = RHS
    rng = random.Random(31)
    eqs = random_system(rng, rows, cols, .5, 60, True, 0)
    aug = O.eqs_to_aug(eqs, cols)
    bits = J.make_rhs(rng, aug, rows, cols, nrhs)
    return eqs, aug, bits, J.oracle_rhs(aug, rows, cols, bits, 1)


@pytest.mark.parametrize("form", ["words", "digits", "device"])
def test_right_hand_sides(form):
    rows, cols, nrhs = RHS
    eqs, aug, bits, want = _rhs_case()
    rhs = J.rhs_words(bits)

    def solve(mode=1, device=0):
        if form == "words":
            return hip.solve_rhs_words(aug, rows, cols, rhs, mode, device)
        if form == "digits":
            return hip.solve_rhs_digits(*digits(eqs, 30), 30, rows, cols, rhs, mode, device)
        stride = hip.padded_stride(cols)
        a, b = hip.DeviceBuffer(rows * stride * 8), hip.DeviceBuffer(rhs.nbytes)
        try:
            a.upload(O.eqs_to_aug(eqs, cols, stride))
            b.upload(rhs)
            return hip.solve_rhs_device(a.ptr, rows, cols, stride, b.ptr, nrhs, rhs.shape[1], mode, device)
        finally:
            a.free()
            b.free()

    def call():
        assert J.solve_many(solve(), 1) == want
    balanced(call, lambda: solve(mode=3))
    balanced(call, lambda: solve(device=99))


# -- a kept factorization ------------------------------------------------------------------------------------------------------------------
def test_kept_handle():
    rows, cols, _ = RHS
    eqs, aug, bits, want = _rhs_case()
    rng = random.Random(32)
    base = in_use(collect=True)
    with pytest.raises(ValueError):
        hip.factor_words(aug, rows, cols, 3)
    assert in_use() == base
    f = hip.factor_words(aug, rows, cols, 1)
    held = in_use()
    # the handle owns the working matrix and the arena, and the solver's streams and events
    assert held["buffers"] == base["buffers"] + 2 and held["streams"] > base["streams"] and held["events"] > base["events"]
    for nrhs in (1, 65):                               # one pass, two passes
        b = J.make_rhs(rng, aug, rows, cols, nrhs)
        many = J.oracle_rhs(aug, rows, cols, b, 1)
        balanced(lambda: J.solve_many(f.solve(J.rhs_words(b)), 1) == many or pytest.fail("Factor.solve"),
                 lambda: f.solve(np.zeros((1, 1), dtype=np.uint64)))          # (one word does not cover 130 rows)
    more = O.eqs_to_aug(random_system(rng, 3, cols, .5, None, True, 0), cols)
    with pytest.raises(ValueError):
        f.append_words(more[:, :1])                    # (one word does not cover 101 bits)
    assert in_use() == held
    f.append_words(more)                               # 133 rows outgrow the 130 factored: a larger matrix replaces the old one, and the
    grown = in_use()                                   # rows' records move from the arena into a buffer of the handle's own
    assert f.rows == rows + 3 and grown == dict(held, buffers=held["buffers"] + 1)
    f.append_words(more)                               # within the capacity now: nothing more is kept
    assert f.rows == rows + 6 and in_use() == grown
    balanced(lambda: f.solve(np.zeros((2, 3), dtype=np.uint64)))
    c = f.copy()                                       # its own matrix, arena and row records, one stream, four timing events
    both = in_use()
    assert both == {"buffers": grown["buffers"] + 3, "streams": grown["streams"] + 1, "events": grown["events"] + 4}
    balanced(lambda: c.solve(np.zeros((1, 3), dtype=np.uint64)))
    c.close()
    assert in_use() == grown
    f.close()
    del f, c
    assert in_use(collect=True) == base


# -- the front-ends, at the smallest shapes their own GPU tests use --------------------------------------------------------------------------
def _job(build, seed: int = 0):
    """the callable of one job of tests/thread_jobs.py (one library call) with its reference checked"""
    name, call, want = build([seed])[0]

    def checked():
        got = call()
        assert T.same(got, want), name
    return checked


def _quad_terms(n: int = 12, rows: int = 20):
    return random_terms(random.Random(41), n, rows, 3)


def _batch_terms(n: int = 8):
    parts = [random_terms(random.Random(42 + s), n, live, 3) for s, live in enumerate((5, 0, 11))]
    lin = np.concatenate([p[0] for p in parts])
    off = np.concatenate([[0]] + [p[1][1:] + sum(len(q[2]) for q in parts[:s]) for s, p in enumerate(parts)]).astype(np.int64)
    ta, tb = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
    return (lin, off, ta, tb, [0, 5, 5, 16]), n


def _linear_form(ref, seed: int, R: int = 24) -> int:
    return ref.DenseMap(random.Random(seed + R), R).y(0)


def _search_all_cases() -> dict:
    """QuadraticSystem.search_all and the two jobs of thread_jobs.search_all_jobs (AffineSpace.quad_search / cubic_search / quartic_search of
    the extension); refused: every one has a consistent point, so max_solutions=0 raises ValueError AFTER the device search has run"""
    from gf2bv_amd import PackedCubicSystem, PackedQuarticSystem, search_all_cubic, search_all_quartic
    from tests.cubic_terms import REGISTER_12, register_zeros
    from tests.quartic_terms import REGISTER4_12, register4_zeros
    q, zeros, _ = _planted(random.Random(7), 8, 40)
    c3, c4, secret = PackedCubicSystem([12]), PackedQuarticSystem([12]), 0x52F
    z3 = tuple(register_zeros(c3, secret, REGISTER_12["taps"], REGISTER_12["pos"], 40))
    z4 = tuple(register4_zeros(c4, secret, count=10, **REGISTER4_12))
    cases = {"search_all quad": (lambda: q.search_all(zeros) == list(q.solve_all(zeros, max_dimension=16)) or pytest.fail("search_all"),
                                 lambda: q.search_all(zeros, max_solutions=0))}
    refused = {"search_all_quartic": lambda: search_all_quartic(c4, z4, max_solutions=0), "search_all_cubic": lambda: search_all_cubic(c3, z3, max_solutions=0)}
    for name, call, want in J.search_all_jobs():       # (the same systems: their references are built there)
        cases[name] = (lambda call=call, want=want, name=name: T.same(call(), want) or pytest.fail(name), refused[name.split()[0]])
    return cases


def _compose_power_on_a_stream(device: int = 0):
    n, k = 65, 11
    m = invertible_affine(7, n)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_b = torch.from_numpy(m.view(np.int64)).cuda()
        d_out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    hip.compose_power_device(d_b.data_ptr(), 2, n, k, d_out.data_ptr(), 4, device=device, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64)[:, :2], CT.power(m, n, k))


@functools.lru_cache(maxsize=None)
def _front_ends() -> dict:
    """name -> (call, refused call or None), built once"""
    quad, cubic, quartic = _quad_terms(), random_cubic_terms(random.Random(43), 6, 8), random_quartic_terms(random.Random(44), 5, 6)
    guess3 = random_cubic_terms(random.Random(1020), 10, 20, max_terms=2)
    (blin, boff, bta, btb, bsys), bn = _batch_terms()
    xl_quad = J.X.quad_aug(J.X.planted_dense(random.Random(45), 9, 8, [0x155]), 9)
    a8, aff = dense(1, 5, CT.form_words(8)), invertible_affine(65, 65)
    cases = {
        "quad_expand_words": (_job(J.quad_expand_jobs), lambda: hip.quad_expand_words(*quad, 12, device=99)),
        "solve_quad_terms": (lambda: hip.solve_quad_terms(*quad, 12, mode=1), lambda: hip.solve_quad_terms(*quad, 12, mode=3)),
        "cubic_expand_words": (_job(J.cubic_expand_jobs), lambda: hip.cubic_expand_words(*cubic, 6, device=99)),
        "solve_cubic_terms": (lambda: hip.solve_cubic_terms(*cubic, 6, mode=1), lambda: hip.solve_cubic_terms(*cubic, 6, device=99)),
        "quartic_expand_words": (_job(J.quartic_expand_jobs), lambda: hip.quartic_expand_words(*quartic, 5, device=99)),
        "solve_quartic_terms": (lambda: hip.solve_quartic_terms(*quartic, 5, mode=1), lambda: hip.solve_quartic_terms(*quartic, 5, device=99)),
        "solve_batch_quad_terms": (lambda: hip.solve_batch_quad_terms(blin, boff, bta, btb, bsys, bn, mode=1),
                                   lambda: hip.solve_batch_quad_terms(blin, boff, bta, btb, bsys, bn, device=99)),
        "xl3_expand_words": (_job(J.xl3_expand_jobs), lambda: hip.xl3_expand_words(xl_quad, 9, device=99)),
        "xl4_expand_words": (_job(J.xl4_expand_jobs), lambda: hip.xl4_expand_words(xl_quad, 9, device=99)),
        "solve_xl3_guess_words": (_job(J.xl3_guess_jobs), lambda: hip.solve_xl3_guess_words(xl_quad, 9, (1, 8), device=99)),
        "solve_xl4_cubic_guess_terms": (lambda: hip.solve_xl4_cubic_guess_terms(*guess3, 10, (9, 4), mode=1),
                                        lambda: hip.solve_xl4_cubic_guess_terms(*guess3, 10, (9, 4), device=99)),
        "compose_words": (lambda: hip.compose_words(a8, 8, CT.identity(8), 8), lambda: hip.compose_words(a8, 8, CT.identity(8), 8, device=99)),
        "compose_power_words": (lambda: hip.compose_power_words(aff, 65, 5), lambda: hip.compose_power_words(aff, 65, 5, device=99)),
        "compose_power_device": (_compose_power_on_a_stream, lambda: _compose_power_on_a_stream(device=99)),
        "stream_ceiling": (lambda: hip.stream_ceiling(4 << 20), lambda: hip.stream_ceiling(1)),
        "lds_clock": (hip.lds_clock, lambda: hip.lds_clock(99)),
        "space_enumerate": (_job(J.space_jobs), lambda: hip.space_enumerate(np.zeros(2, np.uint64), np.ones((1, 2), np.uint64), 0, 4, device=99)),
    }
    for kind, ref, seed in (("quad", QF, 4500), ("cubic", CF, 5500), ("quartic", Q4F, 6500)):
        plan = {"quad": hip.quad_plan, "cubic": hip.cubic_plan, "quartic": hip.quartic_plan}[kind]
        origin, basis = J.plan_space(kind, random.Random(14000))
        search = J.FORMS[kind][1]
        cases[f"{kind}_plan device"] = (_job(lambda seeds, kind=kind: J.plan_jobs(kind, seeds)),
                                        lambda plan=plan, origin=origin, basis=basis: plan(origin, basis, 12, device=99))
        cases[f"{kind}_forms_search"] = (_job(lambda seeds, kind=kind: J.forms_jobs(kind, seeds)), lambda search=search: search([1], 13, device=99))
        # the one GF2BV_ERR_NOMEM return the GPU suite reaches on a device (test_point_cap_exceeded of the three forms files)
        cases[f"{kind}_forms_search over the cap"] = (lambda search=search, f=_linear_form(ref, seed): _over_the_cap(search, f), None)
    cases.update(_search_all_cases())
    return cases


def _over_the_cap(search, f: int):
    with pytest.raises(hip.HipError, match=r"^gf2bv_hip error 4: more common zeros than can be collected$"):
        search([f], 24, max_out=16)


FRONT_END_NAMES = ["quad_expand_words", "solve_quad_terms", "cubic_expand_words", "solve_cubic_terms", "quartic_expand_words", "solve_quartic_terms",
                   "solve_batch_quad_terms", "xl3_expand_words", "xl4_expand_words", "solve_xl3_guess_words", "solve_xl4_cubic_guess_terms",
                   "compose_words", "compose_power_words", "compose_power_device", "search_all quad", "stream_ceiling", "lds_clock", "space_enumerate",
                   "quad_plan device", "quad_forms_search", "quad_forms_search over the cap", "cubic_plan device", "cubic_forms_search",
                   "cubic_forms_search over the cap", "quartic_plan device", "quartic_forms_search", "quartic_forms_search over the cap",
                   "search_all_quartic n12 10 outputs", "search_all_cubic n12 40 outputs"]


@pytest.mark.parametrize("name", FRONT_END_NAMES)
def test_front_ends_and_diagnostics(name):
    cases = _front_ends()
    assert set(cases) == set(FRONT_END_NAMES)
    balanced(*cases[name])


# -- threads -------------------------------------------------------------------------------------------------------------------------------
def test_after_concurrent_callers():
    """four jobs of tests/thread_jobs.py from four threads; the numbers are read only when every thread has been joined"""
    jobs = [build([30 + k])[0] for k, build in enumerate((J.GROUPS["solve_small"], J.rhs_jobs, J.batch_jobs, J.quad_expand_jobs))]
    base = in_use(collect=True)
    assert T.run_concurrently(jobs, 4, 2, seed=300) == []
    assert in_use(collect=True) == base
