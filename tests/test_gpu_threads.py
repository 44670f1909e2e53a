"""The library's threading contract (include/gf2bv_hip.h, "Threading") under concurrent callers, for every entry built since the
single solves: both bindings drop the GIL around every call, so Python threads really are inside the library together.

What shows that these tests would see state shared between calls -- a pool buffer handed back before its stream has drained, a
stream or an uploaded array used by two calls -- is the CPU test of the harness (tests/test_thread_harness_cpu.py: contamination
between concurrent jobs is reported for every thread but one) together with exact equality against references outside the library
(tests/thread_jobs.py); no mutant that shares device state is run.  The thread-local records of part (e) are checked with ordered
threads, so that a record which is not thread-local fails them deterministically.

Every knob is read before a thread starts: nothing here changes the environment."""
import ctypes
import json
import os
import random
import sys
import threading

import numpy as np
import pytest

from gf2bv_amd import _internal, hip
from oracle import gf2_oracle as O
from tests import thread_jobs as J
from tests import threads as T
from tests.child import ROOT, run_child
from tests.systems import random_system

pytestmark = pytest.mark.gpu

THREADS, ROUNDS = 8, 4                   # (measured: every test here takes under 2 s at 2 rounds; 4 give more interleavings)
SEEDS = list(range(8))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


def _alone_then_together(jobs, seed: int, rounds: int = ROUNDS):
    """every job made alone equals its reference; then all of them from THREADS threads"""
    for name, call, want in jobs:
        got = call()
        assert T.same(got, want), (name, "alone", got, want)
    assert T.run_concurrently(jobs, THREADS, rounds, seed) == []


# -- a. same entry, different inputs per thread ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(J.GROUPS))
def test_same_entry_different_inputs(group):
    """8 differently seeded inputs of one entry, each thread running all of them in an order of its own: at any moment the threads
    are inside the same entry with different inputs"""
    _alone_then_together(J.GROUPS[group](SEEDS), seed=100 + list(J.GROUPS).index(group))


# -- b. all entries mixed -------------------------------------------------------------------------------------------------------------------
def test_all_entries_mixed():
    """one job of every entry in one table: pool buffers and streams go from one entry type to another"""
    jobs = J.mixed_jobs()
    assert len(jobs) >= len(J.GROUPS) + 5
    _alone_then_together(jobs, seed=200)


# -- c. one kept factorization shared by all threads ----------------------------------------------------------------------------------------
ROWS, COLS, CAP = 700, 650, 600
NRHS = [1, 3, 64, 65, 2, 8, 130, 5]


def _shared_factor_case():
    rng = random.Random(300)
    eqs = random_system(rng, ROWS, COLS, .5, CAP, True, 0)
    aug = O.eqs_to_aug(eqs, COLS)
    sets = [J.make_rhs(rng, aug, ROWS, COLS, n) for n in NRHS]                          # consistent (even) and random (odd) ones
    more = [rng.getrandbits(COLS + 1) for _ in range(70)] + [0]                         # appended to a copy: the rank rises
    stacked = np.vstack([aug, O.eqs_to_aug(more, COLS)])
    bits2 = J.make_rhs(rng, stacked, ROWS + len(more), COLS, 5)
    return eqs, aug, sets, more, stacked, bits2


def test_shared_factor_ctypes_binding():
    """Factor.solve from 8 threads on right-hand-side sets of their own equals solve_rhs_words (and, before a thread starts, the
    oracle) result for result; copies taken meanwhile, appended to and solved on, equal a fresh factorization of the stacked
    matrix; the shared handle answers afterwards as before"""
    eqs, aug, sets, more, stacked, bits2 = _shared_factor_case()
    rows2 = ROWS + len(more)
    more_aug = O.eqs_to_aug(more, COLS)
    with hip.factor_words(aug, ROWS, COLS, 1) as f:
        jobs = []
        for k, bits in enumerate(sets):
            rhs = J.rhs_words(bits)
            want = J.solve_many(hip.solve_rhs_words(aug, ROWS, COLS, rhs, 1), 1)
            if len(bits) <= 8:
                assert want == J.oracle_rhs(aug, ROWS, COLS, bits, 1)
            jobs.append((f"Factor.solve n{len(bits)}", lambda rhs=rhs: J.solve_many(f.solve(rhs), 1), want))
        rhs2 = J.rhs_words(bits2)
        want2 = J.oracle_rhs(stacked, rows2, COLS, bits2, 1)
        with hip.factor_words(stacked, rows2, COLS, 1) as fresh:
            assert J.solve_many(fresh.solve(rhs2), 1) == want2
            state2 = (rows2, fresh.rank, tuple(fresh.pivots.tolist()))

        def on_a_copy():
            with f.copy() as c:
                c.append_words(more_aug)
                return J.solve_many(c.solve(rhs2), 1), (c.rows, c.rank, tuple(c.pivots.tolist()))
        jobs.append(("Factor.copy + append + solve", on_a_copy, (want2, state2)))
        before = (f.rows, f.rank, tuple(f.pivots.tolist()), f.device_bytes)
        assert before[0] == ROWS and before[1] < state2[1]
        _alone_then_together(jobs, seed=300)
        assert (f.rows, f.rank, tuple(f.pivots.tolist()), f.device_bytes) == before
        for name, call, want in jobs[:3]:
            assert call() == want, name


def test_shared_factor_extension_binding():
    """the same through _internal.m4ri_factor and the Factorization object, against m4ri_solve_rhs"""
    eqs, aug, sets, more, stacked, bits2 = _shared_factor_case()
    as_int = lambda b: sum(int(v) << r for r, v in enumerate(b))          # noqa: E731
    keys = lambda sols: tuple(T.space_key(s) for s in sols)               # noqa: E731
    f = _internal.m4ri_factor(eqs, COLS, 1)
    try:
        jobs = []
        for bits in sets[:5]:
            rhs = [as_int(b) for b in bits]
            want = keys(_internal.m4ri_solve_rhs(eqs, COLS, 1, rhs))
            if len(bits) <= 3:
                assert want == keys([O.m4ri_solve([(e & ~1) | ((r >> i) & 1) for i, e in enumerate(eqs)], COLS, 1) for r in rhs])
            jobs.append((f"Factorization.solve n{len(bits)}", lambda rhs=rhs: keys(f.solve(rhs)), want))
        rhs2 = [as_int(b) for b in bits2]
        want2 = keys(_internal.m4ri_solve_rhs(eqs + more, COLS, 1, rhs2))

        def on_a_copy():
            c = f.copy()
            try:
                c.append(more)
                return keys(c.solve(rhs2)), c.rows
            finally:
                c.close()
        jobs.append(("Factorization.copy + append + solve", on_a_copy, (want2, ROWS + len(more))))
        before = (f.rows, f.rank, f.pivots, f.device_bytes)
        _alone_then_together(jobs, seed=310, rounds=1)
        assert (f.rows, f.rank, f.pivots, f.device_bytes) == before
    finally:
        f.close()


# -- d. getters beside an append ----------------------------------------------------------------------------------------------------------
D_ROWS, D_COLS = 140, 130
D_FREE = [0, 1, 5, 63, 64, 66, 100, 127, 128, 129, 7, 90]          # columns of A that are zero: each chunk gives two of them pivots
D_CHUNKS = 6


def _growing_case():
    """(equation ints of A, the chunks as equation ints, the k + 1 legitimate (rows, rank, pivots) states from the oracle)"""
    rng = random.Random(400)
    keep = (1 << D_COLS) - 1
    for c in D_FREE:
        keep &= ~(1 << c)
    eqs = [(rng.getrandbits(D_COLS) & keep) << 1 for _ in range(D_ROWS)]
    chunks = []
    for k in range(D_CHUNKS):
        own = D_FREE[2 * k:2 * k + 2]
        rows = [((rng.getrandbits(D_COLS) & keep) | (1 << own[0]) | (rng.getrandbits(1) << own[1])) << 1,
                ((rng.getrandbits(D_COLS) & keep) | (1 << own[1])) << 1, 0]
        chunks.append(rows)
    states, stacked = [], list(eqs)
    for k in range(D_CHUNKS + 1):
        w = O.solve_words(O.eqs_to_aug(stacked, D_COLS), len(stacked), D_COLS, 0)
        states.append((len(stacked), int(w["rank"]), tuple(int(p) for p in w["pivcols"])))
        if k < D_CHUNKS:
            stacked += chunks[k]
    assert [s[1] for s in states] == [D_COLS - len(D_FREE) + 2 * k for k in range(D_CHUNKS + 1)]      # the rank grows with every chunk
    return eqs, chunks, states


@pytest.mark.parametrize("binding", ["ctypes", "extension"])
def test_getters_beside_an_append(binding):
    """One thread appends chunks that raise the rank; three threads read rank, rows, pivots and device_bytes all the while.  Every
    pivots value is exactly one of the k + 1 states the handle goes through (never a mixture, never longer than its buffer), rank
    and rows are values of those states and never decrease.  The appender lets the readers get some reads in between two chunks."""
    eqs, chunks, states = _growing_case()
    if binding == "ctypes":
        f = hip.factor_words(O.eqs_to_aug(eqs, D_COLS), D_ROWS, D_COLS, 1)
        append = lambda rows: f.append_words(O.eqs_to_aug(rows, D_COLS))      # noqa: E731
        pivots = lambda: tuple(f.pivots.tolist())                             # noqa: E731
    else:
        f = _internal.m4ri_factor(eqs, D_COLS, 1)
        append, pivots = f.append, lambda: tuple(f.pivots)                    # noqa: E731
    legit_rows, legit_rank, legit_piv = {s[0] for s in states}, {s[1] for s in states}, {s[2]: k for k, s in enumerate(states)}
    problems, done, reads = [], threading.Event(), [0]
    cond, start = threading.Condition(), threading.Barrier(4)

    def reader(t):
        last = [-1, -1, -1, -1]                                               # rank, rows, state of the pivots, device bytes
        try:
            start.wait(timeout=60)
            while True:
                finished = done.is_set()                                      # (one more pass after the last append)
                got = [f.rank, f.rows, legit_piv.get(pivots(), None), f.device_bytes]
                if got[0] not in legit_rank or got[1] not in legit_rows or got[2] is None or got[3] <= 0:
                    problems.append((t, "not a state of the handle", got))
                    return
                if any(g < b for g, b in zip(got, last)):
                    problems.append((t, "went backwards", last, got))
                    return
                last = got
                with cond:
                    reads[0] += 1
                    cond.notify_all()
                if finished:
                    if (got[0], got[1], got[2]) != (states[-1][1], states[-1][0], D_CHUNKS):
                        problems.append((t, "not the final state after the last append", got))
                    return
        except BaseException as e:      # noqa: BLE001
            problems.append((t, f"{type(e).__name__}: {e}"))

    def appender():
        try:
            start.wait(timeout=60)
            for rows in chunks:
                with cond:
                    seen = reads[0]
                    cond.wait_for(lambda: reads[0] >= seen + 6 or len(problems) > 0, timeout=20)
                if problems:
                    break
                append(rows)
        except BaseException as e:      # noqa: BLE001
            problems.append(("appender", f"{type(e).__name__}: {e}"))
        finally:
            done.set()

    pool = [threading.Thread(target=reader, args=(t,)) for t in range(3)] + [threading.Thread(target=appender)]
    try:
        for th in pool:
            th.start()
        for th in pool:
            th.join()
        assert problems == []
        assert reads[0] >= 6 * D_CHUNKS
        assert (f.rows, f.rank, pivots()) == states[-1]
    finally:
        f.close()                       # (every thread has been joined: no call is running on the handle)


# -- e. per-thread state ----------------------------------------------------------------------------------------------------------------------
KINDS = ("quad", "cubic", "quartic")
LAST_TIMES = {"quad": hip.quad_last_times, "cubic": hip.cubic_last_times, "quartic": hip.quartic_last_times}


def _in_order(*steps):
    """run the callables one after the other, each in a thread of its own that starts when the one before has finished (events, no
    sleeps); returns their results, re-raising the first exception"""
    events = [threading.Event() for _ in range(len(steps) + 1)]
    results = [None] * len(steps)

    def run(k):
        events[k].wait(timeout=120)
        try:
            results[k] = ("ok", steps[k]())
        except BaseException as e:      # noqa: BLE001
            results[k] = ("error", e)
        finally:
            events[k + 1].set()
    pool = [threading.Thread(target=run, args=(k,)) for k in range(len(steps))]
    for th in pool:
        th.start()
    events[0].set()
    for th in pool:
        th.join()
    for how, value in results:
        if how == "error":
            raise value
    return [value for _, value in results]


def test_search_records_belong_to_their_thread():
    """Thread A searches with all three degrees and keeps its three records; thread B then runs other searches and a call that fails
    with GF2BV_ERR_ARG; A reads its records again: unchanged.  A thread that never searched reads zeros."""
    cases = {kind: J.forms_case(kind, 13, 50) for kind in KINDS}
    others = {kind: J.forms_case(kind, 18, 51) for kind in KINDS}
    a_go_on, b_done, kept = threading.Event(), threading.Event(), {}

    def thread_a():
        for kind in KINDS:
            forms, zeros = cases[kind]
            assert J.FORMS[kind][1](forms, 13) == (len(zeros), zeros)
            kept[kind] = LAST_TIMES[kind]()
            assert kept[kind]["candidates"] >= len(zeros) > 0, (kind, kept[kind])      # (the record did register this thread's search)
        a_go_on.set()
        assert b_done.wait(timeout=120)
        return {kind: LAST_TIMES[kind]() for kind in KINDS}

    def thread_b():
        assert a_go_on.wait(timeout=120)
        try:
            for kind in KINDS:
                forms, zeros = others[kind]
                assert J.FORMS[kind][1](forms, 18) == (len(zeros), zeros)
                assert LAST_TIMES[kind]()["candidates"] >= len(zeros)
            with pytest.raises(ValueError, match=r"^r_eff must be 0\.\.40$"):
                hip.quartic_forms_search([1], 41)
        finally:
            b_done.set()
        return True

    ta_result = [None]
    ta = threading.Thread(target=lambda: ta_result.__setitem__(0, _capture(thread_a)))
    tb_result = [None]
    tb = threading.Thread(target=lambda: tb_result.__setitem__(0, _capture(thread_b)))
    ta.start()
    tb.start()
    ta.join()
    tb.join()
    assert tb_result[0] == ("ok", True), tb_result[0]
    assert ta_result[0] == ("ok", kept), (ta_result[0], kept)
    never = _in_order(lambda: {kind: LAST_TIMES[kind]() for kind in KINDS})[0]
    assert all(v == 0 for rec in never.values() for v in rec.values()), never


def _capture(fn):
    try:
        return "ok", fn()
    except BaseException as e:      # noqa: BLE001
        return "error", f"{type(e).__name__}: {e}"


def test_error_messages_belong_to_their_thread():
    """Four threads each provoke a different argument error (all returned before any device is touched), one after the other; only
    when all four have failed does each read gf2bv_last_error(): its own message, not the latest one."""
    L = hip.lib()
    aug = np.zeros((100, 2), dtype=np.uint64)
    hs = (ctypes.c_void_p * 4)()
    cnt = ctypes.c_int64()
    out = np.zeros(4, dtype=np.uint64)
    form = np.ones(1, dtype=np.uint64)
    calls = [
        ("r_eff must be 0..40", lambda: L.gf2bv_quartic_forms_search(form.ctypes.data, 1, 41, 0, 4, ctypes.byref(cnt), out.ctypes.data)),
        ("stride_words does not cover cols+1 bits", lambda: L.gf2bv_solve_words(aug.ctypes.data, 100, 100, 1, 0, 0, hs)),
        ("Invalid mode", lambda: L.gf2bv_solve_words(aug.ctypes.data, 100, 100, 2, 7, 0, hs)),
        ("null pointer", lambda: L.gf2bv_solve_rhs_words(aug.ctypes.data, 100, 100, 2, None, 1, 2, 0, 0, hs)),
    ]
    n = len(calls)
    turn = [threading.Event() for _ in range(n + 1)]
    seen = [None] * n

    def run(k):
        try:
            assert turn[k].wait(timeout=60)
            rc = calls[k][1]()
        except BaseException as e:      # noqa: BLE001
            seen[k] = f"{type(e).__name__}: {e}"
            turn[k + 1].set()
            return
        turn[k + 1].set()
        turn[n].wait(timeout=60)                                              # every thread has failed by now
        seen[k] = (rc, L.gf2bv_last_error().decode())
    pool = [threading.Thread(target=run, args=(k,)) for k in range(n)]
    for th in pool:
        th.start()
    turn[0].set()
    for th in pool:
        th.join()
    assert seen == [(1, msg) for msg, _ in calls]
    assert _in_order(lambda: L.gf2bv_last_error().decode()) == [""]         # a thread that never failed


# -- f. first use from many threads, in a fresh process --------------------------------------------------------------------------------------
def test_first_use_from_many_threads():
    """tests/threads_child.py: 8 threads whose FIRST calls into the library are 8 different entries, so that the library handle of
    the binding, the pool, the stream-pair probe, the concurrency cache and every raised-once attribute are first reached together"""
    res = run_child([sys.executable, os.path.join(ROOT, "tests", "threads_child.py")], 120)
    assert res.ok, res.report()
    line = [ln for ln in res.out.splitlines() if ln.startswith("{")][-1]
    report = json.loads(line)
    assert report["threads"] == 8 and report["calls"] >= 16, report
    assert report["mismatches"] == [], report
