"""tests/threads.run_concurrently reports contamination between concurrent callers (no GPU, no library call).

The jobs stand for an entry that keeps state where two calls can meet: each writes (its id, its thread) into a cell, waits at a
barrier until every thread has written, reads the cell back and waits again before anyone writes the next one.  With ONE cell for
all threads exactly one thread per step reads its own value back -- the last writer -- and the harness must report every other one,
each step of each round; with a cell per thread it must report nothing."""
import threading

import numpy as np

from tests import threads as T

THREADS, JOBS, ROUNDS = 4, 3, 2


def _jobs(cell_of, barrier):
    def make(job_id):
        def call():
            cell = cell_of()
            mine = (job_id, threading.get_ident())
            cell["value"] = mine
            barrier.wait(timeout=30)         # every thread has written
            seen = cell["value"]
            barrier.wait(timeout=30)         # every thread has read: the next step may write
            return job_id, seen == mine
        return f"job{job_id}", call, (job_id, True)
    return [make(k) for k in range(JOBS)]


def test_shared_cell_is_reported_for_all_but_one_thread():
    shared = {}
    failures = T.run_concurrently(_jobs(lambda: shared, threading.Barrier(THREADS)), THREADS, ROUNDS, seed=1)
    assert len(failures) == (THREADS - 1) * JOBS * ROUNDS, failures
    per_thread_round = {}
    for t, r, name, detail in failures:
        assert name.startswith("job") and "want" in detail and "False" in detail, (t, r, name, detail)
        per_thread_round[t, r] = per_thread_round.get((t, r), 0) + 1
    assert set(t for t, _ in per_thread_round) <= set(range(THREADS)) and set(r for _, r in per_thread_round) == set(range(ROUNDS))
    # step by step the threads meet in lock-step: every step has exactly one winner, so the failures of a round add up
    for r in range(ROUNDS):
        assert sum(n for (t, rr), n in per_thread_round.items() if rr == r) == (THREADS - 1) * JOBS


def test_cell_per_thread_is_clean():
    local = threading.local()

    def cell_of():
        if not hasattr(local, "cell"):
            local.cell = {}
        return local.cell
    assert T.run_concurrently(_jobs(cell_of, threading.Barrier(THREADS)), THREADS, ROUNDS, seed=1) == []


def test_exceptions_are_recorded_and_a_device_error_stops_its_thread_only():
    calls = []

    def bad_argument():
        calls.append("arg")
        raise ValueError("r_eff must be 0..40")

    def device_error():
        calls.append("hip")
        raise RuntimeError("gf2bv_hip error 3: hipMemcpy: an illegal memory access was encountered")
    failures = T.run_concurrently([("arg", bad_argument, None)], 2, 3, seed=5)
    assert len(failures) == 6 and all(d == "ValueError: r_eff must be 0..40" for _, _, _, d in failures)
    calls.clear()
    failures = T.run_concurrently([("hip", device_error, None)], 2, 3, seed=5)
    assert [(t, r) for t, r, _, _ in failures] == [(0, 0), (1, 0)] and calls == ["hip", "hip"]      # one call a thread, then it stops
    assert T.is_device_error(RuntimeError("gf2bv_amd: HIP solve failed (3): hipStreamSynchronize"))
    assert not T.is_device_error(RuntimeError("gf2bv_hip error 4: more common zeros than can be collected"))


def test_equality_is_exact():
    a = np.arange(6, dtype=np.uint64).reshape(2, 3)
    assert T.same({"x": [a, (1, 2)]}, {"x": (a.copy(), [1, 2])})
    assert not T.same(a, a.astype(np.int64)) and not T.same(a, a.reshape(3, 2)) and not T.same([a], [a + np.uint64(1)])
    w = {"status": 0, "rank": 2, "pivcols": np.array([0, 2]), "origin": np.array([5], dtype=np.uint64), "dim": 1,
         "basis": np.array([[2]], dtype=np.uint64)}
    assert T.oracle_key(w, 1) == (0, 2, (0, 2), (5,), 1, ((2,),)) and T.oracle_key(w, 0) == (0, 2, (0, 2), (5,))
    assert T.oracle_key(dict(w, status=1), 1) == (1, 2, (0, 2))
