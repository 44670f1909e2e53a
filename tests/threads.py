"""Concurrent callers for the suite (a helper module, imported by the tests that need it).

    run_concurrently(jobs, threads, rounds, seed) -> [(thread, round, name, detail), ...]

`jobs` is a list of (name, callable, want).  `threads` Python threads are released together by a barrier; each runs its own seeded
shuffle of ALL jobs, `rounds` times over, and compares every result with `want` by exact equality (`same`).  A mismatch or an
exception is recorded, never raised inside a thread; a thread stops its own loop at the first device error (GF2BV_ERR_HIP: the
device is in an unknown state, nothing more is launched on it), the others run on to their own first one.  The caller asserts once
that the returned list is empty, so a failure shows every mismatch.

Results are compared through `canon`, which turns numpy arrays, sequences and dicts into plain hashable values; `solution_key` and
`oracle_key` bring a hip.Solution and the CPU oracle's dict of the same solve to one such value (status, rank, pivots, then -- for a
solved system -- origin and, in mode 1, dimension and basis: what assert_same_solution of tests/test_gpu_rhs.py compares)."""
from __future__ import annotations

import random
import re
import threading

import numpy as np

MAX_THREADS = 8                          # a GPU command of the suite has 16 CPUs
ERR_HIP = 3                              # GF2BV_ERR_HIP of include/gf2bv_hip.h
_DEVICE_ERROR = re.compile(rf"gf2bv_hip error {ERR_HIP}:|failed \({ERR_HIP}\):")      # hip.HipError / _internal's RuntimeError


def canon(x):
    """x as a value that == compares exactly: arrays with shape and dtype, sequences as tuples, dicts as sorted items"""
    if isinstance(x, np.ndarray):
        return ("ndarray", x.shape, x.dtype.str, x.tobytes())
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    if isinstance(x, dict):
        return tuple(sorted((k, canon(v)) for k, v in x.items()))
    return x


def same(got, want) -> bool:
    return canon(got) == canon(want)


def _key(status, rank, pivots, origin, dimension, basis, mode: int) -> tuple:
    key = (int(status), int(rank), tuple(int(p) for p in pivots))
    if status == 0:
        key += (tuple(int(w) for w in origin),)
        if mode == 1:
            key += (int(dimension), tuple(tuple(int(w) for w in row) for row in basis))
    return key


def solution_key(s, mode: int) -> tuple:
    """a hip.Solution as a comparable value"""
    return _key(s.status, s.rank, s.pivots, s.origin, s.dimension, s.basis, mode)


def oracle_key(w: dict, mode: int) -> tuple:
    """the dict of oracle.gf2_oracle.solve_words as the same value"""
    return _key(w["status"], w["rank"], w["pivcols"], w.get("origin", ()), w.get("dim", 0), w.get("basis", ()), mode)


def space_key(sp):
    """what m4ri_solve returns (None, an int, or an AffineSpace of either the extension or the oracle) as a comparable value"""
    if sp is None or isinstance(sp, int):
        return sp
    return (sp.dimension, sp.origin, tuple(sp.basis))


def is_device_error(e: BaseException) -> bool:
    return isinstance(e, RuntimeError) and bool(_DEVICE_ERROR.search(str(e)))


def _brief(v, limit: int = 300) -> str:
    s = repr(v)
    return s if len(s) <= limit else s[:limit] + f"... ({len(s)} characters)"


def run_concurrently(jobs, threads: int, rounds: int, seed: int) -> list:
    assert 1 <= threads <= MAX_THREADS and rounds >= 1 and jobs
    jobs = list(jobs)
    wants = [canon(want) for _, _, want in jobs]
    failures, lock = [], threading.Lock()
    barrier = threading.Barrier(threads)

    def record(t, r, name, detail):
        with lock:
            failures.append((t, r, name, detail))

    def worker(t: int):
        rng = random.Random(seed * 1000003 + t)
        try:
            barrier.wait()
        except threading.BrokenBarrierError:
            record(t, -1, "<barrier>", "the start barrier broke")
            return
        for r in range(rounds):
            order = list(range(len(jobs)))
            rng.shuffle(order)
            for k in order:
                name, call, _ = jobs[k]
                try:
                    got = canon(call())
                except BaseException as e:      # noqa: BLE001  (recorded, never raised inside a thread)
                    record(t, r, name, f"{type(e).__name__}: {e}")
                    if is_device_error(e):
                        return
                    continue
                if got != wants[k]:
                    record(t, r, name, f"got {_brief(got)}, want {_brief(wants[k])}")

    pool = [threading.Thread(target=worker, args=(t,), name=f"caller-{t}") for t in range(threads)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    return sorted(failures)
