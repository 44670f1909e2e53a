"""First use of the library from many threads at once, in a process of its own (started by tests/test_gpu_threads.py through
tests/child.run_child; nothing else uses the GPU meanwhile).

The inputs and their references -- all from outside the library: the CPU oracle, the set-of-monomials expansion, zero sets known by
construction -- are built first; building them makes no call into libgf2bv_hip.so.  Then 8 threads are released at a barrier and the
FIRST call of each is a different entry: a blocked solve, a one-launch solve, a kept factorization, the quartic, cubic and quadratic
forms searches (the quartic one raises the LDS attribute above 64 KiB), a degree-4 XL expansion, a gang batch.  So the binding's
library handle, the pool singleton, the stream-pair probe, the concurrency cache and each raised-once attribute map are first
reached concurrently.  Each thread then runs every other entry once, starting from its own.  Prints one JSON line:
{"threads": 8, "calls": n, "mismatches": [[thread, step, name, detail], ...]}."""
import json
import os
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import random  # noqa: E402

import gf2bv_amd  # noqa: E402,F401
from gf2bv_amd import hip  # noqa: E402
from oracle import gf2_oracle as O  # noqa: E402
from tests import thread_jobs as J  # noqa: E402
from tests import threads as T  # noqa: E402
from tests.systems import random_system  # noqa: E402


def factor_job():
    """factor_words on 300 x 200 of rank 40, 9 right-hand sides, closed again: against the oracle per right-hand side"""
    rows, cols = 300, 200
    rng = random.Random(17000)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, 40, True, 0), cols)
    bits = J.make_rhs(rng, aug, rows, cols, 9)
    rhs = J.rhs_words(bits)

    def call():
        with hip.factor_words(aug, rows, cols, 1) as f:
            return J.solve_many(f.solve(rhs), 1)
    return "factor_words + Factor.solve", call, J.oracle_rhs(aug, rows, cols, bits, 1)


def main() -> int:
    assert hip._lib is None, "the library was loaded while the inputs were built"
    jobs = [
        J.solve_jobs([30], 2600, 2500, 2300)[0],
        J.solve_jobs([31], 66, 65, None)[0],
        factor_job(),
        J.forms_jobs("quartic", [31])[0],
        J.forms_jobs("cubic", [31])[0],
        J.forms_jobs("quad", [31])[0],
        J.xl4_expand_jobs([32])[0],
        J.batch_jobs([33])[0],
    ]
    assert hip._lib is None, "the library was loaded while the inputs were built"
    n = len(jobs)
    wants = [T.canon(w) for _, _, w in jobs]
    mismatches, lock, barrier, calls = [], threading.Lock(), threading.Barrier(n), [0]

    def worker(t: int):
        barrier.wait(timeout=60)
        for step in range(n):
            name, call, _ = jobs[(t + step) % n]          # step 0: thread t's own entry, the first call of this thread
            try:
                got = T.canon(call())
            except BaseException as e:      # noqa: BLE001
                with lock:
                    mismatches.append([t, step, name, f"{type(e).__name__}: {e}"])
                if T.is_device_error(e):
                    return
                continue
            with lock:
                calls[0] += 1
                if got != wants[(t + step) % n]:
                    mismatches.append([t, step, name, "the result differs from its reference"])

    pool = [threading.Thread(target=worker, args=(t,)) for t in range(n)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    print(json.dumps({"threads": n, "calls": calls[0], "mismatches": sorted(mismatches)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
