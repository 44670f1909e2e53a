"""Times of the quadratic search (QuadraticSystem.search_all -> gf2bv_quad_search) on one GPU; profiles/quad_search_time.txt.

    python tools/quad_search_time.py

* the nlfsr cases of tests/test_gpu_quad_search.py: AffineSpace.quad_search and the whole QuadraticSystem.search_one call
  (wall time), with the phase times of the library (reduction, forms build, affine elimination, device search, relinearised
  solves);
* the device search alone (gf2bv_quad_forms_search) over 2^28 and 2^32 points, as points per second;
* search_all against solve_all at d = 12 and 16 with n = 128 linear unknowns."""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process, as in the tests)

from gf2bv_amd import QuadraticSystem, hip  # noqa: E402
from tests.harness_models import FibonacciLFSR, GaloisLFSR  # noqa: E402
from tests.test_gpu_quad_search import _form, _nlfsr, _vanish_at  # noqa: E402


def nlfsr():
    for kind, seed, count in ((GaloisLFSR, 1, 16384), (GaloisLFSR, 1, 16500), (FibonacciLFSR, 2, 16320)):
        q, zeros, want = _nlfsr(kind, seed, count)
        space = q.solve_raw_space(zeros)
        space.quad_search(q._lin_size)                           # warm
        t0 = time.perf_counter()
        got = space.quad_search(q._lin_size)
        t = (time.perf_counter() - t0) * 1e3
        assert [q.convert_sol(g) for g in got] == [want]
        ph = hip.quad_last_times()
        t0 = time.perf_counter()
        assert q.search_one(zeros) == want                      # the whole call: linearised solve, search, conversion
        t_one = (time.perf_counter() - t0) * 1e3
        print(f"nlfsr {kind.__name__:13s} outputs {count}: d {space.dimension:3d}  quad_search {t:7.2f} ms  search_one {t_one:7.2f} ms  "
              + "  ".join(f"{k} {v:.2f}" for k, v in ph.items()), flush=True)


def direct(re: int, reps: int = 3):
    rng = random.Random(re)
    point = rng.getrandbits(re)
    forms = [_vanish_at(_form(rng, re, 0.3), point, re) for _ in range(64)]
    hip.quad_forms_search(forms, re)
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        count, got = hip.quad_forms_search(forms, re)
        best = min(best, time.perf_counter() - t0)
    assert point in got
    print(f"direct search r_eff {re}: {best * 1e3:9.2f} ms (best of {reps}) = {2 ** re / best:.3e} points/s, {count} zeros", flush=True)


def versus_walk(d: int):
    rng = random.Random(d)
    n = 128
    q = QuadraticSystem([n])
    secret = rng.getrandbits(n)
    raw = secret
    for i in range(1, n):
        if (secret >> i) & 1:
            raw |= (secret & ((1 << i) - 1)) << (n + i * (i - 1) // 2)
    # a space of dimension d through the secret's point, from host integers
    from gf2bv_amd._internal import _space_from_ints
    basis = tuple(rng.getrandbits(q._cols) for _ in range(d))
    space = _space_from_ints(q._cols, raw, basis)
    t0 = time.perf_counter()
    walk = [q.convert_sol(s) for s in space]
    walk = [s for s in walk if s is not None]
    t_walk = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = [q.convert_sol(s) for s in space.quad_search(n)]
    t_search = time.perf_counter() - t0
    assert got == walk
    print(f"n 128, d {d}: host walk (solve_all's loop) {t_walk * 1e3:9.2f} ms, quad_search {t_search * 1e3:8.2f} ms, "
          f"{len(got)} points", flush=True)


if __name__ == "__main__":
    nlfsr()
    for re in (28, 32):
        direct(re)
    for d in (12, 16):
        versus_walk(d)
