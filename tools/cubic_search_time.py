"""Times of the cubic search (search_all_cubic / search_all_xl -> gf2bv_cubic_search) on one GPU; profiles/cubic_search_time.txt.

    python tools/cubic_search_time.py [out.txt]

One process, everything warm, medians of 5 with their ranges:
* the device search alone over 2^28, 2^32 and 2^36 points with 64 dense forms: k_cubic_search (gf2bv_cubic_forms_search) beside
  k_quad_search (gf2bv_quad_forms_search) on 64 dense quadratic forms at the same R, and their ratio; R = 40 once;
* the library-time breakdown (gf2bv_cubic_last_times) of examples/nlfsr_recovery_cubic_search.py and of one degree-3 XL case;
* list(solve_all(..., max_dimension=16)) against search_all_cubic on the same space at d = 12 and d = 16."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402,F401  (one HIP runtime per process, as in the tests)

from gf2bv_amd import PackedCubicSystem, QuadraticSystem, hip, search_all_cubic, search_all_xl  # noqa: E402
from tests import cubic_forms as CF  # noqa: E402
from tests import quad_forms as QF  # noqa: E402
from tests.cubic_terms import REGISTER_12, register_zeros  # noqa: E402

LINES = []


def say(text: str):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps: int = 5) -> tuple:
    """(median, min, max) in seconds of `reps` calls after one warm call, and the last result"""
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def rate(R: int):
    rng = random.Random(R)
    point = rng.getrandbits(R)
    cubic = CF.planted_dense(rng, R, 64, [point])
    quad = QF.planted_dense(rng, R, 64, [point])
    tc, c0, c1, (count, got) = timed(lambda: hip.cubic_forms_search(cubic, R))
    assert point in got
    tq, q0, q1, (count, got) = timed(lambda: hip.quad_forms_search(quad, R))
    assert point in got
    say(f"R {R}: k_cubic_search {tc * 1e3:9.2f} ms [{c0 * 1e3:.2f} .. {c1 * 1e3:.2f}] = {2 ** R / tc:.3e} points/s | "
        f"k_quad_search {tq * 1e3:9.2f} ms [{q0 * 1e3:.2f} .. {q1 * 1e3:.2f}] = {2 ** R / tq:.3e} points/s | ratio {tc / tq:.1f}")


def rate_once(R: int):
    rng = random.Random(R)
    point = rng.getrandbits(R)
    cubic = CF.planted_dense(rng, R, 64, [point])
    t0 = time.perf_counter()
    count, got = hip.cubic_forms_search(cubic, R)
    t = time.perf_counter() - t0
    assert point in got
    say(f"R {R}: k_cubic_search {t * 1e3:9.2f} ms (one run) = {2 ** R / t:.3e} points/s")


def phases() -> str:
    return "  ".join(f"{k} {v:.2f}" for k, v in hip.cubic_last_times().items())


def end_to_end():
    import nlfsr_recovery_cubic_search as ex
    secret = random.Random(1).getrandbits(ex.N_BITS)
    count = ex.smallest_count(secret)
    c = PackedCubicSystem([ex.N_BITS])
    zeros = register_zeros(c, secret, ex.TAPS, ex.SELECT, count)
    space = c.solve_raw_space(zeros)
    t, t0, t1, raws = timed(lambda: space.cubic_search(ex.N_BITS))
    assert [c.convert_sol(r) for r in raws] == [(secret,)]
    say(f"example n 16, {count} outputs, d {space.dimension}: cubic_search {t * 1e3:.2f} ms [{t0 * 1e3:.2f} .. {t1 * 1e3:.2f}]  {phases()}")
    t, t0, t1, sols = timed(lambda: search_all_cubic(c, zeros))
    say(f"  the whole search_all_cubic (linearised solve, search, conversion): {t * 1e3:.2f} ms [{t0 * 1e3:.2f} .. {t1 * 1e3:.2f}]")
    from tests.test_gpu_cubic_search import LFSR, XL_OUTPUTS
    from tests.test_gpu_xl import lfsr_zeros
    q = QuadraticSystem([LFSR[0]])
    zq = lfsr_zeros(q, *LFSR, 40)
    space = q.solve_raw_space_xl(zq)
    t, t0, t1, raws = timed(lambda: space.cubic_search(LFSR[0]))
    assert len(raws) == XL_OUTPUTS[40][2]
    say(f"degree-3 XL n 12, 40 outputs ({len(zq)} equations), d {space.dimension}: cubic_search {t * 1e3:.2f} ms "
        f"[{t0 * 1e3:.2f} .. {t1 * 1e3:.2f}], {len(raws)} points  {phases()}")
    t, t0, t1, sols = timed(lambda: search_all_xl(q, zq))
    say(f"  the whole search_all_xl: {t * 1e3:.2f} ms [{t0 * 1e3:.2f} .. {t1 * 1e3:.2f}]")


def versus_walk(count: int):
    c = PackedCubicSystem([12])
    zeros = register_zeros(c, 0x52F, REGISTER_12["taps"], REGISTER_12["pos"], count)
    d = c.solve_raw_space(zeros).dimension
    tw, w0, w1, walk = timed(lambda: list(c.solve_all(zeros, max_dimension=16)))
    ts, s0, s1, got = timed(lambda: search_all_cubic(c, zeros))
    assert got == walk
    say(f"n 12, d {d}: list(solve_all) {tw * 1e3:9.2f} ms [{w0 * 1e3:.2f} .. {w1 * 1e3:.2f}], search_all_cubic {ts * 1e3:8.2f} ms "
        f"[{s0 * 1e3:.2f} .. {s1 * 1e3:.2f}], {len(got)} points (both with the linearised solve)")


if __name__ == "__main__":
    say(f"tools/cubic_search_time.py on one MI355X (build {hip.build_id()}).  Medians of 5 warm runs in one process [min .. max].")
    say("Phase times are gf2bv_cubic_last_times() in ms: reduction, forms build (k_forms_products<3> + k_forms_sum, every round), affine")
    say("elimination, device search (k_cubic_search + k_forms_check<3>), total library time; levels = rounds of the affine elimination.")
    for R in (28, 32, 36):
        rate(R)
    rate_once(40)
    end_to_end()
    for count in (286, 282):
        versus_walk(count)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")
