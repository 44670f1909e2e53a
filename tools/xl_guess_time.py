"""Times of hybrid XL (guess f unknowns, solve all 2^f degree-3 XL systems as one batch) on one GPU; profiles/xl_guess_time.txt.

    python tools/xl_guess_time.py [--out FILE]

Random dense quadratic systems with one planted point at (n, f) = (40, 8) and (56, 8), m = ceil(1.15 cols3(n') / (n' + 1)) equations
for n' = n - f, so that every one of the 256 assignments' expansions has 15 % more rows than its cols3(n') columns:
* k_quad_specialise and k_xl3_expand_batch alone on resident rows, all 256 assignments: device time (events around the launch, median
  of 7 after a warm launch), stored GB/s, and that against the read-XOR-write and read-only streaming rates
  gf2bv_stream_ceiling_device measures in the same run;
* solve_xl3_guess_words over all 256 assignments end to end (upload, both kernels, the gang solve) against a loop of 256
  solve_xl3_words on the same specialised rows (specialised beforehand, outside the timed window): both alternate in the same
  process, warm; medians of 5 and the spread;
* whether both give the same ranks and origins, how many assignments are consistent, and whether the planted point came back from
  the assignment that holds its guessed bits.
The lines are printed and written to FILE (default profiles/xl_guess_time.txt)."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process, as in the tests)

from gf2bv_amd import hip  # noqa: E402

CASES = ((40, 8), (56, 8))


def planted_rows(n: int, m: int, seed: int):
    """(planted point, m random dense quadratic rows as augmented words that vanish there)"""
    rng = np.random.default_rng(seed)
    cols2 = hip.quad_cols(n)
    w2 = (cols2 + 1 + 63) // 64
    x = int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1) | 1
    point = x
    for i in range(1, n):
        if (x >> i) & 1:
            point |= (x & ((1 << i) - 1)) << (n + i * (i - 1) // 2)
    quad = np.zeros((m, w2), dtype=np.uint64)
    for r in range(m):
        a = int.from_bytes(rng.bytes((cols2 + 7) // 8), "little") & ((1 << cols2) - 1)
        c = bin(a & point).count("1") & 1
        quad[r] = np.frombuffer(int(a | (c << cols2)).to_bytes(8 * w2, "little"), dtype=np.uint64)
    return x, quad


def event_median_us(launch, reps: int = 7) -> float:
    launch()                                           # warm
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e3


def main(out_path: str):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"tools/xl_guess_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    say(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s")
    for n, f in CASES:
        ns, na = n - f, 1 << f
        cols3 = hip.xl3_cols(ns)
        m = math.ceil(1.15 * cols3 / (ns + 1))
        rows = max(m * (ns + 1), cols3)
        guess = tuple(range(2, n, n // f))[:f]
        x, quad = planted_rows(n, m, n)
        right = sum(((x >> g) & 1) << t for t, g in enumerate(guess))
        rest = [u for u in range(n) if u not in guess]
        y = sum(((x >> u) & 1) << k for k, u in enumerate(rest))
        ss = (hip.quad_cols(ns) + 1 + 63) // 64
        ss += ss & 1
        xs = (cols3 + 1 + 63) // 64
        xs += xs & 1
        say(f"n {n}, {f} guessed {guess}: {m} equations, {na} systems of {rows} rows x {cols3} columns over n' = {ns} "
            f"(chunk by gf2bv_xl3_guess_chunk_device: {hip.xl3_guess_chunk(m, n, f)})")
        # -- the two kernels alone, all assignments resident
        d_quad, d_spec, d_xl = hip.DeviceBuffer(quad.nbytes), hip.DeviceBuffer(na * m * ss * 8), hip.DeviceBuffer(na * rows * xs * 8)
        d_quad.upload(quad)
        t_spec = event_median_us(lambda: hip.quad_specialise_device(d_quad.ptr, m, quad.shape[1], n, guess, 0, na, d_spec.ptr, ss, m * ss))
        t_xl = event_median_us(lambda: hip.xl3_expand_batch_device(d_spec.ptr, na, m * ss, m, ss, ns, rows, d_xl.ptr, xs, rows * xs))
        for name, t, nbytes in (("k_quad_specialise ", t_spec, na * m * ss * 8), ("k_xl3_expand_batch", t_xl, na * rows * xs * 8)):
            gbs = nbytes / t / 1e3
            say(f"      {name} {t:10.1f} us for {nbytes / 2 ** 20:9.1f} MiB out: {gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.3f} of the "
                f"read-XOR-write rate, {gbs / ceil['read_gbs']:.3f} of the read-only rate")
        for buf in (d_quad, d_spec, d_xl):
            buf.free()
        # -- end to end: the batch against a loop of single solves on the same specialised rows
        spec = hip.quad_specialise_words(quad, n, guess)                  # outside the timed window
        res = [None, None]

        def batch():
            res[0] = hip.solve_xl3_guess_words(quad, n, guess, mode=0)

        def loop():
            res[1] = [hip.solve_xl3_words(spec[s], ns, 0) for s in range(na)]
        batch()
        loop()                                         # warm, both
        tb, tl = [], []
        for _ in range(5):                             # alternating
            for call, out in ((batch, tb), (loop, tl)):
                t0 = time.perf_counter()
                call()
                out.append((time.perf_counter() - t0) * 1e3)
        same = all(a.status == b.status and a.rank == b.rank and np.array_equal(a.origin, b.origin) for a, b in zip(*res))
        solved = [s for s in range(na) if res[0][s].status == 0]
        hit = res[0][right]
        found = hit.status == 0 and hit.rank == cols3 and hit.origin_int() & ((1 << ns) - 1) == y
        mb, ml = statistics.median(tb), statistics.median(tl)
        say(f"      solve_xl3_guess_words, {na} assignments: median {mb:9.1f} ms (min {min(tb):.1f}, max {max(tb):.1f}) = {mb / na:.3f} ms per system")
        say(f"      loop of {na} solve_xl3_words:            median {ml:9.1f} ms (min {min(tl):.1f}, max {max(tl):.1f}) = {ml / na:.3f} ms per system")
        say(f"      loop / batch: {ml / mb:.2f}; both give the same status, rank and origin for every assignment: {same}")
        say(f"      consistent assignments: {solved} (the planted point's is {right}); rank {hit.rank} of {cols3} there, the planted point came back: {found}")
    say("not measured: other n and f, mode 1 (bases), the factored entry (solve_xl3_guess_quad_terms), several chunks, more than one GPU.")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "xl_guess_time.txt")
    main(out)
