"""Times of degree-4 XL on one GPU; profiles/xl4_expand_time.txt.

    python tools/xl4_expand_time.py [--out FILE]

Random dense quadratic systems with one planted point at n = 24, 32, 40, with the smallest m for which the rank the rows can reach,
m R4 - m - C(m,2) (R4 = 1 + n + C(n,2) rows an equation; f_i f_i = f_i and f_i f_j = f_j f_i are the relations), is at least
1.15 cols4 for cols4 = n + C(n,2) + C(n,3) + C(n,4) columns:
* k_xl4_expand alone on resident quadratic rows: device time (events around the launch, median of 7 after a warm launch), stored
  GB/s, and that against the read-XOR-write and read-only streaming rates gf2bv_stream_ceiling_device measures in the same run;
* solve_device on the resident expansion against solve_xl4_quad_terms end to end (upload of the factored rows, both expansions,
  solve): medians of 5 warm repetitions, same process; the expansion's share of the solve it feeds;
* whether the answer is the planted point (full rank, and the origin's linear part).
Hybrid, (n, f) = (40, 8): the same rule for m over n' = 32 unknowns; k_xl4_expand_batch alone on a chunk of resident specialised rows,
then solve_xl4_guess_words over all 256 assignments, a chunk of gf2bv_xl4_guess_chunk_device assignments a call, against a loop of 256
solve_xl4_words on the same specialised rows (specialised beforehand): both alternate in the same process, warm; medians of 5 and
the spread.
The lines are printed and written to FILE (default profiles/xl4_expand_time.txt)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process, as in the tests)
from xl_expand_time import median_ms, planted_system  # noqa: E402
from xl_guess_time import event_median_us  # noqa: E402

from gf2bv_amd import hip  # noqa: E402

SIZES = (24, 32, 40)
HYBRID = (40, 8)


def equations_for(n: int) -> int:
    """the smallest m with m R4 - m - C(m,2) >= 1.15 cols4"""
    per, need = 1 + hip.quad_cols(n), 1.15 * hip.xl4_cols(n)
    m = 1
    while m * per - m - m * (m - 1) // 2 < need:
        m += 1
    return m


def main(out_path: str):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"tools/xl4_expand_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    say(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s")
    for n in SIZES:
        cols4, per = hip.xl4_cols(n), 1 + hip.quad_cols(n)
        m = equations_for(n)
        rows, stride = max(m * per, cols4), hip.padded_stride(cols4)
        x, quad, terms = planted_system(n, m, n)
        d_quad, aug = hip.DeviceBuffer(quad.nbytes), hip.DeviceBuffer(rows * stride * 8)
        d_quad.upload(quad)
        t = event_median_us(lambda: hip.xl4_expand_device(d_quad.ptr, m, quad.shape[1], n, rows, aug.ptr, stride)) / 1e3      # ms
        gbs = rows * stride * 8 / t / 1e6
        say(f"n {n:2d}: {m} equations x {per} -> {rows} rows x {cols4} columns ({rows * stride * 8 / 2 ** 20:7.1f} MiB out): k_xl4_expand {t * 1e3:9.1f} us  "
            f"{gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.2f} of the read-XOR-write rate, {gbs / ceil['read_gbs']:.2f} of the read-only rate")
        res = [None, None]

        def resident():
            res[0] = hip.solve_device(aug.ptr, rows, cols4, stride, 0)

        def whole():
            res[1] = hip.solve_xl4_quad_terms(*terms, n, 0)
        s, w = median_ms(resident, 5), median_ms(whole, 5)
        same = res[0].rank == res[1].rank and np.array_equal(res[0].origin, res[1].origin)
        found = res[1].status == 0 and res[1].rank == cols4 and res[1].origin_int() & ((1 << n) - 1) == x
        say(f"      solve_device (resident expansion) {s:9.2f} ms, solve_xl4_quad_terms (upload + both expansions + solve) {w:9.2f} ms, "
            f"rank {res[1].rank} of {cols4}, both answers equal: {same}, the planted point: {found}")
        say(f"      expansion / solve it feeds: {t / s:.3f}")
        d_quad.free()
        aug.free()

    n, f = HYBRID
    ns, na = n - f, 1 << f
    cols4, per = hip.xl4_cols(ns), 1 + hip.quad_cols(ns)
    m = equations_for(ns)
    rows = max(m * per, cols4)
    guess = tuple(range(2, n, n // f))[:f]
    x, quad, _ = planted_system(n, m, 4000 + n)
    right = sum(((x >> g) & 1) << t for t, g in enumerate(guess))
    rest = [u for u in range(n) if u not in guess]
    y = sum(((x >> u) & 1) << k for k, u in enumerate(rest))
    chunk = hip.xl4_guess_chunk(m, n, f)
    say(f"hybrid n {n}, {f} guessed {guess}: {m} equations, {na} systems of {rows} rows x {cols4} columns over n' = {ns} "
        f"(chunk by gf2bv_xl4_guess_chunk_device: {chunk})")
    spec = hip.quad_specialise_words(quad, n, guess)                      # outside the timed windows
    ss, xs = spec.shape[2], hip.padded_stride(cols4)
    nb = min(chunk, 32)                                                   # the batched kernel alone: 32 systems resident
    d_spec, d_xl = hip.DeviceBuffer(spec[:nb].nbytes), hip.DeviceBuffer(nb * rows * xs * 8)
    d_spec.upload(np.ascontiguousarray(spec[:nb]))
    t_xl = event_median_us(lambda: hip.xl4_expand_batch_device(d_spec.ptr, nb, m * ss, m, ss, ns, rows, d_xl.ptr, xs, rows * xs))
    gbs = nb * rows * xs * 8 / t_xl / 1e3
    say(f"      k_xl4_expand_batch, {nb} systems: {t_xl:10.1f} us for {nb * rows * xs * 8 / 2 ** 20:9.1f} MiB out: {gbs:6.0f} GB/s stored = "
        f"{gbs / ceil['rmw_gbs']:.3f} of the read-XOR-write rate, {gbs / ceil['read_gbs']:.3f} of the read-only rate")
    d_spec.free()
    d_xl.free()
    res = [None, None]

    def batch():
        res[0] = [r for a0 in range(0, na, chunk) for r in hip.solve_xl4_guess_words(quad, n, guess, a0, min(chunk, na - a0), 0)]

    def loop():
        res[1] = [hip.solve_xl4_words(spec[s], ns, 0) for s in range(na)]
    batch()
    loop()                                             # warm, both
    tb, tl = [], []
    for _ in range(5):                                 # alternating
        for call, out in ((batch, tb), (loop, tl)):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
    same = all(a.status == b.status and a.rank == b.rank and np.array_equal(a.origin, b.origin) for a, b in zip(*res))
    solved = [s for s in range(na) if res[0][s].status == 0]
    hit = res[0][right]
    found = hit.status == 0 and hit.rank == cols4 and hit.origin_int() & ((1 << ns) - 1) == y
    mb, ml = statistics.median(tb), statistics.median(tl)
    say(f"      solve_xl4_guess_words, {na} assignments in chunks of {chunk}: median {mb:9.1f} ms (min {min(tb):.1f}, max {max(tb):.1f}) = {mb / na:.3f} ms per system")
    say(f"      loop of {na} solve_xl4_words:                          median {ml:9.1f} ms (min {min(tl):.1f}, max {max(tl):.1f}) = {ml / na:.3f} ms per system")
    say(f"      loop / batch: {ml / mb:.2f}; both give the same status, rank and origin for every assignment: {same}")
    say(f"      consistent assignments: {solved} (the planted point's is {right}); rank {hit.rank} of {cols4} there, the planted point came back: {found}")
    say("not measured: n above 40, other f, mode 1 (bases), the factored hybrid entry (solve_xl4_guess_quad_terms), more than one GPU, "
        "the share of the upload in the end-to-end times.")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "xl4_expand_time.txt")
    main(out)
