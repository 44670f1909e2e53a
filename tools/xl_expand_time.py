"""Times of degree-3 XL on one GPU; profiles/xl_expand_time.txt.

    python tools/xl_expand_time.py [--out FILE]

Random dense quadratic systems with one planted point at n = 32, 48, 64, m = ceil(1.15 cols3 / (n + 1)) equations, so that the
expansion has 15 % more rows than its cols3 = n + C(n,2) + C(n,3) columns:
* k_xl3_expand alone on resident quadratic rows: device time (events around the launch, median of 7 after a warm launch), stored
  GB/s, and that against the read-XOR-write and read-only streaming rates gf2bv_stream_ceiling_device measures in the same run;
* solve_device on the resident expansion against solve_xl3_quad_terms end to end (upload of the factored rows, both expansions,
  solve): medians of 5 warm repetitions, same process;
* whether the answer is the planted point (full rank, and the origin's linear part).
The lines are printed and written to FILE (default profiles/xl_expand_time.txt)."""
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

SIZES = (32, 48, 64)


def planted_system(n: int, m: int, seed: int):
    """(planted point, quadratic rows as augmented words, the same rows factored: x_i times the sum of its partners j < i)"""
    rng = np.random.default_rng(seed)
    cols2 = hip.quad_cols(n)
    w2, wl = (cols2 + 1 + 63) // 64, (n + 1 + 63) // 64
    x = int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1) | 1
    point = x
    for i in range(1, n):
        if (x >> i) & 1:
            point |= (x & ((1 << i) - 1)) << (n + i * (i - 1) // 2)
    word = lambda v, w: np.frombuffer(int(v).to_bytes(8 * w, "little"), dtype=np.uint64)      # noqa: E731
    quad = np.zeros((m, w2), dtype=np.uint64)
    lin, off, ta, tb = [], [0], [], []
    for r in range(m):
        a = int.from_bytes(rng.bytes((cols2 + 7) // 8), "little") & ((1 << cols2) - 1)
        c = bin(a & point).count("1") & 1
        quad[r] = word(a | (c << cols2), w2)
        lin.append(word(((a & ((1 << n) - 1)) << 1) | c, wl))
        for i in range(1, n):
            run = (a >> (n + i * (i - 1) // 2)) & ((1 << i) - 1)
            if run:
                ta.append(word(1 << (1 + i), wl))
                tb.append(word(run << 1, wl))
        off.append(len(ta))
    return x, quad, (np.array(lin), np.array(off, dtype=np.int64), np.array(ta), np.array(tb))


def median_ms(call, reps: int) -> float:
    call()                                             # warm
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return statistics.median(out) * 1e3


def main(out_path: str):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"tools/xl_expand_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    say(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s")
    for n in SIZES:
        cols3 = hip.xl3_cols(n)
        m = math.ceil(1.15 * cols3 / (n + 1))
        rows, stride = max(m * (n + 1), cols3), hip.padded_stride(cols3)
        x, quad, terms = planted_system(n, m, n)
        d_quad, aug = hip.DeviceBuffer(quad.nbytes), hip.DeviceBuffer(rows * stride * 8)
        d_quad.upload(quad)
        expand = lambda: hip.xl3_expand_device(d_quad.ptr, m, quad.shape[1], n, rows, aug.ptr, stride)      # noqa: E731
        expand()
        torch.cuda.synchronize()
        ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            expand()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms)
        gbs = rows * stride * 8 / t / 1e6
        say(f"n {n:2d}: {m} equations -> {rows} rows x {cols3} columns ({rows * stride * 8 / 2 ** 20:6.1f} MiB out): k_xl3_expand {t * 1e3:8.1f} us  "
            f"{gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.2f} of the read-XOR-write rate, {gbs / ceil['read_gbs']:.2f} of the read-only rate")
        res = [None, None]

        def resident():
            res[0] = hip.solve_device(aug.ptr, rows, cols3, stride, 0)

        def whole():
            res[1] = hip.solve_xl3_quad_terms(*terms, n, 0)
        s, w = median_ms(resident, 5), median_ms(whole, 5)
        same = res[0].rank == res[1].rank and np.array_equal(res[0].origin, res[1].origin)
        found = res[1].status == 0 and res[1].rank == cols3 and res[1].origin_int() & ((1 << n) - 1) == x
        say(f"      solve_device (resident expansion) {s:8.2f} ms, solve_xl3_quad_terms (upload + both expansions + solve) {w:8.2f} ms, "
            f"rank {res[1].rank} of {cols3}, both answers equal: {same}, the planted point: {found}")
        say(f"      expansion / solve it feeds: {t / s:.3f}")
        d_quad.free()
        aug.free()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "xl_expand_time.txt")
    main(out)
