"""Times of degree-4 XL on cubic equations on one GPU; profiles/cubic_xl4_expand_time.txt.

    python tools/cubic_xl4_expand_time.py [--out FILE]

Random dense cubic systems kept factored, with one planted point (tools/cubic_expand_time.py: a dense linear form plus two products of
two and two products of three dense affine forms a row), at n = 16, 24, 32, with the smallest m for which m(n + 1) >= 1.15 cols4 for
cols4 = n + C(n,2) + C(n,3) + C(n,4) columns.  Nothing guarantees the rank of such rows: the rank and the dimension found are reported.
* k_xl4_cubic_expand alone on resident cubic rows: device time (events around the launch, median of 7 after a warm launch), stored
  GB/s, and that against the read-XOR-write and read-only streaming rates gf2bv_stream_ceiling_device measures in the same run;
* solve_device on the resident expansion against solve_xl4_cubic_terms end to end (upload of the factored rows, both expansions,
  solve): medians of 5 warm repetitions, same process; the expansion's share of the solve it feeds;
* whether both answers are equal, and whether the answer is the planted point (full rank, and the origin's linear part).
No threshold is set: the lines are printed and written to FILE (default profiles/cubic_xl4_expand_time.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process, as in the tests)
from cubic_expand_time import median_ms, planted_system  # noqa: E402
from xl_guess_time import event_median_us  # noqa: E402

from gf2bv_amd import hip  # noqa: E402

SIZES = (16, 24, 32)


def equations_for(n: int) -> int:
    """the smallest m with m(n + 1) >= 1.15 cols4"""
    return -(-115 * hip.xl4_cols(n) // (100 * (n + 1)))


def main(out_path: str):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"tools/cubic_xl4_expand_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    say(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s")
    for n in SIZES:
        cols3, cols4 = hip.xl3_cols(n), hip.xl4_cols(n)
        m = equations_for(n)
        rows, stride = max(m * (n + 1), cols4), hip.padded_stride(cols4)
        x, terms = planted_system(n, m, n)
        cubic = hip.cubic_expand_words(*terms, n)      # the m cubic rows, outside the timed windows
        d_cubic, aug = hip.DeviceBuffer(cubic.nbytes), hip.DeviceBuffer(rows * stride * 8)
        d_cubic.upload(cubic)
        t = event_median_us(lambda: hip.xl4_cubic_expand_device(d_cubic.ptr, m, cubic.shape[1], n, rows, aug.ptr, stride)) / 1e3      # ms
        gbs = rows * stride * 8 / t / 1e6
        say(f"n {n:2d}: {m} equations over {cols3} cubic columns x {n + 1} -> {rows} rows x {cols4} columns ({rows * stride * 8 / 2 ** 20:7.1f} MiB out): "
            f"k_xl4_cubic_expand {t * 1e3:9.1f} us  {gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.3f} of the read-XOR-write rate, "
            f"{gbs / ceil['read_gbs']:.3f} of the read-only rate")
        res = [None, None]

        def resident():
            res[0] = hip.solve_device(aug.ptr, rows, cols4, stride, 0)

        def whole():
            res[1] = hip.solve_xl4_cubic_terms(*terms, n, 0)
        s, w = median_ms(resident, 5), median_ms(whole, 5)
        same = res[0].status == res[1].status and res[0].rank == res[1].rank and np.array_equal(res[0].origin, res[1].origin)
        found = res[1].status == 0 and res[1].rank == cols4 and res[1].origin_int() & ((1 << n) - 1) == x
        say(f"      solve_device (resident expansion) {s:9.2f} ms, solve_xl4_cubic_terms (upload + both expansions + solve) {w:9.2f} ms, "
            f"rank {res[1].rank} of {cols4} (dimension {cols4 - res[1].rank}), both answers equal: {same}, the planted point: {found}")
        say(f"      expansion / solve it feeds: {t / s:.3f}")
        d_cubic.free()
        aug.free()
    say("not measured: n above 32, rows of few terms, mode 1 (bases), more than one GPU, the share of the upload and of k_cubic_expand in "
        "the end-to-end times.")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cubic_xl4_expand_time.txt")
    main(out)
