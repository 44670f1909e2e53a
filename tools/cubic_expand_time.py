"""Times of the cubic expansion on one GPU; profiles/cubic_expand_time.txt.

    python tools/cubic_expand_time.py [--out FILE]

Random dense cubic systems kept factored, with one planted point, at n = 32, 64, 96 (5488, 43744, 147536 columns), rows = cols3 + 64;
every row is a dense linear form plus two products of two and two products of three dense affine forms:
* k_cubic_expand alone on resident operands: device time (events around the launch, median of 5 after a warm launch), stored GB/s,
  and that against the read-XOR-write and read-only streaming rates gf2bv_stream_ceiling_device measures in the same run;
* solve_device on the resident expansion against solve_cubic_terms end to end (upload of the factored rows, expansion, solve):
  medians of 5 warm repetitions, same process;
* whether every answer is the planted point (full rank, and the origin is the point's monomials).
The lines are printed and written to FILE (default profiles/cubic_expand_time.txt)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process, as in the tests)

from gf2bv_amd import PackedCubicSystem, hip  # noqa: E402
from gf2bv_amd.packed import _popcount64  # noqa: E402

SIZES = (32, 64, 96)
QUAD_TERMS, CUBIC_TERMS = 2, 2


def planted_system(n: int, rows: int, seed: int):
    """(planted point, the factored rows): the value of an exact product at a point is the product of its operands' values, so the
    constant of every linear part is set to what makes the row vanish there"""
    rng = np.random.default_rng(seed)
    wl = (n + 1 + 63) // 64
    x = int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1) | 1
    point = np.frombuffer(((x << 1) | 1).to_bytes(8 * wl, "little"), dtype=np.uint64)
    keep = np.frombuffer(((1 << (n + 1)) - 1).to_bytes(8 * wl, "little"), dtype=np.uint64)

    def forms(count):
        return rng.integers(0, 1 << 64, size=(count, wl), dtype=np.uint64) & keep

    value = lambda f: (_popcount64(f & point).sum(axis=1) & 1).astype(np.uint64)          # noqa: E731
    lin = forms(rows)
    ta, tb = forms(rows * QUAD_TERMS), forms(rows * QUAD_TERMS)
    ua, ub, uc = forms(rows * CUBIC_TERMS), forms(rows * CUBIC_TERMS), forms(rows * CUBIC_TERMS)
    v = value(lin)
    v ^= np.bitwise_xor.reduce((value(ta) & value(tb)).reshape(rows, QUAD_TERMS), axis=1)
    v ^= np.bitwise_xor.reduce((value(ua) & value(ub) & value(uc)).reshape(rows, CUBIC_TERMS), axis=1)
    lin[:, 0] ^= v
    off2 = np.arange(rows + 1, dtype=np.int64) * QUAD_TERMS
    off3 = np.arange(rows + 1, dtype=np.int64) * CUBIC_TERMS
    return x, (lin, off2, ta, tb, off3, ua, ub, uc)


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

    say(f"tools/cubic_expand_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    say(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s")
    ok = True
    for n in SIZES:
        cols3 = hip.xl3_cols(n)
        rows, stride = cols3 + 64, hip.padded_stride(cols3)
        x, terms = planted_system(n, rows, n)
        want = PackedCubicSystem([n])._raw_point(x)
        bufs = [hip.DeviceBuffer(max(a.nbytes, 8)) for a in terms]
        for b, a in zip(bufs, terms):
            b.upload(a)
        aug = hip.DeviceBuffer(rows * stride * 8)
        expand = lambda: hip.cubic_expand_device(*[b.ptr for b in bufs], rows, rows, n, aug.ptr, stride)      # noqa: E731
        expand()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            expand()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms)
        gbs = rows * stride * 8 / t / 1e6
        say(f"n {n:2d}: {rows} rows x {cols3} columns, {QUAD_TERMS} + {CUBIC_TERMS} terms a row ({rows * stride * 8 / 2 ** 20:7.1f} MiB out): "
            f"k_cubic_expand {t * 1e3:9.1f} us  {gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.3f} of the read-XOR-write rate, "
            f"{gbs / ceil['read_gbs']:.3f} of the read-only rate")
        res = [None, None]

        def resident():
            res[0] = hip.solve_device(aug.ptr, rows, cols3, stride, 0)

        def whole():
            res[1] = hip.solve_cubic_terms(*terms, n, rows, 0)
        s, w = median_ms(resident, 5), median_ms(whole, 5)
        same = res[0].rank == res[1].rank and np.array_equal(res[0].origin, res[1].origin)
        found = all(r.status == 0 and r.rank == cols3 and r.origin_int() == want for r in res)
        say(f"      solve_device (resident expansion) {s:9.2f} ms, solve_cubic_terms (upload + expansion + solve) {w:9.2f} ms, "
            f"rank {res[1].rank} of {cols3}, both answers equal: {same}, the planted point: {found}")
        say(f"      expansion / solve it feeds: {t / s:.3f}")
        ok = ok and same and found
        for b in bufs + [aug]:
            b.free()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("an answer was not the planted point")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cubic_expand_time.txt")
    main(out)
