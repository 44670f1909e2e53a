"""Times of the packed quadratic front-end on one GPU; profiles/quad_expand_time.txt.

    python tools/quad_expand_time.py [--kernel-only]

* the NLFSR example (examples/nlfsr_recovery.py) on both front-ends in the same run: generate (split into the symbolic stepping
  of the register and the rest: products, sums), solve_all, total.  The packed figures are medians of 5 warm repetitions; the
  int front-end's generation is timed ONCE per register kind (it is 15 s and more of host time a run);
* k_quad_expand alone at (n, rows) = (128, 8704), (256, 32960), (360, 65536), two products of dense forms per row: device
  time (events around the launch, median of 7 after a warm launch), output GB/s, and that against the read-XOR-write and
  read-only streaming rates gf2bv_stream_ceiling_device measures in the same run;
* at the same sizes solve_device on the expanded matrix against solve_quad_terms end to end (upload, expansion, solve):
  medians of 5.
--kernel-only: the second part alone (for a rocprofv3 --kernel-trace --stats run)."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process, as in the tests)

from gf2bv_amd import PackedQuadraticSystem, QuadraticSystem, hip  # noqa: E402
from tests.harness_models import FibonacciLFSR, GaloisLFSR  # noqa: E402
from nlfsr_recovery import N_BITS, SELECT, TAPS, keystream  # noqa: E402

SIZES = ((128, 8704), (256, 32960), (360, 65536))


def generate(system, kind, stream):
    """the example's equations: (zeros, seconds in the register's symbolic steps, seconds in all of it)"""
    t0 = time.perf_counter()
    (x,) = system.gens()
    sym = kind(N_BITS, TAPS, x)
    zeros, step = [], 0.0
    for bit in stream:
        s0 = time.perf_counter()
        sym()
        step += time.perf_counter() - s0
        if bit:
            x0, x1, x2 = [sym.state[i] for i in SELECT[:3]]
            zeros.append(system.mul_bit(x0, x1) ^ x0 ^ system.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    return zeros, step, time.perf_counter() - t0


def nlfsr():
    for kind, seed in ((GaloisLFSR, 1), (FibonacciLFSR, 2)):
        secret = random.Random(seed).getrandbits(N_BITS)
        stream = keystream(kind(N_BITS, TAPS, secret), 2 ** 14 + 1000)
        for name, cls, reps in (("packed", PackedQuadraticSystem, 5), ("int", QuadraticSystem, 1)):
            system = cls([N_BITS])
            gens, steps, solves = [], [], []
            for _ in range(reps):
                zeros, step, gen = generate(system, kind, stream)
                gens.append(gen)
                steps.append(step)
            assert list(system.solve_all(zeros)) == [(secret,)]            # warm
            for _ in range(5):
                t0 = time.perf_counter()
                sols = list(system.solve_all(zeros))
                solves.append(time.perf_counter() - t0)
            assert sols == [(secret,)]
            gen, step, solve = statistics.median(gens), statistics.median(steps), statistics.median(solves)
            print(f"nlfsr {kind.__name__:13s} {name:6s} front-end, {len(zeros)} equations: generate {gen:7.3f} s ({reps} run{'s' * (reps > 1)}: stepping "
                  f"{step:6.3f} s, products and sums {gen - step:7.3f} s)  solve_all {solve * 1e3:7.2f} ms  total {gen + solve:7.3f} s", flush=True)


def dense_terms(n: int, rows: int, seed: int):
    rng = np.random.default_rng(seed)
    wl = (n + 1 + 63) // 64

    def forms(count):
        f = rng.integers(0, 1 << 64, size=(count, wl), dtype=np.uint64)
        if (n + 1) & 63:
            f[:, -1] &= np.uint64((1 << ((n + 1) & 63)) - 1)
        return f
    return forms(rows), np.arange(0, 2 * rows + 1, 2, dtype=np.int64), forms(2 * rows), forms(2 * rows)


def kernel_and_solve(kernel_only: bool):
    ceil = hip.stream_ceiling()
    print(f"stream ceilings of this GPU: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written), read-only {ceil['read_gbs']:.0f} GB/s", flush=True)
    for n, rows in SIZES:
        cols = hip.quad_cols(n)
        stride = hip.padded_stride(cols)
        lin, off, ta, tb = dense_terms(n, rows, n)
        bufs = [hip.DeviceBuffer(max(a.nbytes, 16)) for a in (lin, off, ta, tb)]
        for b, a in zip(bufs, (lin, off, ta, tb)):
            b.upload(a)
        aug = hip.DeviceBuffer(rows * stride * 8)
        expand = lambda: hip.quad_expand_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, rows, rows, n, aug.ptr, stride)      # noqa: E731
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
        line = (f"n {n:3d} rows {rows:5d} ({cols} columns, {rows * stride * 8 / 2 ** 20:6.1f} MiB out): k_quad_expand {t * 1e3:8.1f} us  {gbs:6.0f} GB/s stored "
                f"= {gbs / ceil['rmw_gbs']:.2f} of the read-XOR-write rate, {gbs / ceil['read_gbs']:.2f} of the read-only rate")
        if not kernel_only:
            hip.solve_device(aug.ptr, rows, cols, stride, 0)               # warm
            solve, whole = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                res = hip.solve_device(aug.ptr, rows, cols, stride, 0)
                solve.append(time.perf_counter() - t0)
            hip.solve_quad_terms(lin, off, ta, tb, n, rows, 0)
            for _ in range(5):
                t0 = time.perf_counter()
                res2 = hip.solve_quad_terms(lin, off, ta, tb, n, rows, 0)
                whole.append(time.perf_counter() - t0)
            assert res.rank == res2.rank and np.array_equal(res.origin, res2.origin)
            s, w = statistics.median(solve) * 1e3, statistics.median(whole) * 1e3
            line += f" | solve_device (resident matrix) {s:7.2f} ms, solve_quad_terms (upload + expand + solve) {w:7.2f} ms, rank {res.rank}"
        print(line, flush=True)
        for b in bufs + [aug]:
            b.free()


if __name__ == "__main__":
    kernel_only = "--kernel-only" in sys.argv
    print(f"tools/quad_expand_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).", flush=True)
    kernel_and_solve(kernel_only)
    if not kernel_only:
        nlfsr()
