"""Times of `unroll` (gf2bv_compose_unroll_words) on one GPU beside the host's own symbolic stepping; profiles/unroll_time.txt.

    python tools/unroll_time.py [--out FILE]   # every case, each in a fresh process; the lines go to FILE (profiles/unroll_time.txt)
    python tools/unroll_time.py CASE           # one case in this process: nlfsr  xoshiro  mt:COUNT

* nlfsr: examples/nlfsr_recovery_unrolled.py's shape -- the 128-bit Galois register, its five filter inputs, 17384 time steps from 1;
* xoshiro: xoshiro256's state transition, the 64 bits of one state word, 4096 time steps from 0;
* mt:4, mt:16: MT19937's twist map as examples/mt_skip_recovery.py builds it, the whole state (19968 bits), 4 and 16 twists from 0.
Per case: the `unroll` call (wall), the library's kernel time and product count (hip.compose_last_times), and the host stepping the same
symbolic model to the same rows in the same process -- which is how the rows are had without `unroll`.  The rows of the two are
compared.  Warm (one call before the timed ones), medians of 5 with the range.  No ratio is expected in advance."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

CASES = ["nlfsr", "xoshiro", "mt:4", "mt:16"]
REPS = 5


def med(xs) -> str:
    return f"{statistics.median(xs):10.3f} ms  [{min(xs):.3f} .. {max(xs):.3f}]"


def nlfsr_model():
    from gf2bv_amd import PackedLinearSystem
    from nlfsr_recovery import N_BITS, SELECT, TAPS
    from tests.harness_models import GaloisLFSR
    (x,) = PackedLinearSystem([N_BITS]).gens()
    count = 2 ** 14 + 1000

    def the_map():
        sym = GaloisLFSR(N_BITS, TAPS, x)
        sym()
        return (sym.state,)

    def host():
        sym, rows = GaloisLFSR(N_BITS, TAPS, x), []
        for _ in range(count):
            sym()
            rows.append([sym.state[i] for i in SELECT])
        return rows

    return f"nlfsr (n = {N_BITS}, ra = {len(SELECT)}, count = {count}, start = 1)", [x[i] for i in SELECT], the_map, count, 1, host


def xoshiro_model():
    from gf2bv_amd import PackedLinearSystem
    from tests.harness_models import Xoshiro256starstar
    gens = PackedLinearSystem([64] * 4).gens()
    count = 4096

    def the_map():
        sym = Xoshiro256starstar(gens)
        sym.step()
        return tuple(sym.s)

    def host():
        sym, rows = Xoshiro256starstar(gens), []
        for _ in range(count):
            rows.append([sym.s[1]])
            sym.step()
        return rows

    return f"xoshiro256 (n = 256, ra = 64, count = {count}, start = 0)", [gens[1]], the_map, count, 0, host


def mt_model(count: int):
    from gf2bv_amd import PackedLinearSystem
    from tests.harness_models import MT19937
    gens = PackedLinearSystem([32] * 624).gens()

    def the_map():
        one = MT19937(gens)
        one._regenerate()
        return tuple(one.mt)

    def host():
        sym, rows = MT19937(gens), []
        for i in range(count):
            if i:
                sym._regenerate()
            rows.append(list(sym.mt))
        return rows

    return f"MT19937 twist (n = ra = 19968, count = {count}, start = 0)", list(gens), the_map, count, 0, host


def run(kind: str, *rest):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process, as in the tests)
    from gf2bv_amd import hip, unroll
    name, exprs, the_map, count, start, host = {"nlfsr": nlfsr_model, "xoshiro": xoshiro_model, "mt": mt_model}[kind](*(int(x) for x in rest))
    t0 = time.perf_counter()
    images = the_map()
    map_ms = (time.perf_counter() - t0) * 1e3
    items = unroll(exprs, images, count, start=start)
    wall, kern, up, down = [], [], [], []
    for _ in range(REPS):
        del items
        t0 = time.perf_counter()
        items = unroll(exprs, images, count, start=start)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = hip.compose_last_times()
        kern.append(t["ms_kernels"]); up.append(t["ms_upload"]); down.append(t["ms_download"])
    rows = host()
    step = []
    for _ in range(REPS):
        del rows
        t0 = time.perf_counter()
        rows = host()
        step.append((time.perf_counter() - t0) * 1e3)
    assert len(rows) == len(items) == count
    for got, want in zip(items, rows):
        assert all(np.array_equal(g._rows, w._rows) for g, w in zip(got, want))
    w = hip.form_words(sum(len(v) for v in images))
    print(f"{name}: one symbolic step on the host {map_ms:.1f} ms; {count * sum(len(v) for v in exprs) * w * 8 / 1e6:.1f} MB of rows, equal to the host's")
    print(f"    unroll          {med(wall)}   {t['products']} products, kernels {med(kern)}   upload {statistics.median(up):.3f} ms, download {statistics.median(down):.3f} ms")
    print(f"    host stepping   {med(step)}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "unroll_time.txt")
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    if args:
        kind, *rest = args[0].split(":")
        run(kind, *rest)
    else:
        lines = []
        for case in CASES:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), case], check=True, timeout=600, stdout=subprocess.PIPE, text=True)
            print(done.stdout, end="", flush=True)
            lines.append(done.stdout)
        with open(out, "w") as f:
            f.write("".join(lines))
