"""Times of the composition entries (gf2bv_compose_*, k_compose) on one GPU; profiles/compose_time.txt.

    python tools/compose_time.py            # every case, each in a fresh process
    python tools/compose_time.py CASE       # one case in this process: product:N  power:N:LOG2K  twin:N

* one product, dense random, ra = n = nb = 256, 4096, 19968: the library's kernel time (events around the launch), the whole
  compose_words call (upload, kernel, download), and the rate in k_update16's unit -- ra x Wb x 8 bytes of row segments updated per
  256-bit slice, times the slices, per second -- beside the read-XOR-write stream figure of gf2bv_stream_ceiling_device from the
  same process;
* power at n = 19968 with k = 2^20 and 2^40: wall time, kernel time, number of products;
* the numpy twin of the tests (tests/compose_terms.py) at 256 and 4096.
Warm (one call before the timed ones), medians of 5 with the range."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["product:256", "product:4096", "product:19968", "power:19968:20", "power:19968:40", "twin:256", "twin:4096"]
REPS = 5


def med(xs) -> str:
    return f"{statistics.median(xs):10.3f} ms  [{min(xs):.3f} .. {max(xs):.3f}]"


def dense(seed: int, rows: int, words: int):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(rows, words), dtype=np.uint64)


def product(n: int):
    import torch  # noqa: F401  (one HIP runtime per process, as in the tests)
    from gf2bv_amd import hip
    shape = hip.compose_shape()
    w = hip.form_words(n)
    a, b = dense(1, n, w), dense(2, n, w)
    hip.compose_words(a, n, b, n)
    wall, kern, up, down = [], [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        hip.compose_words(a, n, b, n)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = hip.compose_last_times()
        kern.append(t["ms_kernels"]); up.append(t["ms_upload"]); down.append(t["ms_download"])
    slices = -(-(n + 1) // shape["slice_bits"])
    swept = n * w * 8 * slices                             # bytes of row segments updated, one slice at a time
    ceil = hip.stream_ceiling()
    print(f"product n = nb = ra = {n}: kernel {med(kern)}   compose_words {med(wall)}   upload {statistics.median(up):.3f} ms, download {statistics.median(down):.3f} ms")
    print(f"    {slices} slices x {n * w * 8 / 1e6:.2f} MB of C = {swept / 1e9:.3f} GB of segment updates: {swept / statistics.median(kern) / 1e9:.3f} TB/s "
          f"(read-XOR-write stream of this run: {ceil['rmw_gbs'] / 1e3:.3f} TB/s, read-only {ceil['read_gbs'] / 1e3:.3f} TB/s)", flush=True)


def power(n: int, log2k: int):
    import torch  # noqa: F401
    from gf2bv_amd import hip
    b = dense(3, n, hip.form_words(n))
    hip.compose_power_words(b, n, 3)
    wall, kern = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        hip.compose_power_words(b, n, 1 << log2k)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = hip.compose_last_times()
        kern.append(t["ms_kernels"])
    print(f"power n = {n}, k = 2^{log2k}: {t['products']} products   kernels {med(kern)}   compose_power_words {med(wall)}", flush=True)


def twin(n: int):
    from tests import compose_terms as T
    w = T.form_words(n)
    a, b = dense(1, n, w), dense(2, n, w)
    T.substitute(a[:8], n, b, n)
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        T.substitute(a, n, b, n)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"numpy twin n = nb = ra = {n}: {med(wall)}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        kind, *rest = sys.argv[1].split(":")
        {"product": product, "power": power, "twin": twin}[kind](*(int(x) for x in rest))
    else:
        for case in CASES:
            subprocess.run([sys.executable, os.path.abspath(__file__), case], check=True, timeout=300)
