"""Times of hybrid degree-4 XL on cubic equations (guess f unknowns, solve all 2^f systems as one batch) on one GPU;
profiles/cubic_xl4_guess_time.txt.

    timeout -k 10 300 python tools/cubic_xl4_guess_time.py --case 24 8 --out FILE && \
    timeout -k 10 900 python tools/cubic_xl4_guess_time.py --case 32 8 --out FILE --append

One case a process, each under a time limit of its own, the second only after the first ended well.  Every process measures the
streaming rates it compares with itself (gf2bv_stream_ceiling_device), so no figure is set against one of another run.

A case is a random dense factored cubic system with one planted point: per row a dense linear form, two products of two and two
products of three dense affine forms; m the smallest with m(n' + 1) >= 1.15 cols4(n') for n' = n - f, so that every one of the 2^f
assignments' systems has 15 % more rows than columns.  Reported:
* k_cubic_specialise and k_xl4_cubic_expand_batch alone on resident rows, all 2^f assignments: device time (events around the launch,
  median of 7 after a warm launch), bytes stored, and the stored rate against the read-XOR-write streaming rate;
* solve_xl4_cubic_guess_terms over all assignments end to end (upload, k_cubic_expand, both kernels, the gang solve) against a loop of
  2^f solve_xl4_cubic_words on the same specialised rows (specialised beforehand, outside the timed window): the two alternate in the
  same process, warm; medians of 5 with their ranges;
* whether every assignment's status, rank and origin agree between batch and loop, and from how many assignments the planted point
  comes back;
* whether all 2^f assignments fit one chunk (gf2bv_xl4_cubic_guess_chunk_device)."""
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
from tools.xl_guess_time import event_median_us  # noqa: E402


def planted_terms(n: int, m: int, seed: int):
    """(planted point, factored arrays): every operand a random dense affine form over n <= 63 unknowns, the row's constant set so
    that it vanishes at the point"""
    rng = np.random.default_rng(seed)
    form = lambda count: rng.integers(0, 1 << (n + 1), size=(count, 1), dtype=np.uint64)      # noqa: E731  (bit 0 the constant)
    x = int(rng.integers(0, 1 << n)) | 1
    lin, ta, tb, ua, ub, uc = form(m), form(2 * m), form(2 * m), form(2 * m), form(2 * m), form(2 * m)
    at = (x << 1) | 1
    val = lambda a: np.array([bin(int(v) & at).count("1") & 1 for v in a[:, 0]], dtype=np.uint64)      # noqa: E731
    q, c = val(ta) & val(tb), val(ua) & val(ub) & val(uc)
    lin[:, 0] ^= val(lin) ^ q[0::2] ^ q[1::2] ^ c[0::2] ^ c[1::2]
    off = 2 * np.arange(m + 1, dtype=np.int64)
    return x, (lin, off, ta, tb, off.copy(), ua, ub, uc)


def main(n: int, f: int, out_path: str, append: bool):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    if not append:
        say(f"tools/cubic_xl4_guess_time.py on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    ceil = hip.stream_ceiling()
    ns, na = n - f, 1 << f
    cols3s, cols4 = hip.xl3_cols(ns), hip.xl4_cols(ns)
    m = math.ceil(1.15 * cols4 / (ns + 1))
    rows = max(m * (ns + 1), cols4)
    guess = tuple(range(2, n, n // f))[:f]
    x, terms = planted_terms(n, m, n)
    right = sum(((x >> g) & 1) << t for t, g in enumerate(guess))
    rest = [u for u in range(n) if u not in guess]
    y = sum(((x >> u) & 1) << k for k, u in enumerate(rest))
    chunk = hip.xl4_cubic_guess_chunk(m, n, f)
    say(f"n {n}, {f} guessed {guess}: {m} equations, {na} systems of {rows} rows x {cols4} columns over n' = {ns}; this process's stream "
        f"ceiling: read-XOR-write {ceil['rmw_gbs']:.0f} GB/s (bytes read + written)")
    say(f"      chunk by gf2bv_xl4_cubic_guess_chunk_device: {chunk}" + ("" if chunk >= na else f" -- BELOW the {na} assignments: not one chunk"))
    if chunk < na:
        return lines
    cubic = hip.cubic_expand_words(*terms, n)
    ss = (cols3s + 1 + 63) // 64
    ss += ss & 1
    xs = (cols4 + 1 + 63) // 64
    xs += xs & 1
    # -- the two kernels alone, all assignments resident
    d_cubic, d_spec, d_xl = hip.DeviceBuffer(cubic.nbytes), hip.DeviceBuffer(na * m * ss * 8), hip.DeviceBuffer(na * rows * xs * 8)
    d_cubic.upload(cubic)
    t_spec = event_median_us(lambda: hip.cubic_specialise_device(d_cubic.ptr, m, cubic.shape[1], n, guess, 0, na, d_spec.ptr, ss, m * ss))
    t_xl = event_median_us(lambda: hip.xl4_cubic_expand_batch_device(d_spec.ptr, na, m * ss, m, ss, ns, rows, d_xl.ptr, xs, rows * xs))
    for name, t, nbytes in (("k_cubic_specialise      ", t_spec, na * m * ss * 8), ("k_xl4_cubic_expand_batch", t_xl, na * rows * xs * 8)):
        gbs = nbytes / t / 1e3
        say(f"      {name} {t:10.1f} us for {nbytes / 2 ** 20:9.1f} MiB stored: {gbs:6.0f} GB/s = {gbs / ceil['rmw_gbs']:.3f} of the "
            f"read-XOR-write rate")
    for buf in (d_cubic, d_spec, d_xl):
        buf.free()
    # -- end to end: the batch against a loop of single solves on the same specialised rows
    spec = hip.cubic_specialise_words(cubic, n, guess)                    # outside the timed window
    res = [None, None]

    def batch():
        res[0] = hip.solve_xl4_cubic_guess_terms(*terms, n, guess, mode=0)

    def loop():
        res[1] = [hip.solve_xl4_cubic_words(spec[s], ns, 0) for s in range(na)]
    batch()
    loop()                                             # warm, both
    tb, tl = [], []
    for _ in range(5):                                 # alternating
        for call, out in ((batch, tb), (loop, tl)):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
    same = all(a.status == b.status and a.rank == b.rank and (a.status != 0 or np.array_equal(a.origin, b.origin)) for a, b in zip(*res))
    solved = [s for s in range(na) if res[0][s].status == 0]
    back = [s for s in solved if s == right and res[0][s].origin_int() & ((1 << ns) - 1) == y]
    mb, ml = statistics.median(tb), statistics.median(tl)
    say(f"      solve_xl4_cubic_guess_terms, {na} assignments: median {mb:9.1f} ms (min {min(tb):.1f}, max {max(tb):.1f}) = {mb / na:.3f} ms per system")
    say(f"      loop of {na} solve_xl4_cubic_words:            median {ml:9.1f} ms (min {min(tl):.1f}, max {max(tl):.1f}) = {ml / na:.3f} ms per system")
    say(f"      loop / batch: {ml / mb:.2f}; status, rank and origin agree for every assignment: {same}")
    say(f"      consistent assignments: {solved} (the planted point's is {right}); rank {res[0][right].rank} of {cols4} there; the planted point "
        f"came back from {len(back)} assignment(s)")
    return lines


if __name__ == "__main__":
    at = sys.argv.index("--case")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cubic_xl4_guess_time.txt")
    text = main(int(sys.argv[at + 1]), int(sys.argv[at + 2]), out, "--append" in sys.argv)
    with open(out, "a" if "--append" in sys.argv else "w") as fh:
        fh.write("\n".join(text) + "\n")
