"""Times of the quartic expansion on one GPU; profiles/quartic_expand_time.txt.

    python tools/quartic_expand_time.py [--out FILE]

Random dense quartic systems kept factored, with one planted point, at n = 16, 24, 32 (2516, 12950, 41448 columns), rows = cols4 + 64;
every row is a dense linear form plus two products of two, two of three and two of four dense affine forms.  One process a case
(`--case N` is what the parent starts), everything warm, medians of 5 with their ranges:
* k_quartic_expand alone on resident operands: device time (events around the launch), stored GB/s against the read-XOR-write
  streaming rate gf2bv_stream_ceiling_device measures in the same process;
* the same rows with their quartic terms removed (the offsets of the products of four all zero), through the same kernel: what the
  staging with cx_word and the copy with xl_mul_word cost without the new terms;
* solve_device on the resident expansion against solve_quartic_terms end to end (upload of the factored rows, expansion, solve), and
  the expansion's share of the solve it feeds;
* whether every answer is the planted point (full rank, and the origin is the point's monomials).
The lines are printed and written to FILE (default profiles/quartic_expand_time.txt)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (16, 24, 32)
TERMS = (2, 2, 2)                                      # products of two, of three and of four forms a row
CUBIC_SHARE = (0.10, 0.26)                             # k_cubic_expand's share of its solve, profiles/cubic_expand_time.txt


def planted_system(n: int, rows: int, seed: int):
    """(planted point, the thirteen factored arrays): the value of an exact product at a point is the product of its operands'
    values, so the constant of every linear part is set to what makes the row vanish there"""
    import numpy as np  # noqa: PLC0415

    from gf2bv_amd.packed import _popcount64  # noqa: PLC0415
    rng = np.random.default_rng(seed)
    wl = (n + 1 + 63) // 64
    x = int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1) | 1
    point = np.frombuffer(((x << 1) | 1).to_bytes(8 * wl, "little"), dtype=np.uint64)
    keep = np.frombuffer(((1 << (n + 1)) - 1).to_bytes(8 * wl, "little"), dtype=np.uint64)
    value = lambda f: (_popcount64(f & point).sum(axis=1) & 1).astype(np.uint64)          # noqa: E731
    lin = rng.integers(0, 1 << 64, size=(rows, wl), dtype=np.uint64) & keep
    out, v = [lin], value(lin)
    for arity, count in zip((2, 3, 4), TERMS):
        ops = [rng.integers(0, 1 << 64, size=(rows * count, wl), dtype=np.uint64) & keep for _ in range(arity)]
        prod = value(ops[0])
        for f in ops[1:]:
            prod &= value(f)
        v ^= np.bitwise_xor.reduce(prod.reshape(rows, count), axis=1)
        out += [np.arange(rows + 1, dtype=np.int64) * count] + ops
    lin[:, 0] ^= v
    return x, tuple(out)


def spread(values) -> str:
    return f"{statistics.median(values):9.3f} [{min(values):.3f} .. {max(values):.3f}]"


def case(n: int) -> bool:
    import numpy as np  # noqa: PLC0415
    import torch  # noqa: PLC0415  (one HIP runtime per process, as in the tests)

    from gf2bv_amd import PackedQuarticSystem, hip  # noqa: PLC0415
    ceil = hip.stream_ceiling()
    cols4 = hip.xl4_cols(n)
    rows, stride = cols4 + 64, hip.padded_stride(cols4)
    x, terms = planted_system(n, rows, n)
    want = PackedQuarticSystem([n])._raw_point(x)
    bufs = [hip.DeviceBuffer(max(a.nbytes, 8)) for a in terms]
    for b, a in zip(bufs, terms):
        b.upload(a)
    none = hip.DeviceBuffer((rows + 1) * 8)
    none.upload(np.zeros(rows + 1, dtype=np.int64))
    aug = hip.DeviceBuffer(rows * stride * 8)
    ptrs = [b.ptr for b in bufs]

    def device_ms(p) -> list:
        expand = lambda: hip.quartic_expand_device(*p, rows, rows, n, aug.ptr, stride)      # noqa: E731
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
        return ms

    print(f"case n = {n} on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    print(f"n {n:2d}: {rows} rows x {cols4} columns, {' + '.join(map(str, TERMS))} terms a row ({rows * stride * 8 / 2 ** 20:7.1f} MiB out), "
          f"chunks {hip.quartic_chunks(n)}; read-XOR-write rate of this process {ceil['rmw_gbs']:.0f} GB/s")
    cubic_only = device_ms(ptrs[:8] + [none.ptr] + ptrs[9:])
    full = device_ms(ptrs)                             # (last: its rows are the ones the solve below reads)
    t = statistics.median(full)
    gbs = rows * stride * 8 / t / 1e6
    print(f"      k_quartic_expand {spread(full)} ms  {gbs:6.0f} GB/s stored = {gbs / ceil['rmw_gbs']:.3f} of the read-XOR-write rate")
    print(f"      the same rows without their quartic terms {spread(cubic_only)} ms: the quartic terms are "
          f"{1 - statistics.median(cubic_only) / t:.3f} of the kernel's time")
    res = [None, None]

    def timed(call) -> list:
        call()                                         # warm
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def resident():
        res[0] = hip.solve_device(aug.ptr, rows, cols4, stride, 0)

    def whole():
        res[1] = hip.solve_quartic_terms(*terms, n, rows, 0)
    s, w = timed(resident), timed(whole)
    same = res[0].rank == res[1].rank and np.array_equal(res[0].origin, res[1].origin)
    found = all(r.status == 0 and r.rank == cols4 and r.origin_int() == want for r in res)
    print(f"      solve_device (resident expansion) {spread(s)} ms, solve_quartic_terms (upload + expansion + solve) {spread(w)} ms, "
          f"rank {res[1].rank} of {cols4}, both answers equal: {same}, the planted point: {found}")
    share = t / statistics.median(s)
    print(f"      expansion / solve it feeds: {share:.3f}" + (f" -- above k_cubic_expand's {CUBIC_SHARE[0]:.2f} .. {CUBIC_SHARE[1]:.2f}: the first thing to look at"
                                                              if share > CUBIC_SHARE[1] else ""))
    for b in bufs + [aug, none]:
        b.free()
    return same and found


def main(out_path: str):
    lines = ["tools/quartic_expand_time.py, one process a case."]
    ok = True
    for n in SIZES:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(n)], capture_output=True, text=True, timeout=900)
        print(child.stdout, end="", flush=True)
        lines += child.stdout.splitlines()
        if child.returncode != 0:
            print(child.stderr[-2000:], file=sys.stderr)
            ok = False
            break                                      # (nothing more is started on a device a case has failed on)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("a case failed, or an answer was not the planted point")


if __name__ == "__main__":
    if "--case" in sys.argv:
        sys.exit(0 if case(int(sys.argv[sys.argv.index("--case") + 1])) else 1)
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "quartic_expand_time.txt"))
