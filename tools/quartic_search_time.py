"""Times of the quartic search (search_all_quartic / search_all_xl4 -> gf2bv_quartic_search) on one GPU; profiles/quartic_search_time.txt.

    python tools/quartic_search_time.py [out.txt [case ...]]
    python tools/quartic_search_time.py --prepare          (builds the probe libraries of the other lane splits; needs no GPU)

One process per case (this process starts them one after another and never opens the GPU itself), everything warm inside a case,
medians of 5 with their ranges.  The cases:
* rate24, rate28, rate32: the device search alone over 2^R points with 64 dense forms, as the call time of
  gf2bv_quartic_forms_search (host table build, k_quartic_search, no second pass), beside gf2bv_cubic_forms_search on 64 dense cubic
  forms of the same R in the same process, and their ratio;
* example: the library-time breakdown (gf2bv_quartic_last_times) of examples/nlfsr_recovery_quartic_search.py and of one degree-4 XL
  case;
* walk12, walk16: list(solve_all(..., max_dimension=16)) against search_all_quartic on the same n = 12 space at d = 12 and d = 16.
The lane split is a constant of the build (kQuarticWalk in gf2_solver.hip), so another split is another build of the library: for
every L of OTHER_SPLITS the tool copies gf2bv_amd/ and include/ to tools/_probe/walk_L/ (kept out of git), rewrites the constant
there, builds that copy (reused when its sources have not changed) and runs the three rate cases with it, after the cases of the
build's own split and into the same output file."""
import os
import random
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rate24", "rate28", "rate32", "example", "walk12", "walk16")
OTHER_SPLITS = (8, 10)
WALK = re.compile(r"constexpr int kQuarticWalk = (\d+);")


def own_split() -> int:
    with open(os.path.join(ROOT, "gf2bv_amd", "csrc", "gf2_solver.hip")) as f:
        return int(WALK.search(f.read()).group(1))


def probe_root(walk: int) -> str:
    """the tree of a library whose lanes walk `walk` variables, built"""
    root = os.path.join(ROOT, "tools", "_probe", f"walk_{walk}")
    for sub in ("gf2bv_amd", "include"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(root, sub), dirs_exist_ok=True,
                        ignore=shutil.ignore_patterns("*.so", "__pycache__"))
    path = os.path.join(root, "gf2bv_amd", "csrc", "gf2_solver.hip")
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(WALK.sub(f"constexpr int kQuarticWalk = {walk};", text, count=1))
    subprocess.run([sys.executable, os.path.join(root, "gf2bv_amd", "build.py")], check=True, stdout=subprocess.DEVNULL)
    return root


def timed(fn, reps: int = 5) -> tuple:
    """(median, min, max) in seconds of `reps` calls after one warm call, and the last result"""
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def ms(t, lo, hi) -> str:
    return f"{t * 1e3:9.2f} ms [{lo * 1e3:.2f} .. {hi * 1e3:.2f}]"


def rate(R: int):
    from gf2bv_amd import hip
    from tests import cubic_forms as CF
    from tests import quartic_forms as QF
    rng = random.Random(R)
    point = rng.getrandbits(R)
    quartic = QF.planted_dense(rng, R, 64, [point])
    cubic = CF.planted_dense(rng, R, 64, [point])
    t4, lo4, hi4, (count, got) = timed(lambda: hip.quartic_forms_search(quartic, R))
    assert point in got
    t3, lo3, hi3, (count, got) = timed(lambda: hip.cubic_forms_search(cubic, R))
    assert point in got
    print(f"R {R}: k_quartic_search {ms(t4, lo4, hi4)} = {2 ** R / t4:.3e} points/s | k_cubic_search {ms(t3, lo3, hi3)} = "
          f"{2 ** R / t3:.3e} points/s | ratio {t4 / t3:.1f}")


def phases() -> str:
    from gf2bv_amd import hip
    return "  ".join(f"{k} {v:.2f}" for k, v in hip.quartic_last_times().items())


def example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import nlfsr_recovery_quartic_search as ex
    from gf2bv_amd import PackedQuarticSystem, QuadraticSystem, search_all_quartic, search_all_xl4
    secret = 0x52E7
    c = PackedQuarticSystem([ex.N_BITS])
    zeros = ex.equations(c, secret, ex.OUTPUTS)
    space = c.solve_raw_space(zeros)
    t, lo, hi, raws = timed(lambda: space.quartic_search(ex.N_BITS))
    assert [c.convert_sol(r) for r in raws] == [(secret,)]
    print(f"example n 16, {ex.OUTPUTS} outputs, d {space.dimension}: quartic_search {ms(t, lo, hi)}  {phases()}")
    t, lo, hi, sols = timed(lambda: search_all_quartic(c, zeros))
    print(f"  the whole search_all_quartic (linearised solve, search, conversion): {ms(t, lo, hi)}")
    from tests.test_gpu_quartic_search import LFSR, XL4_OUTPUTS
    from tests.test_gpu_xl import lfsr_zeros
    q = QuadraticSystem([LFSR[0]])
    zq = lfsr_zeros(q, *LFSR, 40)
    space = q.solve_raw_space_xl4(zq)
    t, lo, hi, raws = timed(lambda: space.quartic_search(LFSR[0]))
    assert len(raws) == XL4_OUTPUTS[40][2]
    print(f"degree-4 XL n 12, 40 outputs ({len(zq)} equations), d {space.dimension}: quartic_search {ms(t, lo, hi)}, {len(raws)} points  {phases()}")
    t, lo, hi, sols = timed(lambda: search_all_xl4(q, zq))
    print(f"  the whole search_all_xl4: {ms(t, lo, hi)}")


def versus_walk(count: int):
    from gf2bv_amd import PackedQuarticSystem, search_all_quartic
    from tests.quartic_terms import REGISTER4_12, register4_zeros
    c = PackedQuarticSystem([12])
    zeros = register4_zeros(c, 0x52F, count=count, **REGISTER4_12)
    d = c.solve_raw_space(zeros).dimension
    tw, w0, w1, walk = timed(lambda: list(c.solve_all(zeros, max_dimension=16)))
    ts, s0, s1, got = timed(lambda: search_all_quartic(c, zeros))
    assert got == walk
    print(f"n 12, d {d}: list(solve_all) {ms(tw, w0, w1)}, search_all_quartic {ms(ts, s0, s1)}, {len(got)} points "
          f"(both with the linearised solve)")


def run_case(name: str, root: str):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, root)                         # (gf2bv_amd from `root`, the tests' helpers from this tree)
    import torch  # noqa: F401  (one HIP runtime per process, as in the tests)
    if name.startswith("rate"):
        rate(int(name[4:]))
    elif name == "example":
        example()
    else:
        versus_walk({"walk12": 781, "walk16": 777}[name])


def main(argv):
    if len(argv) > 1 and argv[1] == "--case":
        run_case(argv[2], argv[3])
        return
    if len(argv) > 1 and argv[1] == "--prepare":
        print([probe_root(walk) for walk in OTHER_SPLITS])
        return
    sys.path.insert(0, ROOT)
    from gf2bv_amd import hip                        # (the build id is read from the library: no device is opened here)
    lines = [f"tools/quartic_search_time.py on one MI355X (build {hip.build_id()}, L = {own_split()}).  One process per case; medians of "
             "5 warm runs [min .. max].",
             "R ..: the call time of gf2bv_quartic_forms_search / gf2bv_cubic_forms_search on 64 dense forms (table build, search kernel; "
             "no second pass).",
             "Phase times are gf2bv_quartic_last_times() in ms: reduction, forms build (k_forms_products<4> + k_forms_sum, every round), "
             "affine elimination,",
             "device search (k_quartic_search + k_forms_check<4>), total library time; levels = rounds of the affine elimination."]
    print("\n".join(lines), flush=True)
    runs = [(name, ROOT) for name in argv[2:] or CASES]
    ok = True
    for walk in () if argv[2:] else OTHER_SPLITS:
        runs += [(f"other lane split, L = {walk} (a probe build of the same sources):", None)]
        runs += [(name, probe_root(walk)) for name in CASES[:3]]
    for name, root in runs:
        if root is None:
            text = name
        else:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, root], capture_output=True, text=True,
                                  timeout=900)
            ok = done.returncode == 0
            text = done.stdout.strip() if ok else f"{name}: failed with exit status {done.returncode}\n{done.stderr.strip()[-2000:]}"
        print(text, flush=True)
        lines.append(text)
        if not ok:                                   # (nothing more is started on a device after a failure)
            break
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main(sys.argv)
