"""Times of the packed front-ends' kept factorizations, right-hand sides and batches on one GPU; profiles/packed_factor_time.txt.

    python tools/packed_factor_time.py [--small]

Every comparison is between two paths timed in this run on this box (medians of the warm repetitions), and is reported
whichever way it comes out.  Two times per path: the host wall time of the whole step, generation of the equations included
where it says so, and of it the LIBRARY time -- the wall time spent inside the calls that go down to libgf2bv_hip.so (making,
copying, appending to and solving against a factorization, the solves, the quadratic search).
1. one bit_assert guess against a kept quadratic factorization, end to end (bit_assert, copy, add, search_one), n = 128 and 256:
   the int front-end (QuadraticSystem.bit_assert + FactoredSystem), the packed one (PackedQuadraticSystem.factor), and
   PackedQuadraticSystem.search_one afresh on base + guess.  search_one, not solve_one: the base is short of full rank by n / 2
   rows, and solve_one's host walk stops at dimension 16 where the search does not; all three paths make the same call.  The
   base is factored before the first guess (a solve on it), so copy and add run on the device.  The int front-end is skipped at
   n = 256 (its base system cannot be written down); a size whose factorization the device refuses is reported as such.
2. MT19937 at 1 and 32 bits per output: PackedLinearSystem.factor + solve_one against LinearSystem.factor + solve_one,
   generation included.
3. 8 / 32 quadratic systems at n = 128 through solve_one_many against a loop of solve_one.
--small: n = 24 / 40, 1 repetition -- a check that the tool runs, not a measurement."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, as in the tests)

from gf2bv_amd import LinearSystem, PackedLinearSystem, PackedQuadBitVec, PackedQuadraticSystem, QuadraticSystem, hip  # noqa: E402
from gf2bv_amd.packed import _popcount64  # noqa: E402
from tests.harness_models import MT19937  # noqa: E402

from gf2bv_amd.factored import FactoredSystem, PackedFactoredSystem, PackedQuadFactoredSystem  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "packed_factor_time.txt")
LINES = []
LIB = [0.0]                                            # seconds inside library calls since it was last reset


def in_library(fn):
    """fn with its wall time added to LIB (calls do not nest: each wrapped function is a leaf above the library)"""
    def timed(*args, **kwargs):
        t0 = time.perf_counter()
        try:
            return fn(*args, **kwargs)
        finally:
            LIB[0] += time.perf_counter() - t0
    return timed


def timed_class(base):
    """`base` with the methods that call the library timed: making a factorization, appending to one, copying the handles (the
    bookkeeping of a copy is a dict update), solving against one"""
    class Timed(base):
        _factor = in_library(base._factor)
        _append_to = in_library(base._append_to)
        copy = in_library(base.copy)

        def _solve(self, values_list, mode):
            rhs = self.rhs_words(values_list)
            if rhs.shape[0] == 0:
                return []
            return in_library(self._handle(mode).solve)(rhs)
    return Timed


def timed_system(system):
    """the system's own calls into the library, on this instance: the fresh solves and the quadratic search"""
    for name in ("_solve_internal", "_solve_internal_many", "_search_space"):
        if hasattr(system, name):
            setattr(system, name, in_library(getattr(system, name)))
    return system


def say(line: str):
    print(line, flush=True)
    LINES.append(line)


def med(fn, reps: int):
    """median wall time and median library time of `reps` calls after one warm call, and the last result"""
    res = fn()
    ts, ls = [], []
    for _ in range(reps):
        LIB[0] = 0.0
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
        ls.append(LIB[0])
    return statistics.median(ts), statistics.median(ls), res


def planted_terms(n: int, rows: int, seed: int):
    """`rows` factored equations -- one product of dense forms plus a dense linear form each -- that vanish at a planted secret"""
    rng = np.random.default_rng(seed)
    wl = (n + 1 + 63) // 64

    def forms(count):
        f = rng.integers(0, 1 << 64, size=(count, wl), dtype=np.uint64)
        if (n + 1) & 63:
            f[:, -1] &= np.uint64((1 << ((n + 1) & 63)) - 1)
        f[:, 0] &= np.uint64(~1 & (2 ** 64 - 1))                           # constant-free
        return f
    lin, ta, tb = forms(rows), forms(rows), forms(rows)
    secret = int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1)
    point = np.frombuffer((secret << 1).to_bytes(8 * wl, "little"), dtype=np.uint64)
    par = lambda f: (_popcount64(f & point[None, :]).sum(axis=1) & 1).astype(np.uint64)      # noqa: E731
    lin[:, 0] |= par(lin) ^ (par(ta) & par(tb))
    return lin, np.arange(rows + 1, dtype=np.int64), ta, tb, secret


def as_int_exprs(q: QuadraticSystem, lin, ta, tb):
    """the same equations written out on the int front-end (one mul_bit per row)"""
    ints = lambda a: [int.from_bytes(r.tobytes(), "little") for r in a]    # noqa: E731
    return [e ^ q._mul_bit(a, b) for e, a, b in zip(ints(lin), ints(ta), ints(tb))]


def case_guess(n: int, reps: int, with_int: bool):
    cols = hip.quad_cols(n)
    rows = cols - n // 2                                                   # short of full rank: the guess has something to add
    lin, off, ta, tb, secret = planted_terms(n, rows, 100 + n)
    p = timed_system(PackedQuadraticSystem([n]))
    (y,) = p.gens()
    base = [PackedQuadBitVec(lin, off, ta, tb, n)]
    guesses = [(y[i], (secret >> i) & 1) for i in range(reps + 1)]
    try:
        t0 = time.perf_counter()
        fs = timed_class(PackedQuadFactoredSystem)(p, base)
        fs._handle(1)                                                      # factored before the first guess: copy and add run on the device
        t_factor = time.perf_counter() - t0
    except (RuntimeError, MemoryError) as e:
        say(f"guess n {n}: the factorization did not fit or failed ({str(e)[:80]}): skipped")
        return
    it = iter(guesses * 2)

    def packed_guess():
        a, v = next(it)
        with fs.copy() as g:
            g.add(p.bit_assert(a, v))
            return g.search_one([0] * g._nspans)

    def packed_fresh():
        a, v = next(it)
        return p.search_one(base + p.bit_assert(a, v))
    tp, lp, sol = med(packed_guess, reps)
    it = iter(guesses * 2)
    tf, lf, sol2 = med(packed_fresh, reps)
    fs.close()
    line = (f"guess n {n} ({rows} x {cols}): packed factor once {t_factor * 1e3:8.1f} ms; per guess (bit_assert + copy + add + search_one), wall / of it library: "
            f"packed kept {tp * 1e3:8.2f} / {lp * 1e3:8.2f} ms, packed afresh (search_one on base + guess) {tf * 1e3:8.2f} / {lf * 1e3:8.2f} ms")
    assert sol == sol2, (sol, sol2)
    if with_int:
        q = timed_system(QuadraticSystem([n]))
        (x,) = q.gens()
        t0 = time.perf_counter()
        exprs = as_int_exprs(q, lin, ta, tb)
        t_gen = time.perf_counter() - t0
        fq = timed_class(FactoredSystem)(q, exprs)
        fq._handle(1)
        it = iter([(x[i], (secret >> i) & 1) for i in range(reps + 1)] * 2)

        def int_guess():
            a, v = next(it)
            with fq.copy() as g:
                g.add(q.bit_assert(a, v))
                return g.search_one([0] * g._nspans)
        ti, li, sol3 = med(int_guess, reps)
        fq.close()
        assert sol3 == sol, (sol3, sol)
        line += f", int kept {ti * 1e3:8.2f} / {li * 1e3:8.2f} ms (writing the base system's {rows} rows on the host: {t_gen:6.2f} s, once)"
    say(line + f"; answer {'the planted secret' if sol == (secret,) else sol}")


def case_mt(bits: int, reps: int, outputs=None):
    n_out = 19968 // bits + (0 if bits == 32 else 64) if outputs is None else outputs
    r = random.Random(3142)
    state = tuple(r.getstate()[1][:-1])
    out = [r.getrandbits(bits) for _ in range(n_out)] + [0x80000000]

    def run(cls):
        t0 = time.perf_counter()
        lin = cls([32] * 624)
        sym = MT19937(lin.gens())
        exprs = [sym.getrandbits(bits) for _ in range(n_out)] + [lin.gens()[0]]
        t1 = time.perf_counter()
        LIB[0] = 0.0
        with timed_class(PackedFactoredSystem if cls is PackedLinearSystem else FactoredSystem)(lin, exprs) as fs:
            sol = fs.solve_one(out)
            t2, l2 = time.perf_counter(), LIB[0]
            again = fs.solve_one(out)
            t3, l3 = time.perf_counter(), LIB[0]
        assert sol == again
        return sol, t1 - t0, t2 - t1, t3 - t2, l2, l3 - l2
    res = {}
    for name, cls in (("packed", PackedLinearSystem), ("int", LinearSystem)):
        runs = [run(cls) for _ in range(reps + 1)][1:]
        res[name] = runs[-1][0]
        g, f, s, lf, ls = (statistics.median(r[k] for r in runs) for k in (1, 2, 3, 4, 5))
        say(f"mt19937 {bits:2d} bits/output, {n_out} outputs, {name:6s} front-end, wall / of it library: generate {g * 1e3:8.1f} / 0 ms, factor + first solve_one "
            f"{f * 1e3:8.1f} / {lf * 1e3:8.1f} ms, next solve_one {s * 1e3:7.2f} / {ls * 1e3:7.2f} ms, total {(g + f) * 1e3:8.1f} ms; state {'recovered' if res[name] == state else 'NOT recovered'}")
    assert res["packed"] == res["int"]


def case_many(n: int, counts, reps: int):
    cols = hip.quad_cols(n)
    p = timed_system(PackedQuadraticSystem([n]))
    for nsys in counts:
        systems, secrets = [], []
        for s in range(nsys):
            lin, off, ta, tb, secret = planted_terms(n, cols + 64, 1000 * n + s)
            systems.append([PackedQuadBitVec(lin, off, ta, tb, n)])
            secrets.append((secret,))
        try:
            tm, lm, many = med(lambda: p.solve_one_many(systems), reps)
        except RuntimeError as e:
            say(f"many n {n} x {nsys}: the batch did not fit or failed ({str(e)[:80]}): skipped")
            continue
        tl, ll, loop = med(lambda: [p.solve_one(z) for z in systems], reps)
        assert many == loop, "solve_one_many and the loop disagree"
        say(f"many n {n} ({cols + 64} x {cols}) x {nsys} systems: wall / of it library: solve_one_many {tm * 1e3:8.1f} / {lm * 1e3:8.1f} ms, a loop of solve_one {tl * 1e3:8.1f} / {ll * 1e3:8.1f} ms; "
            f"{sum(a == b for a, b in zip(many, secrets))} of {nsys} planted secrets")


if __name__ == "__main__":
    small = "--small" in sys.argv
    say(f"tools/packed_factor_time.py{' --small' if small else ''} on one {torch.cuda.get_device_name(0)} (build {hip.build_id()}).")
    reps = 1 if small else 5
    for n, with_int in ((24, True), (40, False)) if small else ((128, True), (256, False)):
        case_guess(n, reps, with_int)
    for bits in (32, 1):
        case_mt(bits, 1 if small else 3)
    case_many(24 if small else 128, (8, 32), reps)
    if not small:
        with open(OUT, "w") as f:
            f.write("\n".join(LINES) + "\n")
