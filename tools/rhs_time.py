"""Many right-hand sides of one matrix (gf2bv_solve_rhs_*): one JSON line.
  mt19937: n instances of the MT19937 recovery (examples/mt_recovery.py, bs = 32 and bs = 1) -- LinearSystem.solve_one_rhs (one
           elimination) against solve_one_many (lock-step gangs) and a loop of solve_one; ms in all and per instance (best of
           `reps`, warm), plus the phase times of the shared solve (the words entry on the same matrix).
  synth:   the 65536^2 bench system on the device with nrhs right-hand sides (gf2bv_solve_rhs_device) against one gf2bv_solve_device.
usage: rhs_time.py [--reps R] [--out FILE]"""
import argparse, json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (first: one HIP runtime per process, as bench.py)
import numpy as np  # noqa: E402
from gf2bv_amd import LinearSystem, hip  # noqa: E402
from tests.harness_models import MT19937  # noqa: E402

PHASES = ("ms_pack", "ms_eliminate", "ms_backsub", "ms_export", "ms_total")


def best(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, min(ts)


def mt_case(bs, ns, reps):
    lin = LinearSystem([32] * 624)
    mt = lin.gens()
    sym = MT19937(mt)
    eff = ((bs - 1) & bs) or bs
    samples = 624 * 32 // eff
    exprs = [sym.getrandbits(bs) for _ in range(samples)] + [mt[0]]
    cols = lin._cols
    rows_out = []
    for n in ns:
        values, states = [], []
        for s in range(n):
            rand = random.Random(3142 + s)
            states.append(tuple(rand.getstate()[1][:-1]))
            values.append([rand.getrandbits(bs) for _ in range(samples)] + [0x80000000])
        zeros_list = [[e ^ v for e, v in zip(exprs, vals)] for vals in values]
        lin.solve_one_rhs(exprs, values[:1])                                     # warm-up (pool, code objects)
        rhs_res, t_rhs = best(lambda: lin.solve_one_rhs(exprs, values), reps)
        many_res, t_many = best(lambda: lin.solve_one_many(zeros_list), reps)
        loop_res, t_loop = best(lambda: [lin.solve_one(z) for z in zeros_list], min(reps, 2))
        ok = rhs_res == many_res == loop_res == states
        # phases of the shared solve: the words entry on the same matrix and right-hand sides
        eqs, rhs_ints = lin._rhs_eqs(exprs, values)
        eqs += [0] * max(0, cols - len(eqs))
        rows = len(eqs)
        stride = (cols + 1 + 63) // 64
        aug = np.frombuffer(b"".join(((e >> 1) | ((e & 1) << cols)).to_bytes(stride * 8, "little") for e in eqs),
                            dtype=np.uint64).reshape(rows, stride)
        rw = (rows + 63) // 64
        rhs = np.frombuffer(b"".join(b.to_bytes(rw * 8, "little") for b in rhs_ints), dtype=np.uint64).reshape(n, rw)
        st = hip.solve_rhs_words(aug, rows, cols, rhs, 0)[0].stats
        rows_out.append({"bs": bs, "n": n, "rows": rows, "cols": cols, "ok": ok,
                         "solve_one_rhs_ms": round(t_rhs, 2), "solve_one_rhs_ms_per": round(t_rhs / n, 3),
                         "solve_one_many_ms": round(t_many, 2), "solve_one_many_ms_per": round(t_many / n, 3),
                         "solve_one_loop_ms": round(t_loop, 2), "solve_one_loop_ms_per": round(t_loop / n, 3),
                         "rhs_phases": {k: round(st[k], 3) for k in PHASES}})
        print(json.dumps(rows_out[-1]), file=sys.stderr, flush=True)
    return rows_out


def synth_case(nrhs_list, reps):
    n, seed = 65536, 1234
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    rw = (n + 63) // 64
    rng = np.random.default_rng(7)
    torch.cuda.synchronize()
    singles = [hip.solve_device(A.data_ptr(), n, n, stride, 0) for _ in range(reps + 1)][1:]
    one = min(singles, key=lambda s: s.stats["ms_total"]).stats
    out = {"rows": n, "cols": n, "single": {k: round(one[k], 3) for k in PHASES}, "rhs": []}
    for nrhs in nrhs_list:
        rhs = torch.from_numpy(rng.integers(0, 2 ** 64, (nrhs, rw), dtype=np.uint64).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        runs = [hip.solve_rhs_device(A.data_ptr(), n, n, stride, rhs.data_ptr(), nrhs, rw, 0) for _ in range(reps + 1)][1:]
        r = min(runs, key=lambda rs: rs[0].stats["ms_total"])
        st = r[0].stats
        out["rhs"].append({"nrhs": nrhs, **{k: round(st[k], 3) for k in PHASES},
                           "ratio_to_single": round(st["ms_total"] / one["ms_total"], 3),
                           "all_solved": all(s.status == 0 for s in r)})
        print(json.dumps(out["rhs"][-1]), file=sys.stderr, flush=True)
        del rhs
    del A
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "rhs_time", "build": hip.build_id(),
           "mt19937": mt_case(32, (1, 8, 32, 64), a.reps) + mt_case(1, (1, 8, 32, 64), a.reps),
           "synth_65536": synth_case((1, 64, 512), a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
