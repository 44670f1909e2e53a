"""A kept factorization (gf2bv_factor_*): one JSON line.
  mt19937: the MT19937 recovery (examples/mt_recovery.py, bs = 32 and bs = 1): factor time, then one solve of n instances through
           FactoredSystem.solve_one_rhs (host wall time, and the library's phase times of a handle solve on the same right-hand
           sides) next to LinearSystem.solve_one_rhs (one fresh elimination) and solve_one_many from the same run.
  synth:   the 65536^2 bench system on the device: factor time, then 1 and 64 right-hand sides through the handle against
           gf2bv_solve_rhs_device; the device memory the handles hold.
usage: factor_time.py [--reps R] [--out FILE]"""
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
    samples = 624 * 32 // bs
    exprs = [sym.getrandbits(bs) for _ in range(samples)] + [mt[0]]
    cols = lin._cols
    values, states = [], []
    for s in range(max(ns)):
        rand = random.Random(3142 + s)
        states.append(tuple(rand.getstate()[1][:-1]))
        values.append([rand.getrandbits(bs) for _ in range(samples)] + [0x80000000])
    lin.factor(exprs).solve_one_rhs(values[:1])                                # warm-up (pool, code objects)
    fs, t_factor = best(lambda: lin.factor(exprs), 1)
    t0 = time.perf_counter()
    fs.solve_one_rhs(values[:1])                                               # the handle is made on the first solve
    t_first = 1e3 * (time.perf_counter() - t0)
    # the words of the factored matrix for the phase times of a handle solve (hip.Factor on the same matrix)
    eqs = fs._eqs
    stride = (cols + 1 + 63) // 64
    aug = np.frombuffer(b"".join((e >> 1).to_bytes(stride * 8, "little") for e in eqs), dtype=np.uint64).reshape(len(eqs), stride)
    t0 = time.perf_counter()
    hf = hip.factor_words(aug, len(eqs), cols, 0)
    t_factor_words = 1e3 * (time.perf_counter() - t0)
    out = {"bs": bs, "rows": len(eqs), "cols": cols, "factor_ms": round(t_factor_words, 2),
           "factor_then_first_solve_ms": round(t_factor + t_first, 2), "device_bytes": hf.device_bytes, "solves": []}
    for n in ns:
        vals = values[:n]
        zeros_list = [[e ^ v for e, v in zip(exprs, vv)] for vv in vals]
        got, t_handle = best(lambda: fs.solve_one_rhs(vals), reps)
        rhs_res, t_rhs = best(lambda: lin.solve_one_rhs(exprs, vals), reps)
        many_res, t_many = best(lambda: lin.solve_one_many(zeros_list), min(reps, 2))
        words = fs.rhs_words(vals)
        _, t_words = best(lambda: fs.rhs_words(vals), reps)
        runs = [hf.solve(words) for _ in range(reps)]
        st = min(runs, key=lambda r: r[0].stats["ms_total"])[0].stats
        out["solves"].append({"n": n, "ok": got == rhs_res == many_res == states[:n],
                              "handle_ms": round(t_handle, 3), "handle_ms_per": round(t_handle / n, 3),
                              "rhs_words_ms": round(t_words, 3),
                              "handle_phases": {k: round(st[k], 3) for k in PHASES},
                              "solve_one_rhs_ms": round(t_rhs, 2), "solve_one_many_ms": round(t_many, 2)})
        print(json.dumps(out["solves"][-1]), file=sys.stderr, flush=True)
    hf.close()
    fs.close()
    return out


def synth_case(nrhs_list, reps):
    n, seed = 65536, 1234
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    rw = (n + 63) // 64
    rng = np.random.default_rng(7)
    torch.cuda.synchronize()
    hip.factor_device(A.data_ptr(), n, n, stride, 0).close()                   # warm-up
    t0 = time.perf_counter()
    f = hip.factor_device(A.data_ptr(), n, n, stride, 0)
    t_factor = 1e3 * (time.perf_counter() - t0)
    out = {"rows": n, "cols": n, "factor_ms": round(t_factor, 2), "device_bytes": f.device_bytes, "rhs": []}
    for nrhs in nrhs_list:
        rhs = torch.from_numpy(rng.integers(0, 2 ** 64, (nrhs, rw), dtype=np.uint64).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        fresh = min(([hip.solve_rhs_device(A.data_ptr(), n, n, stride, rhs.data_ptr(), nrhs, rw, 0) for _ in range(reps + 1)])[1:],
                    key=lambda rs: rs[0].stats["ms_total"])
        runs = [f.solve_device(rhs.data_ptr(), nrhs, rw) for _ in range(reps + 1)][1:]
        r = min(runs, key=lambda rs: rs[0].stats["ms_total"])
        st, fst = r[0].stats, fresh[0].stats
        same = all(a.status == b.status and np.array_equal(a.origin, b.origin) for a, b in zip(r, fresh))
        out["rhs"].append({"nrhs": nrhs, "same_as_solve_rhs": same, **{k: round(st[k], 3) for k in PHASES},
                           "solve_rhs_device": {k: round(fst[k], 3) for k in PHASES},
                           "ratio_to_fresh": round(st["ms_total"] / fst["ms_total"], 3)})
        print(json.dumps(out["rhs"][-1]), file=sys.stderr, flush=True)
        del rhs
    f.close()
    del A
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "factor_time", "build": hip.build_id(),
           "mt19937": [mt_case(32, (1, 8, 64), a.reps), mt_case(1, (1, 8, 64), a.reps)],
           "synth_65536": synth_case((1, 64), a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
