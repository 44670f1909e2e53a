"""Equations appended to a kept factorization (gf2bv_factor_append_*): one JSON line, append against factoring the stacked matrix.
  mt19937: the MT19937 recovery (bs = 32 and bs = 1), a handle one output short of full rank (the mt[0] row and all outputs but
           the last): append 1 output, and 64 outputs, each on a copy of that handle, plus the first solve after the append;
           next to factoring the stacked rows afresh and the copy itself.
  synth:   the 65536^2 bench system with its last 512 rows zeroed, factored; append 64 and 512 of the original rows from the device
           (each on a copy), the first solve after it, copy(); next to factoring the stacked 65536 + k rows afresh.
GF2BV_TRACE=1 prints the phase split of every append (grow, reduce, new pivots, merge, mode-1 basis) on stderr.
usage: factor_append_time.py [--reps R] [--out FILE] [--only mt|synth]"""
import argparse, json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process, as bench.py)
import numpy as np  # noqa: E402
from gf2bv_amd import LinearSystem, _internal, hip  # noqa: E402
from tests.harness_models import MT19937  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def mt_case(bs, reps):
    lin = LinearSystem([32] * 624)
    mt = lin.gens()
    sym = MT19937(mt)
    samples = 624 * 32 // bs
    outs = [sym.getrandbits(bs) for _ in range(samples + 64)]
    rand = random.Random(3142)
    state = tuple(rand.getstate()[1][:-1])
    values = [rand.getrandbits(bs) for _ in range(samples + 64)]
    cols = lin._cols
    base_exprs = [mt[0]] + outs[:samples - 1]
    res = {"bs": bs}
    fs = lin.factor(base_exprs)
    fs.solve_one([0x80000000] + values[:samples - 1])                       # (the handle exists)
    res["rank_before"] = fs._handles[0].rank
    for k in (1, 64):
        new = outs[samples - 1:samples - 1 + k]
        vals = [0x80000000] + values[:samples - 1 + k]
        t_app, t_solve, t_copy = [], [], []
        for _ in range(reps):
            c, tc = timed(fs.copy)
            _, ta = timed(lambda: c.add(new))
            sol, ts = timed(lambda: c.solve_one(vals))
            assert sol == state, "known answer"
            t_app.append(ta); t_solve.append(ts); t_copy.append(tc)
            c.close()
        eqs = lin._rhs_eqs(base_exprs + new, [])[0]
        eqs += [0] * max(0, cols - len(eqs))
        _internal.m4ri_factor(eqs, cols, 0).close()                          # warm-up
        t_fresh = []
        for _ in range(reps):
            h, tf = timed(lambda: _internal.m4ri_factor(eqs, cols, 0))
            h.close()
            t_fresh.append(tf)
        res[f"k{k}_outputs"] = {"rows_added": len(lin._rhs_eqs(new, [])[0]), "append_ms": min(t_app), "first_solve_ms": min(t_solve),
                                "copy_ms": min(t_copy), "fresh_factor_ms": min(t_fresh)}
    fs.close()
    return res


def synth_case(reps, n=65536, seed=1234):
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n + 512, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    torch.cuda.synchronize()
    A[n:] = A[n - 512:n]
    A[n - 512:n] = 0
    torch.cuda.synchronize()
    planted = hip.planted_solution(n, seed)
    f = hip.factor_device(A.data_ptr(), n, n, stride, 0)
    res = {"n": n, "rank_before": f.rank, "device_bytes_before": f.device_bytes}
    rw = (n + 512 + 63) // 64
    b = ((A[:, n // 64] >> (n % 64)) & 1)
    weights = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64, device=dev)
    pad = torch.zeros(rw * 64, dtype=torch.int64, device=dev)
    pad[:n + 512] = b
    rhs = (pad.view(rw, 64) * weights).sum(dim=1).view(1, rw).contiguous()
    torch.cuda.synchronize()
    for k in (64, 512):
        t_app, t_solve, t_copy = [], [], []
        for _ in range(reps):
            c, tc = timed(f.copy)
            _, ta = timed(lambda: c.append_device(A[n:n + k].data_ptr(), k, stride))
            r, ts = timed(lambda: c.solve_device(rhs.data_ptr(), 1, (n + k + 63) // 64)[0])
            t_app.append(ta); t_solve.append(ts); t_copy.append(tc)
            if k == 512:
                assert r.status == 0 and np.array_equal(r.origin, planted), "known answer"
            rank = c.rank
            dbytes = c.device_bytes
            c.close()
        t_fresh = []
        for _ in range(reps):
            g, tf = timed(lambda: hip.factor_device(A.data_ptr(), n + k, n, stride, 0))
            g.close()
            t_fresh.append(tf)
        res[f"k{k}"] = {"append_ms": min(t_app), "first_solve_ms": min(t_solve), "copy_ms": min(t_copy), "fresh_factor_ms": min(t_fresh),
                        "rank_after": rank, "device_bytes_after": dbytes}
    f.close()
    del A, rhs, pad, b
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("mt", "synth"), default=None)
    a = ap.parse_args()
    out = {"tool": "factor_append_time", "build": hip.build_id(), "device": torch.cuda.get_device_name(0)}
    if a.only != "synth":
        out["mt19937"] = [mt_case(bs, a.reps) for bs in (32, 1)]
    if a.only != "mt":
        out["synth"] = synth_case(a.reps)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
