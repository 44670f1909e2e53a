"""examples/nlfsr_recovery_packed.py with the register stepped on the GPU (unroll).

Same experiment, same assertions.  The host steps the symbolic register ONCE; that step is an affine map of the 128 state bits, and
the five filter inputs at every later time are those five bits with the map substituted again and again -- `unroll`, 15 doublings on
the device for 17384 time steps.  What stays on the host is what depends on the observed keystream: one equation per output bit 1,
built from that time's five rows.  The first 256 unrolled rows are compared with the rows the host gets by stepping.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gf2bv_amd import PackedQuadraticSystem, unroll
from tests.harness_models import FibonacciLFSR, GaloisLFSR

from nlfsr_recovery import N_BITS, SELECT, TAPS, keystream

CHECKED = 256


def equation(qsys, x0, x1, x2):
    return qsys.mul_bit(x0, x1) ^ x0 ^ qsys.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1


def host_stepping(kind, qsys, x, stream):
    """what nlfsr_recovery_packed.py does: (the equations, the five tap bits of every time step) by stepping the symbolic register"""
    sym = kind(N_BITS, TAPS, x)
    zeros, rows = [], []
    for bit in stream:
        sym()
        taps = [sym.state[i] for i in SELECT]
        rows.append(taps)
        if bit:
            zeros.append(equation(qsys, *taps[:3]))
    return zeros, rows


def recover(kind, seed, count=2 ** 14 + 1000, time_host=True):
    secret = random.Random(seed).getrandbits(N_BITS)
    stream = keystream(kind(N_BITS, TAPS, secret), count)
    t0 = time.perf_counter()
    qsys = PackedQuadraticSystem([N_BITS])
    (x,) = qsys.gens()
    sym = kind(N_BITS, TAPS, x)
    sym()                                                  # one symbolic step: the map
    taps = unroll([x[i] for i in SELECT], (sym.state,), count, start=1)
    t1 = time.perf_counter()
    zeros = [equation(qsys, *taps[t][:3]) for t, bit in enumerate(stream) if bit]
    t2 = time.perf_counter()
    sols = list(qsys.solve_all(zeros))
    t3 = time.perf_counter()
    assert sols == [(secret,)], (kind.__name__, len(sols))
    assert qsys.solve_one(zeros) == (secret,)
    # the host's own stepping: the whole stream for its time, its first steps for the comparison
    t4 = time.perf_counter()
    _, rows = host_stepping(kind, qsys, x, stream if time_host else stream[:CHECKED])
    t5 = time.perf_counter()
    checked = min(CHECKED, count)
    for t in range(checked):
        assert all(np.array_equal(u._rows, h._rows) for u, h in zip(taps[t], rows[t])), (kind.__name__, t)
    host = f"host stepping {t5 - t4:.2f}s" if time_host else f"host stepping not timed ({checked} steps)"
    print(f"{kind.__name__:14s} {len(zeros)} equations x {qsys._cols} unknowns: generate {t2 - t0:.2f}s (unroll {t1 - t0:.3f}s, equations {t2 - t1:.2f}s; "
          f"{host})  solve_all {t3 - t2:.3f}s  first {checked} tap rows equal  ok")
    return secret


if __name__ == "__main__":
    recover(GaloisLFSR, 1)
    recover(FibonacciLFSR, 2)
