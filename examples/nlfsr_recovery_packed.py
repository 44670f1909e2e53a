"""examples/nlfsr_recovery.py through the packed quadratic front-end (PackedQuadraticSystem).

Same experiment, same assertions.  The equations stay factored on the host -- per output bit one linear form and two products
of linear forms over the 128 state bits, three 64-bit words each -- and become rows of the 8664 x 8256 linearised system on the
GPU, so generating them costs the symbolic stepping of the register and nothing per product.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import PackedQuadraticSystem
from tests.harness_models import FibonacciLFSR, GaloisLFSR

from nlfsr_recovery import N_BITS, SELECT, TAPS, keystream


def recover(kind, seed, count=2 ** 14 + 1000):
    secret = random.Random(seed).getrandbits(N_BITS)
    stream = keystream(kind(N_BITS, TAPS, secret), count)
    t0 = time.perf_counter()
    qsys = PackedQuadraticSystem([N_BITS])
    (x,) = qsys.gens()
    sym = kind(N_BITS, TAPS, x)
    zeros = []
    for bit in stream:
        sym()
        if bit:
            x0, x1, x2, _, _ = [sym.state[i] for i in SELECT]
            zeros.append(qsys.mul_bit(x0, x1) ^ x0 ^ qsys.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    t1 = time.perf_counter()
    sols = list(qsys.solve_all(zeros))
    t2 = time.perf_counter()
    assert sols == [(secret,)], (kind.__name__, len(sols))
    assert qsys.solve_one(zeros) == (secret,)
    print(f"{kind.__name__:14s} {len(zeros)} equations x {qsys._cols} unknowns: generate {t1 - t0:.2f}s  solve_all {t2 - t1:.3f}s  ok")
    guess_loop(qsys, x, zeros, secret)
    return secret


def guess_loop(qsys, x, base, secret, bits=(0, 1, 2)):
    """Guesses against a kept factorization: the system is factored ONCE (the first search on `fs` makes the factorization), then
    each state bit is tried both ways on a copy of it.  bit_assert(a, v) is `a = v` and its n - 1 products with the other
    unknowns, kept factored on the host; add expands them on the device and appends them to the copy's factorization.  The base
    system has the secret as its only consistent point, so the right guess finds it again and the wrong one finds none."""
    t0 = time.perf_counter()
    with qsys.factor(base) as fs:
        nothing = [0] * len(base)
        assert fs.search_one(nothing) == (secret,)         # factors the base: what copy() copies from here on
        t1 = time.perf_counter()
        for i in bits:
            found = {}
            for v in (0, 1):
                with fs.copy() as g:                       # a device-to-device copy, no factorization
                    g.add(qsys.bit_assert(x[i], v))        # appended to the copy's factorization
                    found[v] = g.search_one(nothing + [0, 0])
            want = (secret >> i) & 1
            assert found[want] == (secret,) and found[1 - want] is None, (i, found)
    t2 = time.perf_counter()
    print(f"{'':14s} {len(base)} equations factored once in {t1 - t0:.3f}s, {2 * len(bits)} bit_assert guesses on copies in {t2 - t1:.3f}s  ok")

if __name__ == "__main__":
    recover(GaloisLFSR, 1)
    recover(FibonacciLFSR, 2)
