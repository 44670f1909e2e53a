"""A filtered LFSR recovered from too few outputs for plain linearisation: degree-3 XL (PackedQuadraticSystem.solve_all_xl).

A 32-bit Galois register behind the filter of examples/nlfsr_recovery.py.  360 output bits give 197 annihilator equations; the
528 columns of the linearised system would need about 528 of them, so its solution space has dimension 331 and solve_all gives up.
Multiplied by 1 and by each of the 32 unknowns on the GPU the same equations are 6501 rows over the 5488 monomials of degree <= 3,
of full rank: the secret is the only solution.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import DimensionTooLargeError, PackedQuadraticSystem
from tests.harness_models import GaloisLFSR

from nlfsr_recovery import filter_bit

N_BITS, TAPS = 32, 0x80200003
SELECT = (3, 9, 15, 21, 27)
OUTPUTS = 360


def recover(seed=1):
    secret = random.Random(seed).getrandbits(N_BITS) | 1
    reg, stream = GaloisLFSR(N_BITS, TAPS, secret), []
    for _ in range(OUTPUTS):
        reg()
        stream.append(filter_bit(*[(reg.state >> i) & 1 for i in SELECT]))
    qsys = PackedQuadraticSystem([N_BITS])
    (x,) = qsys.gens()
    sym = GaloisLFSR(N_BITS, TAPS, x)
    zeros = []
    for bit in stream:
        sym()
        if bit:
            x0, x1, x2, _, _ = [sym.state[i] for i in SELECT]
            zeros.append(qsys.mul_bit(x0, x1) ^ x0 ^ qsys.mul_bit(x1, x2) ^ x1 ^ x2 ^ 1)
    try:
        list(qsys.solve_all(zeros))
        raise AssertionError("plain linearisation should not pin the secret down from so few outputs")
    except DimensionTooLargeError as e:
        dim = e.space.dimension
    t0 = time.perf_counter()
    sols = list(qsys.solve_all_xl(zeros))
    t1 = time.perf_counter()
    assert sols == [(secret,)], len(sols)
    assert qsys.solve_one_xl(zeros) == (secret,)
    print(f"{len(zeros)} equations from {OUTPUTS} outputs: linearised space of dimension {dim} (solve_all gives up); "
          f"degree-3 XL, {len(zeros) * (N_BITS + 1)} rows: solve_all_xl {t1 - t0:.3f}s  ok")
    return secret


if __name__ == "__main__":
    recover()
