"""A filtered LFSR recovered from fewer outputs than degree-3 XL needs: degree-4 XL (PackedQuadraticSystem.solve_all_xl4).

The 16-bit Galois register of tests/test_gpu_xl.py behind the filter of examples/nlfsr_recovery.py.  Degree-3 XL needs 140 output
bits (79 annihilator equations, rank 696 of 696).  The first 44 give 29 equations: multiplied by 1 and by each unknown they are 493
rows of rank 435 over the 696 monomials of degree <= 3, a space of dimension 261, and solve_all_xl gives up.  Multiplied also by each
of the 120 pairs of unknowns on the GPU they are 29 * 137 = 3973 rows of rank 2507 over the 2516 monomials of degree <= 4: a space of
dimension 9, whose 512 points hold the 10 states at which the 29 equations vanish (they use only the outputs that are 1); running
the register from each leaves the secret as the only one that produces all 44 bits.
(The 32-bit register of nlfsr_recovery_xl.py has 41448 quartic columns and 529 rows an equation; the CPU oracle that fixes the numbers
above did not settle its output count in reasonable time, so this example stays at 16 bits.)
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import DimensionTooLargeError, PackedQuadraticSystem
from tests.harness_models import GaloisLFSR

from nlfsr_recovery import filter_bit

N_BITS, TAPS = 16, 0xB400
SELECT = (1, 4, 7, 10, 13)
OUTPUTS = 44


def recover(seed=16):
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
        list(qsys.solve_all_xl(zeros))
        raise AssertionError("degree-3 XL should not pin the secret down from so few outputs")
    except DimensionTooLargeError as e:
        dim3 = e.space.dimension
    t0 = time.perf_counter()
    dim4 = qsys.solve_raw_space_xl4(zeros).dimension
    sols = list(qsys.solve_all_xl4(zeros))
    t1 = time.perf_counter()
    assert (secret,) in sols, len(sols)

    def produces(state):
        reg = GaloisLFSR(N_BITS, TAPS, state)
        for bit in stream:
            reg()
            if filter_bit(*[(reg.state >> i) & 1 for i in SELECT]) != bit:
                return False
        return True
    assert [sol for sol in sols if produces(sol[0])] == [(secret,)]
    rows = len(zeros) * (1 + N_BITS + N_BITS * (N_BITS - 1) // 2)
    print(f"{len(zeros)} equations from {OUTPUTS} outputs: degree-3 XL leaves dimension {dim3} (solve_all_xl gives up); "
          f"degree-4 XL, {rows} rows: dimension {dim4}, {len(sols)} common zeros, one of them produces the outputs: solve_all_xl4 {t1 - t0:.3f}s  ok")
    return secret


if __name__ == "__main__":
    recover()
