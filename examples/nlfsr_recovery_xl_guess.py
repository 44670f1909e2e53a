"""A filtered LFSR recovered from too few outputs even for degree-3 XL: hybrid XL (PackedQuadraticSystem.solve_all_xl_guess).

A 40-bit Galois register behind the filter of examples/nlfsr_recovery.py.  380 output bits give 188 annihilator equations.  Degree-3
XL makes 7708 rows of them over the 10700 monomials of degree <= 3 in 40 unknowns: a space of dimension 2992 at the least, and
solve_all_xl gives up.  With the top 8 state bits guessed, each of the 256 assignments leaves the same 188 equations in 32 unknowns:
6204 rows over 5488 monomials.  On the CPU oracle the right assignment's system has full rank 5488 (with 340 outputs, 170 equations,
it has rank 5269: too few).  The GPU substitutes the guesses, multiplies and solves all 256 systems as one batch; the secret is the
only solution.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import DimensionTooLargeError, PackedQuadraticSystem
from tests.harness_models import GaloisLFSR

from nlfsr_recovery import filter_bit

N_BITS, TAPS = 40, 0xA000140000                        # x^40 + x^38 + x^21 + x^19 + 1
SELECT = (3, 11, 19, 27, 35)
OUTPUTS = 380
GUESS = range(32, 40)


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
        list(qsys.solve_all_xl(zeros))
        raise AssertionError("degree-3 XL should not pin the secret down from so few outputs")
    except DimensionTooLargeError as e:
        dim = e.space.dimension
    guess = [x[i] for i in GUESS]                      # the state bits themselves; their indices would do as well
    t0 = time.perf_counter()
    sols = list(qsys.solve_all_xl_guess(zeros, guess))
    t1 = time.perf_counter()
    assert sols == [(secret,)], len(sols)
    assert qsys.solve_one_xl_guess(zeros, guess) == (secret,)
    print(f"{len(zeros)} equations from {OUTPUTS} outputs: degree-3 XL leaves a space of dimension {dim} (solve_all_xl gives up); "
          f"{len(guess)} bits guessed, {1 << len(guess)} systems of {len(zeros) * (N_BITS - len(guess) + 1)} rows: "
          f"solve_all_xl_guess {t1 - t0:.3f}s  ok")
    return secret


if __name__ == "__main__":
    recover()
