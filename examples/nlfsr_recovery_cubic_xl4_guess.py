"""State recovery of a register whose output filter has a cubic term, from 62 outputs: hybrid degree-4 XL on the packed cubic
front-end (PackedCubicGuessSystem.solve_all_xl4_guess).

The register is the one of nlfsr_recovery_cubic_xl4.py: n = 16 state bits, z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15 each clock, taps 0xB400.
Degree-4 XL needs 149 outputs there (2533 rows over the 2516 monomials of degree <= 4 in 16 unknowns), plain linearisation 696.  Here
the top four state bits are guessed.  Each of the 16 assignments leaves the same 62 cubic equations in 12 unknowns: the GPU
substitutes the guesses into the expanded rows, multiplies every system's equations by 1 and by each of the 12 unknowns -- 806 rows
over 793 monomials -- and solves all 16 systems as one batch.  Only the secret's assignment is consistent, with the secret as its one
solution, while solve_all_xl4 on the same 62 outputs has 1054 rows for 2516 columns and refuses.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import DimensionTooLargeError, PackedCubicGuessSystem
from gf2bv_amd.linsys import xl4_cols

from nlfsr_recovery_cubic_xl4 import N_BITS, SELECT, keystream, step

GUESS = range(12, 16)


def recover(secret, count=62):
    stream = keystream(secret, count)
    t0 = time.perf_counter()
    csys = PackedCubicGuessSystem([N_BITS])
    (x,) = csys.gens()
    s, zero, zeros = [x[g] for g in range(N_BITS)], x[0] ^ x[0], []
    for bit in stream:
        a, b, c, d, e, f = [s[i] for i in SELECT]
        zeros.append(a ^ csys.mul_bit(b, c) ^ csys.mul_bit(csys.mul_bit(d, e), f) ^ bit)
        s = step(s, zero)
    guess = [x[g] for g in GUESS]                      # the state bits themselves; their indices would do as well
    t1 = time.perf_counter()
    sols = list(csys.solve_all_xl4_guess(zeros, guess))
    t2 = time.perf_counter()
    assert sols == [(secret,)], sols
    assert csys.solve_one_xl4_guess(zeros, guess) == (secret,)
    try:
        list(csys.solve_all_xl4(zeros))
        plain = "solved"
    except DimensionTooLargeError as err:
        plain = f"DimensionTooLargeError, dimension {err.space.dimension}"
    assert plain.startswith("DimensionTooLargeError")
    rest = N_BITS - len(guess)
    print(f"{len(zeros)} cubic equations, {len(guess)} bits guessed: {1 << len(guess)} systems of {len(zeros) * (rest + 1)} rows x {xl4_cols(rest)} "
          f"unknowns: generate {t1 - t0:.2f}s  solve_all_xl4_guess {t2 - t1:.3f}s  secret {sols[0][0]:#06x}  ok;  solve_all_xl4 on the same "
          f"outputs: {plain}")
    return secret


if __name__ == "__main__":
    recover(0x52E7)
    recover(0x3A09)
