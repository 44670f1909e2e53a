"""State recovery of a register whose output filter has a cubic term, from a fifth of the keystream: degree-4 XL on the packed cubic
front-end (PackedCubicSystem.solve_all_xl4).

The register is the one of nlfsr_recovery_cubic.py: n = 16 state bits, z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15 each clock, taps 0xB400.
Every output is one cubic equation written with mul_bit and kept factored on the host.  Plain linearisation over the
16 + 120 + 560 = 696 monomials of degree <= 3 needs about 696 outputs (that example takes 736).  Here the GPU also multiplies every
equation by each of the 16 unknowns: 149 outputs give 149 x 17 = 2533 rows over the 696 + 1820 = 2516 monomials of degree <= 4, of
rank 2516, and solve_all_xl4 returns the secret alone -- while solve_all on the same 149 outputs is left with a space of dimension
696 - 149 = 547 and refuses.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import DimensionTooLargeError, PackedCubicSystem
from gf2bv_amd.linsys import xl4_cols

N_BITS, TAPS, SELECT = 16, 0xB400, (1, 4, 7, 10, 13, 15)


def step(state, zero):
    """one clock on ints or on symbolic bits: anything with ^"""
    out, moved = state[0], state[1:] + [zero]
    return [moved[g] ^ out if (TAPS >> g) & 1 else moved[g] for g in range(N_BITS)]


def keystream(secret, count):
    s, bits = [(secret >> g) & 1 for g in range(N_BITS)], []
    for _ in range(count):
        bits.append(s[SELECT[0]] ^ (s[SELECT[1]] & s[SELECT[2]]) ^ (s[SELECT[3]] & s[SELECT[4]] & s[SELECT[5]]))
        s = step(s, 0)
    return bits


def recover(secret, count=149):
    stream = keystream(secret, count)
    t0 = time.perf_counter()
    csys = PackedCubicSystem([N_BITS])
    (x,) = csys.gens()
    s, zero, zeros = [x[g] for g in range(N_BITS)], x[0] ^ x[0], []
    for bit in stream:
        a, b, c, d, e, f = [s[i] for i in SELECT]
        zeros.append(a ^ csys.mul_bit(b, c) ^ csys.mul_bit(csys.mul_bit(d, e), f) ^ bit)
        s = step(s, zero)
    t1 = time.perf_counter()
    sols = list(csys.solve_all_xl4(zeros))
    t2 = time.perf_counter()
    assert sols == [(secret,)], sols
    assert csys.solve_one_xl4(zeros) == (secret,)
    try:
        list(csys.solve_all(zeros))
        plain = "solved"
    except DimensionTooLargeError as err:
        plain = f"DimensionTooLargeError, dimension {err.space.dimension}"
    assert plain.startswith("DimensionTooLargeError")
    print(f"{len(zeros)} cubic equations x {N_BITS + 1} multipliers = {len(zeros) * (N_BITS + 1)} rows x {xl4_cols(N_BITS)} unknowns: "
          f"generate {t1 - t0:.2f}s  solve_all_xl4 {t2 - t1:.3f}s  secret {sols[0][0]:#06x}  ok;  solve_all on the same outputs: {plain}")
    return secret


if __name__ == "__main__":
    recover(0x52E7)
    recover(0x3A09)
