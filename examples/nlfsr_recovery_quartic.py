"""State recovery of a register whose output filter has a four-way AND, through the packed quartic front-end (PackedQuarticSystem).

The register is the one of nlfsr_recovery_cubic.py -- n = 16 state bits, taps 0xB400 -- with a fourth filter term: each clock it
outputs z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15 ^ s_2 s_5 s_8 s_12 and then steps.  The state stays linear in the secret, so every output is
one quartic equation written directly with mul_bit -- the four-way AND as the product of two quadratic bits -- and kept factored on the
host: a linear form and one product each of two, three and four linear forms.  The rows over the 16 + 120 + 560 + 1820 = 2516
monomials of degree <= 4 come into being on the GPU, which solves them; 2516 outputs already give rank 2516, and from the 2560 taken
here solve_all returns the secret alone.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import PackedQuarticSystem

N_BITS, TAPS, SELECT = 16, 0xB400, (1, 4, 7, 10, 13, 15, 2, 5, 8, 12)


def step(state, zero):
    """one clock on ints or on symbolic bits: anything with ^"""
    out, moved = state[0], state[1:] + [zero]
    return [moved[g] ^ out if (TAPS >> g) & 1 else moved[g] for g in range(N_BITS)]


def keystream(secret, count):
    s, bits = [(secret >> g) & 1 for g in range(N_BITS)], []
    for _ in range(count):
        a, b, c, d, e, f, g, h, i, j = [s[k] for k in SELECT]
        bits.append(a ^ (b & c) ^ (d & e & f) ^ (g & h & i & j))
        s = step(s, 0)
    return bits


def recover(seed, count=2560):
    secret = random.Random(seed).getrandbits(N_BITS)
    stream = keystream(secret, count)
    t0 = time.perf_counter()
    qsys = PackedQuarticSystem([N_BITS])
    (x,) = qsys.gens()
    s, zero, zeros = [x[k] for k in range(N_BITS)], x[0] ^ x[0], []
    mul = qsys.mul_bit
    for bit in stream:
        a, b, c, d, e, f, g, h, i, j = [s[k] for k in SELECT]
        zeros.append(a ^ mul(b, c) ^ mul(mul(d, e), f) ^ mul(mul(g, h), mul(i, j)) ^ bit)
        s = step(s, zero)
    t1 = time.perf_counter()
    sols = list(qsys.solve_all(zeros))
    t2 = time.perf_counter()
    assert sols == [(secret,)], len(sols)
    assert qsys.solve_one(zeros) == (secret,)
    print(f"{len(zeros)} quartic equations x {qsys._cols} unknowns: generate {t1 - t0:.2f}s  solve_all {t2 - t1:.3f}s  secret {sols[0][0]:#06x}  ok")
    return secret


if __name__ == "__main__":
    recover(1)
    recover(2)
