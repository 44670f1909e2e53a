"""State recovery of a register whose output filter has a cubic term, through the packed cubic front-end (PackedCubicSystem).

The register has n = 16 state bits s_0 .. s_15.  Each clock it outputs z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15 and then steps: out = s_0,
every bit moves down one place (s_15 becomes 0), and `out` is added to the bits the taps 0xB400 name.  The state stays linear in the
secret, so every output is one cubic equation written directly with mul_bit -- no annihilator, no multiplier -- and kept factored on
the host: a linear form, one product of two and one product of three linear forms.  The rows over the 16 + 120 + 560 = 696 monomials
of degree <= 3 come into being on the GPU, which solves them; 736 outputs give rank 696 and solve_all returns the secret alone.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import PackedCubicSystem

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


def recover(seed, count=736):
    secret = random.Random(seed).getrandbits(N_BITS)
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
    sols = list(csys.solve_all(zeros))
    t2 = time.perf_counter()
    assert sols == [(secret,)], len(sols)
    assert csys.solve_one(zeros) == (secret,)
    print(f"{len(zeros)} cubic equations x {csys._cols} unknowns: generate {t1 - t0:.2f}s  solve_all {t2 - t1:.3f}s  secret {sols[0][0]:#06x}  ok")
    return secret


if __name__ == "__main__":
    recover(1)
    recover(2)
