"""State recovery of the cubic-filter register of nlfsr_recovery_cubic.py from a few dozen outputs instead of 736, with search_all_cubic.

Same register: n = 16 state bits, z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15, taps 0xB400.  Plain linearisation over the 696 monomials of
degree <= 3 needs 696 independent equations before solve_all returns the secret alone; one output short of that its space has more
points than the host walk takes, and with under twenty outputs it has dimension 678 and more: solve_all raises
DimensionTooLargeError.  The information is there all the same -- brute force over the 2^16 states shows from which output count on
the secret is the only state that fits, and that count is used here: 18 outputs for seed 1 (space of dimension 678), 15 for seed 2
(dimension 681).  search_all_cubic reduces the space to cubic forms in r_eff <= 16 variables and searches them on the GPU; with
n <= max_enum it cannot give up, whatever the linearisation left.
"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gf2bv_amd import DimensionTooLargeError, PackedCubicSystem, hip, search_all_cubic, search_one_cubic

N_BITS, TAPS, SELECT = 16, 0xB400, (1, 4, 7, 10, 13, 15)


def step(state, zero):
    """one clock on ints, numpy arrays or symbolic bits: anything with ^"""
    out, moved = state[0], state[1:] + [zero]
    return [moved[g] ^ out if (TAPS >> g) & 1 else moved[g] for g in range(N_BITS)]


def output(s):
    return s[SELECT[0]] ^ (s[SELECT[1]] & s[SELECT[2]]) ^ (s[SELECT[3]] & s[SELECT[4]] & s[SELECT[5]])


def smallest_count(secret):
    """the smallest number of outputs that only the secret produces, by brute force over all 2^16 states at once (CPU)"""
    s = [((np.arange(1 << N_BITS, dtype=np.uint32) >> g) & 1).astype(np.uint8) for g in range(N_BITS)]
    alive, count = np.ones(1 << N_BITS, dtype=bool), 0
    while alive.sum() > 1:
        z = output(s)
        alive &= z == z[secret]
        s, count = step(s, np.zeros_like(s[0])), count + 1
    return count


def recover(seed):
    secret = random.Random(seed).getrandbits(N_BITS)
    count = smallest_count(secret)
    s, stream = [(secret >> g) & 1 for g in range(N_BITS)], []
    for _ in range(count):
        stream.append(output(s))
        s = step(s, 0)
    csys = PackedCubicSystem([N_BITS])
    (x,) = csys.gens()
    s, zero, zeros = [x[g] for g in range(N_BITS)], x[0] ^ x[0], []
    for bit in stream:
        a, b, c, d, e, f = [s[i] for i in SELECT]
        zeros.append(a ^ csys.mul_bit(b, c) ^ csys.mul_bit(csys.mul_bit(d, e), f) ^ bit)
        s = step(s, zero)
    try:
        list(csys.solve_all(zeros))
        raise AssertionError("solve_all should have refused")
    except DimensionTooLargeError as e:
        dim = e.space.dimension
    t0 = time.perf_counter()
    sols = search_all_cubic(csys, zeros)
    t1 = time.perf_counter()
    t = hip.cubic_last_times()
    assert sols == [(secret,)], len(sols)
    assert search_one_cubic(csys, zeros) == (secret,)
    print(f"{count} cubic equations x {csys._cols} unknowns: space of dimension {dim}, solve_all refuses; search_all_cubic {t1 - t0:.3f}s "
          f"(library {t['ms_total']:.1f} ms: reduce {t['ms_reduce']:.1f}, forms {t['ms_forms']:.1f}, affine {t['ms_affine']:.1f}, "
          f"search {t['ms_search']:.1f})  secret {sols[0][0]:#06x}  ok")
    return secret


if __name__ == "__main__":
    recover(1)
    recover(2)
