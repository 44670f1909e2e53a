"""State recovery of the quartic-filter register of nlfsr_recovery_quartic.py from 16 outputs instead of 2560, with search_all_quartic.

Same register: n = 16 state bits, z = s_1 ^ s_4 s_7 ^ s_10 s_13 s_15 ^ s_2 s_5 s_8 s_12, taps 0xB400.  Plain linearisation over the 2516
monomials of degree <= 4 needs 2516 independent equations before solve_all returns the secret alone.  Sixteen outputs leave a space
of dimension 2500, which solve_all refuses with DimensionTooLargeError -- yet brute force over the 2^16 states shows that the secret
is already the only state that fits them, for both secrets used here.  search_all_quartic reduces the space to quartic forms in
r_eff <= 16 variables and searches them on the GPU; with n <= max_enum it cannot give up, whatever the linearisation left.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gf2bv_amd import DimensionTooLargeError, PackedQuarticSystem, hip, search_all_quartic, search_one_quartic

N_BITS, TAPS, SELECT = 16, 0xB400, (1, 4, 7, 10, 13, 15, 2, 5, 8, 12)
OUTPUTS = 16


def step(state, zero):
    """one clock on ints, numpy arrays or symbolic bits: anything with ^"""
    out, moved = state[0], state[1:] + [zero]
    return [moved[g] ^ out if (TAPS >> g) & 1 else moved[g] for g in range(N_BITS)]


def output(s, mul=lambda u, v: u & v):
    a, b, c, d, e, f, g, h, i, j = [s[k] for k in SELECT]
    return a ^ mul(b, c) ^ mul(mul(d, e), f) ^ mul(mul(g, h), mul(i, j))


def fitting_states(secret, count):
    """every state whose first `count` outputs are the secret's, by brute force over all 2^16 states at once (CPU)"""
    s = [((np.arange(1 << N_BITS, dtype=np.uint32) >> g) & 1).astype(np.uint8) for g in range(N_BITS)]
    alive = np.ones(1 << N_BITS, dtype=bool)
    for _ in range(count):
        z = output(s)
        alive &= z == z[secret]
        s = step(s, np.zeros_like(s[0]))
    return [int(v) for v in np.flatnonzero(alive)]


def equations(qsys, secret, count):
    s, stream = [(secret >> g) & 1 for g in range(N_BITS)], []
    for _ in range(count):
        stream.append(output(s))
        s = step(s, 0)
    (x,) = qsys.gens()
    s, zero, zeros = [x[g] for g in range(N_BITS)], x[0] ^ x[0], []
    for bit in stream:
        zeros.append(output(s, qsys.mul_bit) ^ bit)
        s = step(s, zero)
    return zeros


def recover(secret, count=OUTPUTS):
    assert fitting_states(secret, count) == [secret]
    qsys = PackedQuarticSystem([N_BITS])
    zeros = equations(qsys, secret, count)
    try:
        list(qsys.solve_all(zeros))
        raise AssertionError("solve_all should have refused")
    except DimensionTooLargeError as e:
        dim = e.space.dimension
    t0 = time.perf_counter()
    sols = search_all_quartic(qsys, zeros)
    t1 = time.perf_counter()
    t = hip.quartic_last_times()
    assert sols == [(secret,)], len(sols)
    assert search_one_quartic(qsys, zeros) == (secret,)
    print(f"{count} quartic equations x {qsys._cols} unknowns: space of dimension {dim}, solve_all refuses; search_all_quartic {t1 - t0:.3f}s "
          f"(library {t['ms_total']:.1f} ms: reduce {t['ms_reduce']:.1f}, forms {t['ms_forms']:.1f}, affine {t['ms_affine']:.1f}, "
          f"search {t['ms_search']:.1f})  secret {sols[0][0]:#06x}  ok")
    return secret


if __name__ == "__main__":
    recover(0x52E7)
    recover(0x3A09)
