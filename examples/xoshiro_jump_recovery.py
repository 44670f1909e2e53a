"""xoshiro256** seed recovery across a jump(): two outputs, then jump() (2^128 steps, as the reference code's jump function does
for parallel streams), then three more.  Nobody steps a model 2^128 times: the symbolic state after the jump is the one-step map raised
to the 2^128-th power on the GPU and substituted into the state reached so far.

(Three outputs behind the jump, not two: the 256 equations of two outputs on either side of jump() have rank 255 -- two seeds give
the same four outputs, and solve_one could return either.  Across long_jump(), or with no jump, two and two do have rank 256.)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import PackedLinearSystem, power, substitute
from tests.harness_models import Xoshiro256starstar

# xoshiro256starstar.c (Blackman & Vigna, public domain)
JUMP = (0x180ec6d33cfd0aba, 0xd5a61266f0c9392c, 0xa9582618e03fc9aa, 0x39abdc4529b1661c)


def jump(gen: Xoshiro256starstar) -> None:
    """the reference code's jump(): equivalent to 2^128 calls of next()"""
    acc = [0, 0, 0, 0]
    for word in JUMP:
        for b in range(64):
            if (word >> b) & 1:
                acc = [x ^ y for x, y in zip(acc, gen.s)]
            gen.step()
    gen.s = acc


def observe(seed) -> list:
    """what the attacker sees: two outputs, (a jump), three outputs"""
    gen = Xoshiro256starstar(seed)
    outs = [gen(), gen()]
    jump(gen)
    return outs + [gen(), gen(), gen()]


def recover(outs) -> tuple:
    lin = PackedLinearSystem([64] * 4)
    one = Xoshiro256starstar(lin.gens())
    one.step()
    jump_map = power(tuple(one.s), 1 << 128)           # the state transition, 2^128 times
    sym = Xoshiro256starstar(lin.gens())
    zeros = [sym.step() ^ Xoshiro256starstar.untemper(o) for o in outs[:2]]
    sym.s = list(substitute(jump_map, sym.s))          # unknown g of the jump map := bit g of the state reached so far
    zeros += [sym.step() ^ Xoshiro256starstar.untemper(o) for o in outs[2:]]
    return lin.solve_one(zeros)


if __name__ == "__main__":
    gen = Xoshiro256starstar.generate()
    secret = tuple(gen.s)
    outs = observe(secret)
    t0 = time.perf_counter()
    sol = recover(outs)
    print(f"power + substitute + solve_one: {time.perf_counter() - t0:.4f}s")
    assert sol == secret
    check = Xoshiro256starstar(list(sol))
    assert [check(), check()] == outs[:2]
    print("recovered", [hex(v) for v in sol])
