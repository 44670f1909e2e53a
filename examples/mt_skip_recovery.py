"""MT19937 state recovery from outputs that are NOT adjacent: 312 outputs of CPython's `random`, then 1 000 272 outputs nobody saw
(1603 twists, generated for real here), then 312 more.  Stepping a symbolic model through a million outputs is out of the question;
the twist is an affine map of the 19968 state bits, so it is written down once (one symbolic twist on the host), raised to the 1603rd
power on the GPU (15 products of 19969 x 19969 bits) and substituted into the state the first 312 outputs were drawn from."""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gf2bv_amd import PackedLinearSystem, hip, power, substitute
from tests.harness_models import MT19937

SEEN, TWISTS = 312, 1603
SKIP = TWISTS * 624                                    # 1 000 272 outputs


def main():
    rand = random.Random(2718)
    state = tuple(rand.getstate()[1][:-1])
    first = [rand.getrandbits(32) for _ in range(SEEN)]
    for _ in range(SKIP):
        rand.getrandbits(32)
    second = [rand.getrandbits(32) for _ in range(SEEN)]
    following = [rand.getrandbits(32) for _ in range(1000)]

    lin = PackedLinearSystem([32] * 624)
    t0 = time.perf_counter()
    one = MT19937(lin.gens())
    one._regenerate()                                  # the twist, symbolically, once
    twist = tuple(one.mt)
    t1 = time.perf_counter()
    skip = power(twist, TWISTS)
    t2 = time.perf_counter()
    tp = hip.compose_last_times()
    rng = MT19937(lin.gens())
    zeros = [rng.getrandbits(32) ^ o for o in first]   # (the first of them twists: rng.mt is the state after one twist from here on)
    rng.mt = list(substitute(skip, rng.mt))            # 1603 twists later, the read position where it was
    t3 = time.perf_counter()
    ts = hip.compose_last_times()
    zeros += [rng.getrandbits(32) ^ o for o in second] + [lin.gens()[0] ^ 0x80000000]
    t4 = time.perf_counter()
    sol = lin.solve_one(zeros)
    t5 = time.perf_counter()
    assert sol is not None
    check = MT19937(sol).to_python_random()
    assert [check.getrandbits(32) for _ in range(SEEN)] == first
    for _ in range(SKIP):
        check.getrandbits(32)
    assert [check.getrandbits(32) for _ in range(SEEN)] == second
    assert [check.getrandbits(32) for _ in range(1000)] == following
    print(f"twist map on the host {t1 - t0:6.2f}s   power(twist, {TWISTS}) {t2 - t1:6.3f}s   substitute {t3 - t2:6.3f}s   "
          f"equations {t4 - t3 + 0:6.2f}s   solve_one {t5 - t4:6.3f}s   state {'recovered' if sol == state else 'equivalent'}")
    print(f"library, power:      upload {tp['ms_upload']:.1f} ms, {tp['products']} products {tp['ms_kernels']:.1f} ms, download {tp['ms_download']:.1f} ms")
    print(f"library, substitute: upload {ts['ms_upload']:.1f} ms, {ts['products']} product {ts['ms_kernels']:.1f} ms, download {ts['ms_download']:.1f} ms")


if __name__ == "__main__":
    main()
