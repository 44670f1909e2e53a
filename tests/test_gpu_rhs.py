"""Many right-hand sides of one matrix with one elimination (gf2bv_solve_rhs_*, m4ri_solve_rhs, LinearSystem.*_rhs).
The contract: result j of a many-RHS call is bit-identical to what the single-system entry returns for system j alone --
the matrix with its column `cols` replaced by right-hand side j -- status, rank, pivots, dimension, origin and basis."""
import random

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, hip
from oracle import gf2_oracle as O
from tests import harness as H
from tests.harness_models import MT19937
from tests.systems import random_system

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(autouse=True, params=["default", "plain"])
def _heuristics(request, monkeypatch):
    """Every test runs as shipped and with GF2BV_PLAIN=1 (as test_gpu_parity.py does)."""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


def _bits(aug: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """rows x cols 0/1 matrix of the coefficients."""
    cw = (cols + 63) // 64
    by = np.ascontiguousarray(aug[:rows, :cw]).view(np.uint8).reshape(rows, cw * 8)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :cols]


def _rhs_words(bits: np.ndarray) -> np.ndarray:
    """nrhs x rows 0/1 -> nrhs x ceil(rows/64) uint64, bit r of row j = bits[j, r]."""
    nrhs, rows = bits.shape
    rw = (rows + 63) // 64
    padded = np.zeros((nrhs, rw * 64), dtype=np.uint8)
    padded[:, :rows] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(nrhs, rw)


def _make_rhs(rng: random.Random, aug: np.ndarray, rows: int, cols: int, nrhs: int) -> np.ndarray:
    """nrhs x rows 0/1: the even ones planted (b = A x), the odd ones random."""
    A = _bits(aug, rows, cols).astype(np.float32)
    npl = (nrhs + 1) // 2
    X = np.array([[rng.getrandbits(1) for _ in range(cols)] for _ in range(npl)], dtype=np.float32).reshape(npl, cols)
    planted = (A @ X.T).astype(np.int64).T & 1
    out = np.zeros((nrhs, rows), dtype=np.uint8)
    for j in range(nrhs):
        out[j] = planted[j // 2] if j % 2 == 0 else [rng.getrandbits(1) for _ in range(rows)]
    return out


def _with_rhs(aug: np.ndarray, cols: int, b: np.ndarray) -> np.ndarray:
    a = aug.copy()
    w, bit = cols // 64, np.uint64(cols % 64)
    a[:, w] = (a[:, w] & ~(np.uint64(1) << bit)) | (b.astype(np.uint64) << bit)
    return a


def assert_same_solution(got: hip.Solution, want: hip.Solution, mode: int):
    assert got.status == want.status
    assert got.rank == want.rank
    assert np.array_equal(got.pivots, want.pivots)
    if got.status == 0:
        assert np.array_equal(got.origin, want.origin)
        if mode == 1:
            assert got.dimension == want.dimension
            assert np.array_equal(got.basis, want.basis)


def assert_same_oracle(got: hip.Solution, want: dict, mode: int):
    assert got.status == want["status"]
    assert got.rank == want["rank"]
    assert np.array_equal(got.pivots, want["pivcols"])
    if got.status == 0:
        assert np.array_equal(got.origin, want["origin"])
        if mode == 1:
            assert got.dimension == want["dim"]
            assert np.array_equal(got.basis, want["basis"])


def _check_against_single(aug, rows, cols, rhs_bits, mode, rng, oracle_all: bool):
    rhs = _rhs_words(rhs_bits)
    got = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    assert len(got) == rhs_bits.shape[0]
    oracle_js = set(range(len(got))) if oracle_all else {0, 1, len(got) - 1, rng.randrange(len(got))}
    for j, g in enumerate(got):
        a = _with_rhs(aug, cols, rhs_bits[j])
        assert_same_solution(g, hip.solve_words(a, rows, cols, mode), mode)
        if j in oracle_js:
            assert_same_oracle(g, O.solve_words(a, rows, cols, mode), mode)
    return got


# rows, cols, density, rank_cap, zero_rows; nrhs -- every nrhs of {1, 3, 8, 9, 64, 65, 130}, cols % 64 in {0, 1, 63}, cols + nrhs
# crossing a word (64 + 1, 63 + 9) and an 8-word tile of 512 columns (500 + 13, 1023 + 130)
CASES = [
    ((1, 1, .5, None, 0), 1), ((1, 1, .5, None, 0), 3), ((4, 4, .5, None, 1), 8), ((4, 4, .5, None, 0), 65),
    ((64, 63, .5, None, 0), 9), ((64, 63, .5, None, 0), 1), ((64, 64, .5, None, 0), 64), ((64, 64, .5, None, 0), 65),
    ((66, 65, .5, None, 0), 130), ((66, 65, .5, None, 0), 63), ((600, 500, .5, 450, 0), 13), ((300, 200, .5, 40, 0), 8),
    ((300, 200, .5, 40, 0), 64), ((1100, 1023, .5, 900, 0), 3), ((1100, 1023, .5, 900, 0), 130), ((2100, 2048, .02, None, 50), 9),
    ((2100, 2048, .02, None, 50), 64), ((3000, 2500, .5, None, 0), 8), ((9000, 2049, .003, None, 0), 65),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-n{c[1]}")
@pytest.mark.parametrize("mode", [0, 1])
def test_words_path_matches_single_and_oracle(case, mode):
    (rows, cols, dens, cap, zr), nrhs = case
    rng = random.Random(rows * 7919 + cols * 31 + nrhs)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, dens, cap, True, zr), cols)
    rhs_bits = _make_rhs(rng, aug, rows, cols, nrhs)
    got = _check_against_single(aug, rows, cols, rhs_bits, mode, rng, oracle_all=rows * cols <= 300 * 200)
    assert all(g.status == 0 for g in got[::2])                        # the planted ones are consistent
    if cap is not None and rows > 64:
        assert any(g.status == 1 for g in got[1::2]) or nrhs == 1      # random ones on a rank-deficient matrix mostly are not


def test_digits_path_matches_words_path():
    rng = random.Random(5)
    rows, cols, nrhs = 700, 650, 20
    eqs = random_system(rng, rows, cols, .5, 600, True, 3)
    aug = O.eqs_to_aug(eqs, cols)
    rhs = _rhs_words(_make_rhs(rng, aug, rows, cols, nrhs))
    # the equation ints as 30-bit digits, with random garbage in bit 0 (ignored)
    digs, off = [], [0]
    for e in eqs:
        e ^= rng.getrandbits(1)
        while e:
            digs.append(e & ((1 << 30) - 1))
            e >>= 30
        off.append(len(digs))
    for mode in (0, 1):
        a = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
        b = hip.solve_rhs_digits(np.array(digs + [0], dtype=np.uint32), np.array(off), 30, rows, cols, rhs, mode)
        for x, y in zip(a, b):
            assert_same_solution(x, y, mode)


# forced plans (the knobs tests/test_gpu_stress.py uses): each against the single path
@pytest.mark.parametrize("knob,value,shape", [
    ("GF2BV_TWO_LEVEL", "2", (2600, 2500, 2300)), ("GF2BV_TWO_LEVEL", "8", (4200, 4100, 3900)), ("GF2BV_YSWEEP", "1", (1100, 1023, 900)),
    ("GF2BV_BS_INV", "0", (2600, 2500, 2300)), ("GF2BV_BS_INV", "1", (1100, 1023, 900)), ("GF2BV_FAST", "0", (2600, 2500, 2300)),
])
def test_forced_plans(monkeypatch, knob, value, shape):
    monkeypatch.setenv(knob, value)
    rows, cols, cap = shape
    rng = random.Random(rows + cols + len(knob))
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cap, True, 0), cols)
    rhs_bits = _make_rhs(rng, aug, rows, cols, 10)
    rhs = _rhs_words(rhs_bits)
    for mode in (0, 1):
        got = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
        if knob == "GF2BV_TWO_LEVEL":
            assert got[0].stats["outer_blocks"] > 0                      # the plan did engage
        for j, g in enumerate(got):
            assert_same_solution(g, hip.solve_words(_with_rhs(aug, cols, rhs_bits[j]), rows, cols, mode), mode)


def test_large_device_resident_64_rhs():
    """65536^2 synthetic system (the bench system), 64 right-hand sides b_j = b ^ A[:, c_j] built on the device: x_j = planted ^ e_{c_j}."""
    torch = pytest.importorskip("torch")
    n, seed, nrhs = 65536, 1234, 64
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    torch.cuda.synchronize()
    rng = random.Random(99)
    cs = [rng.randrange(n) for _ in range(nrhs)]
    cs[0], cs[1], cs[2] = 0, n - 1, 63
    w = n // 64
    b = (A[:, w] >> (n % 64)) & 1                                         # the synthetic system's own right-hand side
    rw = (n + 63) // 64
    weights = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64, device=dev)
    rhs = torch.empty((nrhs, rw), dtype=torch.int64, device=dev)
    for j, c in enumerate(cs):
        col = (A[:, c // 64] >> (c % 64)) & 1
        rhs[j] = ((b ^ col).view(rw, 64) * weights).sum(dim=1)
    torch.cuda.synchronize()
    got = hip.solve_rhs_device(A.data_ptr(), n, n, stride, rhs.data_ptr(), nrhs, rw, 0)
    planted = hip.planted_solution(n, seed)
    for j, (g, c) in enumerate(zip(got, cs)):
        want = planted.copy()
        want[c // 64] ^= np.uint64(1 << (c % 64))
        assert g.status == 0 and g.rank == n, (j, g.status, g.rank)
        assert np.array_equal(g.origin, want), j
    for j in (0, 5):
        sysj = A.clone()
        sysj[:, w] = (sysj[:, w] & ~(1 << (n % 64))) | (((rhs[j].view(-1, 1) >> torch.arange(64, device=dev)) & 1).view(-1)[:n] << (n % 64))
        torch.cuda.synchronize()
        assert hip.residual_device(sysj.data_ptr(), n, n, stride, got[j].origin) == 0
        del sysj
    del A, rhs
    torch.cuda.empty_cache()


def test_python_contract():
    lin = LinearSystem([16, 9, 5])
    a, b, c = lin.gens()
    secret = (0xBEEF, 0x155, 0x13)
    exprs = [a ^ (b.zeroext(7) << 3), (a >> 4) ^ c.zeroext(11), b ^ (a & 0x1FF)[0:9], c[0] ^ c[4], (a ^ a)[0:3], 1 << 3, 0,
             c[1] ^ c[1] ^ 1]                                       # the last: constant-only, per instance "1 = 0" or 0 = 0
    raw = secret[0] | secret[1] << 16 | secret[2] << 25
    rng = random.Random(3)
    values_list = []
    for i in range(12):
        vals = []
        for e in exprs:
            if isinstance(e, int):                                  # e ^ v = 0 holds at the secret for v = <e, x> ^ constant
                vals.append(rng.getrandbits(1) if i % 3 == 0 else (bin((e >> 1) & raw).count("1") & 1) ^ (e & 1))
            else:
                v = lin.evaluate(e, secret) if i % 2 == 0 else rng.getrandbits(len(e))
                vals.append(v if i % 4 != 2 else v ^ 1)
        values_list.append(vals)
    values_list[5][-1] = 0                                          # constant-only element 1 ^ 0 = 1: inconsistent
    values_list[6][-1] = 1                                          # 1 ^ 1 = 0: a literal zero
    zeros_of = [[e ^ v for e, v in zip(exprs, vals)] for vals in values_list]
    one = lin.solve_raw_one_rhs(exprs, values_list)
    space = lin.solve_raw_space_rhs(exprs, values_list)
    sol = lin.solve_one_rhs(exprs, values_list)
    assert one[5] is None and space[5] is None
    assert sum(x is None for x in one) >= 1 and sum(x is not None for x in one) >= 2
    for i, z in enumerate(zeros_of):
        assert one[i] == lin.solve_raw_one(z)
        assert sol[i] == lin.solve_one(z)
        s1, s2 = space[i], lin.solve_raw_space(z)
        assert (s1 is None) == (s2 is None)
        if s1 is not None:
            assert (s1.origin, s1.basis, s1.dimension) == (s2.origin, s2.basis, s2.dimension)
            assert list(s1) == list(s2)


def test_mt19937_instances():
    bs, n = 32, 8
    outs, states = [], []
    for seed in range(n):
        rand = random.Random(1000 + seed)
        states.append(tuple(rand.getstate()[1][:-1]))
        outs.append([rand.getrandbits(bs) for _ in range(624)])
    lin = LinearSystem([32] * 624)
    mt = lin.gens()
    rng = MT19937(mt)
    exprs = [rng.getrandbits(bs) for _ in range(624)] + [mt[0]]
    values_list = [o + [0x80000000] for o in outs]
    got = lin.solve_one_rhs(exprs, values_list)
    for i in range(n):
        assert got[i] == states[i], i
    assert got[0] == lin.solve_one([e ^ v for e, v in zip(exprs, values_list[0])])


def test_quadratic_golden_system():
    sets = [(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0), (1, 1, 1)]
    for c3 in (0, 1):
        q, zeros = H.quadratic_small_system((0, 0, 0, c3))
        values_list = [list(cs) + [0] * (len(zeros) - 3) for cs in sets]
        got = q.solve_one_rhs(zeros, values_list)
        for cs, g in zip(sets, got):
            _, z = H.quadratic_small_system(cs + (c3,))
            assert g == q.solve_one(z), (cs, c3)
