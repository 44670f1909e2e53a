"""A kept factorization (gf2bv_factor_*, _internal.m4ri_factor, hip.Factor, LinearSystem.factor).  The contract: result j of any
solve on a handle is bit-identical to what gf2bv_solve_rhs_words returns for the same matrix and right-hand side j -- status, rank,
pivots, dimension, origin, basis -- for every call on the handle, in any order, any number of times."""
import random

import numpy as np
import pytest
import torch

from gf2bv_amd import LinearSystem, QuadraticSystem, _internal, hip
from oracle import gf2_oracle as O
from tests import harness as H
from tests import known_answer as KA
from tests.harness_models import MT19937
from tests.systems import random_system
from tests.test_gpu_rhs import _make_rhs, _rhs_words, _with_rhs, assert_same_oracle, assert_same_solution

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(params=["default", "plain"])
def heuristics(request, monkeypatch):
    """As shipped and with GF2BV_PLAIN=1 (both panel paths for every block, events instead of gates)."""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


def _check_handle(f: hip.Factor, aug, rows, cols, rhs_bits, mode, oracle_js=()):
    rhs = _rhs_words(rhs_bits)
    got = f.solve(rhs)
    want = hip.solve_rhs_words(aug, rows, cols, rhs, mode)
    assert len(got) == len(want) == rhs_bits.shape[0]
    for j, (g, w) in enumerate(zip(got, want)):
        assert_same_solution(g, w, mode)
        assert g.dimension == w.dimension
        if j in oracle_js:
            assert_same_oracle(g, O.solve_words(_with_rhs(aug, cols, rhs_bits[j]), rows, cols, mode), mode)
    return got


# rows, cols, density, rank_cap, zero_rows: rank-deficient, rows > cols, cols % 64 in {0, 1, 63}, a short last block, sparse
SHAPES = [(1, 1, .5, None, 0), (4, 4, .5, None, 1), (64, 63, .5, None, 0), (64, 64, .5, None, 0), (66, 65, .5, None, 0),
          (300, 200, .5, 40, 0), (600, 500, .5, 450, 0), (1100, 1023, .5, 900, 0), (2100, 2048, .02, None, 50),
          (3000, 2500, .5, None, 0), (9000, 2049, .003, None, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", [0, 1])
def test_handle_matches_solve_rhs(shape, mode, heuristics):
    rows, cols, dens, cap, zr = shape
    rng = random.Random(rows * 131 + cols * 7 + mode)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, dens, cap, True, zr), cols)
    small = rows * cols <= 300 * 200
    with hip.factor_words(aug, rows, cols, mode) as f:
        assert f.rank == hip.solve_words(aug, rows, cols, mode).rank
        # 130 then 1, 64, 65: full passes, then a short pass behind a full one (slots of the full pass must not leak into it)
        for nrhs in (130, 1, 64, 65):
            rhs_bits = _make_rhs(rng, aug, rows, cols, nrhs)
            got = _check_handle(f, aug, rows, cols, rhs_bits, mode, oracle_js=range(nrhs) if small and nrhs <= 64 else (0, nrhs - 1))
            assert all(g.status == 0 for g in got[::2])                  # the planted ones are consistent


def test_short_pass_after_full_pass_sees_no_stale_slots():
    """A pass of 64 inconsistent right-hand sides, then a pass of 1 consistent one: the second must not see the first's slots."""
    rows, cols = 900, 700
    rng = random.Random(77)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, 650, True, 0), cols)
    with hip.factor_words(aug, rows, cols, 0) as f:
        bad = np.array([[rng.getrandbits(1) for _ in range(rows)] for _ in range(64)], dtype=np.uint8)
        assert all(g.status == 1 for g in _check_handle(f, aug, rows, cols, bad, 0))
        zero = np.zeros((1, rows), dtype=np.uint8)
        g = _check_handle(f, aug, rows, cols, zero, 0)[0]
        assert g.status == 0 and not g.origin.any()


def test_results_do_not_depend_on_history():
    """Three batches on one handle in a shuffled order, interleaved with a second handle and with plain solves: every answer
    equals the one-shot entry's."""
    rng = random.Random(2024)
    shapes = [(1500, 1400, .5, 1300, 0), (800, 777, .5, None, 3)]
    systems = []
    for rows, cols, dens, cap, zr in shapes:
        eqs = random_system(rng, rows, cols, dens, cap, True, zr)
        aug = O.eqs_to_aug(eqs, cols)
        batches = [_make_rhs(rng, aug, rows, cols, n) for n in (5, 64, 70)]
        systems.append((aug, rows, cols, batches, eqs))
    for mode in (0, 1):
        handles = [hip.factor_words(aug, rows, cols, mode) for aug, rows, cols, _, _ in systems]
        order = [(s, b) for s in range(2) for b in range(3)] * 2
        rng.shuffle(order)
        for s, b in order:
            aug, rows, cols, batches, _ = systems[s]
            _check_handle(handles[s], aug, rows, cols, batches[b], mode)
            oaug, orows, ocols, _, oeqs = systems[1 - s]                 # plain solves of the other matrix in between
            assert hip.solve_words(oaug, orows, ocols, mode).rank == handles[1 - s].rank
            _internal.m4ri_solve(oeqs, ocols, mode)
        for h in handles:
            h.close()


def test_device_bytes_and_close():
    rows, cols = 3000, 2900
    rng = random.Random(8)
    eqs = random_system(rng, rows, cols, .5, None, True, 0)
    aug = O.eqs_to_aug(eqs, cols)
    f = hip.factor_words(aug, rows, cols, 0)
    nblocks = (cols + 255) // 256
    assert f.device_bytes >= rows * 32 * nblocks                       # at least the matrix' worth (U) -- it holds U and T
    assert f.device_bytes >= rows * ((cols + 63) // 64 + (rows + 63) // 64) * 8
    f.close()
    with pytest.raises(ValueError):
        f.solve(np.zeros((1, (rows + 63) // 64), dtype=np.uint64))
    F = _internal.m4ri_factor(eqs, cols, 0)
    assert (F.rows, F.cols, F.mode, F.device) == (rows, cols, 0, 0)
    assert F.device_bytes > 0 and F.rank == len(F.pivots)
    F.close()
    with pytest.raises(ValueError):
        F.solve([0])
    with pytest.raises(ValueError):
        F.rank


def test_internal_list_and_array_forms_equal_solve_rhs():
    rng = random.Random(12)
    rows, cols = 700, 650
    eqs = random_system(rng, rows, cols, .5, 600, True, 3)
    aug = O.eqs_to_aug(eqs, cols)
    rhs_bits = _make_rhs(rng, aug, rows, cols, 9)
    rhs_ints = [int("".join(str(int(b)) for b in bits[::-1]), 2) for bits in rhs_bits]
    for mode in (0, 1):
        want = _internal.m4ri_solve_rhs(eqs, cols, mode, rhs_ints)
        with _internal.m4ri_factor(eqs, cols, mode) as F:
            for got in (F.solve(rhs_ints), F.solve(_rhs_words(rhs_bits)), F.solve(rhs_ints)):
                for g, w in zip(got, want):
                    if mode == 0 or g is None:
                        assert g == w
                    else:
                        assert (g.origin, g.basis, g.dimension) == (w.origin, w.basis, w.dimension)


def test_forced_two_level_plan(monkeypatch, heuristics):
    monkeypatch.setenv("GF2BV_TWO_LEVEL", "2")
    rows, cols, cap = 2600, 2500, 2300
    rng = random.Random(rows + cols)
    aug = O.eqs_to_aug(random_system(rng, rows, cols, .5, cap, True, 0), cols)
    for mode in (0, 1):
        with hip.factor_words(aug, rows, cols, mode) as f:
            got = _check_handle(f, aug, rows, cols, _make_rhs(rng, aug, rows, cols, 10), mode)
            assert got[0].stats["outer_blocks"] > 0                      # the plan did engage


def test_python_front_end_equals_linear_system():
    lin = LinearSystem([16, 9, 5])
    a, b, c = lin.gens()
    secret = (0xBEEF, 0x155, 0x13)
    exprs = [a ^ (b.zeroext(7) << 3), (a >> 4) ^ c.zeroext(11), b ^ (a & 0x1FF)[0:9], c[0] ^ c[4], (a ^ a)[0:3], 1 << 3, 0,
             c[1] ^ c[1] ^ 1]
    raw = secret[0] | secret[1] << 16 | secret[2] << 25
    rng = random.Random(3)
    values_list = []
    for i in range(12):
        vals = []
        for e in exprs:
            if isinstance(e, int):
                vals.append(rng.getrandbits(1) if i % 3 == 0 else (bin((e >> 1) & raw).count("1") & 1) ^ (e & 1))
            else:
                v = lin.evaluate(e, secret) if i % 2 == 0 else rng.getrandbits(len(e))
                vals.append(v if i % 4 != 2 else v ^ 1)
        values_list.append(vals)
    values_list[5][-1] = 0
    values_list[6][-1] = 1
    with lin.factor(exprs) as fs:
        one = fs.solve_raw_one_rhs(values_list)
        space = fs.solve_raw_space_rhs(values_list)
        assert one == lin.solve_raw_one_rhs(exprs, values_list)
        assert fs.solve_one_rhs(values_list) == lin.solve_one_rhs(exprs, values_list)
        for i, vals in enumerate(values_list):
            z = [e ^ v for e, v in zip(exprs, vals)]
            assert fs.solve_one(vals) == lin.solve_one(z)
            assert list(fs.solve_all(vals)) == list(lin.solve_all(z))
            s1, s2 = space[i], lin.solve_raw_space(z)
            assert (s1 is None) == (s2 is None)
            if s1 is not None:
                assert (s1.origin, s1.basis, s1.dimension) == (s2.origin, s2.basis, s2.dimension)


def test_quadratic_factor_equals_solve_one_rhs():
    sets = [(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0), (1, 1, 1)]
    for c3 in (0, 1):
        q, zeros = H.quadratic_small_system((0, 0, 0, c3))
        assert isinstance(q, QuadraticSystem)
        values_list = [list(cs) + [0] * (len(zeros) - 3) for cs in sets]
        with q.factor(zeros) as fs:
            assert fs.solve_one_rhs(values_list) == q.solve_one_rhs(zeros, values_list)


@pytest.mark.parametrize("bs", [32, 1])
def test_mt19937_known_answer(bs):
    """examples/mt_recovery.py's scenario, several generators against ONE factorization (k_block_sparse eliminates it)."""
    lin = LinearSystem([32] * 624)
    mt = lin.gens()
    model = MT19937(mt)
    samples = 624 * 32 // bs
    exprs = [model.getrandbits(bs) for _ in range(samples)] + [mt[0]]
    outs, states = [], []
    for seed in [3142] + list(range(1000, 1007)):
        rand = random.Random(seed)
        states.append(tuple(rand.getstate()[1][:-1]))
        outs.append([rand.getrandbits(bs) for _ in range(samples)] + [0x80000000])
    with lin.factor(exprs) as fs:
        for n in (1, 8):
            got = fs.solve_one_rhs(outs[:n])
            assert got == states[:n]
        raw = fs.solve_raw_one_rhs(outs[:2])
    assert raw == lin.solve_raw_one_rhs(exprs, outs[:2])


def _device_rhs_from_column(t, rows, cols):
    """The augmented column `cols` of a device matrix as one right-hand side: [1, ceil(rows / 64)] int64 on the device."""
    rw = (rows + 63) // 64
    b = torch.zeros(rw * 64, dtype=torch.int64, device=t.device)
    b[:rows] = (t[:rows, cols // 64] >> (cols % 64)) & 1
    weights = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64, device=t.device)
    return (b.view(rw, 64) * weights).sum(dim=1).view(1, rw).contiguous()


def _known_answer_case(rows, cols, seed, spec):
    stride = hip.padded_stride(cols)
    t = torch.zeros((rows, stride), dtype=torch.int64, device="cuda")
    hip.synth_device(t.data_ptr(), rows, cols, stride, seed)
    torch.cuda.synchronize()
    KA.apply_torch(t, cols, spec)
    torch.cuda.synchronize()
    rhs = _device_rhs_from_column(t, rows, cols)
    torch.cuda.synchronize()
    f = hip.factor_device(t.data_ptr(), rows, cols, stride, 1)
    got = f.solve_device(rhs.data_ptr(), 1, rhs.shape[1])[0]
    f.close()
    del t, rhs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return got


@pytest.mark.timeout(300)
def test_natural_two_level_shape_known_answer(heuristics):
    """98704 x 98267 (tests/known_answer.py), free columns inside outer panel 1 and an XOR column in the tail."""
    rows, cols, seed = 98704, 98267, 12
    K, bend, nb = KA.plan_two_level(rows, cols)
    B = KA.BLOCK_COLS
    free = KA.place_free_columns(rows, cols, seed, [(K + K // 2) * B + o for o in (40, 130, 201)])
    spec = [KA.zero_col(c) for c in free]
    want = KA.known_answer(rows, cols, seed, spec)
    got = _known_answer_case(rows, cols, seed, spec)
    print(f"[factor] {rows}x{cols} {heuristics}: outer_blocks {got.stats['outer_blocks']} fast_blocks {got.stats['fast_blocks']}")
    KA.assert_same(got, want, 1)
    assert got.stats["outer_blocks"] > 0


@pytest.mark.timeout(300)
def test_search_give_up_and_resume(heuristics):
    """Row 5000 copied over row 4 (its RHS flipped): the one-launch search gives up on a block in the middle of the elimination and
    the host resumes there; the replayed answer is the known (inconsistent) one, and a consistent right-hand side still solves."""
    rows, cols, seed = 66000, 65600, 11
    spec = [KA.copy_row(5000, 4), KA.flip_rhs(4)]
    want = KA.known_answer(rows, cols, seed, spec)
    got = _known_answer_case(rows, cols, seed, spec)
    st = got.stats
    nb = (cols + 255) // 256
    print(f"[factor] give-up {heuristics}: fast_blocks {st['fast_blocks']} outer_blocks {st['outer_blocks']} of {nb}")
    KA.assert_same(got, want, 1)
    assert got.status == 1
    if heuristics == "default":
        assert 0 < st["fast_blocks"] < nb                                  # the search took blocks, and gave one up
    else:
        assert st["fast_blocks"] == 0 or st["fast_blocks"] < nb


def test_large_device_resident_factor():
    """65536^2 synthetic system (the bench system): factor once, then 1 and 64 right-hand sides b_j = b ^ A[:, c_j] against
    solve_rhs_device; x_j = planted ^ e_{c_j}."""
    n, seed, nrhs = 65536, 1234, 64
    stride = hip.padded_stride(n)
    dev = torch.device("cuda:0")
    A = torch.empty((n, stride), dtype=torch.int64, device=dev)
    hip.synth_device(A.data_ptr(), n, n, stride, seed)
    torch.cuda.synchronize()
    rng = random.Random(98)
    cs = [rng.randrange(n) for _ in range(nrhs)]
    cs[0], cs[1] = n - 1, 0
    w = n // 64
    b = (A[:, w] >> (n % 64)) & 1
    rw = (n + 63) // 64
    weights = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64, device=dev)
    rhs = torch.empty((nrhs, rw), dtype=torch.int64, device=dev)
    for j, c in enumerate(cs):
        col = (A[:, c // 64] >> (c % 64)) & 1
        rhs[j] = ((b ^ col).view(rw, 64) * weights).sum(dim=1)
    torch.cuda.synchronize()
    planted = hip.planted_solution(n, seed)
    f = hip.factor_device(A.data_ptr(), n, n, stride, 0)
    assert f.rank == n
    assert f.device_bytes >= n * 32 * (n // 256) * 2                   # U and T: twice the matrix
    for k in (1, 64):
        got = f.solve_device(rhs.data_ptr(), k, rw)
        want = hip.solve_rhs_device(A.data_ptr(), n, n, stride, rhs.data_ptr(), k, rw, 0)
        for j in range(k):
            assert_same_solution(got[j], want[j], 0)
            x = planted.copy()
            x[cs[j] // 64] ^= np.uint64(1 << (cs[j] % 64))
            assert got[j].status == 0 and np.array_equal(got[j].origin, x), j
        print(f"[factor] 65536^2 nrhs {k}: replay {got[0].stats['ms_eliminate']:.3f} ms backsub {got[0].stats['ms_backsub']:.3f} ms "
              f"total {got[0].stats['ms_total']:.3f} ms; solve_rhs_device total {want[0].stats['ms_total']:.3f} ms")
    f.close()
    del A, rhs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
