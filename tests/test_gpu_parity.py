"""Parity of the HIP path against the CPU oracle / golden fixtures.  All through the C ABI
(hip.py -> libgf2bv_hip.so) or the `_internal` boundary (which calls the same ABI).
Bit-exact: integer work, no tolerance anywhere."""
import random

import numpy as np
import pytest

from gf2bv_amd import LinearSystem, _internal, hip, m4ri_solve
from oracle import gf2_oracle as O
from tests import harness as H
from tests.systems import random_system, structured_system

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1, "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(autouse=True, params=["default", "plain"])
def _heuristics(request, monkeypatch):
    """The whole file runs twice (round 6): as shipped, and with GF2BV_PLAIN=1 -- no stream-pair probes, no XCD pinning of gangs, the
    streams hand over through events instead of counters in memory, every block enqueued with both panel paths (no optimistic
    enqueue).  A box where one of those heuristics mis-fires may cost speed (bench.py: plain_ms_per_step), never an answer."""
    if request.param == "plain":
        if request.node.get_closest_marker("default_only"):
            pytest.skip("exercises a heuristic GF2BV_PLAIN=1 turns off")
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


def assert_same(got: hip.Solution, want: dict, mode: int):
    assert got.status == want["status"]
    assert got.rank == want["rank"]
    assert np.array_equal(got.pivots, want["pivcols"])
    if got.status == 0:
        assert np.array_equal(got.origin, want["origin"])
        if mode == 1:
            assert got.dimension == want["dim"]
            assert np.array_equal(got.basis, want["basis"])


SHAPES = [
    # rows, cols, density, rank_cap, consistent, zero_rows
    (1, 1, .5, None, True, 0), (4, 4, .5, None, True, 1), (8, 5, .5, None, True, 0), (64, 63, .5, None, True, 0),
    (64, 64, .5, None, True, 0), (66, 65, .5, None, True, 0), (128, 127, .5, None, True, 0), (130, 128, .5, None, True, 0),
    (200, 129, .5, 77, True, 0), (300, 200, .5, 40, True, 0), (300, 200, .5, 40, False, 0), (300, 200, .1, None, True, 20),
    (300, 200, .5, 0, True, 300), (640, 256, .05, None, True, 0), (1000, 1000, .5, None, True, 0),
    (1100, 1023, .5, 900, True, 0), (1100, 1024, .5, 900, False, 0), (2100, 2048, .02, None, True, 50),
    (3000, 2500, .5, None, True, 0), (5000, 4097, .5, 4000, True, 0), (9000, 2049, .003, None, True, 0),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", [0, 1])
def test_words_path_matches_oracle(shape, mode):
    rows, cols, dens, cap, cons, zr = shape
    rng = random.Random(hash(shape) & 0xFFFF)
    eqs = random_system(rng, rows, cols, dens, cap, cons, zr)
    aug = O.eqs_to_aug(eqs, cols)
    assert_same(hip.solve_words(aug, rows, cols, mode), O.solve_words(aug, rows, cols, mode), mode)


def test_all_zero_and_identity_systems():
    for rows, cols in ((5, 5), (130, 70)):
        aug = np.zeros((rows, O.words_for(cols)), dtype=np.uint64)
        got = hip.solve_words(aug, rows, cols, 1)
        assert got.status == 0 and got.rank == 0 and got.dimension == cols and got.origin_int() == 0
        assert got.basis_ints() == tuple(1 << i for i in range(cols))         # S4 with r = 0: free = 0..cols-1
        aug[0, cols // 64] = np.uint64(1 << (cols % 64))                       # 0 = 1
        assert hip.solve_words(aug, rows, cols, 1).status == 1
    eqs = [(1 << (i + 1)) | (i & 1) for i in range(100)]                       # x_i = i & 1
    got = hip.solve_words(O.eqs_to_aug(eqs, 100), 100, 100, 1)
    assert got.rank == 100 and got.dimension == 0 and got.origin_int() == sum((i & 1) << i for i in range(100))


def test_update_configurations_agree(monkeypatch):
    """Every instantiation of the bulk-update kernel k_update16 (threads, batches in flight, LDS pipelining, register budget:
    GF2BV_UPDATE = index into the solver's table) gives the same bits."""
    rng = random.Random(77)
    rows, cols = 2600, 2500
    eqs = random_system(rng, rows, cols, .5, 2300, True, 0)
    aug = O.eqs_to_aug(eqs, cols)
    want = O.solve_words(aug, rows, cols, 1)
    for cfg in ("0", "1", "2", "3", "4", "5"):
        monkeypatch.setenv("GF2BV_UPDATE", cfg)
        got = hip.solve_words(aug, rows, cols, 1)
        assert_same(got, want, 1)
        assert (got.stats["panels_per_sweep"], got.stats["tables_per_sweep"], got.stats["table_bits"], got.stats["tile_words"]) == (4, 32, 8, 2)


@pytest.mark.parametrize("kind", ["zero_cols", "dup_cols", "dup_head", "dead_head"])
def test_dense_systems_that_leave_the_fast_search_paths(kind):
    """Dense candidates send the first chunk of a panel through the column-wise elimination and nearly full bases
    through the targeted completion; these systems make those paths come up short (missing pivots that never turn
    up, a first chunk of rank 5, dead and duplicate rows at the head of the scan) so that the fall-backs, the packed
    incomplete lists and the merges run -- against the oracle, both modes, several sizes (one and several units)."""
    rng = random.Random(sum(map(ord, kind)))
    for rows, cols in ((70, 64), (200, 130), (700, 640), (2600, 2500), (5000, 1100)):
        eqs = structured_system(rng, rows, cols, kind)
        aug = O.eqs_to_aug(eqs, cols)
        for mode in (0, 1):
            assert_same(hip.solve_words(aug, rows, cols, mode), O.solve_words(aug, rows, cols, mode), mode)


def test_digits_path_equals_words_path():
    """The CPython-digit pack kernel (replaces _internal.c:403-426) against int.to_bytes packing."""
    rng = random.Random(5)
    for rows, cols in ((70, 64), (200, 129), (500, 389)):
        eqs = random_system(rng, rows, cols, .5, None, True, 3)
        eqs[1] = -eqs[1]                                   # sign ignored
        eqs[2] |= 1 << (cols + 7)                          # bits above cols ignored
        digits, off = [], [0]
        for e in eqs:
            v, d = abs(e), []
            while v:
                d.append(v & ((1 << 30) - 1))
                v >>= 30
            digits += d
            off.append(len(digits))
        a = hip.solve_digits(np.array(digits + [0], dtype=np.uint32), np.array(off, dtype=np.int64), 30, rows, cols, 1)
        want = O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, 1)
        assert_same(a, want, 1)
        sp = m4ri_solve(eqs, cols, 1)
        assert sp.origin == a.origin_int() and sp.basis == a.basis_ints()


def test_internal_boundary_kats():
    sp = m4ri_solve([15, 20, 11, 0], 4, 1)                # SURVEY 8a-S hand-derived KAT
    assert (sp.dimension, sp.origin, sp.basis, list(sp)) == (1, 0b0001, (0b0101,), [1, 4])
    assert m4ri_solve([15, 20, 11, 0], 4, 0) == 1
    assert m4ri_solve([2, 3, 0], 1, 0) is None            # x = 0 and x = 1
    assert m4ri_solve([2, 3, 0], 1, 1) is None
    assert type(sp) is _internal.AffineSpace


def test_golden_fixtures_through_linear_system():
    G = H.GOLDEN
    e = G["readme4"]
    lin = LinearSystem(e["sizes"])
    a, b, c, d = lin.gens()
    zeros = [a ^ b ^ c ^ 1, b ^ d, a ^ c ^ 1]
    assert [hex(q) for q in H.padded_eqs(lin, zeros)] == e["eqs"]
    assert [list(s) for s in lin.solve_all(zeros)] == e["expect"]["solve_all"]
    assert list(lin.solve_one(zeros)) == e["expect"]["solve_one"]
    for key, inp in (("simple_linear", None), ("simple_affine", tuple(int(v, 16) for v in G["simple_affine"]["input"]))):
        lin, zeros, expected = H.simple_system(inp)
        sols = list(lin.solve_all(zeros))
        ref = O.m4ri_solve(H.padded_eqs(lin, zeros), 128, 1)
        assert sols == [lin.convert_sol(s) for s in ref]                      # same set AND same Gray order
        assert all(H.magic(*s) == tuple(expected) for s in sols)
        one = lin.solve_one(zeros)
        assert one == lin.convert_sol(ref.origin) and all(lin.evaluate(z, one) == 0 for z in zeros)
    lin, zeros, state, outs = H.xoshiro_system(1, 10)
    assert list(lin.solve_all(zeros)) == [state]
    space = lin.solve_raw_space(zeros)
    assert space.dimension == 0 and space.basis == ()


def test_quadratic_golden_on_the_gpu():
    """golden.json["quadratic"] through QuadraticSystem.solve_all / solve_one: the brute-force solution set."""
    e = H.GOLDEN["quadratic"]
    q, zeros = H.quadratic_small_system(e["consts"])
    sols = sorted(list(s) for s in q.solve_all(zeros))
    assert sols == e["expect"]["solutions"]
    assert list(q.solve_one(zeros)) in e["expect"]["solutions"]
    raw = q.solve_raw_space(zeros)
    ref = O.m4ri_solve(H.padded_eqs(q, zeros), q._cols, 1)
    assert (raw.origin, raw.basis) == (ref.origin, ref.basis)


@pytest.mark.parametrize("name", sorted(H.NLFSR_KINDS))
def test_nlfsr_state_recovery(name):
    """examples/nlfsr.py:36-64: 2**14 + 1000 outputs of the filtered 128-bit LFSR -> ~8700 linearised equations in
    8256 unknowns -> the secret state, by solve_all and by solve_one."""
    q, zeros, secret = H.nlfsr_system(name, 2 ** 14 + 1000)
    assert list(q.solve_all(zeros)) == [(secret,)]
    assert q.solve_one(zeros) == (secret,)


@pytest.mark.parametrize("bs,samples", H.MT_VARIANTS)
def test_mt19937_state_recovery(bs, samples, _heuristics):
    """examples/mt.py: all six variants, sol == state of random.Random(3142)."""
    lin, zeros, state, out = H.mt19937_system(bs, samples)
    sol = lin.solve_one(zeros)
    assert sol == state
    rng = H.MT19937(sol)
    assert all(rng.getrandbits(bs) == o for o in out)
    # which pool of k_block_sparse the variant needs (gf2bv_stats::sparse_blocks by pool size: 1024 / 4096 / 6144 rows)
    st = _mt_stats(bs, samples, _heuristics, lin, zeros)
    assert st["handover_retries"] == 0
    if _heuristics == "plain":                        # (no optimistic enqueue: the search is never switched on)
        assert st["sparse_blocks"] == [0, 0, 0] and st["sparse_giveups"] == 0
    else:
        assert sum(st["sparse_blocks"]) > 0
        if bs == 1:
            assert st["sparse_blocks"][2] > 0         # one bit per output: 4500-5000 rows carry a bit in a block's window


_MT_STATS = {}


def _mt_stats(bs, samples, heuristics, lin=None, zeros=None):
    """stats of the variant's system through solve_words, once per variant and leg"""
    if (bs, samples, heuristics) not in _MT_STATS:
        if lin is None:
            lin, zeros, _, _ = H.mt19937_system(bs, samples)
        eqs = H.padded_eqs(lin, zeros)
        st = hip.solve_words(O.eqs_to_aug(eqs, lin._cols), len(eqs), lin._cols, 0).stats
        print(f"[mt19937] {heuristics} {bs} bits x {samples or 'all'}: sparse pools {st['sparse_blocks']} give-ups {st['sparse_giveups']} "
              f"{st['sparse_giveup_why']} nz_max {st['sparse_nz_max']} fast_blocks {st['fast_blocks']}")
        _MT_STATS[(bs, samples, heuristics)] = st
    return _MT_STATS[(bs, samples, heuristics)]


def test_mt19937_some_variant_runs_the_middle_pool(_heuristics):
    """Behind test_mt19937_state_recovery, whose solves it shares: the middle pool of k_block_sparse (4096 rows) is run by at least one
    of the six variants, so the recoveries exercise all three instantiations."""
    pools = {bs: _mt_stats(bs, samples, _heuristics)["sparse_blocks"] for bs, samples in H.MT_VARIANTS}
    assert any(p[1] > 0 for p in pools.values()) == (_heuristics == "default"), pools      # (GF2BV_PLAIN=1: the search is never switched on)


def test_synthetic_generator_device_equals_host():
    for n, seed in ((100, 5), (1000, 6), (2049, 7)):
        stride = hip.padded_stride(n)
        buf = hip.DeviceBuffer(n * stride * 8)
        hip.synth_device(buf.ptr, n, n, stride, seed)
        dev = buf.download().reshape(n, stride)
        host = O.gen_synthetic(n, n, seed, stride)
        assert np.array_equal(dev, host)
        assert hip.residual_device(buf.ptr, n, n, stride, O.planted_solution(n, seed)) == 0
        x = O.planted_solution(n, seed).copy()
        x[0] ^= np.uint64(1)
        assert hip.residual_device(buf.ptr, n, n, stride, x) == O.check_solution(host, n, n, x) > 0
        buf.free()


def test_device_resident_and_batch_paths():
    n, seeds = 3000, [21, 22, 23, 24, 25]
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(len(seeds) * n * stride * 8)
    for i, s in enumerate(seeds):
        hip.synth_device(buf.ptr + i * n * stride * 8, n, n, stride, s)
    sols = hip.solve_batch_device(buf.ptr, len(seeds), n * stride, n, n, stride, 0)
    for s, sol in zip(seeds, sols):
        want = O.solve_words(O.gen_synthetic(n, n, s), n, n, 0)
        assert_same(sol, want, 0)
    hip.synth_device(buf.ptr, n, n, stride, seeds[0])
    one = hip.solve_device(buf.ptr, n, n, stride, 1, time_kernels=True)
    assert_same(one, O.solve_words(O.gen_synthetic(n, n, seeds[0]), n, n, 1), 1)
    assert one.stats["ms_sweep"] > 0 and 1 <= one.stats["n_sweeps"] <= (n + 63) // 64
    with pytest.raises(ValueError):
        hip.solve_device(buf.ptr + 8, n, n, stride, 0)               # misaligned
    with pytest.raises(ValueError):
        hip.solve_device(buf.ptr, n, n, stride - 1, 0)               # stride % 16 != 0
    buf.free()


@pytest.mark.parametrize("gang", ["1", "2", "3", "8"])
def test_gang_batch_parity(monkeypatch, gang):
    """Lock-step gangs (blockIdx.y = system): full-rank, rank-deficient, sparse, zero-row and inconsistent
    systems side by side, a system count that is no multiple of the gang size, padded system stride, both modes."""
    monkeypatch.setenv("GF2BV_GANG", gang)
    rng = random.Random(4242)
    rows, cols = 1100, 1000
    stride = hip.padded_stride(cols, 2) + 2                    # even, not a multiple of 16 words
    sys_stride = rows * stride + 6
    systems = [random_system(rng, rows, cols),
               random_system(rng, rows, cols, .5, 600),
               random_system(rng, rows, cols, .01, None, True, 50),
               random_system(rng, rows, cols, .5, 900, False),
               random_system(rng, rows, cols, .5, 1),
               [0] * rows,
               random_system(rng, rows, cols)]
    host = np.zeros((len(systems), sys_stride), dtype=np.uint64)
    for i, eqs in enumerate(systems):
        host[i, :rows * stride] = O.eqs_to_aug(eqs, cols, stride).reshape(-1)
    buf = hip.DeviceBuffer(host.nbytes)
    buf.upload(host)
    for mode in (0, 1):
        sols = hip.solve_batch_device(buf.ptr, len(systems), sys_stride, rows, cols, stride, mode)
        for eqs, sol in zip(systems, sols):
            assert_same(sol, O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, mode), mode)
    assert np.array_equal(buf.download().reshape(host.shape), host)          # inputs untouched
    buf.free()


@pytest.mark.parametrize("gang,pin,nt,wgs", [("8", "1", "1", "32"), ("16", "1", "1", "3"), ("16", "1", "0", "32"), ("8", "0", "1", "32"),
                                              ("16", "1", "1", "64")])
def test_gang_bulk_update_with_a_system_per_xcd(monkeypatch, gang, pin, nt, wgs):
    """Round 4: gangs of a multiple of 8 systems launch their bulk update as ONE line of workgroups decoded so that a system's
    workgroups sit on one XCD, one system after the other there (k_update16: xcd_nsys), with streaming row accesses
    (GF2BV_GANG_NT) -- a different grid shape, span partition and instance than single systems use.  16 systems of mixed kind
    (+ a remainder gang of 3: the plain grid), both modes, against the oracle; pinning / streaming off and odd workgroup
    counts per system give the same bits."""
    monkeypatch.setenv("GF2BV_GANG", gang)
    monkeypatch.setenv("GF2BV_XCD_PIN", pin)
    monkeypatch.setenv("GF2BV_GANG_NT", nt)
    monkeypatch.setenv("GF2BV_XCD_WGS", wgs)
    rng = random.Random(8242)
    rows, cols = 2700, 2600
    kinds = [(None, .5, True), (600, .5, True), (None, .01, True), (900, .5, False), (1, .5, True), (cols - 1, .5, True)]
    systems = [random_system(rng, rows, cols, d, cap, cons, 0) for cap, d, cons in (kinds * 4)[:18]] + [[0] * rows]
    augs = np.stack([O.eqs_to_aug(e, cols) for e in systems])
    for mode in (0, 1):
        got = hip.solve_batch_words(augs, rows, cols, mode)
        for a, g in zip(augs, got):
            assert_same(g, O.solve_words(a, rows, cols, mode), mode)
    assert got[0].stats["gang_systems"] == int(gang)


@pytest.mark.parametrize("threads", ["2", "1", "3"])
def test_batched_list_of_int_boundary(monkeypatch, threads):
    """m4ri_solve_many / LinearSystem.solve_*_many == the single-system calls, element by element (gangs of 3 taken by 1 / 2 / 3 host
    threads, each uploading and packing the digits of the gangs it takes)."""
    monkeypatch.setenv("GF2BV_GANG", "3")
    monkeypatch.setenv("GF2BV_BATCH_THREADS", threads)
    rng = random.Random(99)
    cols = 130
    systems = [random_system(rng, 200, cols), random_system(rng, 200, cols, .5, 90), random_system(rng, 200, cols, .5, 100, False),
               [0] * 200, random_system(rng, 200, cols, .02), [-e for e in random_system(rng, 200, cols, .5, 129)],
               [e | (rng.getrandbits(40) << (cols + 1)) for e in random_system(rng, 200, cols)]]     # junk above bit cols
    for mode in (0, 1):
        got = _internal.m4ri_solve_many(systems, cols, mode)
        for eqs, g in zip(systems, got):
            w = m4ri_solve(list(eqs), cols, mode)
            o = O.m4ri_solve(list(eqs), cols, mode)
            if mode == 0 or w is None:
                assert g == w == o
            else:
                assert (g.dimension, g.origin, g.basis) == (w.dimension, w.origin, w.basis) == (o.dimension, o.origin, o.basis)
                if g.dimension <= 8:              # never enumerate a big space: 2**dim Python ints
                    assert list(g) == list(w)
    # LinearSystem level: xoshiro-style instances with different observations, plus a contradictory one
    lin = LinearSystem([8, 8])
    a, b = lin.gens()
    zlist = []
    for k in range(5):
        x, y = rng.getrandbits(8), rng.getrandbits(8)
        zlist.append([(a ^ b.rotl(3)) ^ (x ^ (((y << 3) | (y >> 5)) & 255)), (a & 0xF0) ^ (x & 0xF0), b ^ y])
    zlist.append([a ^ 1, a ^ 2])
    zlist.append([1])
    one = lin.solve_one_many(zlist)
    assert one == [lin.solve_one(z) for z in zlist]
    assert one[-1] is None and one[-2] is None and all(o is not None for o in one[:5])
    spaces = lin.solve_raw_space_many(zlist)
    for z, sp in zip(zlist, spaces):
        ref = lin.solve_raw_space(z)
        assert (sp is None) == (ref is None)
        if sp is not None:
            assert (sp.dimension, sp.origin, sp.basis) == (ref.dimension, ref.origin, ref.basis)


@pytest.mark.parametrize("chunk_mb, devs", [("2", None), ("1", None), ("3", [0, 0, 0])])
def test_batched_list_of_int_in_chunks(monkeypatch, chunk_mb, devs):
    """m4ri_solve_many hands the digits over in chunks of whole systems (GF2BV_BATCH_CHUNK_MB), the gather of one chunk under the solve of
    the one before: 7 systems of 0.94 MB in chunks of 2 / 1 / 4 systems, answers in input order and equal to the oracle's."""
    monkeypatch.setenv("GF2BV_BATCH_CHUNK_MB", chunk_mb)
    rng = random.Random(4711)
    rows, cols = 2700, 2600
    kinds = [(None, .5, True), (700, .5, True), (None, .5, False), (None, .01, True), (cols - 1, .5, True), (3, .5, True)]
    systems = [random_system(rng, rows, cols, d, cap, cons, 0) for cap, d, cons in kinds] + [[0] * rows]
    for mode in (0, 1):
        got = _internal.m4ri_solve_many(systems, cols, mode) if devs is None else _internal.m4ri_solve_many(systems, cols, mode, devs)
        assert len(got) == len(systems)
        for eqs, g in zip(systems, got):
            o = O.m4ri_solve(list(eqs), cols, mode)
            if mode == 0 or o is None:
                assert g == o
            else:
                assert (g.dimension, g.origin, g.basis) == (o.dimension, o.origin, o.basis)
    # an item that is not an int, found while the first chunk is already being solved... is found BEFORE anything runs (type check first)
    bad = [list(e) for e in systems]
    bad[5][7] = "x"
    with pytest.raises(TypeError):
        _internal.m4ri_solve_many(bad, cols, 0)
    assert hip.host_pool_trim() >= 0


def test_batch_sharded_over_devices_from_the_python_boundary(monkeypatch):
    """m4ri_solve_many(..., devices): contiguous shares, one host thread per listed device inside the library
    (gf2bv_solve_batch_digits_multi).  The box has one GPU, so the device list names it twice or three times -- the shares
    then run as concurrent gangs on it -- and the answer must equal the one-device call and the oracle, in input order."""
    monkeypatch.setenv("GF2BV_GANG", "2")
    rng = random.Random(404)
    cols = 190
    systems = [random_system(rng, 230, cols, .5, cap) for cap in (None, 64, 189, 1, None, 100, None)] + [[0] * 230]
    assert _internal.device_count() >= 1 and _internal.get_default_device() == 0
    for mode in (0, 1):
        one = _internal.m4ri_solve_many(systems, cols, mode, 0)
        for devs in ([0, 0], [0, 0, 0], None, "all", [0] * 8, [0] * 11):
            got = _internal.m4ri_solve_many(systems, cols, mode, devs)
            for eqs, g, w in zip(systems, got, one):
                o = O.m4ri_solve(list(eqs), cols, mode)
                if mode == 0 or w is None:
                    assert g == w == o
                else:
                    assert (g.dimension, g.origin, g.basis) == (w.dimension, w.origin, w.basis) == (o.dimension, o.origin, o.basis)
                    assert g.device == 0
    assert m4ri_solve(list(systems[0]), cols, 0, 0) == m4ri_solve(list(systems[0]), cols, 0)
    with pytest.raises(ValueError, match="out of range"):
        _internal.m4ri_solve_many(systems, cols, 0, [0, _internal.device_count()])
    with pytest.raises(ValueError, match="'all'"):
        _internal.m4ri_solve_many(systems, cols, 0, "every")
    lin = LinearSystem([8, 8])
    a, b = lin.gens()
    zl = [[a ^ b ^ k, b ^ (k * 7 & 255)] for k in range(9)]
    assert lin.solve_one_many(zl, devices=[0, 0]) == [lin.solve_one(z) for z in zl]


def test_randomised_shapes_and_configs(monkeypatch):
    """A seeded sweep over shapes, densities, rank caps, zero rows, modes and k_update configurations
    (tests/manual/stress_parity.py runs the open-ended version of this on the GPU box)."""
    rng = random.Random(20260928)
    for it in range(40):
        cols = rng.choice([rng.randint(1, 130), rng.randint(131, 600), 64 * rng.randint(1, 9), 256 * rng.randint(1, 3) + rng.choice([-1, 0, 1])])
        rows = cols + rng.choice([0, 1, rng.randint(0, 64), rng.randint(0, cols), rng.randint(0, 2 * cols)])
        density = rng.choice([0.5, 0.5, 0.1, 0.02])
        cap = rng.choice([None, None, rng.randint(1, cols), max(1, cols - rng.randint(0, 5))])
        mode = rng.randint(0, 1)
        monkeypatch.setenv("GF2BV_UPDATE", rng.choice(["0", "1", "2", "3", "4", "5"]))
        eqs = random_system(rng, rows, cols, density, cap, rng.random() < 0.8, min(rng.choice([0, 0, rows // 3]), rows - 1))
        rng.shuffle(eqs)
        aug = O.eqs_to_aug(eqs, cols)
        assert_same(hip.solve_words(aug, rows, cols, mode), O.solve_words(aug, rows, cols, mode), mode)


def test_batch_words_host_entry():
    """hip.solve_batch_words: host-resident packed systems, odd stride (padded internally), both modes."""
    rng = random.Random(5)
    rows, cols = 400, 321                                   # 6 words per row: even; 321 + 1 bits -> stride 6
    systems = [random_system(rng, rows, cols, .5, cap) for cap in (None, 200, 1)]
    for stride in (6, 7):
        augs = np.stack([O.eqs_to_aug(e, cols, stride) for e in systems])
        for mode in (0, 1):
            for sol, eqs in zip(hip.solve_batch_words(augs, rows, cols, mode), systems):
                assert_same(sol, O.solve_words(O.eqs_to_aug(eqs, cols), rows, cols, mode), mode)


def test_concurrent_gangs_saturating_the_chip(monkeypatch):
    """Two host threads, each driving gangs whose bulk updates fill every CU: search workgroups get dispatched
    late, which once let a unit read the *next* panel's state (every unit must take part in the arrival count)."""
    monkeypatch.setenv("GF2BV_GANG", "6")
    n, nsys = 16384, 24
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(nsys * n * stride * 8)
    for i in range(nsys):
        hip.synth_device(buf.ptr + i * n * stride * 8, n, n, stride, 7000 + i)
    for rep in range(3):
        sols = hip.solve_batch_device(buf.ptr, nsys, n * stride, n, n, stride, 0)
        for i, s in enumerate(sols):
            assert s.solved and s.rank >= n - 8
            assert hip.residual_device(buf.ptr + i * n * stride * 8, n, n, stride, s.origin) == 0
    buf.free()


def test_search_handover_without_co_residency(monkeypatch):
    """GF2BV_SELF_WAIT_US=0: the first search unit of a dense panel never waits for the rest of its launch -- the
    situation on a chip where its workgroups are not co-resident -- and the last arriver publishes from its record.
    Same results, and the hand-over path is seen to have run."""
    monkeypatch.setenv("GF2BV_SELF_WAIT_US", "0")
    monkeypatch.setenv("GF2BV_FAST", "0")           # (the one-launch block search would bypass the per-panel searches on these dense systems)
    from tests.general_cases import COUNTERS as general_counters
    rng = random.Random(77)
    handovers = 0
    for rows, cols, cap in ((3000, 2500, None), (5000, 4097, 4000), (9000, 8200, None)):
        eqs = random_system(rng, rows, cols, .5, cap, True, 0)
        aug = O.eqs_to_aug(eqs, cols)
        for mode in (0, 1):
            got = hip.solve_words(aug, rows, cols, mode)
            assert_same(got, O.solve_words(aug, rows, cols, mode), mode)
            handovers += got.stats["search_handovers"]
            # who publishes is timing, how a panel is published is not: the same counts when unit 0 waits as long as it takes
            with monkeypatch.context() as m:
                m.setenv("GF2BV_SELF_WAIT_US", "1000000")
                waited = hip.solve_words(aug, rows, cols, mode).stats
            assert [got.stats[k] for k in general_counters] == [waited[k] for k in general_counters]
            assert got.stats["general_unit0"] + got.stats["general_adopted"] + got.stats["general_merged"] == (cols + 63) // 64
    assert handovers > 0
    n, stride = 16384, hip.padded_stride(16384)
    buf = hip.DeviceBuffer(n * stride * 8)
    hip.synth_device(buf.ptr, n, n, stride, 99)
    s = hip.solve_device(buf.ptr, n, n, stride, 0)
    assert s.solved and hip.residual_device(buf.ptr, n, n, stride, s.origin) == 0 and s.stats["search_handovers"] > 0
    buf.free()


def test_concurrent_gangs_next_to_a_saturating_stream(monkeypatch):
    """Gangs from two host threads while a third keeps every CU busy with the streaming kernel of the ceiling
    measurement: panel-search workgroups are dispatched late or not together; the solves must stay correct
    (they used to rely on the co-residency of a launch's workgroups and could report an internal time-out)."""
    import threading
    monkeypatch.setenv("GF2BV_GANG", "6")
    n, nsys = 8192, 18
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(nsys * n * stride * 8)
    for i in range(nsys):
        hip.synth_device(buf.ptr + i * n * stride * 8, n, n, stride, 8100 + i)
    stop = threading.Event()

    def hog():
        while not stop.is_set():
            hip.stream_ceiling(1 << 30)

    t = threading.Thread(target=hog)
    t.start()
    try:
        for rep in range(2):
            sols = hip.solve_batch_device(buf.ptr, nsys, n * stride, n, n, stride, 0)
            for i, s in enumerate(sols):
                assert s.solved and s.rank >= n - 8
                assert hip.residual_device(buf.ptr + i * n * stride * 8, n, n, stride, s.origin) == 0
    finally:
        stop.set()
        t.join()
    buf.free()


def test_one_launch_block_search_and_its_fallbacks(monkeypatch):
    """k_block_fast: dense blocks are factorised from a few hundred candidate rows in one launch (fast_blocks > 0, same
    bits as the per-panel searches: GF2BV_FAST=0), and whatever it cannot handle -- a rank cap in the middle of the
    matrix, sparse rows, duplicate columns, fewer alive rows than candidates -- falls back block by block."""
    rng = random.Random(321)
    cases = [(3000, 2900, None, .5), (5000, 4097, 2600, .5), (2600, 2500, None, .02), (1400, 1300, 1290, .5)]
    for rows, cols, cap, dens in cases:
        eqs = random_system(rng, rows, cols, dens, cap, True, 0)
        aug = O.eqs_to_aug(eqs, cols)
        for mode in (0, 1):
            want = O.solve_words(aug, rows, cols, mode)
            monkeypatch.setenv("GF2BV_FAST", "1")
            fast = hip.solve_words(aug, rows, cols, mode)
            monkeypatch.setenv("GF2BV_FAST", "0")
            slow = hip.solve_words(aug, rows, cols, mode)
            assert_same(fast, want, mode)
            assert_same(slow, want, mode)
            assert slow.stats["fast_blocks"] == 0
            if dens == .5 and cap is None:
                assert fast.stats["fast_blocks"] >= (cols // 256) - 2
            # (a sparse system fills in as it is eliminated: its later blocks may well go through the fast search)
    for kind in ("zero_cols", "dup_cols"):
        eqs = structured_system(rng, 2600, 2500, kind)
        aug = O.eqs_to_aug(eqs, 2500)
        monkeypatch.setenv("GF2BV_FAST", "1")
        assert_same(hip.solve_words(aug, 2600, 2500, 1), O.solve_words(aug, 2600, 2500, 1), 1)


def test_back_substitution_paths_agree(monkeypatch):
    """solve_one's blocked parity back-substitution vs the general multi-RHS sweep path (solve_all's)."""
    rng = random.Random(31)
    for rows, cols, cap in ((700, 650, 500), (2200, 2100, None), (5000, 4097, 4000)):
        eqs = random_system(rng, rows, cols, .5, cap, True, 0)
        aug = O.eqs_to_aug(eqs, cols)
        want = O.solve_words(aug, rows, cols, 0)
        monkeypatch.delenv("GF2BV_YSWEEP", raising=False)
        a = hip.solve_words(aug, rows, cols, 0)
        monkeypatch.setenv("GF2BV_YSWEEP", "1")
        b = hip.solve_words(aug, rows, cols, 0)
        monkeypatch.delenv("GF2BV_YSWEEP", raising=False)
        assert_same(a, want, 0)
        assert_same(b, want, 0)
    # kernel bases of up to 7 vectors take the parity path as well (one pass over U for all right-hand sides)
    for rows, cols, cap in ((900, 800, 797), (2300, 2200, 2193), (1500, 1029, 1028)):
        eqs = random_system(rng, rows, cols, .5, cap, True, 0)
        aug = O.eqs_to_aug(eqs, cols)
        want = O.solve_words(aug, rows, cols, 1)
        assert 1 <= want["dim"] <= 7
        monkeypatch.delenv("GF2BV_YSWEEP", raising=False)
        a = hip.solve_words(aug, rows, cols, 1)
        monkeypatch.setenv("GF2BV_YSWEEP", "1")
        b = hip.solve_words(aug, rows, cols, 1)
        monkeypatch.delenv("GF2BV_YSWEEP", raising=False)
        assert_same(a, want, 1)
        assert_same(b, want, 1)


def test_device_path_strides_and_untouched_input():
    """Row-major device input with an even but non-multiple-of-16 stride; the input must survive the solve."""
    n, seed = 1000, 77
    for stride in (O.words_for(n), O.words_for(n) + 2, 50):
        stride += stride & 1
        host = O.gen_synthetic(n, n, seed, stride)
        buf = hip.DeviceBuffer(n * stride * 8)
        buf.upload(host)
        got = hip.solve_device(buf.ptr, n, n, stride, 1)
        assert_same(got, O.solve_words(host, n, n, 1), 1)
        assert np.array_equal(buf.download().reshape(n, stride), host)
        buf.free()


def test_concurrent_solves_from_python_threads():
    """The reference drops the GIL around the solve (_internal.c:429-492); so does the shim, and every call owns
    its streams and buffers: four Python threads solving different systems at once must all be right."""
    from concurrent.futures import ThreadPoolExecutor
    rng = random.Random(404)
    jobs = []
    for rows, cols, cap in ((900, 800, None), (1300, 1200, 1000), (700, 650, 300), (2100, 2048, None)) * 3:
        eqs = random_system(rng, rows, cols, .5, cap, True, 0)
        jobs.append((eqs, cols))

    def run(job):
        eqs, cols = job
        sp = m4ri_solve(eqs, cols, 1)
        return sp.origin, sp.basis

    with ThreadPoolExecutor(4) as ex:
        got = list(ex.map(run, jobs))
    for (eqs, cols), (origin, basis) in zip(jobs, got):
        ref = O.m4ri_solve(eqs, cols, 1)
        assert (origin, basis) == (ref.origin, ref.basis)


def test_stream_handover_through_memory_vs_events(monkeypatch):
    """The two streams of a solve hand over through progress counters in device memory (k_gate / stream memory
    operations) instead of events: same bits either way, also when a block poisons the optimistic enqueue and the host
    resumes (rank cap in the middle), and with more concurrent solves than the runtime has hardware queues -- every wait
    targets work submitted before the waiter, so sharing a queue cannot deadlock (a gate that gave up would surface as an
    error from the solve)."""
    from concurrent.futures import ThreadPoolExecutor
    rng = random.Random(909)
    jobs = []
    for rows, cols, cap in ((2700, 2600, None), (5000, 4097, 2600), (2300, 2200, 2193)):
        eqs = random_system(rng, rows, cols, .5, cap, True, 0)
        aug = O.eqs_to_aug(eqs, cols)
        want = O.solve_words(aug, rows, cols, 1)
        monkeypatch.setenv("GF2BV_FLAG_SYNC", "0")
        assert_same(hip.solve_words(aug, rows, cols, 1), want, 1)
        monkeypatch.setenv("GF2BV_FLAG_SYNC", "1")
        assert_same(hip.solve_words(aug, rows, cols, 1), want, 1)
        jobs.append((aug, rows, cols, want))
    monkeypatch.delenv("GF2BV_FLAG_SYNC", raising=False)

    def run(job):
        aug, rows, cols, _ = job
        return hip.solve_words(aug, rows, cols, 1)

    with ThreadPoolExecutor(12) as ex:
        got = list(ex.map(run, jobs * 8))
    for job, g in zip(jobs * 8, got):
        assert_same(g, job[3], 1)


def test_panel_kernels_fit_beside_the_bulk_update():
    """The panel path of block b + 1 runs BESIDE the bulk update of block b: its kernels must fit into
    what an update workgroup leaves of a CU -- 512 VGPRs per SIMD lane minus the update's two wavefronts, 160 KiB of LDS
    minus its tables.  A kernel that outgrows that still gives the right bits, it just cannot start before an update
    workgroup retires (seen once: k_block_fast at 217 VGPRs and 180-280 us per launch in the bulk-bound part of 65536^2)."""
    res = hip.kernel_resources()
    upd = res["update"]
    free_vgprs = 512 - 2 * ((upd["vgprs"] + 7) // 8 * 8)
    free_lds = 160 * 1024 - upd["lds"]
    for name in ("block_fast", "narrow_all", "prio_window", "panel_step", "block_fast_narrow", "block_sparse"):
        assert res[name]["vgprs"] <= free_vgprs, (name, res)
        assert res[name]["lds"] <= free_lds, (name, res)
    # the outer pass of the two-level elimination (late round 5: sixteen wavefronts, 12 row segments per lane) runs under a budget
    # of 120 registers -- four wavefronts per SIMD and room for the gates of the panel path beside them; the compiler meets it
    # with a few spills OUTSIDE the lookup loop (32 bytes per lane).  A build that spills the loop (seen: 3500 bytes per lane,
    # 30 x slower, still the right bits) fails here
    outer = res["update_outer"]
    assert outer["scratch"] <= 64 and outer["vgprs"] <= 120 and outer["lds"] <= 160 * 1024, outer


def test_stream_ceiling_reports_sane_rates():
    c = hip.stream_ceiling(1 << 30)
    assert 1000 < c["rmw_gbs"] < 8000 and 1000 < c["read_gbs"] < 8000


def test_medium_dense_full_parity():
    """8192 x 8192 dense: full bit-for-bit comparison with the CPU oracle."""
    n, seed = 8192, 1234
    aug = O.gen_synthetic(n, n, seed)
    got = hip.solve_words(aug, n, n, 1)
    assert_same(got, O.solve_words(aug, n, n, 1), 1)


def test_large_dense_properties():
    """BASELINE configs[1] size (65536 x 65536): size-independent properties instead of a CPU re-solve:
    A x = b on a pristine copy (independent residual kernel), free variables zero, pivots strictly
    increasing, and -- when the matrix is full rank -- x equals the planted solution (uniqueness)."""
    _dense_properties(65536, 1234)


@pytest.mark.timeout(300)
def test_target_262144_properties():
    """The north-star size (SURVEY 8a "target": 262144 x 262144, 8 GiB + the 8 GiB working copy): the same properties on the
    FULL-RANK seed 1242 (round 4; tools/find_full_rank_seed.py): rank = N, so A x = b has exactly one solution and equality with
    the generator's planted vector is bit-exactness by uniqueness (SURVEY hard part 7) -- asserted, not conditional."""
    sol = _dense_properties(262144, 1242)
    assert sol.rank == 262144 and np.array_equal(sol.origin, hip.planted_solution(262144, 1242))


def _rank_profile_properties(n, seed):
    """A rank-deficient dense system in mode 1: what pins the COLUMN RANK PROFILE without a CPU re-solve.  The kernel vector of
    free column f expresses column f by pivot columns; under the column rank profile (M4RI's PLE, contract S1) only pivot
    columns LEFT of f can occur -- so the vector's highest set bit is f itself.  Checked for every vector in M4RI's order (S4:
    free = the tail of the transposition replay), together with pivots = sorted complement of the free columns, A (origin ^ v) = b
    by the independent residual kernel (v is in the kernel), origin zero at every free column."""
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(n * stride * 8)
    hip.synth_device(buf.ptr, n, n, stride, seed)
    sp = hip.solve_device(buf.ptr, n, n, stride, 1)
    hip.synth_device(buf.ptr, n, n, stride, seed)
    assert sp.status == 0 and 1 <= sp.dimension <= 8 and sp.rank == n - sp.dimension and sp.stats["handover_retries"] == 0
    piv = sp.pivots
    assert (np.diff(piv) > 0).all()
    order = list(range(n))
    for i, c in enumerate(piv.tolist()):
        order[i], order[c] = order[c], order[i]
    free = order[sp.rank:]
    assert sorted(free) == np.setdiff1d(np.arange(n), piv).tolist()
    assert hip.residual_device(buf.ptr, n, n, stride, sp.origin) == 0
    for f, v in zip(free, sp.basis):
        top = int(np.flatnonzero(v)[-1])
        assert 64 * top + int(v[top]).bit_length() - 1 == f                 # nothing right of the free column
        assert [g for g in free if (int(v[g >> 6]) >> (g & 63)) & 1] == [f]  # S4: zero at every other free column
        assert not (int(sp.origin[f >> 6]) >> (f & 63)) & 1
        assert hip.residual_device(buf.ptr, n, n, stride, sp.origin ^ v) == 0
    buf.free()
    return sp


def test_rank_deficient_65536_keeps_the_column_rank_profile():
    for seed in range(1235, 1260):                          # (P(full rank) = 0.29: the first deficient seed after the headline's)
        stride = hip.padded_stride(65536)
        buf = hip.DeviceBuffer(65536 * stride * 8)
        hip.synth_device(buf.ptr, 65536, 65536, stride, seed)
        rank = hip.solve_device(buf.ptr, 65536, 65536, stride, 0).rank
        buf.free()
        if rank < 65536:
            break
    _rank_profile_properties(65536, seed)


@pytest.mark.timeout(300)
def test_rank_deficient_262144_keeps_the_column_rank_profile():
    """seed 1234 at the north-star size has rank 262143 (round 3's bench seed): the second case beside the full-rank one."""
    sp = _rank_profile_properties(262144, 1234)
    assert sp.dimension == 1


@pytest.mark.timeout(300)
def test_two_level_beyond_the_target_size_hands_over_without_retry():
    """327680 x 327680 (12.5 GiB + the working copy; ~2.5 s): the two-level schedule with 1280 row blocks per all-rows launch.
    Round 3 built a look-ahead that waited for the bulk update INSIDE k_prio_window: its workgroups, spinning with 17 KiB of LDS
    each, sat on every CU before the bulk update they were waiting for had been placed (133 KiB of a CU) -- a deadlock until the
    gate time-out; every solve of this size ran twice (9.9 s instead of 2.5 s) and was still bit-exact, so only the retry
    counter shows it."""
    _dense_properties(327680, 1234, repeat=False)


@pytest.mark.timeout(120)
def test_tall_system_hands_over_without_retry():
    """400000 x 3000: 1563 row blocks per all-rows launch on a one-level schedule; the result against the residual check."""
    rows, cols = 400000, 3000
    stride = hip.padded_stride(cols)
    buf = hip.DeviceBuffer(rows * stride * 8)
    hip.synth_device(buf.ptr, rows, cols, stride, 77)
    sol = hip.solve_device(buf.ptr, rows, cols, stride, 0)
    hip.synth_device(buf.ptr, rows, cols, stride, 77)
    assert sol.status == 0 and sol.rank == cols and sol.stats["handover_retries"] == 0
    assert hip.residual_device(buf.ptr, rows, cols, stride, sol.origin) == 0
    buf.free()


def _dense_properties(n, seed, repeat=True):
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(n * stride * 8)
    hip.synth_device(buf.ptr, n, n, stride, seed)
    sol = hip.solve_device(buf.ptr, n, n, stride, 0)
    hip.synth_device(buf.ptr, n, n, stride, seed)
    assert sol.status == 0 and hip.residual_device(buf.ptr, n, n, stride, sol.origin) == 0
    # no hand-over gate expired on the way (the call would have repeated the solve with events and still be right --
    # at several times the run time, and the device would stay on events for the rest of the process)
    assert sol.stats["handover_retries"] == 0
    piv = sol.pivots
    assert len(piv) == sol.rank and (np.diff(piv) > 0).all() and sol.rank >= n - 8
    free = np.setdiff1d(np.arange(n), piv)
    x = sol.origin
    assert all(not (int(x[f >> 6]) >> (f & 63)) & 1 for f in free)
    if sol.rank == n:
        assert np.array_equal(x, O.planted_solution(n, seed)) and np.array_equal(x, hip.planted_solution(n, seed))
    # linearity: the solution of the system with RHS flipped on a pivot-consistent way is covered by
    # mode 1 at a smaller size (test_words_path_matches_oracle); here: solving twice is deterministic
    if repeat:
        hip.synth_device(buf.ptr, n, n, stride, seed)
        again = hip.solve_device(buf.ptr, n, n, stride, 0)
        assert np.array_equal(again.origin, sol.origin) and again.rank == sol.rank
    buf.free()
    return sol


def test_pinned_host_staging_is_recycled():
    """Round 5: gf2bv_host_alloc hands a binding page-locked staging for its digit gather and keeps up to four idle buffers: the same
    pages come back for the next call of the same size; a solve out of such a buffer equals the solve out of pageable memory."""
    import ctypes
    L = hip.lib()
    p1, p2 = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.gf2bv_host_alloc(8 << 20, ctypes.byref(p1)) == 0 and p1.value
    L.gf2bv_host_free(p1)
    assert L.gf2bv_host_alloc(8 << 20, ctypes.byref(p2)) == 0 and p2.value == p1.value
    rng = random.Random(3)
    rows, cols = 1500, 1400
    eqs = random_system(rng, rows, cols, .5, 1300, True, 0)
    aug = O.eqs_to_aug(eqs, cols)
    want = hip.solve_words(aug, rows, cols, 1)
    buf = (ctypes.c_uint64 * aug.size).from_address(p2.value)
    np.frombuffer(buf, dtype=np.uint64)[:] = aug.reshape(-1)
    res = ctypes.c_void_p()
    assert L.gf2bv_solve_words(p2.value, rows, cols, aug.shape[1], 1, 0, ctypes.byref(res)) == 0
    got = hip._take(res, 1)
    L.gf2bv_host_free(p2)
    assert got.rank == want.rank and np.array_equal(got.origin, want.origin) and np.array_equal(got.basis, want.basis)
