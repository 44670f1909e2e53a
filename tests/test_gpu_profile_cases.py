"""Column rank profiles with holes on every solve path: the built systems of tests/profile_cases.py -- many free columns BETWEEN pivot
columns of one word, panel, block and back-substitution group, each a dense combination of the pivot columns left of it -- against
their known answers (status, rank, pivots, origin, dimension and the basis in order; tests/known_answer.assert_same).  In the systems of
tests/systems.random_system(rank_cap=...) pivot r of a panel sits at column bit r and a pivot's rank index is its column less a
constant; here neither holds, and every entry of U in a free column and every kernel vector is dense.  So these tests are the ones that
tell a pivot's index inside its panel from its bit inside the word: pcs[] of k_bs_inv, pcb / pc[] of k_bs_near2 / k_bs_near, the
right-hand-side bit of k_bs_far, k_extract_y / k_scatter_solution / k_unwind, the stage / prow fill of k_update16, k_block_trsm,
k_outer_trsm / k_outer_apply, k_append_backreduce and the host's S4 replay.

Legs: one system through hip.solve_words under the switches that pick the kernels; a gang; groups of right-hand sides; a kept
factorization; appended equations that close holes; the column-slab schedule at world sizes 1 and 2."""
import functools
import socket

import numpy as np
import pytest
import torch

from gf2bv_amd import hip, slab
from oracle import gf2_oracle as O
from tests import known_answer as KA
from tests import profile_cases as PC

pytestmark = pytest.mark.gpu

GENERAL = {"GF2BV_FAST": "0", "GF2BV_SPARSE_FAST": "0"}
LEGS = {
    "shipped": {},
    "plain": {"GF2BV_PLAIN": "1"},
    "general": GENERAL,                                   # every panel through search_panel
    "events": {"GF2BV_FLAG_SYNC": "0"},
    "bs_inv0": {"GF2BV_BS_INV": "0"},                     # k_bs_near
    "bs_inv1": {"GF2BV_BS_INV": "1"},                     # k_bs_inv + k_bs_near2
    "ysweep": {"GF2BV_YSWEEP": "1"},                      # the table sweeps over Y
}
BLOCKED = {"GF2BV_SMALL": "0"}                            # the small_* cases on the blocked path


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1 and torch.cuda.is_available(), "gpu tests need an MI355X; the product path has no CPU fallback"


def _solve(monkeypatch, env, call):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        return call()


def _line(what, mode, leg, st):
    print(f"[profile] {what} mode {mode} {leg}: small {st['small_path']} fast_blocks {st['fast_blocks']} outer_blocks {st['outer_blocks']} "
          f"general {st['general_unit0']}+{st['general_adopted']}+{st['general_merged']} handovers {st['search_handovers']} "
          f"retries {st['handover_retries']} gang {st['gang_systems']}")


# -- one system -------------------------------------------------------------------------------------------------------------------------------
def _single_legs(name):
    if not name.startswith("small_"):
        return [(leg, env, 0) for leg, env in LEGS.items()]
    return [("shipped", {}, 1), ("blocked", BLOCKED, 0)] + [(leg, {**env, **BLOCKED}, 0) for leg, env in LEGS.items() if env]


SINGLE = [(name, leg, env, small) for name in PC.NAMES for leg, env, small in _single_legs(name)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,leg,env,small", SINGLE, ids=[f"{n}-{leg}" for n, leg, _, _ in SINGLE])
def test_single_system(monkeypatch, name, leg, env, small, mode):
    c = PC.case(name)
    got = _solve(monkeypatch, env, lambda: hip.solve_words(c.aug, c.rows, c.cols, mode))
    st = got.stats
    _line(name, mode, leg, st)
    KA.assert_same(got, c.want, mode)
    assert st["handover_retries"] == 0 and st["small_path"] == small
    if leg == "general":
        assert st["fast_blocks"] == 0
        assert st["general_unit0"] + st["general_adopted"] + st["general_merged"] == (c.cols + 63) // 64


MORE = {
    **{f"two_level_{k}": {"GF2BV_TWO_LEVEL": str(k)} for k in (2, 4)},
    **{f"two_level_{k}_chain": {"GF2BV_TWO_LEVEL": str(k), "GF2BV_OUTER_CHAIN": "1"} for k in (2, 4)},
    **{f"two_level_{k}_plain": {"GF2BV_TWO_LEVEL": str(k), "GF2BV_PLAIN": "1"} for k in (2, 4)},
    **{f"two_level_{k}_chain_plain": {"GF2BV_TWO_LEVEL": str(k), "GF2BV_OUTER_CHAIN": "1", "GF2BV_PLAIN": "1"} for k in (2, 4)},
    **{f"update_{u}": {"GF2BV_UPDATE": str(u)} for u in (1, 2, 3, 4, 5)},
}


def _outer_panels_kept(c, env) -> bool:
    """Whether a forced plan keeps any outer panel.  As shipped, a system of 8 blocks or more whose block 0 takes the one-launch search
    gets the later blocks enqueued without the general steps; the first block that search cannot take -- the first one with a free
    column -- is handed back, and hand_back() cuts the plan back to the start of that block's outer panel (forward_block,
    enqueue_forward in gf2_solver.hip; expected_outer_blocks of tests/test_gpu_known_answers.py).  `every_5th` has its first hole in
    block 1, inside outer panel 0 for K = 2 and K = 4: nothing is left of the plan, by design.  GF2BV_PLAIN=1 enqueues both paths for
    every block and keeps the plan."""
    nblocks = (c.cols + PC.B - 1) // PC.B
    if "GF2BV_PLAIN" in env or nblocks < 8:
        return True
    return c.free[0] // PC.B >= int(env["GF2BV_TWO_LEVEL"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("leg", list(MORE))
@pytest.mark.parametrize("name", ["alternate", "edges", "block_free", "every_5th"])
def test_outer_panels_and_bulk_updates(monkeypatch, name, leg, mode):
    """forced outer panels of 2 and of 4 blocks (k_outer_trsm / k_outer_apply, P = T x S and the chain of panel steps), as shipped and
    with GF2BV_PLAIN=1 -- where every case keeps its outer panels -- and every bulk update kernel of the table"""
    c = PC.case(name)
    env = MORE[leg]
    got = _solve(monkeypatch, env, lambda: hip.solve_words(c.aug, c.rows, c.cols, mode))
    st = got.stats
    _line(name, mode, leg, st)
    KA.assert_same(got, c.want, mode)
    assert st["handover_retries"] == 0 and st["small_path"] == 0
    if leg.startswith("two_level"):
        if _outer_panels_kept(c, env):
            assert st["outer_blocks"] > 0
        else:
            assert st["outer_blocks"] == 0


# -- a gang -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("gang_bs", [None, "0"])
def test_gang_of_five_profiles(monkeypatch, gang_bs, mode):
    """five systems of 1500 x 1300 = gangs of 3 + 2, the last one inconsistent: one back-substitution chain per gang, and with
    GF2BV_GANG_BS=0 one per system"""
    cs = [PC.case(n) for n in PC.GANG]
    assert {(c.rows, c.cols) for c in cs} == {(1500, 1300)}
    augs = np.stack([c.aug for c in cs])
    env = {"GF2BV_GANG": "3", **({} if gang_bs is None else {"GF2BV_GANG_BS": gang_bs})}
    got = _solve(monkeypatch, env, lambda: hip.solve_batch_words(augs, 1500, 1300, mode))
    assert [g.stats["gang_systems"] for g in got] == [3, 3, 3, 2, 2]
    assert [g.status for g in got] == [0, 0, 0, 0, 1]
    for c, g in zip(cs, got):
        _line(c.name, mode, f"gang, GANG_BS {gang_bs}", g.stats)
        KA.assert_same(g, c.want, mode)
        assert g.stats["handover_retries"] == 0 and g.stats["small_path"] == 0


# -- groups of right-hand sides -----------------------------------------------------------------------------------------------------------------
def _assert_rhs(got, name, nrhs, mode):
    want = PC.rhs_oracle(name)
    assert len(got) == nrhs
    for j, g in enumerate(got):
        assert g.status == (1 if j in PC.BAD_RHS else 0), j
        KA.assert_same(g, want[j], mode)
        assert g.stats["handover_retries"] == 0


@pytest.mark.parametrize("inv", [None, "0", "1"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["group_edge", "every_5th"])
def test_groups_of_right_hand_sides(monkeypatch, name, mode, inv):
    """solve_rhs_words with 1, 9 and 65 right-hand sides (b = A x, two of them with a bit flipped): result j is the oracle's answer for
    system j, with GF2BV_BS_INV unset, 0 and 1"""
    c = PC.case(name)
    bits = PC.rhs_bits(name)
    env = {} if inv is None else {"GF2BV_BS_INV": inv}
    for nrhs in PC.NRHS:
        got = _solve(monkeypatch, env, lambda: hip.solve_rhs_words(c.aug, c.rows, c.cols, PC.rhs_words(bits[:nrhs]), mode))
        _assert_rhs(got, name, nrhs, mode)


# -- a kept factorization -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["edges", "every_5th"])
def test_kept_factorization(name, mode):
    c = PC.case(name)
    bits = PC.rhs_bits(name)
    with hip.factor_words(c.aug, c.rows, c.cols, mode) as f:
        assert f.rank == c.want["rank"] and np.array_equal(f.pivots, c.want["pivcols"])
        for nrhs in PC.NRHS:
            _assert_rhs(f.solve(PC.rhs_words(bits[:nrhs])), name, nrhs, mode)
        own = PC.unpack_bits(c.aug, c.cols + 1)[:, c.cols][None, :]          # the system's own right-hand side: the known answer itself
        KA.assert_same(f.solve(PC.rhs_words(own))[0], c.want, mode)


# -- appended equations that close holes -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _append_state(k: int):
    """the append pair's handle after k of B's rows: A (1100 equations, padded to 1300 rows with 0 = 0 as the entries ask) and B[:k]
    stacked, six right-hand sides -- the stack's own, then b = M x -- and the oracle's mode-1 answer for each"""
    p = PC.append_pair()
    pad = np.zeros((p.cols - p.rows_a, p.a.shape[1]), dtype=np.uint64)
    m = np.vstack([p.a, pad, p.b[:k]])
    rng = np.random.default_rng(k)
    x = rng.integers(0, 2, size=(p.cols, 5)).astype(np.float32)
    bits = np.vstack([PC.unpack_bits(m, p.cols + 1)[:, p.cols][None, :],
                      ((PC.unpack_bits(m, p.cols).astype(np.float32) @ x).astype(np.int64) & 1).astype(np.uint8).T])
    want = tuple(O.solve_words(PC.with_rhs(m, p.cols, b), m.shape[0], p.cols, 1) for b in bits)
    return m, bits, want


def _check_appended(f, k, mode):
    m, bits, want = _append_state(k)
    assert f.rows == m.shape[0]
    got = f.solve(PC.rhs_words(bits))
    assert len(got) == 6
    for g, w in zip(got, want):
        assert w["status"] == 0
        KA.assert_same(g, w, mode)
        assert g.stats["handover_retries"] == 0
    assert f.rank == want[0]["rank"] and np.array_equal(f.pivots, want[0]["pivcols"])
    return got


@pytest.mark.parametrize("steps", [1, 4], ids=["one_call", "four_calls"])
@pytest.mark.parametrize("mode", [0, 1])
def test_appends_close_holes(mode, steps):
    """A has the 128 dense free columns of `alternate` (and, with 1100 equations, the last 72 pivot columns free as well); B's 400 rows
    give pivots to all but 20 of the 128, between the pivots A already has (k_append_backreduce).  After the last append: the known
    answer of the stack -- 20 free columns, A's origin, their kernel vectors in order; after each earlier one: the oracle's."""
    p = PC.append_pair()
    pad = np.zeros((p.cols - p.rows_a, p.a.shape[1]), dtype=np.uint64)
    with hip.factor_words(np.vstack([p.a, pad]), p.cols, p.cols, mode) as f:
        got = _check_appended(f, 0, mode)
        assert f.rank == p.rows_a
        per = len(p.b) // steps
        for k in range(per, len(p.b) + 1, per):
            f.append_words(p.b[k - per:k])
            got = _check_appended(f, k, mode)
        assert f.rank == p.want["rank"] and np.array_equal(f.pivots, p.want["pivcols"])
        KA.assert_same(got[0], p.want, mode)                      # (the stack's own right-hand side)
        for g in got[1:]:
            assert g.rank == p.want["rank"] and np.array_equal(g.pivots, p.want["pivcols"])
            if mode == 1:
                assert g.dimension == 20 and np.array_equal(np.asarray(g.basis).reshape(20, -1), p.want["basis"])


# -- the column-slab schedule -----------------------------------------------------------------------------------------------------------------
def _padded(c):
    stride = hip.padded_stride(c.cols)
    host = np.zeros((c.rows, stride), dtype=np.uint64)
    host[:, :c.aug.shape[1]] = c.aug
    return host, stride


def _as_dict(sol):
    return {"status": sol.status, "rank": sol.rank, "dim": 0, "pivcols": np.array(sol.pivots).copy(), "origin": np.array(sol.origin).copy(),
            "basis": None, "handover_retries": sol.stats["handover_retries"]}


@pytest.mark.parametrize("name", ["alternate", "group_edge"])
def test_slab_world_size_1(name):
    c = PC.case(name)
    host, stride = _padded(c)
    aug = torch.from_numpy(host.view(np.int64).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    eng = slab.HipSlabEngine(aug.data_ptr(), c.rows, c.cols, stride, 1, 0, 0)
    try:
        for b in range(eng.nblocks):
            eng.apply(b, eng.factor(b))
        eng.finish_local()
        got = eng.solve()
    finally:
        eng.close()
    KA.assert_same(got, c.want, 0)
    assert got.stats["handover_retries"] == 0


def _slab_worker(rank, world, port, host, rows, cols, stride, q):
    import os

    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda", 0)                      # both ranks on the box's one GPU, as in tests/test_gpu_slab.py
        aug = torch.from_numpy(host.view(np.int64).reshape(-1)).to(dev)
        sol = slab.solve_one_sharded(aug, rows, cols, stride, 0)
        if rank == 0:
            q.put(_as_dict(sol))
        else:
            assert sol is None
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["alternate", "group_edge"])
def test_slab_world_size_2(name):
    import torch.multiprocessing as mp
    c = PC.case(name)
    host, stride = _padded(c)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_slab_worker, args=(r, 2, port, host, c.rows, c.cols, stride, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = q.get(timeout=200)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:                                    # a worker that is still there must not outlive the test
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    KA.assert_same(got, c.want, 0)
    assert got["handover_retries"] == 0
