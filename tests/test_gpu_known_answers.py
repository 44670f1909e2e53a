"""Known-answer tests at the sizes that run the natural elimination plans (no GF2BV_TWO_LEVEL): synthetic systems edited so that
the whole answer -- status, rank, pivots, origin and the kernel basis in order -- is known without a CPU re-solve
(tests/known_answer.py), with free columns placed from the mirrored plan where the schedule is thinnest: inside an outer panel, on
its edges, at the hand-over to the one-level tail, in the short last block.  The stats show which path ran."""
import numpy as np
import pytest
import torch

from gf2bv_amd import hip
from oracle import gf2_oracle as O
from tests import known_answer as KA

pytestmark = pytest.mark.gpu

B = KA.BLOCK_COLS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1 and torch.cuda.is_available(), "gpu tests need an MI355X; the product path has no CPU fallback"


@pytest.fixture(autouse=True, params=["default", "plain"])
def heuristics(request, monkeypatch):
    """Every test twice, as in test_gpu_parity.py: as shipped (optimistic enqueue of fast blocks, cut back by hand_back() when the
    search gives up inside an outer panel) and with GF2BV_PLAIN=1 (both panel paths for every block)."""
    if request.param == "plain":
        monkeypatch.setenv("GF2BV_PLAIN", "1")
    return request.param


def _device_system(rows, cols, seed, spec, nsys=1):
    """A (nsys * rows) x stride int64 device tensor: system i = k_synth(seed + i) edited by spec[i]."""
    stride = hip.padded_stride(cols)
    t = torch.zeros((nsys * rows, stride), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for i in range(nsys):
        hip.synth_device(t.data_ptr() + i * rows * stride * 8, rows, cols, stride, seed + i)
    torch.cuda.synchronize()
    for i in range(nsys):
        KA.apply_torch(t[i * rows:(i + 1) * rows], cols, spec[i] if nsys > 1 else spec)
    torch.cuda.synchronize()
    return t, stride


def _release():
    """Give the device memory of the last case back (its tensor deleted by the caller)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_torch_edits_equal_numpy_edits(heuristics):
    """The device applier against the host one, word for word (bit 63 of a word, the RHS word, every kind of edit), and the solve
    of the edited device system against its known answer."""
    rows, cols, seed = 1200, 1087, 31                   # cols % 64 = 63: the RHS is bit 63 of the last word
    planted = O.planted_solution(cols, seed)
    z = KA.place_free_columns(rows, cols, seed, [63, 127, 500, 1086])
    spec = (KA.free_columns(planted, [0, 191, 256 + 63]) + [KA.zero_col(z[0]), KA.col_xor(z[1], [1, 2, 64, 100])]
            + KA.free_columns(planted, range(512, 768)) + [KA.col_xor(z[3], [5, 383, 1000]), KA.zero_col(z[2])]
            + [KA.zero_row(0), KA.copy_row(7, 1), KA.copy_row(1100, 2), KA.fold_col(1085), KA.zero_row(1199)])
    t, stride = _device_system(rows, cols, seed, spec)
    host = KA.apply_numpy(O.gen_synthetic(rows, cols, seed, stride), cols, spec)
    assert np.array_equal(t.cpu().numpy().view(np.uint64), host)
    want = KA.known_answer(rows, cols, seed, spec)
    assert want["dim"] == 3 + 256 + 4
    KA.assert_same(hip.solve_device(t.data_ptr(), rows, cols, stride, 1), want, 1)
    KA.apply_torch(t, cols, [KA.copy_row(50, 3), KA.flip_rhs(3)])
    host = KA.apply_numpy(host, cols, [KA.copy_row(50, 3), KA.flip_rhs(3)])
    assert np.array_equal(t.cpu().numpy().view(np.uint64), host)
    got = hip.solve_device(t.data_ptr(), rows, cols, stride, 1)
    KA.assert_same(got, KA.known_answer(rows, cols, seed, spec + [KA.copy_row(50, 3), KA.flip_rhs(3)]), 1)
    assert got.status == 1
    del t
    _release()


# rows, cols, seed: tall systems (>= 400 rows more than columns); the plans are checked by tests/test_known_answer_cpu.py
SHAPES = {
    "66000x65600": (66000, 65600, 11),          # one-level; 1025 panels: the last block holds one
    "98704x98267": (98704, 98267, 12),          # K = 8, bend 128 of 384; cols % 64 = 27
    "131472x131072": (131472, 131072, 13),      # K = 8, bend 256 of 512; the RHS is a word of its own
    "197008x196607": (197008, 196607, 14),      # K = 12, bend 504 of 768
}
PLACEMENTS = ["full_rank", "mid_panel1", "block_in_panel0", "panel_edge", "handover", "short_last", "col0", "xor_tail",
              "head_rows", "inconsistent_early", "inconsistent_late"]
LARGEST = ["full_rank", "handover", "xor_tail"]        # 197008 x 196607: the cut-back with K = 12 and the one-level tail
CASES = [(s, p) for s in SHAPES for p in (LARGEST if s == "197008x196607" else PLACEMENTS)]


def _in_block(columns, b):
    assert all(c // B == b for c in columns), (columns, b)
    return columns


def placement(name, rows, cols, seed):
    """(spec, free columns, whether the stats have an expectation) of one placement, from the mirrored plan."""
    K, bend, nb = KA.plan_two_level(rows, cols)
    P = K or 8                                          # (one-level shape: the same positions, in blocks)
    tail = bend if bend else nb // 2                    # first block of the one-level part (one-level shape: the middle)
    planted = O.planted_solution(cols, seed)

    def near(b, offsets):
        return _in_block(KA.place_free_columns(rows, cols, seed, [b * B + o for o in offsets]), b)

    if name == "full_rank":
        free, spec = [], []
    elif name == "mid_panel1":                          # a few columns in the middle block of the second outer panel
        free = near(P + P // 2, (40, 130, 201))
        spec = [KA.zero_col(c) for c in free]
    elif name == "block_in_panel0":                     # a whole pivotless block inside outer panel 0
        free = list(range((P // 2) * B, (P // 2 + 1) * B))
        spec = KA.free_columns(planted, free)
    elif name == "panel_edge":                          # the last column of outer panel 1 and the first of panel 2
        free = [2 * P * B - 1, 2 * P * B]
        spec = KA.free_columns(planted, free)
    elif name == "handover":                            # blocks bend - 1 and bend: the last two-level block and the first one-level one
        free = near(tail - 1, (100,)) + near(tail, (7, 250))
        spec = [KA.zero_col(c) for c in free]
    elif name == "short_last":                          # the short last block and the last column
        free = [(nb - 1) * B + 1, cols - 1]
        spec = KA.free_columns(planted, free)
    elif name == "col0":                                # column 0 (block 0 not fast: no optimistic enqueue) and one in panel 1
        free = [0] + near(P + 1, (60,))
        spec = KA.free_columns(planted, [0]) + [KA.zero_col(free[1])]
    elif name == "xor_tail":                            # XOR columns in the one-level tail, sources in earlier outer panels
        c1, c2 = near(tail + (nb - tail) // 2, (30, 200))
        free = [c1, c2]
        spec = [KA.col_xor(c1, [3, P * B + 77, tail * B - 1]), KA.col_xor(c2, [B + 5, 2 * P * B + 9, c1 - 1, c1 + 1])]
    elif name == "head_rows":                           # dead and duplicated rows where the search starts, a free column in panel 1
        free = near(P + 2, (128,))
        spec = ([KA.zero_row(j) for j in range(3)] + [KA.copy_row(200 + j % 3, j) for j in range(3, 9)]
                + [KA.copy_row(3, 9), KA.zero_col(free[0])])
    elif name == "inconsistent_early":                  # a copy near the head with its RHS flipped (row 5000 dies with row 4)
        free, spec = [], [KA.copy_row(5000, 4), KA.flip_rhs(4)]
    elif name == "inconsistent_late":                   # a copy in the last rows with its RHS flipped
        free, spec = [], [KA.copy_row(rows // 2, rows - 2), KA.flip_rhs(rows - 2)]
    else:
        raise ValueError(name)
    # (a duplicated row leaves a zero row alive in the candidate pool of the one-launch search, which may give up on that block and
    # cut the plan back there: 98704 x 98267 with row 5000 copied to row 4 runs 24 blocks in outer panels, not 128)
    return spec, free, name not in ("head_rows", "inconsistent_early")


def expected_outer_blocks(rows, cols, free, mode):
    """Blocks the outer panels took.  Plain mode: the plan less the blocks without a pivot (the outer pass skips them).  Default mode:
    the one-launch search takes block 0 of a dense system, the later fast blocks are enqueued without the general steps, and the
    first block it cannot take (a free column) poisons the panel path: hand_back() cuts the plan back to that block's outer panel.
    With a free column in block 0 nothing is enqueued optimistically, and the plain rule holds."""
    K, bend, nb = KA.plan_two_level(rows, cols)
    if not K:
        return 0
    per_block = {}
    for c in free:
        per_block[c // B] = per_block.get(c // B, 0) + 1
    pivotless = sum(1 for b, n in per_block.items() if b < bend and n == min(B, cols - b * B))
    if mode == "plain" or 0 in per_block or not per_block or min(per_block) >= bend:
        return bend - pivotless
    return min(per_block) // K * K


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape,name", CASES, ids=[f"{s}-{p}" for s, p in CASES])
def test_natural_plan_known_answer(shape, name, heuristics):
    rows, cols, seed = SHAPES[shape]
    spec, free, stats_expected = placement(name, rows, cols, seed)
    want = KA.known_answer(rows, cols, seed, spec)
    assert want["dim"] == len(free)
    t, stride = _device_system(rows, cols, seed, spec)
    got = hip.solve_device(t.data_ptr(), rows, cols, stride, 1)
    del t
    _release()
    st = got.stats
    K, bend, nb = KA.plan_two_level(rows, cols)
    print(f"[known-answer] {shape} {name} {heuristics}: K {K} bend {bend} blocks {nb} free-blocks {sorted({c // B for c in free})} "
          f"outer_blocks {st['outer_blocks']} fast_blocks {st['fast_blocks']} search_handovers {st['search_handovers']} "
          f"ms_total {st['ms_total']:.1f}")
    KA.assert_same(got, want, 1)
    assert st["handover_retries"] == 0
    if stats_expected:
        assert st["outer_blocks"] == expected_outer_blocks(rows, cols, free, heuristics), st


def test_gang_records_land_in_their_own_slots(heuristics):
    """Five systems of 32968 x 32755 in one batch call (gangs keep the one-level plan), each with its own placement, system 2
    inconsistent: every record equals its own system's known answer."""
    rows, cols, seed = 32968, 32755, 40
    planted = [O.planted_solution(cols, seed + i) for i in range(5)]
    specs = [
        [],
        [KA.zero_col(c) for c in KA.place_free_columns(rows, cols, seed + 1, [300, 5000, 20000])]
        + [KA.col_xor(KA.place_free_columns(rows, cols, seed + 1, [30000])[0], [7, 151, 12346])],
        KA.free_columns(planted[2], [B * 10 + 3]) + [KA.copy_row(100, 30000), KA.flip_rhs(30000)],
        KA.free_columns(planted[3], range(0, B)) + [KA.zero_row(r) for r in range(5)],
        KA.free_columns(planted[4], [0, cols - 1, cols - 2]) + [KA.copy_row(9, r) for r in range(4)],
    ]
    t, stride = _device_system(rows, cols, seed, specs, nsys=5)
    got = hip.solve_batch_device(t.data_ptr(), 5, rows * stride, rows, cols, stride, 1)
    del t
    _release()
    assert [g.status for g in got] == [0, 0, 1, 0, 0]
    assert [g.dimension for g in got] == [0, 4, 1, B, 3]
    for i, g in enumerate(got):
        KA.assert_same(g, KA.known_answer(rows, cols, seed + i, specs[i]), 1)
        assert g.stats["handover_retries"] == 0
