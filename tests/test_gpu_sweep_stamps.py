"""time_kernels: the bulk-update launches stamp the clock themselves (k_update16: t_first / t_last) and the host reads the stamps once
after the solve -- ms_sweep must still be a time inside the elimination, for one system, for a gang and for a two-level plan (whose
outer passes keep their event pairs), the answers must not depend on the switch, and an untimed solve reports no sweep time."""
import numpy as np
import pytest
import torch

from gf2bv_amd import hip
from oracle import gf2_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert hip.device_count() >= 1 and torch.cuda.is_available(), "gpu tests need an MI355X"


def _synth(n, seeds):
    stride = hip.padded_stride(n)
    buf = hip.DeviceBuffer(len(seeds) * n * stride * 8)
    for i, s in enumerate(seeds):
        hip.synth_device(buf.ptr + i * n * stride * 8, n, n, stride, s)
    return buf, stride


def _same(a, b):
    assert a.status == b.status and a.rank == b.rank
    assert np.array_equal(a.pivots, b.pivots) and np.array_equal(a.origin, b.origin)
    assert np.array_equal(a.basis, b.basis)


# What one bulk-update launch takes at the very least: a table build (~1.5 us of LDS work, k_update16's own comment) behind a memory
# round trip (an HBM miss is ~900 cycles = 0.4 us, MI355X_MICROARCH.md) -- 1 us is under both together.  With it the sum must
# account for EVERY launch the stats count: a sweep time made of one launch's stamps, or of a two-level plan's event pairs
# alone, falls short.  (A slot that no launch stamped, or stamps that could not be read, make ms_sweep negative.)
MIN_LAUNCH_MS = 1e-3


def _inside(sol):
    st = sol.stats
    print("ms_sweep", st["ms_sweep"], "ms_eliminate", st["ms_eliminate"], "bulk_launches", st["bulk_launches"])
    assert 0 < st["ms_sweep"] <= st["ms_eliminate"], (st["ms_sweep"], st["ms_eliminate"])
    assert st["bulk_launches"] >= 4
    assert st["ms_sweep"] >= st["bulk_launches"] * MIN_LAUNCH_MS, (st["ms_sweep"], st["bulk_launches"])


@pytest.mark.parametrize("mode", [0, 1])
def test_one_system(mode):
    n = 3000                                    # 12 blocks: every block but the last launches a bulk update
    buf, stride = _synth(n, [31])
    timed = hip.solve_device(buf.ptr, n, n, stride, mode, time_kernels=True)
    plain = hip.solve_device(buf.ptr, n, n, stride, mode)
    buf.free()
    _inside(timed)
    assert plain.stats["ms_sweep"] == 0
    _same(timed, plain)
    want = O.solve_words(O.gen_synthetic(n, n, 31), n, n, mode)
    assert timed.rank == want["rank"] and np.array_equal(timed.origin, want["origin"])


def test_gang_of_three(monkeypatch):
    monkeypatch.setenv("GF2BV_GANG", "3")
    n, seeds = 1100, [41, 42, 43]
    buf, stride = _synth(n, seeds)
    timed = hip.solve_batch_device(buf.ptr, len(seeds), n * stride, n, n, stride, 0, time_kernels=True)
    plain = hip.solve_batch_device(buf.ptr, len(seeds), n * stride, n, n, stride, 0)
    buf.free()
    for t, p in zip(timed, plain):
        assert t.stats["gang_systems"] == 3
        _inside(t)
        assert p.stats["ms_sweep"] == 0
        _same(t, p)
    assert len({t.stats["ms_sweep"] for t in timed}) == 1       # one set of launches served the gang


def test_forced_two_level_plan(monkeypatch):
    monkeypatch.setenv("GF2BV_TWO_LEVEL", "2")
    n = 2600                                    # 11 blocks: outer panels of two blocks (event pairs) around inner updates (stamps)
    buf, stride = _synth(n, [51])
    timed = hip.solve_device(buf.ptr, n, n, stride, 0, time_kernels=True)
    plain = hip.solve_device(buf.ptr, n, n, stride, 0)
    buf.free()
    assert timed.stats["outer_blocks"] > 0
    _inside(timed)
    assert plain.stats["ms_sweep"] == 0
    _same(timed, plain)
