"""bench.py --dump-outputs without a GPU: the float encoding of solutions and records, the fixed sample of a large batch job, the
size limit.  (The dumps of real runs: tests/test_gpu_external.py.)"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def test_bits_are_the_words_bit_for_bit():
    rng = np.random.default_rng(3)
    for cols in (1, 63, 64, 65, 200):
        words = rng.integers(0, 2 ** 63, size=(cols + 63) // 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        words[-1] &= np.uint64((1 << (cols % 64 or 64)) - 1)
        x = bench.bits_f32(words, cols)
        assert x.dtype == np.float32 and x.shape == (cols,)
        assert int("".join(str(int(b)) for b in x[::-1]), 2) == int.from_bytes(words.tobytes(), "little")
    rec = words.view(np.int64)[None, :].repeat(3, axis=0)            # int64 words of a record: the same bits
    assert np.array_equal(bench.bits_f32(rec, cols), np.stack([bench.bits_f32(words, cols)] * 3))


def test_records_of_a_small_job_are_all_there():
    cols, total = 130, 5
    rec = np.zeros((total, 2 + 3), dtype=np.int64)
    rec[:, 1] = np.arange(total) + 100
    rec[:, 2] = np.arange(total)
    rec[:, 4] = -1                                                     # bit 63 of the last word set: beyond cols, cut off
    d = bench.records_arrays(rec, cols)
    assert d["x"].shape == (total, cols) and np.array_equal(d["x_systems"], np.arange(total))
    assert np.array_equal(d["rank"], rec[:, 1]) and np.array_equal(d["status"], np.zeros(total))
    assert np.array_equal(d["x"][:, :3], [[(i >> b) & 1 for b in range(3)] for i in range(total)])
    assert d["x"][:, 128:].sum() == 2 * total
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())


def test_a_large_job_is_sampled_the_same_way_every_run():
    cols, total = 32768, 512                                           # BASELINE configs[3]: all solution bits would be 64 MiB
    rec = np.zeros((total, bench.batch.record_words(cols)), dtype=np.int64)
    rec[:, 2] = np.arange(total)
    a, b = bench.records_arrays(rec, cols), bench.records_arrays(rec, cols)
    assert np.array_equal(a["x_systems"], b["x_systems"]) and np.array_equal(a["x"], b["x"])
    idx = a["x_systems"].astype(np.int64)
    assert 0 < len(idx) < total and np.all(np.diff(idx) > 0) and idx[-1] < total
    assert np.array_equal(a["x"][:, :16] @ (2.0 ** np.arange(16)), idx)  # row k of x is system x_systems[k]
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES_MAX and a["status"].shape == (total,)


def test_dump_writes_npy_files_and_refuses_too_much(tmp_path):
    arrays = {"x": np.ones(10, dtype=np.float32), "rank": np.array([7.0])}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["rank.npy", "x.npy"]
    assert np.array_equal(np.load(tmp_path / "out" / "x.npy"), arrays["x"])
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_BYTES_MAX // 4 + 1, dtype=np.float32)})
    assert not os.path.exists(tmp_path / "big")
