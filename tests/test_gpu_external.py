"""Everything in the GPU suite that talks to an external runtime -- RCCL, torch.distributed.run, bench.py launches -- each in a CHILD
process with a wall-clock limit of its own (tests/child.py), ordered behind every in-process test (tests/conftest.py).

Round 5's driver run (GPUTEST_r05: rc 1) waited 240 s inside `init_process_group("nccl", world_size=1, device_id=...)` called from
the pytest process, right behind a 64-system batch, and the in-process guard then ended pytest itself.  Here the same sequence runs in
a child (`rccl_child.py gather --after-solve 64`) beside its A/B partners -- RCCL on a device that has NOT run a solve, RCCL without
the library in the process at all -- and a child that never returns costs exactly one failed test
(`test_a_hung_child_costs_one_test`)."""
import json
import os
import socket
import sys

import pytest

from tests.child import ROOT, rccl_child, rccl_control, run_child

pytestmark = [pytest.mark.gpu, pytest.mark.external, pytest.mark.timeout(900)]


def _free_port() -> str:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_a_hung_child_costs_one_test():
    """The runner's contract: a child that never returns is killed at its limit (its whole process group), the caller gets a
    result to assert on -- and the suite goes on.  `rccl_child.py hang` is the test-only knob."""
    res = rccl_child("hang", limit_s=5)
    assert res.timed_out and not res.ok and res.seconds < 30
    assert "hanging on purpose" in res.out and "killed after its limit" in res.report()
    res = run_child([sys.executable, "-c", "import os, sys; os.write(2, b'bye'); sys.exit(7)"], 30)
    assert not res.ok and res.rc == 7 and not res.timed_out and res.err == "bye"


def _require_rccl():
    """RCCL world-1 init + all_gather from a process that never loads this library.  If THAT does not come up, the box has no usable
    RCCL and nothing below can say anything about the product: skipped, with the log."""
    ctl = rccl_control()
    if not ctl.ok:
        pytest.skip("RCCL does not come up on this box even without libgf2bv_hip.so in the process:\n" + ctl.report())
    return ctl


def _child_info(res):
    assert res.ok, res.report() + "\n=== control (torch only, no library) ===\n" + rccl_control().report(800)
    return json.loads([ln for ln in res.out.splitlines() if ln.startswith("CHILD_OK ")][-1][9:])


def test_rccl_control_without_the_library():
    ctl = _require_rccl()
    info = json.loads([ln for ln in ctl.out.splitlines() if ln.startswith("CHILD_OK ")][-1][9:])
    assert info["mode"] == "control" and info["init_seconds"] < 100


def test_gather_records_over_rccl_on_a_fresh_device():
    """The end-of-job collective with the backend the multi-GPU run uses (RCCL), world size 1, on a device that has not run a
    solve when RCCL comes up: 5 systems of 2048^2, records gathered on the device, residual 0, two systems word for word against the
    oracle, an uneven split."""
    _require_rccl()
    info = _child_info(rccl_child("gather"))
    assert info["init_seconds"] < 100


def test_gather_records_over_rccl_behind_a_64_system_batch():
    """Round 5's sequence, kept as the permanent A/B: 64 x 32768^2 as gangs (two host threads, streaming launches, the pinned
    staging pool, a probed stream pair for the single solve behind them) and THEN RCCL's eager single-device connect in the same
    process.  A caller who initialises RCCL after solving must not hang: if this fails where the fresh-device test passes, the
    library's state is the cause."""
    _require_rccl()
    info = _child_info(rccl_child("gather", "--after-solve", "64", limit_s=400))
    assert info["solved_before_init"] == 64 and info["pool_idle_bytes_before_init"] > 0 and info["init_seconds"] < 100


def test_slab_schedule_over_rccl_world_size_1():
    """The column-slab schedule with the backend of the multi-GPU run on this box's one GPU: the per-block broadcast of the DEVICE
    payload tensor is issued although there is nobody to receive it, so dist.broadcast on device memory, the stream ordering around
    it and the import of the records are the code the 8-GPU run executes.  Checked against the oracle (in the child)."""
    _require_rccl()
    _child_info(rccl_child("slab"))


def test_bench_batch_mode_end_to_end():
    """bench.py --workload batch (what --gpus N > 1 runs on every rank), launched through torch.distributed.run."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "batch", "--steps", "2",
           "--warmup", "1", "--batch-total", "12", "--batch-n", "4096", "--no-cpu-baseline"]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["scaling"] == "strong" and line["n_gpus"] == 1 and line["config"]["systems_total"] == 12
    assert line["parity_gate"]["all_ranks_ok"] and line["parity_gate"]["residual_rows_rank0"] == 0
    assert line["parity_gate"]["gathered_records"] == 12
    assert line["value"] > 0 and line["roofline"]["achieved"] > 0


def test_bench_sharded_mode_single_rank():
    """bench.py --workload sharded (ONE system, column slabs over the ranks) at world size 1: the schedule end to end."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "sharded", "--n", "8192", "--steps", "2", "--warmup", "1"]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["scaling"] == "strong" and line["parity_gate"]["residual_rows"] == 0 and line["parity_gate"]["all_solved"]


def test_bench_dump_outputs_are_the_last_step(tmp_path):
    """--dump-outputs: what the timed path returned in its last timed step, as float .npy files.  The headline solve_one at a
    full-rank size (the planted vector is the only solution, the pivots are every column) with --steps 3, and a batch job whose
    records are checked against the CPU oracle."""
    import numpy as np

    from gf2bv_amd import hip
    from oracle import gf2_oracle as O
    n, seed = 32768, 1234                                    # bench.FULL_RANK_SEEDS
    single = tmp_path / "single"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--steps", "3", "--warmup", "1", "--no-batch-c4",
           "--no-extra-legs", "--no-cpu-baseline", "--no-plain-leg", "--target-n", "0", "--dump-outputs", str(single)]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["rank"] == n
    assert sorted(os.listdir(single)) == ["pivots.npy", "rank.npy", "status.npy", "x.npy"]
    d = {k: np.load(single / (k + ".npy")) for k in ("x", "status", "rank", "pivots")}
    assert d["x"].dtype == np.float32 and d["status"].dtype == d["rank"].dtype == d["pivots"].dtype == np.float64
    planted = np.unpackbits(hip.planted_solution(n, seed).view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(d["x"], planted) and d["status"].tolist() == [0] and d["rank"].tolist() == [n]
    assert np.array_equal(d["pivots"], np.arange(n))

    nb, total = 2048, 5
    job = tmp_path / "batch"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "batch", "--steps", "2", "--warmup", "1",
           "--batch-total", str(total), "--batch-n", str(nb), "--no-cpu-baseline", "--dump-outputs", str(job)]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["parity_gate"]["all_ranks_ok"]
    d = {k: np.load(job / (k + ".npy")) for k in ("x", "status", "rank", "x_systems")}
    assert d["x"].shape == (total, nb) and np.array_equal(d["x_systems"], np.arange(total))
    for i in (0, total - 1):                                 # system i: generator seed 5000 + i (bench.BATCH_SEED0)
        want = O.solve_words(O.gen_synthetic(nb, nb, 5000 + i), nb, nb, 0, algo=1)
        assert d["status"][i] == want["status"] and d["rank"][i] == want["rank"]
        assert np.array_equal(d["x"][i], np.unpackbits(np.asarray(want["origin"], dtype=np.uint64).view(np.uint8), bitorder="little")[:nb])


def test_bench_two_ranks_sharing_the_gpu():
    """bench.py --gpus 2 --full as the driver launches it (torch.distributed.run, one process per rank): the default line is
    the N = 1 workload on every rank (weak scaling: one system per GPU per step) plus, with --full, the configs[3] job sharded
    over the ranks as `batch_c4` -- shard bounds, barriers, max-over-ranks timing, the gathers and the JSON line -- with both ranks
    pinned to this box's one GPU and gloo standing in for RCCL (which cannot put two ranks on one device)."""
    env = dict(os.environ, GF2BV_BENCH_DEVICE="0", GF2BV_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--size", "8192", "--batch-total", "9", "--batch-n", "4096"]
    out = run_child(cmd, 300, env=env)
    assert out.ok, out.report()
    lines = [ln for ln in out.out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                    # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and "8192x8192" in line["config"]["workload"]
    assert line["parity_gate"]["all_ranks_ok"] and line["parity_gate"]["residual_rows"] == 0
    assert "cpu_baseline" not in line and "target_262144" not in line and line["value"] > 0 and line["roofline"]["achieved"] > 0
    c4 = line["batch_c4"]
    assert c4["n_gpus"] == 2 and c4["scaling"] == "strong" and c4["config"]["systems_total"] == 9
    assert c4["parity_gate"]["all_ranks_ok"] and c4["parity_gate"]["gathered_records"] == 9
    assert c4["systems_per_s"] > 0 and c4["roofline"]["achieved"] > 0


def test_bench_three_ranks_sharing_the_gpu():
    """Multi-GPU readiness without a multi-GPU node (no scaling curve can be taken here: N > 1 is UNMEASURED on hardware):
    `bench.py --gpus 3 --full` as the driver launches it -- three ranks under torch.distributed.run -- all pinned to this
    box's one GPU with gloo standing in for RCCL, at reduced sizes: the shard bounds of configs[3] at world 3 (24 systems
    -> 8 per rank, what 512 / 8 = 64 per rank exercises), gang sizing for a rank's share, the order of the gathered records,
    barriers and max-over-ranks timing, one JSON line from rank 0.  Three ranks, not eight: the suite keeps at most six
    processes on a GPU at once, the pytest process and the launcher included (the world-8 plan of the real job:
    test_distributed_cpu.py)."""
    env = dict(os.environ, GF2BV_BENCH_DEVICE="0", GF2BV_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "2", "--warmup", "1",
           "--full", "--size", "4096", "--batch-total", "24", "--batch-n", "2048"]
    out = run_child(cmd, 600, env=env)
    assert out.ok, out.report()
    lines = [ln for ln in out.out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 3 and line["scaling"] == "weak" and line["parity_gate"]["all_ranks_ok"]
    assert "cpu_baseline" not in line and "c3_mt19937" not in line and line["value"] > 0
    c4 = line["batch_c4"]
    assert c4["n_gpus"] == 3 and c4["scaling"] == "strong" and c4["config"]["systems_total"] == 24
    assert c4["config"]["systems_per_gpu"] == 8 and c4["parity_gate"]["all_ranks_ok"] and c4["parity_gate"]["gathered_records"] == 24
    assert c4["systems_per_s"] > 0


def test_bench_default_line_carries_the_scale_anchor():
    """N = 1, --full: the same line shape (headline + `batch_c4` with its roofline), here at reduced sizes."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--n", "8192", "--batch-total", "6",
           "--batch-n", "4096", "--no-cpu-baseline"]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["scaling"] == "weak" and line["parity_gate"]["residual_rows"] == 0
    c4 = line["batch_c4"]
    assert c4["n_gpus"] == 1 and c4["config"]["systems_total"] == 6 and c4["parity_gate"]["all_ranks_ok"]
    assert c4["roofline"]["frac"] > 0 and c4["roofline"]["end_to_end_frac"] > 0
    # the reference's own example timings ride along at N = 1: configs[2] x 6 variants, configs[4], host-resident input
    c3 = line["c3_mt19937"]["variants"]
    assert [v["bits_per_output"] for v in c3] == [32, 17, 9, 1, 1337, 137]
    assert all(v["recovered_state_equals_known_answer"] and v["m4ri_solve_ms"]["warm"] > 0 and v["device_ms"]["eliminate"] > 0 for v in c3)
    c5 = line["c5_xoshiro"]
    assert c5["recovered_seed_equals_known_answer"] and c5["solutions"] == 1 and c5["solve_all_ms"]["warm_median"] > 0
    h2d = line["h2d_inclusive"]
    assert h2d["phases_ms"]["pack_h2d"] > 0 and h2d["ms_per_solve"]["second"] > 0


def test_bench_plain_line_is_the_headline_only():
    """Without --full a run sets up, warms up, times its steps and prints the headline line with its parity gate: none of the
    legs that take runs of their own (plain leg, stream ceiling, north-star size, batch_c4, example legs, CPU baseline)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--n", "8192"]
    out = run_child(cmd, 300)
    assert out.ok, out.report()
    line = json.loads([ln for ln in out.out.splitlines() if ln.startswith("{")][-1])
    assert line["unit"] == "row-XORs/s" and line["higher_is_better"] and line["dtype"] == "u64" and line["steps"] == 2
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["n_gpus"] == 1
    assert line["parity_gate"]["residual_rows"] == 0 and line["parity_gate"]["all_ranks_ok"]
    assert line["roofline"]["achieved"] > 0 and "persistent_rmw_stream_GBs" not in line["roofline"]
    for extra in ("plain_ms_per_step", "target_262144", "batch_c4", "c3_mt19937", "c5_xoshiro", "h2d_inclusive", "cpu_baseline"):
        assert extra not in line, extra
