"""bench.py on the GPU box, as child processes (a test process that has initialised the GPU must not
exec; it may start children): the line the driver parses, and the collectives of the N > 1 path run
through torch's nccl backend (RCCL) with the one rank a one-GPU box can give it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(*flags, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, *flags], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_carries_the_contract_fields():
    d = _run("--full", "--steps", "2", "--warmup", "1", "--paths-per-gpu", "4000000", "--no-cpu-baseline")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["ranks"] == 1 and d["backend"] == "none" and d["unit"] == "paths/s"
    assert d["value"] == pytest.approx(4000000 * 2 / (d["ms_per_step"] * 2e-3), rel=1e-6)
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert r["kernel_ms"] <= d["ms_per_step"] * 1.001  # HIP-event kernel time fits inside the step
    assert d["result"]["hist_total"] == 4000000
    v = d["valu"]
    assert 0 < v["frac"] < 1
    # round 4: the clock sampled by the launches themselves; the loop priced at class cost is a bound (<= 1), the
    # same loop at the probes' measured costs rides beside it; the library says what it was built from
    assert 1.2 < v["held_clock_ghz"] < 2.5
    if v["weighted_model"] is None:
        # profiles/pmc_traffic.json belongs to other kernel sources than this build's: bench.py prices nothing with it
        # (tests/test_measurement_cpu.py is the test that fails until the profile pass has been run again)
        assert v["weighted_frac"] is None and v["weighted_frac_measured_costs"] is None
    else:
        assert 0.5 < v["weighted_frac"] <= 1.0 and v["weighted_frac"] < v["weighted_frac_measured_costs"] < 1.12 * v["weighted_frac"]
        assert v["weighted_model"]["class_clk_per_block"] == 2 * v["weighted_model"]["valu_insts_per_block"] + 2 * v["weighted_model"]["half_rate_insts_per_block"]
    assert len(d["build_digest"]) == 64
    y = d["hbm_bound_kernels"]["box_yardstick"]
    assert 1000 < y["fill_GBps"] < 8000 and 20 < y["sum_GBps"] < 8000  # the sum is over this run's 4e6 values: microseconds
    assert d["hbm_bound_kernels"]["keepdata"]["vs_box_fill"] == pytest.approx(d["hbm_bound_kernels"]["keepdata"]["GBps"] / y["fill_GBps"])


def test_plain_run_prints_the_headline_only():
    """A plain run sets up, warms up, times --steps steps and prints the headline; what is measured beside it
    (pricing against the roofs, neighbour kernels, CPU baseline, group launcher) is --full's."""
    d = _run("--steps", "3", "--warmup", "1", "--paths-per-gpu", "1000003")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["value"] == pytest.approx(1000003 * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)
    assert d["result"]["hist_total"] == 1000003
    for key in ("roofline", "valu", "hbm_bound_kernels", "cpu_baseline", "group_single_process", "dumped_outputs"):
        assert key not in d, key


def _oracle_paths(oracle, table, positions):
    """The oracle's final value of single paths of bench.py's default workload (Gaussian, 360 periods)."""
    import bench
    return np.array([oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 360, 1, bench.SEED, first_path=int(p),
                                                          table=table))["final"][0] for p in positions], dtype=np.float32)


def test_dump_outputs_are_the_oracle_values_and_repeat_bit_for_bit(tmp_path, oracle, table):
    """--dump-outputs: the last timed step's final values, block means / variances and statistics record, the
    same bits in a second run, and the final values and bucket counts those of the CPU oracle."""
    import bench
    n = 20011
    lines = [_run("--steps", "2", "--warmup", "1", "--paths-per-gpu", str(n), "--dump-outputs", str(tmp_path / d))
             for d in ("a", "b")]
    names = ["chunk_mean", "chunk_var", "final_values", "histogram", "stats"]
    assert lines[0]["dumped_outputs"] == lines[1]["dumped_outputs"] == names
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    for k, a in got.items():
        assert a.dtype in (np.float32, np.float64), k
        again = np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == again.dtype and np.array_equal(a.view(np.uint8), again.view(np.uint8)), k
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 360, n, bench.SEED, table=table, n_bins=100,
                                             hist_lo=0.0, hist_hi=20000.0))
    assert got["final_values"].dtype == np.float32 and got["final_values"].size == n
    assert np.array_equal(got["final_values"].view(np.uint32), o["final"].view(np.uint32))
    assert np.array_equal(got["histogram"], o["hist"].astype(np.float64))
    cm, cv = oracle.chunk_mean_var(o["final"])
    np.testing.assert_allclose(got["chunk_mean"], cm, rtol=1e-6)
    np.testing.assert_allclose(got["chunk_var"], cv, rtol=1e-5, atol=1e-6 * float(np.max(cv) + 1))
    assert got["stats"][0] == n and got["stats"][1] == o["stats"].below == lines[0]["result"]["below_initial"]
    assert got["stats"][4] / n == pytest.approx(lines[0]["result"]["mean"], rel=1e-12)


def test_dump_outputs_of_the_default_workload_stay_under_64_mb(tmp_path, oracle, table):
    """The default workload (1e8 paths): its final values are written as the fixed sample of bench.sample_positions,
    the 390625 block means and variances whole, all of it under 64 MB."""
    import bench
    n = bench.PATHS_PER_GPU
    d = _run("--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path))
    assert d["config"]["paths_rank0"] == n and d["steps"] == 1
    assert sum(os.path.getsize(tmp_path / f"{k}.npy") for k in d["dumped_outputs"]) <= 64 << 20
    pos = bench.sample_positions(n)
    final = np.load(tmp_path / "final_values.npy")
    assert final.dtype == np.float32 and final.size == pos.size > 0.9 * bench.DUMP_SAMPLE
    assert np.load(tmp_path / "chunk_mean.npy").size == np.load(tmp_path / "chunk_var.npy").size == (n + 255) // 256
    assert np.load(tmp_path / "histogram.npy").sum() + np.load(tmp_path / "stats.npy")[2:4].sum() == n
    picks = np.linspace(0, pos.size - 1, 24).astype(np.int64)  # first, last and evenly spaced samples
    want = _oracle_paths(oracle, table, pos[picks])
    assert np.array_equal(final[picks].view(np.uint32), want.view(np.uint32))


def test_rccl_collectives_of_the_multi_rank_path_run_with_one_rank():
    """--rehearse-rccl: the process group is really initialised with backend nccl (= RCCL on ROCm) and the
    step's all_gather of the 864-byte statistics record, the barriers and the max-reduce of the time go
    through it; the merged record must be the rank's own."""
    d = _run("--rehearse-rccl", "--config", "3", "--total-paths", "3000001", "--steps", "2", "--warmup", "1",
             "--no-cpu-baseline")
    assert d["ranks"] == 1 and d["backend"].startswith("rccl") and d["n_gpus"] == 1
    assert d["result"]["hist_total"] == 3000001
    plain = _run("--config", "3", "--total-paths", "3000001", "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert plain["result"] == d["result"]  # gathered and merged == read directly


def test_two_self_launched_ranks_share_the_gpu_and_merge_to_the_single_rank_result():
    """`python bench.py --gpus 2 --backend gloo`: bench.py starts its own two ranks (both on this box's
    one GPU), each simulates its half of the global path ids, the records are gathered and merged in
    rank order: count, below-count and histogram total equal the one-rank run over the same ids, mean
    and standard deviation to 1e-12."""
    two = _run("--gpus", "2", "--backend", "gloo", "--config", "3", "--total-paths", "5000001", "--steps", "2",
               "--warmup", "1", timeout=600)
    one = _run("--config", "3", "--total-paths", "5000001", "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert two["n_gpus"] == 2 and two["ranks"] == 2 and two["backend"] == "gloo" and two["launcher"] == "self"
    assert len(two["devices"]) == 2 and all("cuda:0" in d for d in two["devices"])
    assert two["config"]["paths_all_ranks"] == 5000001 and two["config"]["paths_rank0"] == 2500001  # the remainder is kept
    assert two["result"]["hist_total"] == one["result"]["hist_total"] == 5000001
    assert two["result"]["below_initial"] == one["result"]["below_initial"]
    assert two["result"]["mean"] == pytest.approx(one["result"]["mean"], rel=1e-12)
    assert two["result"]["std"] == pytest.approx(one["result"]["std"], rel=1e-10)


def test_two_ranks_config1_weak_scaling_conserves_counts_and_equals_one_rank_over_the_same_ids():
    """BASELINE configs[1] shape with two self-launched ranks (weak scaling: every rank its own
    paths-per-gpu, rank r the ids [r n, (r + 1) n)): rank count, total paths, count conservation, and the
    merged record equal to ONE rank simulating the ids [0, 2 n)."""
    n = 3_000_000
    two = _run("--gpus", "2", "--backend", "gloo", "--config", "1", "--paths-per-gpu", str(n), "--steps", "2", "--warmup", "1",
               timeout=600)
    one = _run("--config", "1", "--paths-per-gpu", str(2 * n), "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert two["n_gpus"] == 2 and two["ranks"] == 2 and two["backend"] == "gloo" and two["launcher"] == "self"
    assert two["scaling"] == "weak" and two["config"]["paths_rank0"] == n and two["config"]["paths_all_ranks"] == 2 * n
    assert two["config"]["outputs"] == "all" and two["config"]["mode"] == "gaussian" and two["config"]["n_periods"] == 360
    assert two["result"]["hist_total"] == 2 * n == one["result"]["hist_total"]
    assert two["result"]["below_initial"] == one["result"]["below_initial"]
    assert two["result"]["mean"] == pytest.approx(one["result"]["mean"], rel=1e-12)
    assert two["result"]["std"] == pytest.approx(one["result"]["std"], rel=1e-10)
    assert two["value"] == pytest.approx(2 * n * 2 / (two["ms_per_step"] * 2e-3), rel=1e-6)  # whole-job paths / max-over-ranks time


def test_two_ranks_config4_host_buffers_equal_the_halves_of_the_one_rank_run():
    """BASELINE configs[4] shape (P = 1000, final values to pinned host memory through the side-stream
    pipeline, no collective) with two self-launched ranks: each rank's host buffer is, bit for bit, its
    half of what one rank computes for the whole id range (digests of the buffers; the remainder of the odd
    total goes to rank 0)."""
    total = 2_000_001
    two = _run("--gpus", "2", "--backend", "gloo", "--config", "4", "--total-paths", str(total), "--steps", "2", "--warmup", "1",
               "--hash-shards", "2", timeout=600)
    one = _run("--config", "4", "--total-paths", str(total), "--steps", "2", "--warmup", "1", "--hash-shards", "2",
               "--no-cpu-baseline")
    assert two["n_gpus"] == 2 and two["ranks"] == 2 and two["scaling"] == "strong"
    assert two["config"]["paths_all_ranks"] == total and two["config"]["paths_rank0"] == 1_000_001
    assert two["config"]["outputs"] == "host" and two["config"]["n_periods"] == 1000
    assert "no collective" in two["config"]["parallelism"]
    assert len(two["host_digests"]) == 2 and two["host_digests"] == one["host_digests"]
    assert two["host_digests"][0] != two["host_digests"][1]
    assert two["host_pipeline"]["bytes_to_host_per_step"] == 4.0 * 1_000_001


def test_four_self_launched_ranks_config3_remainder_and_merge():
    """Four ranks (four processes on this box's one GPU; the pool allows six) over an N that is not a
    multiple of four: every rank's id range, the remainder, and the merged record equal to one rank's."""
    total = 4_000_003
    four = _run("--gpus", "4", "--backend", "gloo", "--config", "3", "--total-paths", str(total), "--steps", "2",
                "--warmup", "1", timeout=600)
    one = _run("--config", "3", "--total-paths", str(total), "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert four["n_gpus"] == 4 and four["ranks"] == 4 and len(four["devices"]) == 4
    assert four["config"]["paths_all_ranks"] == total and four["config"]["paths_rank0"] == 1_000_001
    assert four["result"]["hist_total"] == one["result"]["hist_total"] == total
    assert four["result"]["below_initial"] == one["result"]["below_initial"]
    assert four["result"]["mean"] == pytest.approx(one["result"]["mean"], rel=1e-12)
    assert four["result"]["std"] == pytest.approx(one["result"]["std"], rel=1e-10)


def test_ranks_made_by_torchrun_run_the_real_step():
    """The driver's N > 1 command line -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 ...` -- with the real step (both ranks on this
    box's one GPU, hence gloo for the record gather): ONE JSON line from rank 0, launcher "external", the
    merged record equal to one rank's."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    total = 3_000_001
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--backend", "gloo",
                        "--config", "3", "--total-paths", str(total), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    two = json.loads(lines[0])
    one = _run("--config", "3", "--total-paths", str(total), "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert two["launcher"] == "external" and two["ranks"] == 2 and two["n_gpus"] == 2 and two["backend"] == "gloo"
    assert two["config"]["paths_all_ranks"] == total and two["config"]["paths_rank0"] == 1_500_001
    assert two["result"]["hist_total"] == one["result"]["hist_total"] == total
    assert two["result"]["below_initial"] == one["result"]["below_initial"]
    assert two["result"]["mean"] == pytest.approx(one["result"]["mean"], rel=1e-12)


def _check_group_leg(leg, n_all, result):
    assert "error" not in leg, leg
    assert leg["value"] > 0 and leg["ms_per_step"] > 0 and leg["merge_ms"] >= 0 and leg["engines_ms"] > 0
    assert leg["result"]["below_initial"] == result["below_initial"]
    assert leg["result"]["mean"] == pytest.approx(result["mean"], rel=1e-12)


def test_self_launched_run_attaches_the_one_process_group_launcher():
    """after the ranks of `python bench.py --gpus 2` have finished, their GPU-less parent
    starts ONE fresh child that runs the same workload through the C ABI's one-process launcher (smmc_group_*:
    one host thread + engine per device) and attaches `group_single_process` to rank 0's line.  On this
    one-GPU box both shards sit on device 0, so the host-merge leg runs and the RCCL leg (which needs distinct
    devices) reports why it cannot -- as an error string inside the object, never as a lost line."""
    total = 5_000_001
    two = _run("--full", "--gpus", "2", "--backend", "gloo", "--config", "3", "--total-paths", str(total), "--steps", "2",
               "--warmup", "1", timeout=600)
    g = two["group_single_process"]
    assert g["devices"] == 2 and g["paths"] == total and g["outputs"] == "stats" and g["n_periods"] == 360
    _check_group_leg(g["host"], total, two["result"])
    assert g["host"]["device_list"] == [0, 0] and g["host"]["comm_init_ms"] == 0.0
    assert "distinct devices" in g["rccl"]["error"]
    # config 4's shape: final values into pinned host memory through every shard's pipeline
    total4 = 2_000_001
    four = _run("--full", "--gpus", "2", "--backend", "gloo", "--config", "4", "--total-paths", str(total4), "--steps", "2",
                "--warmup", "1", timeout=600)
    g4 = four["group_single_process"]
    assert g4["outputs"] == "host" and g4["n_periods"] == 1000 and g4["paths"] == total4
    assert "error" not in g4["host"] and g4["host"]["value"] > 0


def test_group_child_with_one_device_runs_both_merge_back_ends_to_the_same_bits():
    """`bench.py --group-child 1`: one device allows the RCCL leg too (ncclCommInitAll over one device, the
    grouped all-reduce): its merged record equals the host merge's bit for bit, the communicator's set-up
    time is reported, and both equal the plain one-rank run of the workload."""
    total = 3_000_001
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--group-child", "1", "--config", "3", "--total-paths", str(total), "--steps", "2",
                        "--warmup", "1"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    g = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    one = _run("--config", "3", "--total-paths", str(total), "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    _check_group_leg(g["host"], total, one["result"])
    _check_group_leg(g["rccl"], total, one["result"])
    assert g["rccl_equals_host_merge"] is True and g["rccl"]["comm_init_ms"] > 0


def test_ranks_made_by_torchrun_attach_the_group_launcher_from_rank_zero():
    """Under an external launcher there is no GPU-less parent of ours: rank 0 -- timed region over, process
    group destroyed, engine closed -- starts the fresh child itself."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    total = 3_000_001
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--full", "--gpus", "2", "--backend",
                        "gloo", "--config", "3", "--total-paths", str(total), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    two = json.loads(lines[0])
    g = two["group_single_process"]
    assert two["launcher"] == "external" and g["devices"] == 2 and g["paths"] == total
    _check_group_leg(g["host"], total, two["result"])
