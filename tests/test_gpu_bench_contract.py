"""bench.py on a real GPU: one JSON line with the contract's keys, the roofline / cpu_baseline objects,
and numbers that are consistent with each other (--full); a plain run times the headline alone and dumps what its last
step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "6", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # stdout is the JSON line and nothing else: what libraries print to file descriptor 1 (RCCL's version banner when the
    # one-rank group comes up) goes to stderr (bench.py: claim_stdout)
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), r.stdout[:400]
    # the line stays small enough for any line-oriented reader (round 5's had grown to 32 KB and the driver's record of it
    # did not parse): contract keys + compact roofline / cpu_baseline / parity / collective + six numbers per extra block
    assert len(r.stdout) < 8192, len(r.stdout)
    line = json.loads(r.stdout)
    check_line(line)
    # everything else lives, whole, in the side file the line names
    with open(os.path.join(ROOT, line["detail"])) as f:
        d = json.load(f)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data"):
        assert line[k] == d[k], k
    assert line["roofline"]["kernel_ms"] == d["roofline"]["kernel_ms"] and line["roofline"]["frac"] == d["roofline"]["frac"]
    assert line["cpu_baseline"]["value"] == d["cpu_baseline"]["value"]
    check_detail(d)


def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """Without --full: the contract's keys and nothing measured beside the headline (no parity, roofline, CPU figure,
    collective or side file); --dump-outputs writes the last timed step's episode returns and per-candidate costs, and
    they are the CPU oracle's on the seeded inputs of BASELINE config 3."""
    env = dict(os.environ, OCD_BENCH_DETAIL=str(tmp_path / "detail.json"))
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), r.stdout[:400]
    line = json.loads(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "generation_cost_checksum"):
        assert k in line, k
    assert line["steps"] == 5 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "f32"
    assert line["unit"] == "episodes/s" and line["higher_is_better"] is True and line["metric"].startswith("MPC episode rollouts/sec at H=10")
    assert line["config"]["episodes_per_generation"] == 2048
    assert abs(line["value"] - 2048 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-6
    for k in ("roofline", "parity", "cpu_baseline", "collective", "cma_generation_ms", "config2", "predicted_strong_scaling",
              "detail"):
        assert k not in line, k
    assert not (tmp_path / "detail.json").exists()
    returns, costs = np.load(out_dir / "returns.npy"), np.load(out_dir / "costs.npy")
    assert sorted(os.listdir(out_dir)) == ["costs.npy", "returns.npy"]
    assert returns.dtype == np.float32 and returns.shape == (2048,) and costs.dtype == np.float64 and costs.shape == (64,)
    from l4dc_mpc_ocd_amd import scenarios, sharding
    assert np.array_equal(costs, sharding.fitness_from_returns(returns, 64, 32, 1))
    assert float(np.sum(costs)) == line["generation_cost_checksum"]
    # the inputs bench.py seeds for config 3 (workload(): inits from seed 1003, candidates from seed 2003)
    cfg = scenarios.BASELINE_CONFIGS[3]
    scn = scenarios.SCENARIOS[cfg["scenario"]](horizon=cfg["horizon"])
    inits = scn.init_dist.sample(cfg["n_inits"], seed=1003)
    w32 = np.stack([scenarios.planner_weights_fp32(c) for c in scn.candidate_weights(cfg["pop"], seed=2003)])
    import oracle_lib
    ref = oracle_lib.load().rollout(scn.desc, inits, w32)["returns"]
    assert np.array_equal(returns.view(np.uint32), np.asarray(ref, dtype=np.float32).view(np.uint32))


TIMING = bool(os.environ.get("OCD_TIMING_ASSERTS"))     # absolute wall-clock thresholds of the builder's box: opt-in


def check_line(d):
    """The printed line by itself: what a reader who never opens the side file gets."""
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "collective", "detail",
              "cma_generation_ms", "predicted_strong_scaling"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert "config 3" in d["config"]["workload"] and "model" not in d["config"] and d["config"]["episodes_per_generation"] == 2048
    rf = d["roofline"]
    assert set(rf) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "binding", "binding_frac"}
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert abs(rf["achieved"] - 2048 * 48 / (rf["kernel_ms"] * 1e-3) / 1e9) < 1e-9      # algorithmic bytes / HIP-event launch time
    assert rf["kernel"] == "void ocd::mpc_kernel<10, 1, 3, 2, false, true>(ocd::KernelParams)"
    assert rf["binding"] == "valu" and 0.05 < rf["binding_frac"] < 1
    assert not any(isinstance(v, str) and len(v) > 100 for v in rf.values())            # no prose in the roofline object
    assert rf["kernel_ms"] <= d["ms_per_step"] * 1.03
    assert abs(d["value"] - 2048 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "episodes/s" and 0 < len(cb["sample"]) <= 120
    par = d["parity"]
    assert par["episodes_checked"] >= 256 and par["bitwise_equal"] == par["episodes_checked"] == par["within_1e-4_rel"] and par["argmin_flips"] == 0
    co = d["collective"]
    assert co["ranks_seen"] == 1 and co["backend"].startswith("nccl") and co["all_gather_us"] > 0 and co["in_timed_step"] is False
    blocks = ("config2", "config4_share8", "config5_share8", "config4_whole", "config5_whole", "reference_h5",
              "reference_h6_extra", "reference_h5_x28", "config1")
    for name in blocks:
        b = d[name]
        assert set(b) <= {"episodes", "ms_per_step", "value", "kernel_ms", "binding_frac", "parity_ok", "cma_generation_ms",
                          "eval_weights_ms", "world_step_ms", "runs", "launch_groups", "generation_ms_ratio_to_one_run", "cpu_value"}, (name, b)
        assert b["kernel_ms"] > 0 and b["episodes"] > 0 and b["parity_ok"] is True, (name, b)
    assert [d[n]["episodes"] for n in blocks] == [128, 2048, 4096, 16384, 32768, 27, 27, 756, 3]
    # the strong-scaling prediction: rows [N, generation ms, speed-up, efficiency] for N = 1, 2, 4, 8, flagged as a prediction
    ps = d["predicted_strong_scaling"]
    assert "NOT an N-GPU run" in ps["measured_on"]
    for c in ("config4", "config5"):
        rows = ps[c]
        assert [r[0] for r in rows] == [1, 2, 4, 8] and rows[0][2] == 1.0 and rows[0][3] == 1.0
        assert all(0 < r[3] <= 1.05 for r in rows) and rows[3][1] < rows[0][1]


def check_detail(d):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "cma_generation_ms", "config2",
              "config4_share8", "config5_share8", "config4_whole", "config5_whole", "reference_h5", "reference_h6_extra", "reference_h5_x28", "config1", "collective"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert "config 3" in d["config"]["workload"] and "model" not in d["config"]
    assert d["config"]["episodes_per_generation"] == 2048
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    # achieved = algorithmic bytes per launch / the kernel's launch duration measured with HIP events
    assert abs(rf["achieved"] - 2048 * rf["algorithmic_bytes_per_episode"] / (rf["kernel_ms"] * 1e-3) / 1e9) < 1e-9
    assert rf["traffic"] is None or rf["traffic"] > 0
    # the step (launch + D2H + float64 reduction) cannot be faster than the kernel alone, nor much slower
    assert rf["kernel_ms"] <= d["ms_per_step"] * 1.03 and d["ms_per_step"] < rf["kernel_ms"] + (0.5 if TIMING else 5.0)
    assert abs(d["value"] - 2048 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "episodes/s" and cb["sample"]
    assert d["cma_generation_ms"] > rf["kernel_ms"] * 0.9
    assert d["config2"]["episodes_per_generation"] == 128 and d["config2"]["value"] > 0
    assert 0 < d["valu"]["frac"] < 1
    # counters replayed from the committed profile say so, and live apart from the measured objects
    assert "issue_utilisation" not in d["valu"]
    if rf["traffic"] is not None:
        assert "NOT observed in this run" in rf["traffic_source"] and d["profiled"]["source"] == rf["traffic_source"]
    # the per-GPU shares of BASELINE configs 4 / 5 over 8 GPUs, run on this one GPU
    s4, s5 = d["config4_share8"], d["config5_share8"]
    assert s4["episodes_per_gpu"] == 2048 and s4["episodes_per_generation"] == 16384 and s4["emulated_rank"] == "0/8"
    assert s5["episodes_per_gpu"] == 4096 and s5["episodes_per_generation"] == 32768
    for sb in (s4, s5):
        assert abs(sb["value"] - sb["episodes_per_gpu"] / (sb["ms_per_step"] * 1e-3)) / sb["value"] < 1e-6
        assert sb["roofline"]["kernel_ms"] <= sb["ms_per_step"] * 1.04      # (six timed steps: one slow launch moves their mean)
    # ... and the two configs whole on this one GPU (the shared-SIMD builds of the chunked kernel), parity attached
    w4, w5 = d["config4_whole"], d["config5_whole"]
    assert w4["episodes_per_gpu"] == 16384 and w5["episodes_per_gpu"] == 32768 and "emulated_rank" not in w4
    for wb in (w4, w5):
        assert wb["parity"]["episodes_checked"] >= 256 and wb["parity"]["bitwise_equal"] == wb["parity"]["episodes_checked"]
        assert abs(wb["value"] - wb["episodes_per_gpu"] / (wb["ms_per_step"] * 1e-3)) / wb["value"] < 1e-6
        assert wb["roofline"]["kernel_ms"] <= wb["ms_per_step"] * 1.04 and wb["roofline"]["launch"]["mapping"] == "chunked"
    if TIMING:
        assert w4["ms_per_step"] < 17.0 and w5["ms_per_step"] < 35.0    # (measured 14.1 / 30.3 ms; before the work items 18.3 / 37.7)
    sp = d["cma"]["host_split_ms"]
    assert set(sp) >= {"ask", "normalise", "launch", "kernel_gather_readback", "reduce", "tell"}
    # the launch kernel_ms times writes where the timed step's launch writes
    assert rf["launch"]["returns_written_to"].startswith("pinned host memory")
    assert d["cma"]["generations_run"] == 48 and d["cma"]["generations_timed"] == 32 and d["cma"]["n_nonfinite"] == 0
    assert d["cma"]["stop_reason"] == {"maxiter": 48.0}
    # RCCL has executed: a one-rank group ran the real gather path on device memory (outside the timed step)
    co = d["collective"]
    assert "error" not in co, co
    assert co["ranks_seen"] == 1 and co["backend"].startswith("nccl") and co["all_gather_us"] > 0 and co["in_timed_step"] is False
    # the reference's own shapes, each with its CMA-ES generation wall-clock and a CPU figure beside it
    r5, r6 = d["reference_h5"], d["reference_h6_extra"]
    assert r5["episodes_per_generation"] == 27 and "H=5, n_iter=100, K=3" in r5["workload"]
    assert r6["episodes_per_generation"] == 27 and "H=6, n_iter=200, K=6" in r6["workload"]
    for rb in (r5, r6):
        assert rb["cma"]["popsize"] == 9 and rb["cma_generation_ms"] > rb["roofline"]["kernel_ms"] * 0.9
        assert rb["cpu_baseline"]["value"] > 0 and rb["cpu_baseline"]["kind"] == "port"
    # BASELINE config 1: the scalar drop-in API and the object-by-object path, with the CPU oracle beside them
    c1 = d["config1"]
    assert c1["episodes"] == 3 and c1["kernel_ms"] <= c1["eval_weights_ms"] and c1["world_steps_timed"] == 45
    if TIMING:
        assert c1["eval_weights_ms"] < c1["kernel_ms"] + 0.3
        assert 0.05 < c1["world_step_ms"] < 0.45                     # (measured 0.21; round 4: 0.39 ms per world.step())
    assert c1["parity"]["eval_weights_cost_bitwise_equal"] and c1["parity"]["world_step_returns_bitwise_equal"]
    assert c1["cpu_baseline"]["cores"] == 1 and c1["cpu_baseline"]["value"] > 0
    # 28 independent runs of the reference's shape in lockstep: one launch per generation, about the wall time of ONE run
    x28 = d["reference_h5_x28"]
    assert x28["runs"] == 28 and x28["episodes_per_generation"] == 28 * 27 and x28["lockstep"] is True and x28["launch_groups"] in (2, 4) and x28["host_threads"] >= 1   # (four where the probe finds four hardware queues)
    assert x28["generation_ms_ratio_to_one_run"] <= (1.3 if TIMING else 3.0), x28      # (28 runs one after the other: 28)
    assert x28["kernel_ms"] <= x28["cma_generation_ms"] and x28["cpu_baseline"]["value"] > 0
    assert x28["launch"]["workgroups"] >= 28 and x28["stop_reason"] == ["maxiter"]
    for blk in (d["config2"], s4, s5):
        assert blk["cpu_baseline"]["value"] > 0 and blk["cpu_baseline"]["cores"] >= 1
    # every block that names a BASELINE config carries an untimed parity object against the CPU oracle
    for blk, n_min in ((d, 256), (d["config2"], 128), (s4, 256), (s5, 256)):
        par = blk["parity"]
        assert par["episodes_checked"] >= n_min and par["bitwise_equal"] == par["episodes_checked"] == par["within_1e-4_rel"]
        assert par["argmin_flips"] == 0 and par["plan_steps_checked"] >= par["episodes_checked"] * 10 and par["ranks"] == 1
    # counters and the rocprof kernel average are replayed only from a profile of THIS kernel built from THESE sources; then
    # the profile's steady-state kernel average must agree with the live step (it may not exceed it beyond box variation)
    rp = rf["rocprof"]
    assert rf["kernel_symbol"] == "void ocd::mpc_kernel<10, 1, 3, 2, false, true>(ocd::KernelParams)"
    if rp["replayed"]:
        assert rp["kernel_name"] == rf["kernel_symbol"]
        # the committed rocprofv3 average and the live HIP-event time describe the same kernel: within 10 % on any box
        # (4 % on the box the profile was taken on: OCD_TIMING_ASSERTS)
        tol = 0.04 if TIMING else 0.10
        assert abs(rp["kernel_steady_avg_ms"] - rf["kernel_ms"]) <= tol * rf["kernel_ms"], (rp, rf["kernel_ms"])
    else:
        assert rf["traffic"] is None and rp["why"]
    # the parsed roofline object names the bound that binds (fp32 vector issue) beside the contract's HBM figures
    assert rf["binding"] == "valu" and abs(rf["binding_frac"] - d["valu"]["frac"]) < 1e-12 and 0.05 < rf["binding_frac"] < 1
