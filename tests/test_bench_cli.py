"""bench.py's launch contract (CPU, no GPU call): `--gpus N` never degrades to a smaller run silently (VERDICT r2 / ADVICE r2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)


def test_more_gpus_than_visible_is_an_error_not_a_smaller_run():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box has the GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout) and "{" not in r.stdout


def test_world_size_must_equal_gpus():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in (r.stderr + r.stdout)
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=4 but --gpus 1" in (r.stderr + r.stdout)


def test_counter_traffic_is_quoted_only_for_the_kernel_sources_it_was_collected_on(tmp_path, monkeypatch):
    """roofline.traffic comes from profiles/latest_*_pmc_summary.json and carries the hash of the kernel sources: a stale file yields
    None and says why."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    tag = bench.kernel_source_tag()
    assert len(tag) == 16
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_tag", lambda: tag)
    rec = {"dpmm::niw_sweep_direct_kernel<4, 4, 2, true>": {"FETCH_SIZE": {"median": 1000.0, "n": 3}, "WRITE_SIZE": {"median": 10.0, "n": 3}}}
    (prof / "latest_bench_pmc_summary.json").write_text(json.dumps(dict(rec, _meta={"kernel_source_tag": tag, "collected": "now"})))
    t, src = bench.pmc_traffic("bench", "niw_sweep_direct_kernel")
    assert t == (2 * 1000.0 + 10.0) * 1024.0 and "latest_bench_pmc_summary.json" in src
    (prof / "latest_bench_pmc_summary.json").write_text(json.dumps(dict(rec, _meta={"kernel_source_tag": "0" * 16})))
    t, src = bench.pmc_traffic("bench", "niw_sweep_direct_kernel")
    assert t is None and "stale" in src
    t, src = bench.pmc_traffic("mult", "mult_sweep")
    assert t is None and src is None


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _fat_record():
    """A record at least as fat as round 5's 20 KB line: every block the default run adds, long texts, a 260-entry K history."""
    legs = {name: {"n": 10 ** 7, "ms_per_step": 2.5, "sweep_kernel_ms": 1.9, "workload": "w" * 300, "host_ms_per_step": {f"t{i}": 0.001 * i for i in range(12)},
                   "roofline": {f"k{i}": 1.2345678901 * i for i in range(25)}} for name in
            ("overlap_var4", "overlap_var1", "inseparable", "k256", "c2", "c3_shard", "shard8_projection", "c4", "c5_shard")}
    roof = {"kernel": "niw_lean_kernel+niw_sweep_direct_kernel+niw_sub_kernel", "bound": "hbm", "achieved": 2431.123456789, "peak": 8000.0, "unit": "GB/s",
            "frac": 0.30389, "hbm_frac": 0.30389, "traffic": 2.83e9, "traffic_source": "s" * 400, "traffic_is_current": True, "traffic_frac": 0.33,
            "algorithmic_bytes_per_launch": 2.6e9, "avg_launch_ms": 1.0721189320087432, "lean_kernel_ms": 1.0, "mfma_pipe_frac": 0.3403521610697151,
            "frac_definition": "d" * 1500, "launches_ms": {"a" * 90: 1.0, "note": "n" * 300}, "dense_f32_frac": 0.733, "dense_launch_ms": 14.58,
            "pruning_factor": 1087.6, "stats_kernels_ms": 0.456, "pmc_frac": 0.35, "mfma_busy": 0.37}
    return {"metric": "Gibbs iterations/sec, N=10M D=64 NIW", "value": 614.4183087120751, "unit": "iterations/s", "n_gpus": 1, "steps": 20, "warmup": 5, "settle": 100,
            "ms_per_step": 1.6275556665884021, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "NIW D=64 N=10000000 ... MixtureVar 100 ..." + "x" * 300, "points_per_gpu": 10 ** 7, "parallelism": "p" * 200, "master": "m" * 500,
                       "worker_options_overridden": None,
                       "also_measured": {"host_master_it_per_s": 551.5, "host_master_ratio_to_headline": 0.8976, "host_cpu_model": "AMD EPYC 9575F 64-Core Processor",
                                         "growth": {"it_per_s_whole_run": 537.19, "K_final": 32, "K_true": 32, "nmi": 1.0, "moving_labels_it_per_s": 602.9},
                                         "shard8": {"shard_ms_per_step": 0.3264, "shard_ms_per_step_one_collective_form": 0.3214, "assumed_allreduce_ms_per_step": 0.04,
                                                    "projected_speedup_1_to_8": 4.5, "speedup_without_collectives": 4.99},
                                         **{f"{n}_ms_per_step": 2.49220949990558 for n in ("overlap_var4", "overlap_var1", "k256", "c2", "c4", "c5_shard")},
                                         "inseparable_sweep_kernel_ms": 22.2, "inseparable_full_evals_per_tile": 32.0, "c4_traffic_frac": None}},
            "roofline": roof, "comm": {f"c{i}": i for i in range(12)}, "blocks": {"it_per_s": [600.0] * 5},
            "host_ms_per_step": {f"t{i}": 0.001 * i for i in range(14)},
            "growth": {"K_history": list(range(260)), "it_per_s_whole_run": 537.0}, "host_master": {"note": "h" * 400, "it_per_s": 551.5},
            "legs": legs,
            "cpu_baseline": {"value": 0.2846, "unit": "iterations/s", "cores": 16, "kind": "port", "parallelism": "multiprocess",
                             "cpu_model": "AMD EPYC 9575F 64-Core Processor", "julia_found": False, "sample": "s" * 420, "sample_fraction": 1.0}}


def test_the_contract_line_is_compact_and_parses(tmp_path, monkeypatch, capsys):
    """round 5's ONE stdout line had grown to 20 KB and the driver recorded `parsed: null`.  The line the driver reads -- the LAST
    line of stdout -- stays under 4 KB whatever the run measured, parses, and carries the contract fields + roofline + cpu_baseline; the
    rest goes to bench_details.json and stderr."""
    import json
    bench = _bench_module()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    rec = _fat_record()
    assert len(json.dumps(rec)) > 12000
    bench.emit(rec)
    cap = capsys.readouterr()
    last = cap.out.splitlines()[-1]
    assert len(cap.out.splitlines()) == 1 and len(last) < 4096 and len(last.encode()) < 8192
    line = json.loads(last)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == rec["value"] and line["ms_per_step"] == rec["ms_per_step"]
    assert "workload" in line["config"] and "MixtureVar" in line["config"]["workload"] and "model" not in line["config"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "hbm_frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms"):
        assert k in line["roofline"], k
    assert line["roofline"]["bound"] in ("hbm", "mfma") and abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-3
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert "legs" not in line and "growth" not in line and "K_history" not in last
    full = json.loads((tmp_path / "bench_details.json").read_text())
    assert full["growth"]["K_history"] == list(range(260)) and "legs" in full
    assert "bench.py details: " in cap.err


def test_traffic_is_reported_whenever_a_counter_summary_exists(tmp_path, monkeypatch):
    """`roofline.traffic` silently became null when the committed summary carried another source tag.  With
    allow_stale the figure is reported and the text says which sources it was collected on; a matching tag reports it as current."""
    import json
    bench = _bench_module()
    tag = bench.kernel_source_tag()
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_tag", lambda: tag)
    rec = {"dpmm::niw_lean_kernel": {"FETCH_SIZE": {"median": 1000.0}, "WRITE_SIZE": {"median": 10.0}},
           "dpmm::niw_sweep_direct_kernel<4, 4, 2, true, false, true, true>": {"FETCH_SIZE": {"median": 100.0}, "WRITE_SIZE": {"median": 1.0}}}
    f = tmp_path / "profiles" / "latest_bench_pmc_summary.json"
    f.write_text(json.dumps(dict(rec, _meta={"kernel_source_tag": tag, "collected": "now"})))
    t, src = bench.pmc_traffic("bench", bench.SWEEP_KERNELS_64, allow_stale=True)
    assert t == (2 * 1100.0 + 11.0) * 1024.0 and "stale" not in src and bench.pmc_is_current("bench")
    f.write_text(json.dumps(dict(rec, _meta={"kernel_source_tag": "f" * 16})))
    t, src = bench.pmc_traffic("bench", bench.SWEEP_KERNELS_64, allow_stale=True)
    assert t == (2 * 1100.0 + 11.0) * 1024.0 and "stale" in src and not bench.pmc_is_current("bench")


def test_the_committed_counter_summaries_parse_for_the_kernels_the_bench_quotes():
    """Whatever tag the committed summaries carry, the kernels bench.py looks for are in them (a renamed kernel would make traffic null for ever)."""
    bench = _bench_module()
    t, _ = bench.pmc_traffic("bench", bench.SWEEP_KERNELS_64, allow_stale=True)
    assert t is not None and t > 1e9
    t, _ = bench.pmc_traffic("mult", "mult_sweep", allow_stale=True)
    assert t is not None and t > 1e8


def test_options_default_to_a_plain_run(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


def test_threaded_generation_is_bit_identical_to_the_one_call_generator():
    import importlib
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    load_package()
    host = importlib.import_module("dpmmsubclusters_jl_amd.host")
    bench = _bench_module()
    N, D, K, lo, hi = 230000, 8, 4, 12345, 230000
    X0, y0 = host.gaussian_mixture_shard(N, D, K, 100.0, bench.DATA_SEED, lo, hi)
    X1, y1 = bench.gaussian_mixture_shard_threaded(host, N, D, K, 100.0, bench.DATA_SEED, lo, hi, threads=4, part=50000)
    assert np.array_equal(X0, X1) and np.array_equal(y0, y1)


class _FakeWorker:
    def __init__(self, n):
        rng = np.random.default_rng(3)
        self.lab, self.sub = rng.integers(1, 33, n), rng.integers(1, 3, n)

    def get_labels(self):
        return self.lab.copy(), self.sub.copy()


class _FakeSampler:
    def __init__(self, K, D, big):
        rng = np.random.default_rng(4)
        self.params = {"mu": rng.normal(size=(3 * K, D)), "R": rng.normal(size=(3 * K, D, big)), "logdet": rng.normal(size=3 * K)}
        self.weights, self.lr_weights = np.full(K, 1.0 / K), np.full((K, 2), 0.5)
        self.N = rng.integers(0, 1000, (K, 3)).astype(np.float64)
        self.K = K


def test_dump_outputs_are_float_arrays_within_the_limit_and_repeatable(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, at most 64 MB in all, the same files for the same state (fixed, seeded samples)."""
    bench = _bench_module()
    n = 3 * bench.DUMP_POINTS
    wk, s = _FakeWorker(n), _FakeSampler(32, 64, 1000)          # R has 6.1 M entries: sampled
    names = bench.dump_outputs(str(tmp_path / "a"), s, wk)
    bench.dump_outputs(str(tmp_path / "b"), s, wk)
    assert {"labels", "sub_labels", "point_index", "mu", "R", "logdet", "weights", "lr_weights", "counts", "K"} <= set(names)
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name
        total += (tmp_path / "a" / (name + ".npy")).stat().st_size
    assert total <= 64 << 20
    idx = np.load(tmp_path / "a" / "point_index.npy").astype(np.int64)
    assert len(idx) == bench.DUMP_POINTS and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "labels.npy"), wk.lab[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "mu.npy"), s.params["mu"])
    assert np.load(tmp_path / "a" / "R.npy").size == bench.DUMP_ENTRIES and float(np.load(tmp_path / "a" / "K.npy")[0]) == 32


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_the_steps_and_dumps_the_last_ones_outputs(tmp_path):
    """A plain run (no --full) prints the contract line for exactly --steps timed steps, measures nothing beside the headline block,
    and --dump-outputs writes the state of its last step."""
    import json
    n = 200000
    r = _run(["--gpus", "1", "--points", str(n), "--steps", "7", "--warmup", "2", "--settle", "5", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["value"] > 0
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6 * 1e3
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line, k
    d = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("bench.py details: ")][-1][len("bench.py details: "):])
    for k in ("blocks", "growth", "host_master", "legs", "cpu_baseline"):
        assert k not in d, k
    out = tmp_path / "out"
    files = sorted(out.iterdir())
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    arrs = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    K = int(arrs["K"][0])
    assert K >= 1 and len(arrs["labels"]) == n and len(arrs["sub_labels"]) == n
    assert arrs["labels"].min() >= 0 and arrs["labels"].max() <= K and np.isfinite(arrs["mu"]).all()
    assert int(arrs["counts"].reshape(-1, 3)[:K, 0].sum()) == n
