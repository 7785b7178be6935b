"""The bench line the driver parses: every key of the contract, on the line recorded with the final build of the round
(profiles/r03_bench_final.json = stdout of `python bench.py --full` on one MI355X; a plain run prints the headline keys
only), the --dump-outputs files, and a plain run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config")
FULL_KEYS = ("roofline", "cpu_baseline", "reference_cpu_captured", "time_to_solution", "smoother_size_sweep", "residual_floor")


def test_recorded_bench_line_has_the_contract_keys():
    line = open(os.path.join(ROOT, "profiles", "r03_bench_final.json")).read().strip()
    assert "\n" not in line                                   # ONE JSON line
    d = json.loads(line)
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in HEADLINE_KEYS + ("roofline", "cpu_baseline"):
        assert k in d, k
    assert base["metric"].startswith(d["metric"]) and d["metric"].startswith("MDoF/s per V-cycle")   # BASELINE's headline clause
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 4097 * 4097 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    # a roofline fraction: bytes the launch must move / time / peak, never above 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.0 < r["frac"] <= 1.0
    assert abs(r["achieved"] - r["bytes_per_launch"] / (r["launch_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["unfused_equivalent_gbs"] > r["achieved"]                      # the per-operator accounting lives under its own key
    assert r["traffic"] is None or (0.9 * r["bytes_per_launch"] < r["traffic"] < 1.5 * r["bytes_per_launch"] and r["traffic_source"])
    for p in ("f32", "f64"):
        for name, k in r["kernels"][p].items():
            assert 0.0 < k["frac"] <= 1.0, (p, name)
    s = r["smoother_hbm"]                                                   # the north-star kernel, HBM proper, beside its ceiling
    assert 0.0 < s["frac"] <= 1.0 and 0.5 < s["frac_of_stream_ceiling"] <= 1.05 and s["target_frac"] == 0.70
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["unit"] == d["unit"]
    ref = d["reference_cpu_captured"]                                       # the reference's own CPU V-cycle at the bench size
    assert ref["kind"] == "reference" and ref["cores"] == 1 and "4097^2" in ref["sample"] and 20.0 < ref["seconds_per_cycle"] < 40.0
    assert d["iterations"] == d["steps"] and d["residual_floor"] > 0 and 1 <= d["iterations_to_floor"] <= 40
    assert d["iterations_to_1e-10_absolute"] is None                        # unreachable at 4097^2 in fp64: the floor says why
    # round 3: time to solution per policy, the adaptive policy never behind double, the size sweep
    t = d["time_to_solution"]
    for pol in ("adaptive", "double", "defect"):
        assert t[pol]["iterations_to_floor"] >= 1 and t[pol]["time_to_floor_ms"] > 0
    assert t["adaptive"]["time_to_floor_ms"] <= 1.05 * t["double"]["time_to_floor_ms"]
    assert d["switch_reason"] in ("fp32_skipped", "fp32_floor", "threshold", "stagnation")
    assert [row["n"] for row in d["smoother_size_sweep"]["rows"]] == [4097, 8193, 16385]
    assert "span" in r["kernel"] and "span_leg_nomid" in r["kernels"]["f64"]      # the spanning leg is the dominant kernel
    assert r["build"] and ("traffic_is_from_this_build" in r)


class _FakeEngine:
    def __init__(self, n):
        self.n = n

    def get_solution(self, dtype):
        return np.arange(self.n * self.n, dtype=dtype).reshape(self.n, self.n)


@pytest.mark.parametrize("n", [4097, 129])
def test_dump_outputs_files(tmp_path, n):
    """--dump-outputs: fp64 .npy files, at most 64 MB in all; the bench-size iterate as a fixed seeded sample with its
    row-major indices, a small one whole."""
    import bench
    r = {"residual_history": [1.0, 0.5, 0.25], "precision_codes": [0, 1, 1]}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _FakeEngine(n), r)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b), name          # the same sample every run
        total += a.nbytes
    assert total <= 64 * 2**20
    assert np.array_equal(np.load(tmp_path / "a" / "residual_history.npy"), r["residual_history"])
    assert np.array_equal(np.load(tmp_path / "a" / "precision_codes.npy"), r["precision_codes"])
    if n * n * 8 <= bench.DUMP_FULL_BYTES:
        assert names == ["precision_codes.npy", "residual_history.npy", "solution.npy"]
        assert np.array_equal(np.load(tmp_path / "a" / "solution.npy"), _FakeEngine(n).get_solution(np.float64))
    else:
        u, idx = np.load(tmp_path / "a" / "solution_sample.npy"), np.load(tmp_path / "a" / "solution_sample_index.npy")
        assert u.shape == idx.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(idx) > 0)
        assert np.array_equal(u, idx)                                        # the fake iterate is its own index


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run: exactly --steps timed steps, the headline keys, none of the --full diagnostics, and the outputs of
    the LAST timed step under --dump-outputs: the residual norm of the dumped iterate, recomputed with the oracle, is the
    engine's residual_last (and not the norm after any earlier step, e.g. the warm-up)."""
    from oracle import mg_oracle as O
    import bench
    n, K = 129, 8
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                          "--grid-n", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in HEADLINE_KEYS:
        assert k in d, k
    for k in FULL_KEYS:
        assert k not in d, k
    assert d["steps"] == d["iterations"] == K and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - n * n / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    hist = np.load(tmp_path / "residual_history.npy")
    assert hist.shape == (K,) and hist[-1] == d["residual_last"] and hist[0] == d["residual_first"]
    codes = np.load(tmp_path / "precision_codes.npy")
    assert codes.shape == (K,) and int(np.sum(codes == 0)) == d["cycles_fp32"]
    u = np.load(tmp_path / "solution.npy")
    assert u.shape == (n, n) and u.dtype == np.float64 and np.all(np.isfinite(u))
    hx, hy = O.grid_spacing(n, n)
    rn = float(O.l2_norm(O.residual(u, bench.sine_rhs(n, n), hx, hy, -1.0), hx, hy))
    assert int(np.argmin(np.abs(hist - rn))) == K - 1, (rn, hist)
    if codes[-1] == 1:                                   # an fp64 last cycle: the same norm up to summation order
        assert abs(rn / hist[-1] - 1.0) < 1e-4, (rn, hist[-1])
