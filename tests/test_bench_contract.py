"""The driver depends on bench.py's output contract (BASELINE.json): exactly one
JSON line on stdout with the required keys.  This lane catches contract breaks
before the driver does."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {
    "metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int,
    "warmup": int, "ms_per_step": float, "higher_is_better": bool, "scaling": str,
    "dtype": str, "data": str, "config": dict,
}


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, "bench.py", *extra, "--steps", "3", "--warmup", "1",
         "--network", "FC", "--dataset", "MNIST", "--batch-size", "8",
         "--device", "cpu"],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must be EXACTLY one line, got {len(lines)}"
    return json.loads(lines[0])


def test_plain_run_skips_extra_arms_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the reference arm and the loss-readback step do not run (their
    keys are null); --dump-outputs writes the last timed step's updated parameters,
    identical from run to run on CPU (same seeded inputs, reproducible autograd),
    and runs that step from the seeded start state."""
    import numpy as np

    dumps = {}
    for name, lr in (("a", "0.01"), ("b", "0.01"), ("c", "0.02"), ("d", "0.03")):
        r = _run_bench("--lr", lr, "--dump-outputs", str(tmp_path / name))
        for k, ty in REQUIRED.items():
            assert isinstance(r[k], ty), (k, type(r[k]))
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        assert r["vs_baseline"] is None and r["baseline_images_per_sec"] is None
        assert r["final_loss"] is None
        assert os.listdir(tmp_path / name) == ["params.npy"]
        assert os.path.getsize(tmp_path / name / "params.npy") <= 64e6
        dumps[name] = np.load(tmp_path / name / "params.npy")
    a, c, d = dumps["a"], dumps["c"], dumps["d"]
    assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all()
    np.testing.assert_array_equal(a, dumps["b"])
    # The dumped step started from the seeded start state with zero momentum, so
    # params = start - lr * g with ONE g for every lr: the dump is linear in lr.
    # Had the step run from the state the earlier steps left, those steps (taken
    # at another lr) would have moved g.  Bound: a few float32 ulps of max|param|.
    atol = 8 * np.finfo(np.float32).eps * np.abs(a).max()
    assert np.abs(c - a).max() > 100 * atol, "the dumped step changed nothing"
    np.testing.assert_allclose(d - c, c - a, rtol=0, atol=atol)


def test_bench_stdout_is_one_contract_json_line():
    r = _run_bench("--full")
    for k, ty in REQUIRED.items():
        assert k in r, f"missing contract key {k}"
        assert isinstance(r[k], ty), (k, type(r[k]))
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["scaling"] == "weak"
    assert r["higher_is_better"] is True
    assert "vs_baseline" in r  # may be float or null for approach=baseline
    cfg = r["config"]
    for k in ("model", "global_batch", "parallelism", "topology"):
        assert k in cfg, f"missing config key {k}"
    # honesty telemetry
    for k in ("final_loss", "skipped_updates"):
        assert k in r, f"missing telemetry key {k}"
