"""CPU: bench.py's command line through a dry run (--dry-run: the host walk over 1/1000 of the rows).
A plain run prints the headline figure alone; --dump-outputs writes the last step's verdict words."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_steps_verdicts(tmp_path):
    import yaml

    import bench
    import kwgpu as K

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dry-run", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1  # one JSON result line on stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "requests/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["metric"] == bench.METRIC
    assert abs(d["value"] - d["config"]["total_requests"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    # nothing beside the headline figure without --full
    for k in ("kernel_ms", "roofline", "weak_scaling", "cpu_baseline", "timing_modes", "gather",
              "verdicts_final_allowed_fraction"):
        assert d[k] is None, k

    v = np.load(tmp_path / "dump" / "verdicts.npy")
    rows = np.load(tmp_path / "dump" / "rows.npy")
    assert v.dtype == np.float64 and rows.dtype == np.float64
    assert v.nbytes + rows.nbytes <= 64 << 20
    # the same seeded workload evaluated here: the dump holds exactly those words, row for row
    synth, default_rows, _ = bench.CONFIGS["c4_64"]
    n = default_rows // 1000
    with open(os.path.join(ROOT, "configs", "c4_64.yml")) as f:
        env = K.EvaluationEnvironment(yaml.safe_load(f))
    ids = env.policy_ids()
    want = K.SynthBatch(synth, n, seed=bench.SEED).batch().debug_host_walk(env, ids).reshape(n, len(ids))
    assert v.shape == want.shape and np.array_equal(rows, np.arange(n))
    assert np.array_equal(v, want.astype(np.float64))


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    """Above DUMP_WORDS the dump keeps a row sample drawn with the bench's seed: the same rows every
    time, sorted, distinct, and the words of exactly those rows."""
    import bench

    npol = 64
    n = 2 * bench.DUMP_WORDS // npol + 37
    words = (np.arange(n * npol, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), words, n, npol, 0, 1)
    va, ra = np.load(tmp_path / "a" / "verdicts.npy"), np.load(tmp_path / "a" / "rows.npy")
    assert np.array_equal(va, np.load(tmp_path / "b" / "verdicts.npy"))
    assert np.array_equal(ra, np.load(tmp_path / "b" / "rows.npy"))
    assert va.shape == (bench.DUMP_WORDS // npol, npol) and va.nbytes + ra.nbytes <= 64 << 20
    r = ra.astype(np.int64)
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < n
    assert np.array_equal(va, words.reshape(n, npol)[r].astype(np.float64))
