"""bench.py --dump-outputs and the step arguments: the files the option writes and the arguments it refuses (without a GPU), and what a
plain run leaves to --full (GPU)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_every_array_as_float64(tmp_path):
    b = _bench()
    idx = np.arange(4096, dtype=np.int32).reshape(-1, 1) * 24
    score = np.linspace(-170.0, 3.0, 4096).reshape(-1, 1)
    b.dump_outputs(str(tmp_path / "d"), idx=idx, score=score)
    assert sorted(os.listdir(tmp_path / "d")) == ["idx.npy", "score.npy"]
    i, s = np.load(tmp_path / "d" / "idx.npy"), np.load(tmp_path / "d" / "score.npy")
    assert i.dtype == s.dtype == np.float64 and i.shape == s.shape == (4096, 1)
    assert np.array_equal(i, idx) and np.array_equal(s, score)


def test_dump_above_the_limit_keeps_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4096 + 1000)
    m = 500
    idx, score = np.arange(m).reshape(-1, 1), np.arange(m, dtype=np.float64).reshape(-1, 1) / 7
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), idx=idx, score=score)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= b.DUMP_LIMIT_BYTES
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert 0 < len(rows) < m and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "idx.npy")[:, 0], rows)
    assert np.array_equal(np.load(tmp_path / "a" / "score.npy"), score[rows])
    for f in ("rows.npy", "idx.npy", "score.npy"):                      # the same sample in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_steps_below_one_are_refused():
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-500:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_what_a_full_run_dumps(tmp_path):
    """A plain run stops after the timed steps: its line carries the headline fields and none of what --full measures, and its
    dump and headline fields are those of a --full run of the same arguments."""
    import json
    common = ["--steps", "1", "--warmup", "0", "--db", "6001", "--queries", "130"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-extra"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *common, *extra, "--dump-outputs", str(tmp_path / name)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "queries/s" and plain["higher_is_better"] is True
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"):
        assert plain[key] == full[key], key
    assert not {"roofline", "parity", "collective", "per_rank", "cpu_baseline", "extra"} & set(plain)
    assert {"roofline", "parity", "collective", "per_rank"} <= set(full) and full["parity"]["planted_top1_correct"] == 130
    for f in ("idx.npy", "score.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f))
