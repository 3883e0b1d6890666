"""bench.py's stdout contract: the driver parses the LAST stdout line, and
r05's 18,962-byte line was not parsed.  The full result of a
real run (profiles/r05/bench_final.log, every informational leg included)
goes through bench.emit(): the printed line must be the last stdout line,
parse as JSON, stay <= 4 KB and carry the contract keys, the roofline and the
cpu_baseline; the full result must land in the side file."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config")


def _full_result():
    with open(os.path.join(ROOT, "profiles", "r05", "bench_final.log")) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def test_compact_line_parses_and_fits(tmp_path):
    full = _full_result()
    assert len(json.dumps(full)) > 3 * bench.STDOUT_LIMIT  # the stub really is the oversized line
    side = tmp_path / "detail.json"
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(full, str(side))
    lines = buf.getvalue().strip().splitlines()
    line = lines[-1]
    assert len(line.encode()) <= bench.STDOUT_LIMIT
    d = json.loads(line)
    for k in CONTRACT:
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "bytes_per_launch_algorithmic"):
        assert k in d["roofline"], k
    assert d["roofline"]["frac"] == full["roofline"]["frac"]
    for k in ("value", "unit", "cores", "kind", "sample", "parity_bit_exact_on_sample"):
        assert k in d["cpu_baseline"], k
    assert "n11" in d["perf_mode"] and "Mpatches_per_s" in d["perf_mode"]["n11"]
    assert d["scaling_leg"]["fast"]["ranks_store_equal"] is True
    # the side file holds everything
    assert json.loads(side.read_text()) == full


def _records(n):
    import numpy as np

    from densepoints_amd import PATCH_DTYPE

    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, size=n * PATCH_DTYPE.itemsize, dtype=np.uint8)
    kids = np.frombuffer(raw.tobytes(), dtype=PATCH_DTYPE).copy()
    for f in ("pos", "normal", "score"):  # finite floats, so that == compares them
        kids[f] = rng.standard_normal(kids[f].shape).astype(np.float32)
    return kids, rng.integers(0, 2, size=n, dtype=np.uint8)


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.steps, a.warmup, a.dump_outputs, a.detail) == (False, 7, 2, None, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.detail.endswith("bench_detail.json")


def test_dump_outputs_holds_every_field_exactly(tmp_path):
    import numpy as np

    kids, acc = _records(1000)
    bench.dump_outputs(str(tmp_path / "o"), kids, acc)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in os.listdir(tmp_path / "o")}
    assert set(got) == {"rows", "accept"} | set(kids.dtype.names)
    assert all(a.dtype in (np.float32, np.float64) and len(a) == 1000 for a in got.values())
    assert np.array_equal(got["rows"], np.arange(1000)) and np.array_equal(got["accept"], acc)
    for f in ("pos", "normal", "score", "ref", "seq", "evals", "rgb", "flags", "parent"):
        assert np.array_equal(got[f], kids[f]), f
    for f in ("vis", "cand"):
        w = got[f].astype(np.uint64)
        back = np.stack([w[:, 0] | (w[:, 1] << np.uint64(32)), w[:, 2] | (w[:, 3] << np.uint64(32))], axis=1)
        assert np.array_equal(back, kids[f]), f


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path, monkeypatch):
    import numpy as np

    kids, acc = _records(1000)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 20000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), kids, acc)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= 20000
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert 100 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "pos.npy"), kids["pos"][rows])
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


def test_compact_sheds_legs_before_exceeding_limit(tmp_path):
    full = _full_result()
    full["config"]["workload"] = "x" * 5000  # pathological: the contract part alone is large
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(full, None)
    line = buf.getvalue().strip().splitlines()[-1]
    d = json.loads(line)
    assert "value" in d and "roofline" in d and "cpu_baseline" in d
    assert "perf_mode" not in d and "seed_generation" not in d
