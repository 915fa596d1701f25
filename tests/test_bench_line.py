"""bench.py's printed line (CPU): the contract's keys, north_star's CSR SpMV target last, and the whole line inside the
8 KB of stdout the driver records -- checked on the full record of a round-5 run (profiles/r05zc_bench.json)."""
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _full_record():
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "r05zc_bench.json")) if ln.startswith("{")]
    return json.loads(lines[-1])


def test_compact_line_fits_the_driver_tail_with_the_csr_target_last():
    full = _full_record()
    line = bench.compact_line(full)
    text = json.dumps(line)
    assert len(text) < 6000, len(text)
    for k in CONTRACT:
        assert k in line, k
    assert list(line)[-1] == "roofline_csr_spmv"
    cs = line["roofline_csr_spmv"]
    assert cs["frac"] == bench._r(full["roofline_csr_spmv"]["frac"])
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(cs)
    # the tail the driver keeps (8 183 characters in round 5) holds the whole object
    assert '"roofline_csr_spmv"' in text[-8000:]
    # every solve_level run survives, as one row
    assert len(line["solve_level"]["runs"]) == len(full["solve_level"]["runs"])
    assert line["roofline"]["avg_launch_us"] == bench._r(full["roofline"]["avg_launch_us"])


def test_compact_line_without_optional_sections():
    full = _full_record()
    for k in ("spmv_A", "roofline_csr_spmv", "mg_apply", "solve_level", "time_to_solution", "host_buffer_matvec"):
        full[k] = None
    full["cpu_baseline"] = None
    line = bench.compact_line(full)
    assert line["cpu_baseline"] is None and line["vs_baseline"] is None   # contract keys stay, even when null
    assert "roofline_csr_spmv" not in line and "mg_apply" not in line


def test_compact_line_of_a_plain_run():
    """Without --full the record has no section beside the headline: the contract's keys stay (null where unmeasured)."""
    full = _full_record()
    for k in ("roofline", "roofline_second_f_solve", "spmv_A", "roofline_csr_spmv", "mg_apply", "solve_level",
              "time_to_solution", "host_buffer_matvec", "cpu_baseline"):
        full[k] = None
    line = bench.compact_line(full)
    for k in CONTRACT:
        assert k in line, k
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"]
    assert set(line) == set(CONTRACT), set(line) ^ set(CONTRACT)
    json.dumps(line, allow_nan=False)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: a float64 .npy of the output vector; above the size limit the same seeded sample every time."""
    import numpy as np
    torch = pytest.importorskip("torch")
    out = torch.arange(1000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), out, 0, 1)
    a = np.load(tmp_path / "a" / "apply_out.npy")
    assert a.dtype == np.float64 and np.array_equal(a, out.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 200)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), out, 1, 2)   # two ranks share the limit: 100 entries each
    b, c = (np.load(tmp_path / d / "apply_out_rank1.npy") for d in ("b", "c"))
    assert b.shape == (100,) and np.array_equal(b, c)
    idx = (b * 2).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(out.numpy()[idx], b)
