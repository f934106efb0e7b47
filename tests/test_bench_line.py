"""bench.py's stdout line without a GPU: compact() applied to a full record of the size a real run produces (profiles/r04_bench.json:
22 KB, the record whose one-line form was cut by the driver's 8,000-byte stdout tail in round 4) stays under 4,000 bytes and keeps
every contract key, the roofline's numbers and cpu_baseline. The GPU contract tests assert the same on live runs."""
import importlib.util
import json
import os

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bench():
    spec = importlib.util.spec_from_file_location("rd_bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _full(n_ranks=1):
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench.json")))
    legs = {}
    for k, v in full["e2e_cli"].items():            # the round-4 record's legs under this round's names, + the three new ones
        if isinstance(v, dict) and "reads_per_s" in v:
            legs["plain_to_plain" if k == "large" else k] = dict(v, reads_per_s_after_first_chunk=1.07 * v["reads_per_s"])
    for extra in ("bgzf_to_plain", "bgzf_to_gz_host_parse", "plain_to_plain_host_parse", "seqlike_plain_to_gz", "seqlike_bgzf_to_gz", "seqlike_gz_to_gz"):
        legs[extra] = dict(legs["plain_to_gz"])          # (round 6: the three legs on sequencer-like files; the *_host_parse legs left the line)
    full["roofline"].update(effective_clock_ghz=1.873, package_power_w=1288.4)
    full["e2e_cli"] = legs
    full["cpu_baseline"]["sample_short"] = "first 229376 reads of rank 0's R1 stream; C port (AVX + OpenMP) of the padded 100-step BiLSTM, batch 1024/thread, 16 threads, 12.3 s"
    full["n_gpus"] = n_ranks
    full["config"]["ranks"] = [{"rank": r, "local_rank": r, "device": "cuda:%d" % r, "device_uuid": "GPU-%032x" % r, "pid": 1000 + r,
                                "first_gather_s": 0.1234, "step0_label_counts": [1000000, 48576, 0]} for r in range(n_ranks)]
    return full


def test_compact_line_fits_the_drivers_tail():
    b = _bench()
    for n in (1, 8):
        full = _full(n)
        line = json.dumps(b.compact(full), separators=(",", ":"))
        assert len(line) < 3500, len(line)
        j = json.loads(line)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                  "data", "config", "roofline", "cpu_baseline"):
            assert k in j, k
        assert j["value"] == full["value"] and j["ms_per_step"] == full["ms_per_step"] and "workload" in j["config"]
        assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(j["roofline"])
        assert {"value", "unit", "cores", "kind", "sample"} <= set(j["cpu_baseline"])
        assert abs(j["roofline"]["frac"] - j["roofline"]["achieved"] / j["roofline"]["peak"]) < 1e-4
        assert j["e2e_bgzf_to_gz"]["rps"] > 0 and j["e2e_plain_to_plain"]["host_cores_busy"] > 0 and "ranks" not in j["config"]
        assert j["e2e_seqlike_gz_to_gz"]["rps"] > 0 and "e2e_bgzf_to_gz_host_parse" not in j and j["roofline"]["effective_clock_ghz"] == 1.873
        assert "parity_sample" in j and j["alt_fp32_frac"] > 0.5


def test_emit_writes_the_full_record_and_prints_one_line(tmp_path, capsys):
    b = _bench()

    class A:
        full_out = str(tmp_path / "full.json")
        verbose = False
    full = _full()
    b.emit(full, A)
    out = capsys.readouterr().out
    assert out.endswith("\n") and out.count("\n") == 1 and len(out) < 4000
    assert json.load(open(A.full_out))["e2e_cli"]["gz_to_gz"]["calls"]          # the nested per-call records live in the file


def test_compact_line_of_a_plain_run():
    """a plain run (no --full) measures no roofline, no alt kernels, no CLI legs and no CPU baseline: its line keeps the contract keys"""
    b = _bench()
    full = _full()
    for k in ("roofline", "alt_fp32_kernel", "alt_no_prefix_table", "encoder", "device_gzip", "e2e_cli", "cpu_baseline", "parity_sample"):
        full.pop(k, None)
    for k in ("kernel_only_reads_per_s", "gpu_over_cpu", "timed_regions", "device_path_over_kernel_only"):
        full["config"].pop(k, None)
    j = json.loads(json.dumps(b.compact(full), separators=(",", ":")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config"):
        assert k in j, k
    assert j["value"] == full["value"] and j["ms_per_step"] == full["ms_per_step"] and j["dtype"] == full["dtype"]
    assert "roofline" not in j and "cpu_baseline" not in j and "full_record" not in j and "kernel_only_reads_per_s" not in j["config"]


def test_dump_outputs_float32_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per array; above the cap the same seeded sample of rows from every array, indices alongside"""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(3)
    lg = [torch.randn(1000, 2, generator=g), torch.randn(1000, 2, generator=g)]
    lab = torch.randint(-1, 2, (1000,), generator=g, dtype=torch.int8)
    b.dump_outputs(str(tmp_path / "all"), lg, lab)
    got = {n: np.load(str(tmp_path / "all" / (n + ".npy"))) for n in ("logits_r1", "logits_r2", "labels")}
    assert all(a.dtype == np.float32 for a in got.values()) and not (tmp_path / "all" / "sample_rows.npy").exists()
    assert (got["logits_r1"] == lg[0].numpy()).all() and (got["logits_r2"] == lg[1].numpy()).all() and (got["labels"] == lab.numpy()).all()
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 4000)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), lg, lab)
    rows = np.load(str(tmp_path / "s1" / "sample_rows.npy"))
    assert rows.dtype == np.float64 and (rows == np.load(str(tmp_path / "s2" / "sample_rows.npy"))).all()
    r = rows.astype(np.int64)
    assert len(r) == len(set(r.tolist())) and 0 < len(r) < 1000
    sizes = sum(os.path.getsize(str(p)) for p in (tmp_path / "s1").iterdir())
    assert sizes < 4000 + 4 * 128                                    # (+ the .npy headers)
    assert (np.load(str(tmp_path / "s1" / "logits_r2.npy")) == lg[1].numpy()[r]).all()
    assert (np.load(str(tmp_path / "s1" / "labels.npy")) == lab.numpy()[r]).all()
