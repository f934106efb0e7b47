#!/usr/bin/env python
"""--ubam_output measured (detect.py --ubam_output, ubam.py, csrc/rd_bam_encode.hpp), in the manner of tools/bam_bench.py. Prints one
JSON line per measurement and appends it to --out (default profiles/ubam_bench.jsonl).
    python tools/ubam_bench.py [--reads 4194304] [--calls 3] [--only kernel|cli] [--keep DIR] [--out FILE]
  kernel  rd_bam_encode ALONE on a resident chunk of 2^20 reads of 100 bp and of 8,192 reads of 10 kb: 20 calls timed with device
          events, median with lowest-highest; the bytes it moves - the text read once (the '+' lines and the comments are not, the
          whole text is counted all the same), the raw bytes written once, per record 28 bytes of the chunk's tables read and 8 of
          raw_start plus 12 of the workspace written and read again - as TB/s and as the fraction of an HBM-bound pass at 8 TB/s.
          The neighbouring figures of the README: raw gather 0.12 / 0.25, rd_bam_index 0.067 / 0.085.
  cli     `--reads` single-end reads of 100 bp, plain FASTQ input: -> .bam --ubam_output against -> .fq.gz without the flag (the
          parent's behaviour and the yardstick). One untimed warm-up call of each leg, then `--calls` timed calls of each, the legs
          ALTERNATING in one process (model load excluded: Predictor.timing["detect_s"]); the ratio of the medians, whether the
          with-flag median lies inside the yardstick's spread, the bytes written and the peak of torch's allocator on both legs.
The input is written by a process that never touches the GPU."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = None


def emit(doc):
    line = json.dumps(doc)
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def _us(v):
    return {"median": round(statistics.median(v), 1), "lowest": round(v[0], 1), "highest": round(v[-1], 1)}


def _make(job):
    """`reads` reads of 100 bp as plain FASTQ (bam_bench's rows: 'r' + 9 digits, NovaSeq-like binned qualities)"""
    import bam_bench
    path, reads = job
    if os.path.exists(path):
        return
    step = 1 << 18
    with open(path + ".tmp", "wb") as fh:
        for first in range(0, reads, step):
            fh.write(bam_bench._rows(min(step, reads - first), first, 100, seed=1000 + first // step)[0].tobytes())
    os.replace(path + ".tmp", path)


def bench_kernel(calls=20):
    import numpy as np
    import torch
    import bam_bench
    from ribodetector_amd import bam, ubam
    dev = torch.device("cuda:0")
    for shape, n, length in (("short", 1 << 20, 100), ("long", 8192, 10000)):
        step = max(1, (64 << 20) // (2 * length))
        fq = np.concatenate([bam_bench._rows(min(step, n - f), f, length, seed=7 + f // step)[0] for f in range(0, n, step)])
        frec = fq.shape[1]
        text = torch.from_numpy(fq.reshape(-1)).to(dev)
        rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * frec
        so = (rs[:-1] + bam_bench.NAME + 1).contiguous()
        sl = torch.full((n,), length, dtype=torch.int32, device=dev)
        cap = bam.ubam_bound(text.numel(), n)
        raw = torch.empty(((cap + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
        flags = ubam.flags_word()
        us = bam_bench._events(lambda: ubam.encode(text, rs, so, sl, n, flags, raw_cap=cap, raw=raw), calls)
        _, raw_start, info = ubam.encode(text, rs, so, sl, n, flags, raw_cap=cap, raw=raw)
        info = info.cpu().tolist()
        k = n // 2
        a, b = int(raw_start[k]), int(raw_start[k + 1])
        assert info[3] == 0 and info[0] == n and info[2] == info[7] == -1 and bytes(raw[a:b].cpu().numpy()) == bam.from_fastq(fq[k].tobytes()), info
        med = statistics.median(us)
        moved = text.numel() + info[1] + n * (28 + 2 * 8 + 2 * 12)
        emit({"measurement": "kernel_ubam", "what": "rd_bam_encode", "shape": shape, "read_len": length, "records": n, "text_bytes": text.numel(),
              "raw_bytes": info[1], "calls": calls, "us_per_call": _us(us), "bytes_moved": moved, "TB_per_s": round(moved / med / 1e6, 3),
              "fraction_of_hbm_bound_pass_at_8TBps": round(moved / 8e12 / (med * 1e-6), 4),
              "neighbours_fraction_short_long": {"rd_bam_raw_tab + rd_bam_raw_gather": [0.12, 0.25], "rd_bam_index": [0.067, 0.085]}})
        del text, raw
        torch.cuda.empty_cache()


def bench_cli(d, reads, calls):
    import torch
    from ribodetector_amd import detect
    src = os.path.join(d, "se_%d.fq" % reads)
    argv = {"fq_to_fqgz": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_yard.fq.gz")],
            "fq_to_ubam": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_out.bam"), "--ubam_output"]}
    for k in argv:
        detect.main(argv[k], log_level="WARNING")
    secs, peak, last = {k: [] for k in argv}, {}, {}
    for _ in range(calls):
        for k in argv:
            torch.cuda.reset_peak_memory_stats()
            last[k] = detect.main(argv[k], log_level="WARNING")
            secs[k].append(last[k].timing["detect_s"])
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    rate = {k: sorted(reads / s for s in v) for k, v in secs.items()}
    med = {k: statistics.median(v) for k, v in rate.items()}
    yard = rate["fq_to_fqgz"]
    m = med["fq_to_ubam"]
    outside = 0.0 if yard[0] <= m <= yard[-1] else (m / yard[0] - 1 if m < yard[0] else m / yard[-1] - 1)
    same = all(getattr(last["fq_to_ubam"], a) == getattr(last["fq_to_fqgz"], a) for a in ("num_read", "num_rrna", "num_nonrrna"))
    emit({"measurement": "short_ubam_output", "reads": reads, "read_len": 100, "calls": calls, "flow": "single-end x.fq -> .fq.gz | .bam --ubam_output",
          "input_bytes": os.path.getsize(src), "output_bytes": {k: os.path.getsize(v[5]) for k, v in argv.items()},
          "reads_per_s": {k: {"median": round(statistics.median(v)), "lowest": round(v[0]), "highest": round(v[-1])} for k, v in rate.items()},
          "ratio_of_medians": round(m / med["fq_to_fqgz"], 4), "with_flag_median_inside_yardstick_spread": bool(outside == 0.0),
          "outside_the_spread_by": round(outside, 4), "peak_allocated_MB": {k: round(v / 1e6) for k, v in peak.items()},
          "flag_adds_MB": round((peak["fq_to_ubam"] - peak["fq_to_fqgz"]) / 1e6), "same_counts": bool(same),
          "counters": dict(last["fq_to_ubam"]._ubam_total[0]), "which_pass_holds_the_time": "not measured"})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 22)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["kernel", "cli"])
    ap.add_argument("--keep", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubam_bench.jsonl"))
    a = ap.parse_args()
    OUT = a.out
    d = a.keep or tempfile.mkdtemp(prefix="rdubam", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        if a.only != "kernel":
            import multiprocessing as mp
            with mp.get_context("spawn").Pool(1) as pool:          # (before anything initialises the GPU)
                pool.map(_make, [(os.path.join(d, "se_%d.fq" % a.reads), a.reads)])
        import ribodetector_amd  # noqa: F401
        if a.only != "cli":
            bench_kernel()
        if a.only != "kernel":
            bench_cli(d, a.reads, a.calls)
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
