#!/usr/bin/env python
"""CLI reads/s of --interleaved against the same pairs as two files (100 bp paired-end, -e rrna, FASTQ in tmpfs, default chunking);
prints one JSON line. Flows:
    two_files         r_1.fq, r_2.fq -> two plain files         (the baseline: the path --interleaved does not touch)
    il_to_il          il.fq          -> one interleaved plain file
    il_to_split       il.fq          -> two plain files
    ilgz_to_ilgz      il.fq.gz (one gzip stream, zlib level 6) -> one interleaved .gz
Every flow runs in a process of its own: one untimed warm-up call, then `--calls` timed calls of detect() (model load excluded:
Predictor.timing["detect_s"]); the median counts. Each flow's record also holds the last call's `ingest` and main-thread stage times,
which name the stage when a flow falls behind.
    python tools/interleaved_bench.py [--pairs 2000000] [--calls 3] [--keep DIR]
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def interleave_files(p1, p2, out):
    """4-line FASTQ records of p1 and p2 alternately -> out"""
    with open(p1, "rb") as f1, open(p2, "rb") as f2, open(out, "wb") as fo:
        while True:
            a = [f1.readline() for _ in range(4)]
            if not a[0]:
                break
            fo.write(b"".join(a))
            fo.write(b"".join(f2.readline() for _ in range(4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None, help="make the input files in this directory and leave them there")
    ap.add_argument("--leg-timeout", type=int, default=600, help="seconds a flow's process may take")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import ribodetector_amd  # noqa: F401
    from ribodetector_amd import detect, synth
    if a.leg:                                   # one flow: warm-up, then `calls` timed detect() calls
        argv = json.loads(a.leg)
        detect.main(argv, log_level="WARNING")
        runs = [detect.main(argv, log_level="WARNING") for _ in range(a.calls)]
        last = runs[-1]
        print(json.dumps({"seconds": [p.timing["detect_s"] for p in runs], "pairs": last.num_read, "ingest": last.timing["ingest"],
                          "main_thread_s": {k: round(v, 4) for k, v in last._stage_s.items()}, "thread_cpu_s": last.thread_cpu_s}, default=str))
        return
    d = a.keep or tempfile.mkdtemp(prefix="rdil", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        files = []
        for mate in (1, 2):
            arena, off, _ = synth.reads_numpy(a.pairs, 100, seed=mate)
            p = os.path.join(d, "r_%d.fq" % mate)
            synth.write_fastq_realistic(p, arena, off, mate, seed=mate)
            files.append(p)
        il = os.path.join(d, "il.fq")
        interleave_files(files[0], files[1], il)
        with open(il, "rb") as fi, gzip.open(il + ".gz", "wb", compresslevel=6) as fo:
            shutil.copyfileobj(fi, fo, 16 << 20)
        o = lambda name: os.path.join(d, name)      # noqa: E731
        flows = {"two_files": ["-i", *files, "-o", o("o_1.fq"), o("o_2.fq")],
                 "il_to_il": ["-i", il, "--interleaved", "-o", o("o_il.fq")],
                 "il_to_split": ["-i", il, "--interleaved", "-o", o("s_1.fq"), o("s_2.fq")],
                 "ilgz_to_ilgz": ["-i", il + ".gz", "--interleaved", "-o", o("o_il.fq.gz")]}
        res = {}
        for k, io in flows.items():
            argv = ["-l", "100", "-e", "rrna"] + io
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", json.dumps(argv), "--calls", str(a.calls)], capture_output=True, text=True,
                               timeout=a.leg_timeout)
            if r.returncode != 0:
                raise RuntimeError("flow %s failed:\n%s" % (k, r.stderr[-3000:]))
            res[k] = json.loads(r.stdout.strip().splitlines()[-1])
            if res[k]["pairs"] != a.pairs:
                raise RuntimeError("flow %s classified %d pairs of %d" % (k, res[k]["pairs"], a.pairs))
            res[k]["median_s"] = statistics.median(res[k]["seconds"])
            res[k]["reads_per_s"] = round(2 * a.pairs / res[k]["median_s"])
        same = open(o("o_1.fq"), "rb").read() == open(o("s_1.fq"), "rb").read() and open(o("o_2.fq"), "rb").read() == open(o("s_2.fq"), "rb").read()
        base = res["two_files"]["reads_per_s"]
        print(json.dumps({"pairs": a.pairs, "calls": a.calls, "reads_per_s": {k: v["reads_per_s"] for k, v in res.items()},
                          "ratio_to_two_files": {k: round(v["reads_per_s"] / base, 4) for k, v in res.items()},
                          "split_outputs_equal_two_file_outputs": same, "flows": res}))
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
