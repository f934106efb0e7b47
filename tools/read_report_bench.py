#!/usr/bin/env python
"""CLI reads/s with and without --read_report on the BASELINE config (100 bp paired-end, -e rrna, plain FASTQ in tmpfs, default
chunking), for a plain and a .gz report; prints one JSON line. Every leg runs in a process of its own: one untimed warm-up call, then
`--calls` timed calls of detect() (model load excluded: Predictor.timing["detect_s"]); the best call counts.
    python tools/read_report_bench.py [--reads 4000000] [--calls 3]
"""
import argparse
import json
import os
import shutil
import sys
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000, help="pairs")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import ribodetector_amd  # noqa: F401
    from ribodetector_amd import detect, synth
    if a.leg:                                   # one leg: warm-up, then the best detect() time of `calls` calls
        argv = json.loads(a.leg)
        detect.main(argv, log_level="WARNING")
        print(min(detect.main(argv, log_level="WARNING").timing["detect_s"] for _ in range(a.calls)))
        return
    d = tempfile.mkdtemp(prefix="rdrep", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        files = []
        for mate in (1, 2):
            arena, off, _ = synth.reads_numpy(a.reads, 100, seed=mate)
            p = os.path.join(d, "r_%d.fq" % mate)
            synth.write_fastq_realistic(p, arena, off, mate, seed=mate)
            files.append(p)
        outs = [os.path.join(d, "o_1.fq"), os.path.join(d, "o_2.fq")]
        legs = {"no_report": [], "report_plain": ["--read_report", os.path.join(d, "rep.tsv")],
                "report_gz": ["--read_report", os.path.join(d, "rep.tsv.gz")]}
        best = {}
        for k, extra in legs.items():
            argv = ["-l", "100", "-i", *files, "-o", *outs, "-e", "rrna", *extra]
            r = subprocess.run([sys.executable, __file__, "--leg", json.dumps(argv), "--calls", str(a.calls)], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("leg %s failed:\n%s" % (k, r.stderr[-3000:]))
            best[k] = float(r.stdout.strip().splitlines()[-1])
        sizes = {k: os.path.getsize(v[1]) for k, v in legs.items() if v}
        rate = {k: 2 * a.reads / v for k, v in best.items()}
        print(json.dumps({"pairs": a.reads, "calls": a.calls, "reads_per_s": {k: round(v) for k, v in rate.items()},
                          "seconds": {k: round(v, 3) for k, v in best.items()},
                          "ratio_plain": round(rate["report_plain"] / rate["no_report"], 4), "ratio_gz": round(rate["report_gz"] / rate["no_report"], 4),
                          "report_bytes": sizes}))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
