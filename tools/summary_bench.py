#!/usr/bin/env python
"""CLI reads/s with and without --summary: 100 bp paired-end, plain FASTQ in tmpfs -> .gz outputs, default chunking (chunks of 2^20
pairs). One process: one untimed warm-up call of each leg, then `--calls` timed calls of each, ALTERNATING the two legs (model load
excluded: Predictor.timing["detect_s"]). Prints one JSON line: per leg the median rate and the lowest and highest of its calls - the
with-flag median is to be read against the run-to-run spread of the no-flag leg.
    python tools/summary_bench.py [--reads 2097152] [--calls 3] [--keep DIR]
--keep DIR: leave the inputs in DIR (and reuse them when they are there), e.g. for a profiler run of the same command:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o x -- python tools/summary_bench.py --keep DIR --profile_leg
--profile_leg: ONE call with --summary and nothing else; --trace OUT then prints the rd_summary_* kernels' times from OUT's kernel trace.
--kernel: rd_summary_accumulate ALONE on a 2^20-pair chunk of 100 bp records resident in HBM (218-byte records, as tools' constant-style
FASTQ), timed with device events: us per call (check + accumulate pass) and the rate over the sequence bytes and over the whole text.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def trace_times(root):
    """{kernel: [us per launch]} of the rd_summary_* kernels in a rocprofv3 --kernel-trace output directory"""
    out = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                if "rd_summary" in r["Kernel_Name"]:
                    name = "rd_summary_" + r["Kernel_Name"].split("rd_summary_")[1].split("(")[0]
                    out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def kernel_alone(pairs, calls):
    import torch
    from ribodetector_amd.summary import DeviceSummary
    dev, rec, ln = torch.device("cuda:0"), 218, 100
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    mates, logits = [], []
    for _ in (0, 1):
        text = acgt[torch.randint(0, 4, (pairs * rec,), device=dev, generator=g)]
        off = torch.arange(pairs, dtype=torch.int64, device=dev) * rec + 14
        mates.append((text, off, torch.full((pairs,), ln, dtype=torch.int32, device=dev)))
        logits.append(torch.randn((pairs, 2), device=dev, generator=g) * 4)
    labels = (logits[0][:, 1] + logits[1][:, 1] > logits[0][:, 0] + logits[1][:, 0]).to(torch.int8)
    ds = DeviceSummary(dev)
    for _ in range(3):
        info = ds.add(mates[0], logits[0], mates[1], logits[1], labels)
    torch.cuda.synchronize()
    assert int(info[0]) == 0 and int(ds.result()[:3].sum()) == 3 * pairs
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for k in range(calls):
        ds.add(mates[0], logits[0], mates[1], logits[1], labels)
        ev[k + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))
    med = statistics.median(us)
    print(json.dumps({"kernel_alone": "rd_summary_accumulate", "pairs": pairs, "read_len": ln, "calls": calls,
                      "us_per_call": {"median": round(med, 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)},
                      "sequence_GB_per_s": round(2 * pairs * ln / med / 1e3, 1), "text_GB_per_s": round(2 * pairs * rec / med / 1e3, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 21, help="pairs")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--profile_leg", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--kernel", action="store_true")
    a = ap.parse_args()
    if a.kernel:
        kernel_alone(1 << 20, 20)
        return
    if a.trace:
        t = trace_times(a.trace)
        print(json.dumps({"kernel_us": {k: {"launches": len(v), "largest": round(max(v), 1), "all": [round(x, 1) for x in v]} for k, v in sorted(t.items())}}))
        return
    import ribodetector_amd  # noqa: F401
    from ribodetector_amd import detect, synth
    d = a.keep or tempfile.mkdtemp(prefix="rdsum", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        files = [os.path.join(d, "r_%d.fq" % mate) for mate in (1, 2)]
        for mate, p in zip((1, 2), files):
            if not os.path.exists(p):
                arena, off, _ = synth.reads_numpy(a.reads, 100, seed=mate)
                synth.write_fastq_realistic(p, arena, off, mate, seed=mate)
        outs = [os.path.join(d, "o_1.fq.gz"), os.path.join(d, "o_2.fq.gz")]
        js = os.path.join(d, "summary.json")
        legs = {"no_summary": [], "summary": ["--summary", js]}
        argv = {k: ["-l", "100", "-i", *files, "-o", *outs, "-e", "rrna", *extra] for k, extra in legs.items()}
        if a.profile_leg:
            detect.main(argv["summary"], log_level="WARNING")
            print(json.dumps({"profiled": "summary", "reads": json.load(open(js))["reads"]}))
            return
        for k in legs:
            detect.main(argv[k], log_level="WARNING")
        secs = {k: [] for k in legs}
        for _ in range(a.calls):
            for k in legs:
                secs[k].append(detect.main(argv[k], log_level="WARNING").timing["detect_s"])
        rate = {k: sorted(2 * a.reads / s for s in v) for k, v in secs.items()}
        med = {k: statistics.median(v) for k, v in rate.items()}
        print(json.dumps({"pairs": a.reads, "calls": a.calls, "flow": "plain -> .gz, 100 bp pairs, -e rrna",
                          "reads_per_s": {k: {"median": round(med[k]), "lowest": round(v[0]), "highest": round(v[-1])} for k, v in rate.items()},
                          "ratio_of_medians": round(med["summary"] / med["no_summary"], 4),
                          "inside_no_flag_spread": bool(rate["no_summary"][0] <= med["summary"] <= rate["no_summary"][-1]),
                          "summary_reads": json.load(open(js))["reads"]}))
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
