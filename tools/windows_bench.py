#!/usr/bin/env python
"""CLI rates with and without --windows, in one process: per measurement one untimed warm-up call of each leg, then `--calls` timed
calls of each, ALTERNATING the legs (model load excluded: Predictor.timing["detect_s"]). Prints one JSON line per measurement: per leg
the median rate and the lowest and highest of its calls.
    python tools/windows_bench.py [--reads 4194304] [--calls 3] [--keep DIR] [--only flag|long|kernel]
  flag    what the flag costs when nothing is long: `--reads` pairs of 100 bp, plain FASTQ in tmpfs -> .gz, -e rrna, with and without
          --windows (three table passes per mate and chunk and one host wait per chunk). The with-flag median is to be read against the
          run-to-run spread of the no-flag leg.
  long    what windows cost where they apply: `--reads` single-end reads of 300 bp, plain -> .gz, at -l 100 (truncated), at -l 100
          --windows (W = 3) and at -l 300; reads/s and windows/s (= classify entries per second: the reads of the legs without the flag)
  kernel  rd_window_plan / rd_window_fill / rd_window_fuse ALONE on a chunk of 2^20 reads resident in HBM, timed with device events:
          us per call and the bytes each moves; one chunk of 100 bp reads (W = 1) and one of 300 bp reads (W = 3)
--keep DIR: leave the inputs in DIR (and reuse them when they are there), e.g. for a profiler run of one with-flag call:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o x -- python tools/windows_bench.py --keep DIR --profile_leg
--trace OUT then prints the rd_window_* kernels' times from OUT's kernel trace, and the run's kernel time in all. The plan's offsets
pass is the shared scan's instantiation over the window rule (csrc/rd_scan.hpp); it is listed as rd_window_off_kernel, the name it
had as a kernel of its own in the lines already under profiles/. The plan's base pass (rd_scan_base_kernel) was never listed.
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
    """({kernel: [us per launch]} of the rd_window_* kernels, us of all kernels) in a rocprofv3 --kernel-trace output directory"""
    out, total = {}, 0.0
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                total += us
                if "rd_window_" in r["Kernel_Name"]:
                    out.setdefault("rd_window_" + r["Kernel_Name"].split("rd_window_")[1].split("(")[0], []).append(us)
                elif "rd_scan_off_kernel" in r["Kernel_Name"] and "WnLen" in r["Kernel_Name"]:
                    out.setdefault("rd_window_off_kernel", []).append(us)
    return out, total


def _make(job):
    path, reads, length, mate, seed = job
    from ribodetector_amd import synth
    if not os.path.exists(path):
        arena, off, _ = synth.reads_numpy(reads, length, seed=seed)
        synth.write_fastq_realistic(path, arena, off, mate, seed=seed)
    return path


def make_inputs(d, reads, which):
    """the input files of the measurements, written side by side (processes that never touch the GPU)"""
    import multiprocessing as mp
    jobs = []
    if "flag" in which:
        jobs += [(os.path.join(d, "p100_%d.fq" % m), reads, 100, m, m) for m in (1, 2)]
    if "long" in which:
        jobs += [(os.path.join(d, "s300.fq"), reads, 300, 1, 3)]
    if jobs:
        with mp.get_context("spawn").Pool(len(jobs)) as pool:
            pool.map(_make, jobs)
    return d


def timed_legs(argv, calls, units):
    """{leg: sorted units per second of its timed calls}, the legs alternating; the last Predictor of every leg"""
    from ribodetector_amd import detect
    last = {}
    for k in argv:
        detect.main(argv[k], log_level="WARNING")
    secs = {k: [] for k in argv}
    for _ in range(calls):
        for k in argv:
            last[k] = detect.main(argv[k], log_level="WARNING")
            secs[k].append(last[k].timing["detect_s"])
    return {k: sorted(units / s for s in v) for k, v in secs.items()}, last


def _mlh(v, scale=1.0):
    return {"median": round(statistics.median(v) * scale), "lowest": round(v[0] * scale), "highest": round(v[-1] * scale)}


def bench_flag(d, reads, calls):
    files = [os.path.join(d, "p100_%d.fq" % m) for m in (1, 2)]
    outs = [os.path.join(d, "o_%d.fq.gz" % m) for m in (1, 2)]
    argv = {k: ["-l", "100", "-i", *files, "-o", *outs, "-e", "rrna", *extra] for k, extra in (("no_flag", []), ("windows", ["--windows"]))}
    rate, last = timed_legs(argv, calls, 2 * reads)
    med = {k: statistics.median(v) for k, v in rate.items()}
    print(json.dumps({"measurement": "flag", "pairs": reads, "calls": calls, "flow": "plain -> .gz, 100 bp pairs, -e rrna",
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["windows"] / med["no_flag"], 4),
                      "inside_no_flag_spread": bool(rate["no_flag"][0] <= med["windows"] <= rate["no_flag"][-1]),
                      "windows_classified": last["windows"]._win_total}))


def bench_long(d, reads, calls):
    src, out = os.path.join(d, "s300.fq"), os.path.join(d, "o_s.fq.gz")
    argv = {"l100_truncated": ["-l", "100", "-i", src, "-o", out], "l100_windows": ["-l", "100", "-i", src, "-o", out, "--windows"],
            "l300": ["-l", "300", "-i", src, "-o", out]}
    rate, last = timed_legs(argv, calls, reads)
    w = last["l100_windows"]._win_total[0]
    print(json.dumps({"measurement": "long", "reads": reads, "read_len": 300, "calls": calls, "flow": "plain -> .gz, single-end",
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()},
                      "windows_per_s": {k: _mlh(v, w / reads if k == "l100_windows" else 1.0) for k, v in rate.items()},
                      "windows_classified": w, "rrna": {k: p.num_rrna for k, p in last.items()}}))


def bench_kernel(n, calls):
    import torch
    from ribodetector_amd import _native as N
    lib, dev = N.lib(), torch.device("cuda:0")
    st = N.stream_ptr(dev)
    for ln in (100, 300):
        rec = 2 * ln + 18
        off = torch.arange(n, dtype=torch.int64, device=dev) * rec + 14
        lens = torch.full((n,), ln, dtype=torch.int32, device=dev)
        first = torch.empty(n + 1, dtype=torch.int64, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        ws = torch.empty(int(lib.rd_window_workspace_bytes(n)), dtype=torch.uint8, device=dev)

        def plan():
            N.check(lib.rd_window_plan(N.ptr(lens), n, 100, 100, 32, N.ptr(first), N.ptr(info), N.ptr(ws), ws.numel(), st), "rd_window_plan")
        plan()
        total = int(info.cpu()[1])
        wo, wl = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
        wlog = torch.randn((total, 2), device=dev)
        logits, labels = torch.empty((n, 2), device=dev), torch.empty(n, dtype=torch.uint8, device=dev)

        def fill():
            N.check(lib.rd_window_fill(N.ptr(off), N.ptr(lens), N.ptr(first), n, 100, 100, 32, total, N.ptr(wo), N.ptr(wl), st), "rd_window_fill")

        def fuse():
            N.check(lib.rd_window_fuse(N.ptr(wlog), N.ptr(first), n, 0, 0, N.ptr(logits), N.ptr(labels), st), "rd_window_fuse")
        # bytes each call moves: plan reads the lengths twice and writes win_first; fill reads the read table and win_first and writes the
        # window table; fuse reads win_first and the windows' logits and writes the reads' logits and labels
        moved = {"plan": 2 * 4 * n + 8 * (n + 1), "fill": (8 + 4 + 8) * n + 12 * total, "fuse": 8 * (n + 1) + 8 * total + 9 * n}
        res = {}
        for name, fn in (("plan", plan), ("fill", fill), ("fuse", fuse)):
            for _ in range(3):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
            ev[0].record()
            for k in range(calls):
                fn()
                ev[k + 1].record()
            torch.cuda.synchronize()
            us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))
            med = statistics.median(us)
            res[name] = {"us_per_call": {"median": round(med, 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)}, "bytes": moved[name],
                         "GB_per_s": round(moved[name] / med / 1e3, 1)}
        print(json.dumps({"measurement": "kernel", "reads": n, "read_len": ln, "windows": total, "calls": calls, "kernels": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 22, help="pairs (flag) / reads (long)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--only", default=None, choices=["flag", "long", "kernel"])
    ap.add_argument("--profile_leg", action="store_true", help="ONE call of the with-flag leg of `flag` and nothing else")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        t, total = trace_times(a.trace)
        print(json.dumps({"all_kernels_us": round(total, 1), "kernel_us": {k: {"launches": len(v), "sum": round(sum(v), 1), "largest": round(max(v), 1)}
                                                                           for k, v in sorted(t.items())}}))
        return
    which = [a.only] if a.only else ["flag", "long", "kernel"]
    if a.profile_leg:
        which = ["flag"]
    d = a.keep or tempfile.mkdtemp(prefix="rdwin", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        make_inputs(d, a.reads, which)          # (before anything initialises the GPU)
        import ribodetector_amd  # noqa: F401
        if a.profile_leg:
            from ribodetector_amd import detect
            files = [os.path.join(d, "p100_%d.fq" % m) for m in (1, 2)]
            p = detect.main(["-l", "100", "-i", *files, "-o", os.path.join(d, "o_1.fq.gz"), os.path.join(d, "o_2.fq.gz"), "-e", "rrna", "--windows"], log_level="WARNING")
            print(json.dumps({"profiled": "windows", "pairs": p.num_read, "windows_classified": p._win_total}))
            return
        if "flag" in which:
            bench_flag(d, a.reads, a.calls)
        if "long" in which:
            bench_long(d, a.reads, a.calls)
        if "kernel" in which:
            bench_kernel(1 << 20, 20)
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
