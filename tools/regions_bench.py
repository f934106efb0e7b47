#!/usr/bin/env python
"""CLI rates with --windows and with --windows --regions, in one process: per measurement one untimed warm-up call of each leg, then
`--calls` timed calls of each, ALTERNATING the legs (model load excluded: Predictor.timing["detect_s"]). Prints one JSON line per
measurement: per leg the median rate and the lowest and highest of its calls, and whether the with-flag median lies inside the
no-flag leg's spread.
    python tools/regions_bench.py [--reads 4194304] [--contigs 512] [--calls 3] [--keep DIR] [--only reads|contigs|kernel] [--out PATH]
Every line is also appended to --out (default profiles/regions_bench.jsonl).
  reads    the 300 bp workload of tools/windows_bench.py: `--reads` single-end reads of 300 bp, plain FASTQ in tmpfs -> .gz, -l 100
           --windows (W = 3), without and with --regions (a plain file beside the outputs)
  contigs  a FASTA of `--contigs` contigs of 400 kb at --max_windows 4096 (4,000 windows each), without and with --regions
  kernel   rd_region_format ALONE on a chunk of 2^20 reads resident in HBM (W = 3, synthetic window logits, every fifth window rRNA),
           timed with device events: us per call of its six launches together, the bytes they move, and the output's size
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


OUT = os.path.join(ROOT, "profiles", "regions_bench.jsonl")


def emit(doc):
    line = json.dumps(doc)
    print(line)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def _make_contigs(job):
    path, n, length, seed = job
    from ribodetector_amd import synth
    if not os.path.exists(path):
        arena, off, _ = synth.reads_numpy(n, length, seed=seed, rrna_frac=0.3)
        b = arena.tobytes()
        with open(path, "wb") as fh:
            for i in range(n):
                s = b[off[i]:off[i + 1]]
                fh.write(b">contig.%d\n" % i + b"".join(s[k:k + 80] + b"\n" for k in range(0, len(s), 80)))
    return path


def make_inputs(d, reads, contigs, which):
    import multiprocessing as mp

    import windows_bench as WB
    jobs = []
    if "reads" in which:
        jobs.append((WB._make, (os.path.join(d, "s300.fq"), reads, 300, 1, 3)))
    if "contigs" in which:
        jobs.append((_make_contigs, (os.path.join(d, "contigs.fa"), contigs, 400000, 5)))
    if jobs:
        with mp.get_context("spawn").Pool(len(jobs)) as pool:
            for r in [pool.apply_async(fn, (job,)) for fn, job in jobs]:
                r.get()


def bench_cli(name, d, argv, units, calls, what):
    import windows_bench as WB
    legs = {"windows": argv, "windows_regions": argv + ["--regions", os.path.join(d, "regions.bed")]}
    rate, last = WB.timed_legs(legs, calls, units)
    med = {k: statistics.median(v) for k, v in rate.items()}
    p = last["windows_regions"]
    emit({"measurement": name, "units": units, "calls": calls, "flow": what, "units_per_s": {k: WB._mlh(v) for k, v in rate.items()},
                      "ratio_of_medians": round(med["windows_regions"] / med["windows"], 4),
                      "inside_no_flag_spread": bool(rate["windows"][0] <= med["windows_regions"] <= rate["windows"][-1]),
                      "windows_classified": p._win_total, "regions": p._reg_total[0], "reads_with_regions": p._reg_total[1],
                      "regions_file_bytes": os.path.getsize(os.path.join(d, "regions.bed")), "format_repeats": p.regions_repeats})


def bench_kernel(n, calls):
    import torch
    from ribodetector_amd import _native as N
    lib, dev = N.lib(), torch.device("cuda:0")
    st = N.stream_ptr(dev)
    rec, W = 2 * 300 + 40, 3
    hdr = b"@A00123:45:HXXXXXXXX:1:1101:10000:10000 1:N:0:ACGT\n"
    text = torch.full((n * rec,), 65, dtype=torch.uint8, device=dev)
    text.view(n, rec)[:, :len(hdr)] = torch.tensor(list(hdr), dtype=torch.uint8, device=dev)
    rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * rec
    lens = torch.full((n,), 300, dtype=torch.int32, device=dev)
    first = torch.arange(n + 1, dtype=torch.int64, device=dev) * W
    total = n * W
    wlog = torch.randn((total, 2), device=dev)
    wlog[:, 1] = torch.where(torch.arange(total, device=dev) % 5 == 0, wlog[:, 0] + 2.0, wlog[:, 0] - 2.0)
    ws = torch.empty(int(lib.rd_region_workspace_bytes(n, total)), dtype=torch.uint8, device=dev)
    out = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)

    def fmt():
        N.check(lib.rd_region_format(N.ptr(text), text.numel(), N.ptr(rs), N.ptr(lens), N.ptr(first), N.ptr(wlog), None, 0, None, None, None, None,
                                     1, n, 100, N.ptr(out), out.numel(), N.ptr(info), N.ptr(ws), ws.numel(), st), "rd_region_format")
    for _ in range(3):
        fmt()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for k in range(calls):
        fmt()
        ev[k + 1].record()
    torch.cuda.synchronize()
    i = [int(x) for x in info.cpu()]
    assert i[3] == 0, i
    us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))
    med = statistics.median(us)
    # bytes moved: the count pass reads 64 header bytes (in 16-byte steps up to the id's end: 48 here), the tables and the windows' logits
    # and writes the unit tables; the off pass reads and writes those; the line pass reads the logits again and writes 24 bytes a line;
    # the write pass reads the line table and the ids and writes the text
    lines = i[4]
    moved = n * (48 + 16 + 4 + 16 + 20) + 8 * total + n * 32 + 8 * total + n * 36 + 24 * lines + 24 * lines + 39 * lines + i[1]
    emit({"measurement": "kernel", "reads": n, "windows": total, "calls": calls, "regions": lines, "out_bytes": i[1],
                      "us_per_call": {"median": round(med, 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)}, "bytes": moved,
                      "GB_per_s": round(moved / med / 1e3, 1), "us_at_8_TB_per_s": round(moved / 8e6, 1)})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 22)
    ap.add_argument("--contigs", type=int, default=512)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--only", default=None, choices=["reads", "contigs", "kernel"])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    OUT = a.out
    which = [a.only] if a.only else ["reads", "contigs", "kernel"]
    d = a.keep or tempfile.mkdtemp(prefix="rdreg", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        make_inputs(d, a.reads, a.contigs, which)          # (before anything initialises the GPU)
        import ribodetector_amd  # noqa: F401
        if "reads" in which:
            bench_cli("reads", d, ["-l", "100", "-i", os.path.join(d, "s300.fq"), "-o", os.path.join(d, "o_s.fq.gz"), "--windows"], a.reads, a.calls,
                      "plain -> .gz, single-end 300 bp, W = 3")
        if "contigs" in which:
            bench_cli("contigs", d, ["-l", "100", "-i", os.path.join(d, "contigs.fa"), "-o", os.path.join(d, "o_c.fa.gz"), "--windows",
                                     "--max_windows", "4096"], a.contigs, a.calls, "FASTA of 400 kb contigs -> .gz, --max_windows 4096")
        if "kernel" in which:
            bench_kernel(1 << 20, 20)
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
