#!/usr/bin/env python
"""BAM input against the same reads as BGZF FASTQ, in one process: per measurement one untimed warm-up call of each leg, then `--calls`
timed calls of each, ALTERNATING the legs (model load excluded: Predictor.timing["detect_s"]). Prints one JSON line per measurement.
    python tools/bam_bench.py [--reads 4194304] [--long_reads 262144] [--calls 3] [--keep DIR] [--only short|long|kernel] [--trace OUT]
  short   `--reads` single-end reads of 100 bp: x.bam -> .gz against x.fq.gz (BGZF, the same reads, the same bgzip-style members) -> .gz.
          The FASTQ leg is the yardstick - the existing path: the BAM leg's median is to be read against that leg's run-to-run spread.
  long    `--long_reads` reads of 10 kb with --windows, the same two legs
  kernel  rd_bam_index ALONE on a batch of each shape resident in HBM (the inflated bytes, as the feeder hands them over), 20 calls timed
          with device events: us per call, the bytes it moves, the fraction of an HBM-bound pass at 8 TB/s that is, and the segments the
          in-order pass had to walk again. The split over the walk / stitch / table / emit kernels is not visible to events around one
          call of the C ABI: run this measurement under  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/bam_bench.py
          --only kernel  and print the split with --trace OUT.
  --bam_output   the same three measurements for BAM OUTPUT (detect.py --bam_output, csrc/rd_bam_raw.hpp): short / long time x.bam -> .bam
          --bam_output against x.bam -> .fq.gz - the same input file, the existing path is the yardstick; kernel times rd_bam_raw_tab +
          rd_bam_raw_gather (every record of the batch, one piece) behind one rd_bam_index call on the resident batch.
  --shard        the measurements of --bam_shard (data_loader/bam_shard.py, csrc/rd_bam_shard.hpp): kernel times rd_bam_find_start on a 1 MiB
          probe of either shape, and rd_bam_count against rd_bam_index - the yardstick, timed in the same process - on the same resident
          batch; short times fastx_parser.plan_ranges over BamViews for two ranks that share the GPU (threads of this process: host-side
          evidence only), one file and two files, and the one-rank CLI with and without --bam_shard, the legs alternating.
  --bam_tags     the measurements of --bam_tags (bamtags.py, csrc/rd_bam_tagtext.hpp): short = `--reads` reads of 100 bp with NM:i XS:A RG:Z
          (the records of tools/groups_bench.py) -> .gz, the legs no flag (the yardstick: the behaviour without the feature) and --bam_tags RG,
          alternating, with the peak of torch's allocator in each leg; long = `--long_reads` reads of 10 kb with MM:Z of 2 kB and ML:B:C of
          2,000 elements, --bam_tags MM,ML --windows --chunk_size 1; kernel = rd_bam_tag_splice ALONE on a resident chunk of both
          shapes, 20 calls with device events. With float values (--bam_tag_floats, csrc/rd_float_text.hpp): kernel adds rd_float_text
          ALONE on 2^24 resident values (uniform random bit patterns; qs-like values 5.0-40.0) and rd_bam_tag_splice_ex with floats on
          over the 100 bp shape with a qs:f tag (list qs,RG) against the SAME call on records whose qs is a qs:i of 7 digits - existing
          code, the yardstick - the two alternating; short adds `--reads` reads with qs:f -> .gz, --bam_tags qs,RG without (the
          yardstick: the values are skipped) and with --bam_tag_floats.
Every fourth record of the BAM files is stored on the reverse strand (flag 0x10, bases reverse-complemented, qualities reversed), so
that the text the two legs see is the same. The inputs are written by processes that never touch the GPU."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

SHAPES = {"short": 100, "long": 10000}
NAME = 11                      # 'r' + 9 digits + NUL


def trace_times(root):
    """({kernel: [us per launch]} of the rd_bam_* kernels and the begin kernel, us of all kernels) in a rocprofv3 --kernel-trace directory"""
    out, total = {}, 0.0
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                total += us
                for key in ("rd_bam_", "rd_fq_begin_", "rd_gz_", "rd_select_"):
                    if key in r["Kernel_Name"]:
                        out.setdefault(key + r["Kernel_Name"].split(key)[1].split("(")[0].split("<")[0], []).append(us)
    return out, total


def _rows(n, first, length, seed):
    """(FASTQ text, BAM records) of n reads of `length` (even) bases as two uint8 matrices, one row per read"""
    import numpy as np
    from ribodetector_amd import bam, synth
    arena, _, _ = synth.reads_numpy(n, length, seed=seed)
    seq = arena.reshape(n, length)
    rng = np.random.default_rng(seed)
    phred = np.array([37, 25, 11, 2], np.uint8)[rng.choice(4, size=(n, length), p=[0.90, 0.06, 0.03, 0.01])]      # NovaSeq-like bins
    idx = first + np.arange(n, dtype=np.int64)
    name = np.empty((n, NAME), np.uint8)
    name[:, 0] = ord("r")
    for k in range(9):
        name[:, 9 - k] = 48 + (idx // 10 ** k) % 10
    name[:, 10] = 0
    fq = np.empty((n, 2 * length + NAME + 5), np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1:NAME] = name[:, :10]
    fq[:, NAME] = 10
    fq[:, NAME + 1:NAME + 1 + length] = seq
    fq[:, NAME + 1 + length:NAME + 4 + length] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, NAME + 4 + length:NAME + 4 + 2 * length] = phred + 33
    fq[:, -1] = 10
    code = np.zeros(256, np.uint8)
    for c, ch in enumerate(bam.CODES):
        code[ch] = c
    comp = np.zeros(16, np.uint8)
    for c in range(16):
        comp[c] = bam.CODES.index(bam.COMPLEMENT[c])
    codes, qual = code[seq], phred.copy()
    rev = (idx % 4) == 3
    codes[rev] = comp[codes[rev]][:, ::-1]
    qual[rev] = qual[rev][:, ::-1]
    block = 32 + NAME + length // 2 + length
    rec = np.empty((n, 4 + block), np.uint8)
    fixed = struct.pack("<iiiBBHHHIiii", block, -1, -1, NAME, 0, 4680, 0, 4, length, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    rec[rev, 18] = 4 | 0x10
    rec[:, 36:36 + NAME] = name
    rec[:, 36 + NAME:36 + NAME + length // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, 36 + NAME + length // 2:] = qual
    return fq, rec


def _make(job):
    d, shape, reads, bam_only = job
    from ribodetector_amd import bam, synth
    length = SHAPES[shape]
    fq_gz, bam_path = os.path.join(d, "%s_%d.fq.gz" % (shape, reads)), os.path.join(d, "%s_%d.bam" % (shape, reads))
    if (bam_only or os.path.exists(fq_gz)) and os.path.exists(bam_path):
        return
    step = max(1, (64 << 20) // (2 * length))
    with open(fq_gz + ".raw", "wb") as f1, open(bam_path + ".raw", "wb") as f2:
        f2.write(bam.encode_header(text=b"@HD\tVN:1.6\tSO:unsorted\n"))
        for first in range(0, reads, step):
            fq, rec = _rows(min(step, reads - first), first, length, seed=1000 + first // step)
            f1.write(fq.tobytes())
            f2.write(rec.tobytes())
    for raw, dst in ((fq_gz + ".raw", fq_gz), (bam_path + ".raw", bam_path)):
        if not (bam_only and dst == fq_gz):      # (the BAM output measurements read the BAM file only)
            synth.bgzip_file(raw, dst, level=6, threads=8)
        os.remove(raw)


def make_inputs(d, jobs):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(len(jobs)) as pool:
        pool.map(_make, [(d,) + j for j in jobs])


def timed_legs(argv, calls, units):
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


def _mlh(v):
    return {"median": round(statistics.median(v)), "lowest": round(v[0]), "highest": round(v[-1])}


def bench_cli(d, shape, reads, calls):
    extra = ["--windows", "--chunk_size", "1"] if shape == "long" else []       # (chunks of 32,768 reads: 0.65 GB of text at 10 kb)
    src = {"bam": os.path.join(d, "%s_%d.bam" % (shape, reads)), "fastq_bgzf": os.path.join(d, "%s_%d.fq.gz" % (shape, reads))}
    argv = {k: ["-l", "100", "-i", src[k], "-o", os.path.join(d, "o_%s.fq.gz" % k)] + extra for k in src}
    rate, last = timed_legs(argv, calls, reads)
    med = {k: statistics.median(v) for k, v in rate.items()}
    ix = last["bam"].ingest[os.path.basename(src["bam"])]["indexer"]
    same = all(getattr(last["bam"], a) == getattr(last["fastq_bgzf"], a) for a in ("num_read", "num_rrna", "num_nonrrna"))
    print(json.dumps({"measurement": shape, "reads": reads, "read_len": SHAPES[shape], "calls": calls,
                      "flow": "single-end -> .gz" + (", --windows --chunk_size 1" if extra else ""), "input_bytes": {k: os.path.getsize(v) for k, v in src.items()},
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["bam"] / med["fastq_bgzf"], 4),
                      "bam_median_inside_fastq_spread": bool(rate["fastq_bgzf"][0] <= med["bam"] <= rate["fastq_bgzf"][-1]),
                      "same_counts": bool(same), "rrna": last["bam"].num_rrna, "bam_records": ix["bam_records"], "bam_skipped": ix["bam_skipped"],
                      "segments_walked_again": ix["bam_rewalked_segments"], "batches": ix["batches"]}), flush=True)


def bench_cli_bam_output(d, shape, reads, calls):
    """x.bam -> .fq.gz (the yardstick) against x.bam -> .bam --bam_output: one input file, the legs alternating"""
    extra = ["--windows", "--chunk_size", "1"] if shape == "long" else []
    src = os.path.join(d, "%s_%d.bam" % (shape, reads))
    argv = {"bam_to_fqgz": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_yard.fq.gz")] + extra,
            "bam_to_bam": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_out.bam"), "--bam_output"] + extra}
    rate, last = timed_legs(argv, calls, reads)
    med = {k: statistics.median(v) for k, v in rate.items()}
    yard = rate["bam_to_fqgz"]
    same = all(getattr(last["bam_to_bam"], a) == getattr(last["bam_to_fqgz"], a) for a in ("num_read", "num_rrna", "num_nonrrna"))
    outside = 0.0 if yard[0] <= med["bam_to_bam"] <= yard[-1] else (med["bam_to_bam"] / yard[0] - 1 if med["bam_to_bam"] < yard[0] else med["bam_to_bam"] / yard[-1] - 1)
    print(json.dumps({"measurement": shape + "_bam_output", "reads": reads, "read_len": SHAPES[shape], "calls": calls,
                      "flow": "single-end x.bam -> .fq.gz | .bam --bam_output" + (", --windows --chunk_size 1" if extra else ""), "input_bytes": os.path.getsize(src),
                      "output_bytes": {"bam_to_fqgz": os.path.getsize(argv["bam_to_fqgz"][5]), "bam_to_bam": os.path.getsize(argv["bam_to_bam"][5])},
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["bam_to_bam"] / med["bam_to_fqgz"], 4),
                      "bam_output_median_inside_fastq_output_spread": bool(outside == 0.0), "outside_the_spread_by": round(outside, 4),
                      "same_counts": bool(same), "non_rrna": last["bam_to_bam"].num_nonrrna}), flush=True)


def bench_kernel(calls, batch_bytes=128 << 20, raw_view=False):
    import numpy as np
    import torch
    from ribodetector_amd import _native as N
    lib, dev = N.lib(), torch.device("cuda:0")
    st = N.stream_ptr(dev)
    for shape, length in SHAPES.items():
        size = 36 + NAME + length // 2 + length
        n = batch_bytes // size
        step = max(1, (64 << 20) // (2 * length))
        raw = b"".join(_rows(min(step, n - f), f, length, seed=7 + f // step)[1].tobytes() for f in range(0, n, step))
        pad, end = 64, 64 + len(raw)
        text = torch.zeros(((end + 64 + 127) // 64) * 64, dtype=torch.uint8, device=dev)
        text[pad:end] = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
        window = end - pad
        cap_rec, norm_cap = window // 37 + 2, ((4 * window // 3 + 64 + 255) // 256) * 256
        norm = torch.empty(norm_cap, dtype=torch.uint8, device=dev)
        rec_tab, hdr_tab = torch.empty(cap_rec, dtype=torch.int64, device=dev), torch.empty(cap_rec, dtype=torch.int32, device=dev)
        summary = torch.zeros(8, dtype=torch.int64, device=dev)
        ws = torch.empty(int(lib.rd_bam_index_workspace_bytes(end)), dtype=torch.uint8, device=dev)

        def index():
            N.check(lib.rd_bam_index(N.ptr(text), pad, end, None, None, 1, N.ptr(norm), norm_cap, N.ptr(rec_tab), N.ptr(hdr_tab), cap_rec, N.ptr(summary),
                                     N.ptr(ws), ws.numel(), st), "rd_bam_index")
        if raw_view:                             # the raw view behind ONE framing of the batch: the table, then every record gathered as one piece
            index()
            src = N.C.c_void_p(lib.rd_bam_index_src(N.ptr(ws), end))
            raw_tab = torch.empty(cap_rec, dtype=torch.int64, device=dev)
            ns = cap_rec // 4096 + 3
            samples = torch.empty(ns, dtype=torch.int32, device=dev)
            out = torch.empty(((window + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
            raw_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
            cursor = torch.zeros(2, dtype=torch.int64, device=dev)

            def index():      # noqa: F811
                N.check(lib.rd_bam_raw_tab(N.ptr(text), src, N.ptr(summary), N.ptr(raw_tab), cap_rec, 4096, N.ptr(samples), ns, st), "rd_bam_raw_tab")
                N.check(lib.rd_bam_raw_gather(N.ptr(text), src, N.ptr(raw_tab), N.ptr(summary), 0, n, window, N.ptr(out), out.numel(), N.ptr(cursor),
                                              N.C.c_void_p(cursor.data_ptr() + 8), N.ptr(raw_start), st), "rd_bam_raw_gather")
        for _ in range(3):
            index()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
        ev[0].record()
        for k in range(calls):
            index()
            ev[k + 1].record()
        torch.cuda.synchronize()
        s = summary.cpu().numpy()
        status, rewalked, norm_bytes = int(s[6]) & 0xffffffff, (int(s[6]) >> 32) & 0xffffffff, int(s[7])
        assert status == 0 and int(s[3]) == n and norm_bytes == n * (2 * length + NAME + 5), (status, int(s[3]), n, norm_bytes)
        us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))
        med = statistics.median(us)
        if raw_view:
            assert int(cursor.cpu()[1]) == window and bytes(out[:window].cpu().numpy()) == raw and int(samples.cpu()[-1]) == window
            # every byte of the window is read once and written once; per record: 4 bytes of src_tab and a 32-byte sector for block_size
            # read, 8 bytes of raw_tab written, read and written again (the add pass), read by the gather, and 8 of raw_start written
            moved = 2 * window + (4 + 32 + 4 * 8 + 8) * n
            print(json.dumps({"measurement": "kernel_raw", "what": "rd_bam_raw_tab + rd_bam_raw_gather", "shape": shape, "read_len": length, "records": n,
                              "raw_bytes": window, "calls": calls, "us_per_call": {"median": round(med, 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)},
                              "bytes_moved": moved, "TB_per_s": round(moved / med / 1e6, 3),
                              "fraction_of_hbm_bound_pass_at_8TBps": round(moved / 8e12 / (med * 1e-6), 4)}), flush=True)
            continue
        # the window is read by the walk (staged once) and again by the emit pass (names, bases, qualities: all but the fixed fields and
        # tags); `norm` is written once; per record 16 bytes of tables and 8 of the segment lists are written and read
        moved = 2 * window + norm_bytes + 2 * 24 * n
        print(json.dumps({"measurement": "kernel", "shape": shape, "read_len": length, "records": n, "window_bytes": window, "norm_bytes": norm_bytes,
                          "segments": window // N.BAM_SEGMENT + 1, "segments_walked_again": rewalked, "calls": calls,
                          "us_per_call": {"median": round(med, 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)}, "bytes_moved": moved,
                          "GB_per_s": round(moved / med / 1e3, 1), "fraction_of_hbm_bound_pass_at_8TBps": round(moved / 8e12 / (med * 1e-6), 4),
                          "records_per_s": round(n / (med * 1e-6)), "kernel_split": "not measured here (see --trace)"}), flush=True)


def _events(fn, calls, warm=3):
    """sorted us per call of fn(), by device events"""
    import torch
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for k in range(calls):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))


def _us(v):
    return {"median": round(statistics.median(v), 1), "lowest": round(v[0], 1), "highest": round(v[-1], 1)}


def bench_shard_kernels(calls, batch_bytes=128 << 20, probe=1 << 20):
    """--shard: rd_bam_find_start on a 1 MiB probe, and rd_bam_count against rd_bam_index (the yardstick, in this process) on the same
    resident batch, for both shapes"""
    import numpy as np
    import torch
    from ribodetector_amd import _native as N
    from ribodetector_amd import bam
    lib, dev = N.lib(), torch.device("cuda:0")
    st = N.stream_ptr(dev)
    for shape, length in SHAPES.items():
        size = 36 + NAME + length // 2 + length
        n = batch_bytes // size
        step = max(1, (64 << 20) // (2 * length))
        raw = b"".join(_rows(min(step, n - f), f, length, seed=7 + f // step)[1].tobytes() for f in range(0, n, step))
        pad, end = 64, 64 + len(raw)
        text = torch.zeros(((end + 64 + 127) // 64) * 64, dtype=torch.uint8, device=dev)
        text[pad:end] = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
        # the probe: [0, 1 MiB) of the batch's bytes, asked from offset 1 (inside the first record), the window goes on behind it
        win = text[pad:pad + probe + 64].clone()
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        us = _events(lambda: N.check(lib.rd_bam_find_start(N.ptr(win), 1, probe, probe, 0, N.ptr(info), st), "rd_bam_find_start"), calls)
        got = [int(x) for x in info.cpu()]
        want = bam.find_record_start(raw[:probe], 1, probe, False)
        assert (got[0], got[1]) == want and got[0] == size, (got, want, size)
        print(json.dumps({"measurement": "shard_find_start", "shape": shape, "read_len": length, "probe_bytes": probe, "calls": calls, "found": got[0],
                          "undecided": got[1], "us_per_call": _us(us), "GB_per_s": round(probe / statistics.median(us) / 1e3, 1)}), flush=True)
        window = end - pad
        cap_rec, norm_cap = window // 37 + 2, ((4 * window // 3 + 64 + 255) // 256) * 256
        norm = torch.empty(norm_cap, dtype=torch.uint8, device=dev)
        rec_tab, hdr_tab = torch.empty(cap_rec, dtype=torch.int64, device=dev), torch.empty(cap_rec, dtype=torch.int32, device=dev)
        s_i, s_c = torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        ws_i = torch.empty(int(lib.rd_bam_index_workspace_bytes(end)), dtype=torch.uint8, device=dev)
        ws_c = torch.empty(max(int(lib.rd_bam_count_workspace_bytes(end)), 256), dtype=torch.uint8, device=dev)

        def index():
            N.check(lib.rd_bam_index(N.ptr(text), pad, end, None, None, 1, N.ptr(norm), norm_cap, N.ptr(rec_tab), N.ptr(hdr_tab), cap_rec, N.ptr(s_i),
                                     N.ptr(ws_i), ws_i.numel(), st), "rd_bam_index")

        def count():
            N.check(lib.rd_bam_count(N.ptr(text), pad, end, None, None, 1, N.ptr(s_c), N.ptr(ws_c), ws_c.numel(), st), "rd_bam_count")
        ui, uc = _events(index, calls), _events(count, calls)
        ui2 = _events(index, calls)                                  # (the yardstick once more behind the count: its own run-to-run spread)
        a, b = s_i.cpu().numpy(), s_c.cpu().numpy()
        assert (a == b).all() and int(b[3]) == n and int(b[6]) == 0, (a, b)
        print(json.dumps({"measurement": "shard_count", "shape": shape, "read_len": length, "records": n, "window_bytes": window, "calls": calls,
                          "rd_bam_index_us": _us(ui), "rd_bam_index_again_us": _us(ui2), "rd_bam_count_us": _us(uc),
                          "count_over_index": round(statistics.median(uc) / statistics.median(ui), 4),
                          "workspace_bytes": {"index": ws_i.numel(), "count": ws_c.numel()}, "summaries_equal": True}), flush=True)


def bench_shard_plan(d, reads, world=2):
    """--shard: the seconds fastx_parser.plan_ranges takes with BamView on the device for `world` ranks that share the one GPU - here
    threads of this process with an in-process all_gather, so HOST-SIDE EVIDENCE ONLY: no launcher, no process group, one GPU.
    One file, and the two-file case (the same file as both mates: every cut is verified by count_records)"""
    import threading
    import time
    import torch
    from ribodetector_amd.data_loader import bam_shard
    from ribodetector_amd.data_loader import fastx_parser as fx
    src = os.path.join(d, "short_%d.bam" % reads)
    t0 = time.perf_counter()
    index = fx.BgzfView.build_index(src)
    t_index = time.perf_counter() - t0
    for paths in ([src], [src, src]):
        res, slots, bar, secs = [None] * world, [None] * world, threading.Barrier(world), [0.0] * world

        def work(r):
            torch.cuda.set_device(0)

            def ag(obj):
                slots[r] = obj
                bar.wait()
                out = list(slots)
                bar.wait()
                return out
            views = [bam_shard.BamView(p, index=index, device=torch.device("cuda:0")) for p in paths]
            t = time.perf_counter()
            res[r] = [tuple(x) for x in fx.plan_ranges(paths, r, world, ag, views=views)]
            secs[r] = time.perf_counter() - t
            res[r].append([v.stats for v in views])
        th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        print(json.dumps({"measurement": "shard_plan_ranges", "evidence": "host-side only: %d threads of one process share one GPU" % world, "files": len(paths),
                          "reads": reads, "world": world, "member_index_s": round(t_index, 3), "plan_ranges_s_per_rank": [round(s, 3) for s in secs],
                          "ranges": [r[:-1] for r in res], "view_stats_rank0": res[0][-1]}), flush=True)


def bench_shard_cli(d, reads, calls):
    """--shard: the one-rank CLI with and without --bam_shard on the same file, the legs alternating: nothing is added on one rank"""
    src = os.path.join(d, "short_%d.bam" % reads)
    argv = {"without": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_without.fq.gz")],
            "with_bam_shard": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_with.fq.gz"), "--bam_shard"]}
    rate, last = timed_legs(argv, calls, reads)
    med = {k: statistics.median(v) for k, v in rate.items()}
    same = open(argv["without"][5], "rb").read() == open(argv["with_bam_shard"][5], "rb").read()
    print(json.dumps({"measurement": "shard_one_rank_cli", "reads": reads, "read_len": 100, "calls": calls, "flow": "single-end x.bam -> .fq.gz, one rank",
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["with_bam_shard"] / med["without"], 4),
                      "with_flag_median_inside_no_flag_spread": bool(rate["without"][0] <= med["with_bam_shard"] <= rate["without"][-1]),
                      "outputs_byte_identical": bool(same)}), flush=True)


def _make_tagged(job):
    """the BAM files of the --bam_tags measurements: groups_bench's records (short: its 100 bp file; long: 10 kb with MM:Z and ML:B:C)"""
    d, shape, reads = job
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import groups_bench
    from ribodetector_amd import bam, synth
    if shape == "short":
        groups_bench._make((d, reads))
        return
    path = os.path.join(d, "mm_%d.bam" % reads)
    if os.path.exists(path):
        return
    step = 4096
    with open(path + ".raw", "wb") as fh:
        fh.write(bam.encode_header(text=b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:grp000\n"))
        for first in range(0, reads, step):
            rec = groups_bench.records(min(step, reads - first), SHAPES["long"], 1, True, seed=3 + first // step)[0]
            rec[:, 36 + NAME:36 + NAME + SHAPES["long"] // 2] &= 0x77          # (bases among = A C M G R S V: no code the text cannot hold)
            rec[:, 36 + NAME:36 + NAME + SHAPES["long"] // 2] |= 0x11
            fh.write(rec.tobytes())
    synth.bgzip_file(path + ".raw", path, level=1, threads=8)
    os.remove(path + ".raw")


def bench_cli_bam_tags(d, shape, reads, calls):
    """x.bam -> .fq.gz without the flag (the yardstick) against the same with --bam_tags: one input file, the legs alternating"""
    import torch
    from ribodetector_amd import detect
    extra = ["--windows", "--chunk_size", "1"] if shape == "long" else []
    src = os.path.join(d, ("rg_%d.bam" if shape == "short" else "mm_%d.bam") % reads)
    tags = "RG" if shape == "short" else "MM,ML"
    argv = {"no_flag": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_plain.fq.gz")] + extra,
            "bam_tags": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_tags.fq.gz"), "--bam_tags", tags] + extra}
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
    yard = rate["no_flag"]
    outside = 0.0 if yard[0] <= med["bam_tags"] <= yard[-1] else (med["bam_tags"] / yard[0] - 1 if med["bam_tags"] < yard[0] else med["bam_tags"] / yard[-1] - 1)
    same = all(getattr(last["bam_tags"], a) == getattr(last["no_flag"], a) for a in ("num_read", "num_rrna", "num_nonrrna"))
    print(json.dumps({"measurement": shape + "_bam_tags", "reads": reads, "read_len": SHAPES[shape], "calls": calls, "tags": tags,
                      "flow": "single-end x.bam -> .fq.gz, without | with --bam_tags " + tags + (", --windows --chunk_size 1" if extra else ""),
                      "input_bytes": os.path.getsize(src), "output_bytes": {k: os.path.getsize(v[5]) for k, v in argv.items()},
                      "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["bam_tags"] / med["no_flag"], 4),
                      "with_flag_median_inside_no_flag_spread": bool(outside == 0.0), "outside_the_spread_by": round(outside, 4),
                      "peak_allocated_MB": {k: round(v / 1e6) for k, v in peak.items()}, "flag_adds_MB": round((peak["bam_tags"] - peak["no_flag"]) / 1e6),
                      "same_counts": bool(same), "copied": last["bam_tags"]._tag_total[0]["copied"], "splice_repeats": sum(t.repeats for t in last["bam_tags"]._tags)}),
          flush=True)


def _make_qs(job):
    """the BAM file of the float measurement: groups_bench's 100 bp records with qs:f (5.0-40.0) in front of RG:Z"""
    d, reads = job
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from ribodetector_amd import bam, synth
    path = os.path.join(d, "qs_%d.bam" % reads)
    if os.path.exists(path):
        return
    ids = [b"grp%03d" % g for g in range(24)]
    step = 1 << 18
    with open(path + ".raw", "wb") as fh:
        fh.write(bam.encode_header(text=b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@RG\tID:" + i + b"\n" for i in ids)))
        for first in range(0, reads, step):
            n = min(step, reads - first)
            _, rec = _rows(n, first, 100, seed=1000 + first // step)
            w = rec.shape[1]
            full = np.zeros((n, w + 7 + 10), np.uint8)
            full[:, :w] = rec
            full[:, :4] = np.frombuffer(struct.pack("<i", full.shape[1] - 4), np.uint8)
            full[:, w:w + 3] = np.frombuffer(b"qsf", np.uint8)
            full[:, w + 3:w + 7] = np.random.default_rng(first).uniform(5.0, 40.0, n).astype(np.float32).view(np.uint8).reshape(n, 4)
            full[:, w + 7:w + 10] = np.frombuffer(b"RGZ", np.uint8)
            full[:, w + 10:-1] = np.frombuffer(b"".join(ids), np.uint8).reshape(len(ids), 6)[((first + np.arange(n)) // 1000) % len(ids)]
            fh.write(full.tobytes())
    synth.bgzip_file(path + ".raw", path, level=6, threads=8)
    os.remove(path + ".raw")


def bench_cli_bam_tag_floats(d, reads, calls):
    """qs_N.bam -> .fq.gz with --bam_tags qs,RG: without --bam_tag_floats (the yardstick: qs is skipped and counted) against with it"""
    src = os.path.join(d, "qs_%d.bam" % reads)
    argv = {k: ["-l", "100", "-i", src, "-o", os.path.join(d, "o_%s.fq.gz" % k), "--bam_tags", "qs,RG"] + fl
            for k, fl in (("skipped", []), ("floats", ["--bam_tag_floats"]))}
    rate, last = timed_legs(argv, calls, reads)
    med = {k: statistics.median(v) for k, v in rate.items()}
    yard = rate["skipped"]
    total = {k: last[k]._tag_total[0] for k in argv}
    assert total["floats"]["copied"] == [reads, reads] and total["floats"]["float_values_skipped"] == 0 and total["skipped"]["float_values_skipped"] == reads
    out_bytes = {k: os.path.getsize(v[5]) for k, v in argv.items()}
    print(json.dumps({"measurement": "short_bam_tag_floats", "reads": reads, "read_len": 100, "calls": calls, "tags": "qs,RG",
                      "flow": "single-end x.bam (qs:f, RG:Z) -> .fq.gz, --bam_tags qs,RG without | with --bam_tag_floats", "input_bytes": os.path.getsize(src),
                      "output_bytes": out_bytes, "reads_per_s": {k: _mlh(v) for k, v in rate.items()}, "ratio_of_medians": round(med["floats"] / med["skipped"], 4),
                      "with_flag_median_inside_no_flag_spread": bool(yard[0] <= med["floats"] <= yard[-1]),
                      "text_bytes_added_per_record": round(sum(len(b"\tqs:f:%g" % x) for x in (5.0 + 35.0 * k / 997 for k in range(997))) / 997, 1),
                      "gz_bytes_added_per_record": round((out_bytes["floats"] - out_bytes["skipped"]) / reads, 2)}), flush=True)


def bench_kernel_float_text(calls):
    """rd_float_text alone on 2^24 resident values: uniform random bit patterns, and qs-like values 5.0-40.0"""
    import numpy as np
    import torch
    from ribodetector_amd import bam, bamtags
    dev = torch.device("cuda:0")
    n = 1 << 24
    rng = np.random.default_rng(1)
    for what, host in (("uniform random bit patterns", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)),
                       ("qs-like values 5.0-40.0", rng.uniform(5.0, 40.0, n).astype(np.float32).view(np.uint32))):
        bits = torch.from_numpy(host.view(np.int32)).to(dev)
        us = _events(lambda: bamtags.float_text(bits), calls)
        text, length = bamtags.float_text(bits)
        text, length = text[:4096].cpu().numpy(), length[:4096].cpu().numpy()
        assert all(text[k, :length[k]].tobytes() == bam.float_g(int(host[k])) for k in range(4096))
        med = statistics.median(us)
        print(json.dumps({"measurement": "kernel_float_text", "what": "rd_float_text", "values": n, "distribution": what, "calls": calls, "us_per_call": _us(us),
                          "values_per_s": round(n / (med * 1e-6)), "bytes_moved": 21 * n, "TB_per_s": round(21 * n / med / 1e6, 3),
                          "fraction_of_hbm_bound_pass_at_8TBps": round(21 * n / 8e12 / (med * 1e-6), 4)}), flush=True)
        del bits
    torch.cuda.empty_cache()


def bench_kernel_bam_tags_floats(calls):
    """rd_bam_tag_splice_ex with floats on over 2^20 records of 100 bp with qs:f (list qs,RG) against rd_bam_tag_splice over the same
    records with qs:i of 7 digits (existing code, the yardstick): the legs alternate, one event pair per call"""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import groups_bench
    from ribodetector_amd import bam, bamtags
    dev = torch.device("cuda:0")
    n, length, tags = 1 << 20, 100, [b"qs", b"RG"]
    base, size, t_bytes, _ = groups_bench.records(n, length, 1, False)
    rng = np.random.default_rng(2)
    frec = 2 * length + NAME + 5
    fq = np.full((n, frec), ord("A"), np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1:NAME] = ord("r")
    fq[:, NAME] = fq[:, NAME + 1 + length] = fq[:, NAME + 3 + length] = fq[:, -1] = 10
    fq[:, NAME + 2 + length] = ord("+")
    text = torch.from_numpy(fq.reshape(-1)).to(dev)
    rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * frec
    st = torch.arange(n + 1, dtype=torch.int64, device=dev) * (size + 7)
    legs = {}
    for leg, letter, values in (("qs_f", b"f", rng.uniform(5.0, 40.0, n).astype(np.float32).view(np.uint8)),
                                ("qs_i", b"i", rng.integers(10 ** 6, 10 ** 7, n).astype(np.int32).view(np.uint8))):
        rec = np.zeros((n, size + 7), np.uint8)
        rec[:, :size] = base
        rec[:, :4] = np.frombuffer(struct.pack("<i", size + 3), np.uint8)
        rec[:, size:size + 3] = np.frombuffer(b"qs" + letter, np.uint8)
        rec[:, size + 3:] = values.reshape(n, 4)
        raw = torch.from_numpy(rec.reshape(-1)).to(dev)
        cap = bamtags.default_hint(text.numel(), raw.numel())
        out = torch.empty(((cap + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
        legs[leg] = (rec, raw, cap, out, leg == "qs_f")
    call = {leg: (lambda v=v: bamtags.splice(text, rs, v[1], st, n, tags, v[2], out=v[3], floats=v[4])) for leg, v in legs.items()}
    for _ in range(3):
        for leg in call:
            call[leg]()
    ev = {leg: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for leg in call}
    for k in range(calls):
        for leg in call:
            ev[leg][k][0].record()
            call[leg]()
            ev[leg][k][1].record()
    torch.cuda.synchronize()
    us = {leg: sorted(a.elapsed_time(b) * 1e3 for a, b in ev[leg]) for leg in call}
    tagged = {}
    for leg, (rec, raw, cap, out, floats) in legs.items():
        _, out_start, info = call[leg]()
        info = info.cpu().tolist()
        k = n // 2
        a, b = int(out_start[k]), int(out_start[k + 1])
        data = bam.encode_header() + rec[k].tobytes()
        want = fq[k].tobytes()[:NAME] + bam.tag_comment(data, bam.header_len(data), tags, floats=floats)[0] + fq[k].tobytes()[NAME:]
        assert info[3] == 0 and info[5] == 0 and info[8:10] == [n, n] and bytes(out[a:b].cpu().numpy()) == want, info
        tagged[leg] = info[1]
    med = {leg: statistics.median(v) for leg, v in us.items()}
    print(json.dumps({"measurement": "kernel_bam_tags_floats", "what": "rd_bam_tag_splice_ex (RD_BAM_TAGS_FLOATS) on qs:f | rd_bam_tag_splice on qs:i, alternating",
                      "read_len": length, "records": n, "tags": ["qs", "RG"], "tagged_bytes": tagged, "calls": calls, "us_per_call": {k: _us(v) for k, v in us.items()},
                      "ratio_of_medians_f_over_i": round(med["qs_f"] / med["qs_i"], 4),
                      "float_median_inside_int_spread": bool(us["qs_i"][0] <= med["qs_f"] <= us["qs_i"][-1])}), flush=True)


def bench_kernel_bam_tags(calls):
    """rd_bam_tag_splice alone on a resident chunk of both shapes: 2^20 records of 100 bp (RG) and 8,192 of 10 kb (MM, ML)"""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import groups_bench
    from ribodetector_amd import bam, bamtags
    dev = torch.device("cuda:0")
    for shape, n, length, long_tags, tags in (("short", 1 << 20, 100, False, [b"RG"]), ("long", 8192, 10000, True, [b"MM", b"ML"])):
        rec, size, t_bytes, _ = groups_bench.records(n, length, 1, long_tags)
        frec = 2 * length + NAME + 5
        fq = np.full((n, frec), ord("A"), np.uint8)
        fq[:, 0] = ord("@")
        fq[:, 1:NAME] = ord("r")
        fq[:, NAME] = fq[:, NAME + 1 + length] = fq[:, NAME + 3 + length] = fq[:, -1] = 10
        fq[:, NAME + 2 + length] = ord("+")
        raw = torch.from_numpy(rec.reshape(-1)).to(dev)
        text = torch.from_numpy(fq.reshape(-1)).to(dev)
        rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * frec
        st = torch.arange(n + 1, dtype=torch.int64, device=dev) * size
        cap = bamtags.default_hint(text.numel(), raw.numel())
        out = torch.empty(((cap + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
        us = _events(lambda: bamtags.splice(text, rs, raw, st, n, tags, cap, out=out), calls)
        _, out_start, info = bamtags.splice(text, rs, raw, st, n, tags, cap, out=out)
        info = info.cpu().tolist()
        k = n // 2
        a, b = int(out_start[k]), int(out_start[k + 1])
        data = bam.encode_header() + rec[k].tobytes()
        want = fq[k].tobytes()[:NAME] + bam.tag_comment(data, bam.header_len(data), tags)[0] + fq[k].tobytes()[NAME:]
        assert info[3] == 0 and info[8:8 + len(tags)] == [n] * len(tags) and bytes(out[a:b].cpu().numpy()) == want, info
        med = statistics.median(us)
        # the text is read and the tagged text written once; the raw view's fixed part and tags are read by every walk, the values again by the
        # count and the write pass; per record and tag 21 bytes of tables are written and read twice, per record 25 bytes of tables
        value_bytes = info[1] - text.numel()
        moved = text.numel() + info[1] + n * (36 + t_bytes) * len(tags) + 2 * value_bytes + n * (len(tags) * 21 * 3 + 25 * 3)
        print(json.dumps({"measurement": "kernel_bam_tags", "what": "rd_bam_tag_splice", "shape": shape, "read_len": length, "records": n, "tags": [t.decode() for t in tags],
                          "text_bytes": text.numel(), "raw_bytes": raw.numel(), "tagged_bytes": info[1], "calls": calls, "us_per_call": _us(us),
                          "bytes_moved": moved, "TB_per_s": round(moved / med / 1e6, 3),
                          "fraction_of_hbm_bound_pass_at_8TBps": round(moved / 8e12 / (med * 1e-6), 4)}), flush=True)
        del raw, text, out
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 22, help="reads of the short leg")
    ap.add_argument("--long_reads", type=int, default=1 << 18, help="reads of the long leg")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--only", default=None, choices=["short", "long", "kernel"])
    ap.add_argument("--trace", default=None)
    ap.add_argument("--bam_output", action="store_true", help="the measurements of BAM output instead")
    ap.add_argument("--shard", action="store_true", help="the measurements of --bam_shard instead")
    ap.add_argument("--bam_tags", action="store_true", help="the measurements of --bam_tags instead")
    a = ap.parse_args()
    if a.trace:
        t, total = trace_times(a.trace)
        print(json.dumps({"all_kernels_us": round(total, 1), "kernel_us": {k: {"launches": len(v), "sum": round(sum(v), 1), "median": round(statistics.median(v), 1),
                                                                               "largest": round(max(v), 1)} for k, v in sorted(t.items())}}))
        return
    which = [a.only] if a.only else ["short", "long", "kernel"]
    if a.shard:                                  # (the 100 bp file only: the probes and the batch of the 10 kb shape are made in memory)
        which = [w for w in which if w != "long"]
    if a.bam_tags:
        d = a.keep or tempfile.mkdtemp(prefix="rdbam", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        os.makedirs(d, exist_ok=True)
        try:
            jobs = [(d, s, n) for s, n in (("short", a.reads), ("long", a.long_reads)) if s in which]
            if jobs:
                import multiprocessing as mp
                with mp.get_context("spawn").Pool(len(jobs)) as pool:          # (before anything initialises the GPU)
                    pool.map(_make_tagged, jobs)
                    pool.map(_make_qs, [(d, n) for _, s, n in jobs if s == "short"])
            import ribodetector_amd  # noqa: F401
            for _, s, n in jobs:
                bench_cli_bam_tags(d, s, n, a.calls)
                if s == "short":
                    bench_cli_bam_tag_floats(d, n, a.calls)
            if "kernel" in which:
                bench_kernel_bam_tags(20)
                bench_kernel_float_text(20)
                bench_kernel_bam_tags_floats(20)
        finally:
            if not a.keep:
                shutil.rmtree(d, ignore_errors=True)
        return
    jobs = [(s, n, a.bam_output or a.shard) for s, n in (("short", a.reads), ("long", a.long_reads)) if s in which]
    d = a.keep or tempfile.mkdtemp(prefix="rdbam", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        if jobs:
            make_inputs(d, jobs)                 # (before anything initialises the GPU)
        import ribodetector_amd  # noqa: F401
        if a.shard:
            if "kernel" in which:
                bench_shard_kernels(20)
            for s, n, _ in jobs:
                bench_shard_plan(d, n)
                bench_shard_cli(d, n, a.calls)
            return
        for s, n, _ in jobs:
            (bench_cli_bam_output if a.bam_output else bench_cli)(d, s, n, a.calls)
        if "kernel" in which:
            bench_kernel(20, raw_view=a.bam_output)
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
