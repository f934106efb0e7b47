#!/usr/bin/env python
"""What --read_groups costs: the three kernels alone, and the CLI with and without the flag. Prints one JSON line per measurement.
    python tools/groups_bench.py [--only kernel|cli] [--reads 4194304] [--calls 3] [--keep DIR]
  kernel  rd_bam_tag_find, rd_bam_group_rows and rd_bam_group_accumulate, each ALONE on a raw view resident in HBM, 20 calls timed with
          device events (median us per call), for both lane mappings of the find kernel (RD_TAG_LANES = 4 / 16) and the one the
          library chooses. Shapes: (a) 2^20 records of 100 bp with NM:i, XS:A and RG:Z, one read group; (b) the same with 384 groups;
          (c) 8,192 records of 10 kb with MM:Z of about 2 KB and ML:B:C of 2,000 values in front of RG. The yardstick is
          rd_summary_accumulate on the FASTQ view of the same records (single-end), timed the same way.
  cli     `--reads` single-end reads of 100 bp in a BAM file (the records of tools/bam_bench.py with the tags of shape (a), 24 groups)
          -> .gz output: the legs --summary and --summary --read_groups, one untimed warm-up call of each, then `--calls` timed calls of
          each, ALTERNATING (model load excluded). The no-flag leg is the yardstick: the with-flag median is to be read against its
          run-to-run spread. Also the peak of torch's allocator in each leg: what keep_raw adds to HBM.
The inputs are written by a process that never touches the GPU."""
import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAME = 11


def records(n, length, groups, long_tags, seed=1):
    """(records uint8[n, size], size, tag bytes per record, ids): n records of `length` bases whose tags are NM:i XS:A [MM:Z ML:B:C] RG:Z"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ids = [b"grp%03d" % g for g in range(groups)]
    tags = [np.frombuffer(b"NMi" + struct.pack("<i", 3) + b"XSA+", np.uint8)]
    if long_tags:
        mm = b"MMZC+m?," + b",".join(b"%d" % x for x in rng.integers(0, 30, 800)) + b";"
        mm = mm[:2040] + b";\0"
        tags += [np.frombuffer(mm + b"MLBC" + struct.pack("<I", 2000), np.uint8), rng.integers(0, 256, 2000, dtype=np.uint8)]
    head = np.concatenate(tags)
    t_bytes = len(head) + 3 + 6 + 1
    block = 32 + NAME + length // 2 + length + t_bytes
    rec = np.zeros((n, 4 + block), np.uint8)
    rec[:, :36] = np.frombuffer(struct.pack("<iiiBBHHHIiii", block, -1, -1, NAME, 0, 4680, 0, 4, length, -1, -1, 0), np.uint8)
    rec[:, 36:36 + NAME - 1] = ord("r")
    rec[:, 36 + NAME:36 + NAME + length // 2] = rng.integers(0, 256, (n, length // 2), dtype=np.uint8)
    rec[:, 36 + NAME + length // 2:36 + NAME + length // 2 + length] = 30
    t0 = 4 + block - t_bytes
    rec[:, t0:t0 + len(head)] = head
    rec[:, t0 + len(head):t0 + len(head) + 3] = np.frombuffer(b"RGZ", np.uint8)
    which = rng.integers(0, groups, n)
    rec[:, t0 + len(head) + 3:t0 + len(head) + 9] = np.frombuffer(b"".join(ids), np.uint8).reshape(groups, 6)[which]
    return rec, 4 + block, t_bytes, ids


def _times(fn, calls):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for k in range(calls):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(calls))
    return {"median": round(statistics.median(us), 1), "lowest": round(us[0], 1), "highest": round(us[-1], 1)}


def bench_kernels(calls=20):
    import torch
    from ribodetector_amd import bam, groups
    from ribodetector_amd.summary import DeviceSummary
    dev = torch.device("cuda:0")
    for shape, (n, length, G, long_tags) in (("a", (1 << 20, 100, 1, False)), ("b", (1 << 20, 100, 384, False)), ("c", (8192, 10000, 1, True))):
        rec, size, t_bytes, ids = records(n, length, G, long_tags)
        raw = torch.from_numpy(rec.reshape(-1)).to(dev)
        rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * size
        header = bam.encode_header(text=b"".join(b"@RG\tID:" + i + b"\n" for i in ids))
        dg = groups.DeviceGroups(dev, header)
        labels = torch.randint(-1, 2, (n,), device=dev, dtype=torch.int8)
        out = {"shape": shape, "records": n, "read_len": length, "groups": G, "record_bytes": size, "tag_bytes": t_bytes, "view_MB": round(n * size / 1e6, 1),
               "calls": calls, "find_us": {}}
        want = None
        for lanes in ("4", "16", None):
            if lanes is None:
                os.environ.pop("RD_TAG_LANES", None)
            else:
                os.environ["RD_TAG_LANES"] = lanes
            out["find_us"][lanes or "chosen"] = _times(lambda: groups.tag_find(raw, rs, n, b"RG"), calls)
            got = [t.cpu() for t in groups.tag_find(raw, rs, n, b"RG")]
            want = want or got
            assert all(torch.equal(x, y) for x, y in zip(got, want)) and int((got[0] < 0).sum()) == 0 and int(got[1].min()) == 6
        vo, vl, vt = groups.tag_find(raw, rs, n, b"RG")
        out["rows_us"] = _times(lambda: dg.dict.rows(raw, vo, vl, vt), calls)
        rows = dg.dict.rows(raw, vo, vl, vt)
        view = (raw, rs, rows, 0, 1)
        out["accumulate_us"] = _times(lambda: groups.accumulate(dg.acc, G, labels, view), calls)
        dg.acc.zero_()
        info = groups.accumulate(dg.acc, G, labels, view)
        acc = dg.result()
        assert int(info[0]) == 0 and groups.units_per_class(acc, G) == [int((labels == v).sum()) for v in (-1, 0, 1)] and int(acc[1:-1:2].sum()) == n * length
        # bytes the three kernels have to move: the fixed part and the tags of every record, the tables they write and read
        out["bytes_MB"] = {"find": round(n * (36 + t_bytes + 8 + 13) / 1e6, 1), "rows": round(n * (13 + 6 + 4) / 1e6, 1), "accumulate": round(n * (4 + 8 + 4 + 1) / 1e6, 1)}
        # the yardstick: rd_summary_accumulate over the FASTQ view of the same records (single-end)
        frec = 2 * length + NAME + 5
        text = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n * frec,), device=dev)]
        off = torch.arange(n, dtype=torch.int64, device=dev) * frec + NAME + 1
        ln = torch.full((n,), length, dtype=torch.int32, device=dev)
        logits = torch.randn((n, 2), device=dev) * 4
        ds = DeviceSummary(dev)
        lab01 = (logits[:, 1] > logits[:, 0]).to(torch.int8)
        out["summary_accumulate_us"] = _times(lambda: ds.add((text, off, ln), logits, None, None, lab01), calls)
        three = out["find_us"]["chosen"]["median"] + out["rows_us"]["median"] + out["accumulate_us"]["median"]
        out["three_kernels_us"] = round(three, 1)
        out["ratio_to_summary_pass"] = round(three / out["summary_accumulate_us"]["median"], 3)
        print(json.dumps(out), flush=True)
        del raw, rs, text, rec
        torch.cuda.empty_cache()


def _make(job):
    d, reads = job
    import bam_bench
    import numpy as np
    from ribodetector_amd import bam, synth
    path = os.path.join(d, "rg_%d.bam" % reads)
    if os.path.exists(path):
        return
    ids = [b"grp%03d" % g for g in range(24)]
    tags = b"NMi" + struct.pack("<i", 3) + b"XSA+" + b"RGZ"
    step = 1 << 18
    with open(path + ".raw", "wb") as fh:
        fh.write(bam.encode_header(text=b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@RG\tID:" + i + b"\tSM:s" + i[3:] + b"\n" for i in ids)))
        for first in range(0, reads, step):
            n = min(step, reads - first)
            _, rec = bam_bench._rows(n, first, 100, seed=1000 + first // step)
            full = np.zeros((n, rec.shape[1] + len(tags) + 7), np.uint8)
            full[:, :rec.shape[1]] = rec
            full[:, :4] = np.frombuffer(struct.pack("<i", full.shape[1] - 4), np.uint8)
            full[:, rec.shape[1]:rec.shape[1] + len(tags)] = np.frombuffer(tags, np.uint8)
            which = ((first + np.arange(n)) // 1000) % len(ids)              # (runs of one group, as a demultiplexer's output has them)
            full[:, rec.shape[1] + len(tags):-1] = np.frombuffer(b"".join(ids), np.uint8).reshape(len(ids), 6)[which]
            fh.write(full.tobytes())
    synth.bgzip_file(path + ".raw", path, level=6, threads=8)
    os.remove(path + ".raw")


def bench_cli(d, reads, calls):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(1) as pool:
        pool.map(_make, [(d, reads)])
    import torch
    from ribodetector_amd import detect
    src, js = os.path.join(d, "rg_%d.bam" % reads), os.path.join(d, "summary.json")
    legs = {"summary": [], "summary_read_groups": ["--read_groups"]}
    argv = {k: ["-l", "100", "-i", src, "-o", os.path.join(d, "o_%s.fq.gz" % k), "--summary", js] + extra for k, extra in legs.items()}
    for k in legs:
        detect.main(argv[k], log_level="WARNING")
    secs, peak, doc = {k: [] for k in legs}, {}, {}
    for _ in range(calls):
        for k in legs:
            torch.cuda.reset_peak_memory_stats()
            secs[k].append(detect.main(argv[k], log_level="WARNING").timing["detect_s"])
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
            doc[k] = json.load(open(js))
    rate = {k: sorted(reads / s for s in v) for k, v in secs.items()}
    med = {k: statistics.median(v) for k, v in rate.items()}
    rg = doc["summary_read_groups"]["read_groups"]
    assert "read_groups" not in doc["summary"] and sum(g["units"]["total"] for g in rg["groups"]) == reads
    print(json.dumps({"cli": "BAM (24 read groups) -> .gz, 100 bp single-end", "reads": reads, "calls": calls,
                      "reads_per_s": {k: {"median": round(med[k]), "lowest": round(v[0]), "highest": round(v[-1])} for k, v in rate.items()},
                      "ratio_of_medians": round(med["summary_read_groups"] / med["summary"], 4),
                      "inside_no_flag_spread": bool(rate["summary"][0] <= med["summary_read_groups"] <= rate["summary"][-1]),
                      "peak_allocated_MB": {k: round(v / 1e6) for k, v in peak.items()},
                      "keep_raw_adds_MB": round((peak["summary_read_groups"] - peak["summary"]) / 1e6),
                      "groups_with_reads": sum(1 for g in rg["groups"] if g["units"]["total"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernel", "cli"], default=None)
    ap.add_argument("--reads", type=int, default=1 << 22)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        bench_kernels()
    if a.only in (None, "cli"):
        d = a.keep or tempfile.mkdtemp(prefix="rdgrp", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        os.makedirs(d, exist_ok=True)
        try:
            bench_cli(d, a.reads, a.calls)
        finally:
            if not a.keep:
                shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
