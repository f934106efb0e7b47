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
  --tags  the legs of --ubam_tags instead (into profiles/ubam_tags_bench.jsonl). kernel: rd_bam_encode_ex with listed names on 2^20
          reads of 100 bp with '\\tRG:Z:lib7' and on 8,192 reads of 10 kb with MM:Z 2 kB + ML:B:C x 2,000, against rd_bam_encode on the
          same records without the comment, alternating. cli: the 100 bp file with the RG comment, --ubam_output with and without
          --ubam_tags RG.
  --tags --floats  the legs of --ubam_tag_floats instead (appended to the same file). kernel: rd_float_parse ALONE on 2^24 resident
          values - %g texts of uniform random bit patterns, and qs-like 5.0-40.0 with 4 decimals - next to rd_float_text on the same
          patterns in the same process; rd_bam_encode_ex with the bit set on 2^20 reads of 100 bp with '\\tqs:f:dd.dddd\\tRG:Z:lib7'
          against the SAME call on records whose qs is a qs:i of 7 digits (existing code), and on 8,192 reads of 10 kb with a B:f array
          of 2,000 elements beside MM / ML against the same records without the bit (the array counted and left out). cli: the 100 bp
          file with '\\tqs:f:12.3456\\tRG:Z:lib7', --ubam_output --ubam_tags qs,RG with and without --ubam_tag_floats.
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


def _with_comment(fq, comment):
    """the rows of bam_bench._rows with `comment` (uint8[n, c], or bytes for every row) behind the names"""
    import numpy as np
    import bam_bench
    n = fq.shape[0]
    if isinstance(comment, bytes):
        comment = np.broadcast_to(np.frombuffer(comment, np.uint8), (n, len(comment)))
    return np.ascontiguousarray(np.concatenate([fq[:, :bam_bench.NAME], comment, fq[:, bam_bench.NAME:]], axis=1))


def _mm_ml(n, seed):
    """'\\tMM:Z:C+m?' ',d' x 1,000 ';' (2 kB) and '\\tML:B:C' ',ddd' x 2,000 (values 100..255: rows of one width), per row"""
    import numpy as np
    rng = np.random.default_rng(seed)
    mm = np.empty((n, 1000, 2), np.uint8)
    mm[:, :, 0] = ord(",")
    mm[:, :, 1] = 48 + rng.integers(0, 10, (n, 1000), dtype=np.uint8)
    v = rng.integers(100, 256, (n, 2000))
    ml = np.empty((n, 2000, 4), np.uint8)
    ml[:, :, 0] = ord(",")
    ml[:, :, 1], ml[:, :, 2], ml[:, :, 3] = 48 + v // 100, 48 + (v // 10) % 10, 48 + v % 10
    head = lambda t: np.broadcast_to(np.frombuffer(t, np.uint8), (n, len(t)))      # noqa: E731
    return np.concatenate([head(b"\tMM:Z:C+m?"), mm.reshape(n, -1), head(b";\tML:B:C"), ml.reshape(n, -1)], axis=1)


def _alternate(fns, calls, warm=3):
    """{leg: sorted us per call} of the legs, ALTERNATING in one process, by device events"""
    import torch
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ev = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}


def bench_kernel_tags(calls=20):
    """rd_bam_encode_ex with listed names on a resident chunk whose header lines carry a comment, against rd_bam_encode on the SAME
    records with the comment dropped - this build's n_names == 0 instances, the launches the parent makes; the parent's own binary is
    not loaded next to it -, the two alternating. Bytes moved by the tags leg: the text read once and the comments twice more (the
    count and the tag pass), the raw bytes written once and the tag bytes once more (zeros, then the tags), per record 80 bytes of
    tables and workspace and 48 per listed name."""
    import numpy as np
    import torch
    import bam_bench
    from ribodetector_amd import bam, ubam
    dev = torch.device("cuda:0")
    for shape, n, length, names in (("short", 1 << 20, 100, [b"RG"]), ("long", 8192, 10000, [b"MM", b"ML"])):
        step = max(1, (64 << 20) // (2 * length))
        fq = np.concatenate([bam_bench._rows(min(step, n - f), f, length, seed=7 + f // step)[0] for f in range(0, n, step)])
        tagged = _with_comment(fq, b"\tRG:Z:lib7" if shape == "short" else _mm_ml(n, 5))
        legs, keep = {}, {}
        for leg, rows, tags in (("tags", tagged, names), ("no_comment", fq, [])):
            text = torch.from_numpy(rows.reshape(-1)).to(dev)
            rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * rows.shape[1]
            so = (rs[:-1] + rows.shape[1] - 2 * length - 4).contiguous()
            sl = torch.full((n,), length, dtype=torch.int32, device=dev)
            cap = bam.ubam_bound(text.numel(), n)
            raw = torch.empty(((cap + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
            keep[leg] = (text, rs, so, sl, cap, raw, tags)
            legs[leg] = (lambda a: (lambda: ubam.encode(a[0], a[1], a[2], a[3], n, ubam.flags_word(), raw_cap=a[4], raw=a[5], tags=a[6])))(keep[leg])
        us = _alternate(legs, calls)
        text, rs, so, sl, cap, raw, tags = keep["tags"]
        _, raw_start, info = ubam.encode(text, rs, so, sl, n, ubam.flags_word(), raw_cap=cap, raw=raw, tags=tags)
        info = info.cpu().tolist()
        k = n // 2
        a, b = int(raw_start[k]), int(raw_start[k + 1])
        assert info[3] == 0 and info[0] == n and info[8] == 0 and bytes(raw[a:b].cpu().numpy()) == bam.from_fastq(tagged[k].tobytes(), tags=tags), info
        comment = (tagged.shape[1] - fq.shape[1]) * n
        tag_bytes = info[1] - len(bam.from_fastq(fq[k].tobytes())) * n
        med = {leg: statistics.median(v) for leg, v in us.items()}
        moved = text.numel() + 2 * comment + info[1] + tag_bytes + n * (80 + 48 * len(tags))
        emit({"measurement": "kernel_ubam_tags", "what": "rd_bam_encode_ex against rd_bam_encode on the text without the comment", "shape": shape,
              "read_len": length, "records": n, "names": [t.decode() for t in tags], "text_bytes": text.numel(), "comment_bytes": comment,
              "raw_bytes": info[1], "tag_bytes": tag_bytes, "copied": info[10:], "calls": calls, "us_per_call": {leg: _us(v) for leg, v in us.items()},
              "ratio_of_medians_tags_over_no_comment": round(med["tags"] / med["no_comment"], 3), "bytes_moved": moved,
              "TB_per_s": round(moved / med["tags"] / 1e6, 3), "fraction_of_hbm_bound_pass_at_8TBps": round(moved / 8e12 / (med["tags"] * 1e-6), 4),
              "yardstick": "this build's rd_bam_encode (n_names == 0); the parent's binary next to it: not measured",
              "which_pass_holds_the_time": "not measured"})
        del keep, legs, text, raw
        torch.cuda.empty_cache()


def _make_tagged(job, comment=b"\tRG:Z:lib7"):
    """_make's file with '\\tRG:Z:lib7' behind every name"""
    import bam_bench
    path, reads = job
    if os.path.exists(path):
        return
    step = 1 << 18
    with open(path + ".tmp", "wb") as fh:
        for first in range(0, reads, step):
            fh.write(_with_comment(bam_bench._rows(min(step, reads - first), first, 100, seed=1000 + first // step)[0], comment).tobytes())
    os.replace(path + ".tmp", path)


def _make_qs(job):
    _make_tagged(job, b"\tqs:f:12.3456\tRG:Z:lib7")


def _digits(v, width):
    """uint8[n, width]: the decimal digits of the whole numbers v, zero-padded"""
    import numpy as np
    out = np.empty((len(v), width), np.uint8)
    for c in range(width):
        out[:, width - 1 - c] = 48 + (v // 10 ** c) % 10
    return out


def bench_kernel_float_parse(calls=20):
    """rd_float_parse alone on 2^24 resident values, next to rd_float_text on the same bit patterns. Bytes moved by the parse: the text
    read once, 8 bytes of the table read and 5 written per value; by the formatter 4 read and 17 written."""
    import numpy as np
    import torch
    from ribodetector_amd import _native as N
    from ribodetector_amd import bam, bamtags
    dev, n = torch.device("cuda:0"), 1 << 24
    rng = np.random.default_rng(3)
    for what in ("uniform_bit_patterns_as_%g", "qs_like_5_to_40_with_4_decimals"):
        if what.startswith("uniform"):
            bits = torch.from_numpy(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
            slots, lens = bamtags.float_text(bits)             # the texts come from the formatter: uint8[n, 16] and their lengths
            keep = torch.arange(16, device=dev)[None, :] < lens[:, None].to(torch.int64)
            text = slots[keep].contiguous()
            start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            start[1:] = torch.cumsum(lens.to(torch.int64), 0)
            del slots, keep
        else:
            v = rng.integers(50000, 400000, n)
            rows = np.concatenate([_digits(v // 10000, 2), np.full((n, 1), ord("."), np.uint8), _digits(v % 10000, 4)], axis=1)
            text = torch.from_numpy(rows.reshape(-1)).to(dev)
            start = torch.arange(n + 1, dtype=torch.int64, device=dev) * 7
            bits = torch.from_numpy((v / 10000.0).astype(np.float32).view(np.int32)).to(dev)
        out, status = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        slot, ln = torch.empty(16 * n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        lib, st = N.lib(), N.stream_ptr(dev)
        us = _alternate({"rd_float_parse": lambda: N.check(lib.rd_float_parse(N.ptr(text), N.ptr(start), n, N.ptr(out), N.ptr(status), st), "rd_float_parse"),
                         "rd_float_text": lambda: N.check(lib.rd_float_text(N.ptr(bits), n, N.ptr(slot), N.ptr(ln), st), "rd_float_text")}, calls)
        k = [0, 1, n // 2, n - 1]
        host = bytes(text.cpu().numpy())
        s = start.cpu().numpy()
        assert int(status.max()) == 0 and [int(out[i]) & 0xffffffff for i in k] == [bam.float_from_text(host[s[i]:s[i + 1]]) for i in k]
        med = {leg: statistics.median(v) for leg, v in us.items()}
        moved = {"rd_float_parse": text.numel() + 13 * n, "rd_float_text": 21 * n}
        emit({"measurement": "kernel_float_parse", "what": "rd_float_parse next to rd_float_text, alternating", "values": n, "distribution": what,
              "text_bytes": text.numel(), "calls": calls, "us_per_call": {leg: _us(v) for leg, v in us.items()},
              "values_per_s": {leg: round(n / m * 1e6) for leg, m in med.items()}, "bytes_moved": moved,
              "TB_per_s": {leg: round(moved[leg] / m / 1e6, 3) for leg, m in med.items()},
              "fraction_of_hbm_bound_pass_at_8TBps": {leg: round(moved[leg] / 8e12 / (m * 1e-6), 4) for leg, m in med.items()}})
        del text, start, bits, out, status, slot, ln
        torch.cuda.empty_cache()


def bench_kernel_tag_floats(calls=20):
    """rd_bam_encode_ex with RD_UBAM_TAG_FLOATS. short: 2^20 reads of 100 bp, list qs,RG, floats on - '\\tqs:f:dd.dddd\\tRG:Z:lib7' against
    the SAME call on '\\tqs:i:ddddddd\\tRG:Z:lib7' (existing code: the integer path; both comments are 24 bytes). long: 8,192 reads of
    10 kb with MM, ML and '\\tXF:B:f' ',d.ddd' x 2,000, list MM,ML,XF, with the bit against without it (the array counted and left out)."""
    import numpy as np
    import torch
    import bam_bench
    from ribodetector_amd import bam, ubam
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    for shape, n, length, names in (("short", 1 << 20, 100, [b"qs", b"RG"]), ("long", 8192, 10000, [b"MM", b"ML", b"XF"])):
        step = max(1, (64 << 20) // (2 * length))
        fq = np.concatenate([bam_bench._rows(min(step, n - f), f, length, seed=7 + f // step)[0] for f in range(0, n, step)])
        head = lambda t: np.broadcast_to(np.frombuffer(t, np.uint8), (n, len(t)))      # noqa: E731
        if shape == "short":
            v = rng.integers(50000, 400000, n)
            qs_f = np.concatenate([head(b"\tqs:f:"), _digits(v // 10000, 2), head(b"."), _digits(v % 10000, 4), head(b"\tRG:Z:lib7")], axis=1)
            qs_i = np.concatenate([head(b"\tqs:i:"), _digits(rng.integers(10 ** 6, 10 ** 7, n), 7), head(b"\tRG:Z:lib7")], axis=1)
            rows = {"floats": (_with_comment(fq, qs_f), True), "yardstick_qs_i": (_with_comment(fq, qs_i), True)}
            yard = "the same call on records whose qs is a qs:i of 7 digits"
        else:
            el = np.empty((n, 2000, 6), np.uint8)
            el[:, :, 0], el[:, :, 2] = ord(","), ord(".")
            d = rng.integers(0, 10000, (n, 2000))
            el[:, :, 1], el[:, :, 3], el[:, :, 4], el[:, :, 5] = 48 + d // 1000, 48 + (d // 100) % 10, 48 + (d // 10) % 10, 48 + d % 10
            tagged = _with_comment(fq, np.concatenate([_mm_ml(n, 5), head(b"\tXF:B:f"), el.reshape(n, -1)], axis=1))
            rows = {"floats": (tagged, True), "yardstick_left_out": (tagged, False)}
            yard = "the same records and list without the bit: the array is counted and left out"
        legs, keep = {}, {}
        for leg, (r, fl) in rows.items():
            text = torch.from_numpy(r.reshape(-1)).to(dev)
            rs = torch.arange(n + 1, dtype=torch.int64, device=dev) * r.shape[1]
            so = (rs[:-1] + r.shape[1] - 2 * length - 4).contiguous()
            sl = torch.full((n,), length, dtype=torch.int32, device=dev)
            cap = bam.ubam_bound(text.numel(), n)
            raw = torch.empty(((cap + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
            keep[leg] = (text, rs, so, sl, cap, raw, fl)
            legs[leg] = (lambda a: (lambda: ubam.encode(a[0], a[1], a[2], a[3], n, ubam.flags_word(), raw_cap=a[4], raw=a[5], tags=names, floats=a[6])))(keep[leg])
        us = _alternate(legs, calls)
        text, rs, so, sl, cap, raw, _ = keep["floats"]
        _, raw_start, info = ubam.encode(text, rs, so, sl, n, ubam.flags_word(), raw_cap=cap, raw=raw, tags=names, floats=True)
        info = info.cpu().tolist()
        k = n // 2
        a, b = int(raw_start[k]), int(raw_start[k + 1])
        assert info[3] == 0 and info[0] == n and info[8] == info[9] == 0 and min(info[10:]) == n, info
        assert bytes(raw[a:b].cpu().numpy()) == bam.from_fastq(rows["floats"][0][k].tobytes(), tags=names, floats=True)
        med = {leg: statistics.median(v) for leg, v in us.items()}
        other = [leg for leg in med if leg != "floats"][0]
        lo, hi = us[other][0], us[other][-1]
        emit({"measurement": "kernel_ubam_tag_floats", "what": "rd_bam_encode_ex | RD_UBAM_TAG_FLOATS", "shape": shape, "read_len": length, "records": n,
              "names": [t.decode() for t in names], "text_bytes": text.numel(), "raw_bytes": info[1], "calls": calls, "yardstick": yard,
              "us_per_call": {leg: _us(v) for leg, v in us.items()}, "ratio_of_medians_floats_over_yardstick": round(med["floats"] / med[other], 3),
              "floats_median_inside_yardstick_spread": bool(lo <= med["floats"] <= hi), "which_pass_holds_the_time": "not measured"})
        del keep, legs, text, raw
        torch.cuda.empty_cache()


def bench_cli_tag_floats(d, reads, calls):
    """`reads` reads of 100 bp with '\\tqs:f:12.3456\\tRG:Z:lib7': --ubam_output --ubam_tags qs,RG with and without --ubam_tag_floats
    (without: the parent's behaviour and the yardstick), the legs alternating"""
    import torch
    from ribodetector_amd import detect
    src = os.path.join(d, "se_qs_%d.fq" % reads)
    base = ["-l", "100", "-i", src, "-o"]
    argv = {"tags": base + [os.path.join(d, "o_tags.bam"), "--ubam_output", "--ubam_tags", "qs,RG"],
            "tag_floats": base + [os.path.join(d, "o_floats.bam"), "--ubam_output", "--ubam_tags", "qs,RG", "--ubam_tag_floats"]}
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
    yard, m = rate["tags"], med["tag_floats"]
    outside = 0.0 if yard[0] <= m <= yard[-1] else (m / yard[0] - 1 if m < yard[0] else m / yard[-1] - 1)
    emit({"measurement": "short_ubam_tag_floats", "reads": reads, "read_len": 100, "calls": calls,
          "flow": "single-end x.fq with qs:f and RG:Z comments -> .bam --ubam_output --ubam_tags qs,RG | + --ubam_tag_floats",
          "input_bytes": os.path.getsize(src), "output_bytes": {k: os.path.getsize(v[5]) for k, v in argv.items()},
          "reads_per_s": {k: {"median": round(statistics.median(v)), "lowest": round(v[0]), "highest": round(v[-1])} for k, v in rate.items()},
          "ratio_of_medians": round(m / med["tags"], 4), "with_flag_median_inside_no_flag_spread": bool(outside == 0.0),
          "outside_the_spread_by": round(outside, 4), "peak_allocated_MB": {k: round(v / 1e6) for k, v in peak.items()},
          "flag_adds_MB": round((peak["tag_floats"] - peak["tags"]) / 1e6), "tag_counts": {k: last[k]._ubam_tag_total[0] for k in argv},
          "second_calls": last["tag_floats"]._ubam[0].repeats, "which_pass_holds_the_time": "not measured"})


def bench_cli_tags(d, reads, calls):
    """`reads` reads of 100 bp with '\\tRG:Z:lib7': --ubam_output with and without --ubam_tags RG, the legs alternating"""
    import torch
    from ribodetector_amd import detect
    src = os.path.join(d, "se_rg_%d.fq" % reads)
    argv = {"ubam": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_plain.bam"), "--ubam_output"],
            "ubam_tags": ["-l", "100", "-i", src, "-o", os.path.join(d, "o_tags.bam"), "--ubam_output", "--ubam_tags", "RG"]}
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
    yard, m = rate["ubam"], med["ubam_tags"]
    outside = 0.0 if yard[0] <= m <= yard[-1] else (m / yard[0] - 1 if m < yard[0] else m / yard[-1] - 1)
    emit({"measurement": "short_ubam_tags", "reads": reads, "read_len": 100, "calls": calls, "flow": "single-end x.fq with RG:Z comments -> .bam --ubam_output | + --ubam_tags RG",
          "input_bytes": os.path.getsize(src), "output_bytes": {k: os.path.getsize(v[5]) for k, v in argv.items()},
          "reads_per_s": {k: {"median": round(statistics.median(v)), "lowest": round(v[0]), "highest": round(v[-1])} for k, v in rate.items()},
          "ratio_of_medians": round(m / med["ubam"], 4), "with_flag_median_inside_no_flag_spread": bool(outside == 0.0),
          "outside_the_spread_by": round(outside, 4), "peak_allocated_MB": {k: round(v / 1e6) for k, v in peak.items()},
          "flag_adds_MB": round((peak["ubam_tags"] - peak["ubam"]) / 1e6), "tag_counts": last["ubam_tags"]._ubam_tag_total[0],
          "second_calls": last["ubam_tags"]._ubam[0].repeats, "which_pass_holds_the_time": "not measured"})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--tags", action="store_true", help="the --ubam_tags legs (default --out: profiles/ubam_tags_bench.jsonl)")
    ap.add_argument("--floats", action="store_true", help="with --tags: the --ubam_tag_floats legs")
    ap.add_argument("--reads", type=int, default=1 << 22)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["kernel", "cli"])
    ap.add_argument("--keep", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    OUT = a.out or os.path.join(ROOT, "profiles", "ubam_tags_bench.jsonl" if a.tags else "ubam_bench.jsonl")
    d = a.keep or tempfile.mkdtemp(prefix="rdubam", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    try:
        if a.only != "kernel":
            import multiprocessing as mp
            with mp.get_context("spawn").Pool(1) as pool:          # (before anything initialises the GPU)
                if a.tags and a.floats:
                    pool.map(_make_qs, [(os.path.join(d, "se_qs_%d.fq" % a.reads), a.reads)])
                elif a.tags:
                    pool.map(_make_tagged, [(os.path.join(d, "se_rg_%d.fq" % a.reads), a.reads)])
                else:
                    pool.map(_make, [(os.path.join(d, "se_%d.fq" % a.reads), a.reads)])
        import ribodetector_amd  # noqa: F401
        if a.tags and a.floats:
            if a.only != "cli":
                bench_kernel_float_parse()
                bench_kernel_tag_floats()
            if a.only != "kernel":
                bench_cli_tag_floats(d, a.reads, a.calls)
            return
        if a.only != "cli":
            bench_kernel_tags() if a.tags else bench_kernel()
        if a.only != "kernel":
            bench_cli_tags(d, a.reads, a.calls) if a.tags else bench_cli(d, a.reads, a.calls)
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
