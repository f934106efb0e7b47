"""BAM tags in the FASTQ header lines (`--bam_tags MM,ML,RG`): the TAGGED view of a chunk - its FASTQ text with every record's listed
tags behind the read name, '@name\\tMM:Z:...\\tML:B:C,...' - built on the device from the chunk's FASTQ view and its raw records
(DeviceChunk.dev, DeviceChunk.raw): C ABI rd_bam_tag_splice, csrc/rd_bam_tagtext.hpp. The rule is bam.py (tag_comment,
fastq_text_tagged); float-typed values (f, B:f) are not copied, they are counted - or, with floats on (`--bam_tag_floats`: C ABI
rd_bam_tag_splice_ex with RD_BAM_TAGS_FLOATS), written in printf's %g form, the rule of bam.float_g (float_text: the formatter alone).

The tagged text has no bound linear in the FASTQ text (a B:c element of one byte prints as up to five), so the buffer is sized by a
hint - the text's bytes plus twice the raw view's - and a chunk that needs more is spliced a second time with the exact size the
first call reported (fault 1).
"""
import os

import numpy as np
import torch

from . import _native as N
from . import bam

HINT_ENV = "RD_BAM_TAGS_HINT"
INFO_WORDS = 8 + N.BAM_TAGS_MAX


def parse_list(text):
    """the names of --bam_tags LIST (bam.parse_tag_list); RuntimeError names the flag"""
    try:
        return bam.parse_tag_list(text)
    except ValueError as e:
        raise RuntimeError("--bam_tags: {} (checked before anything touches a device)".format(e))


def default_hint(text_bytes, raw_bytes):
    """bytes reserved for a chunk's tagged text when RD_BAM_TAGS_HINT is not set: the text plus twice the raw view (which holds the
    names, the bases and the qualities besides the tags: twice its bytes is room for values that print as four times theirs when the
    tags are half of a record)"""
    env = os.environ.get(HINT_ENV)
    if env:
        return max(16, int(env))
    return int(text_bytes) + 2 * int(raw_bytes)


def float_text(bits):
    """(text uint8[n, 16], len uint8[n]) of the float32 values with the bit patterns `bits` (a contiguous int32 or uint32 tensor of n
    entries on the device; a float32 tensor is read as its bits): one call of rd_float_text on the current stream. Row k holds
    bam.float_g of value k in its first len[k] bytes and zeros behind. Asynchronous."""
    if bits.dtype == torch.float32:
        bits = bits.view(torch.int32)
    if bits.dtype not in (torch.int32, torch.uint32) or not bits.is_contiguous() or bits.dim() != 1:
        raise TypeError("float_text: bits must be a contiguous 1-d int32, uint32 or float32 tensor")
    n, dev = int(bits.numel()), bits.device
    text = torch.empty((n, N.FLOAT_TEXT_SLOT), dtype=torch.uint8, device=dev)
    length = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().rd_float_text(N.ptr(bits), n, N.ptr(text), N.ptr(length), N.stream_ptr(dev)), "rd_float_text")
    return text, length


def splice(text, rec_start, raw, raw_start, n_rec, tags, out_cap, out=None, floats=False):
    """one call of rd_bam_tag_splice (floats: of rd_bam_tag_splice_ex with RD_BAM_TAGS_FLOATS) on the current stream: (out, out_start
    int64[n_rec + 1], info int64[8 + TAGS_MAX]), all on the device. out: a uint8 buffer of at least out_cap bytes (made here when None).
    Asynchronous."""
    n_rec, tags = int(n_rec), [bytes(t) for t in tags]
    if any(len(t) != 2 for t in tags):
        raise ValueError("splice: a tag has 2 bytes")
    for t, name in ((text, "text"), (raw, "raw")):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError("splice: %s must be a contiguous uint8 tensor" % name)
    for t, name in ((rec_start, "rec_start"), (raw_start, "raw_start")):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < n_rec + 1:
            raise TypeError("splice: %s must be a contiguous int64 tensor of n_rec + 1 entries" % name)
    dev = text.device
    lib = N.lib()
    out_cap = int(out_cap)
    if out is None:
        out = torch.empty(((max(out_cap, 0) + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
    if out.numel() < out_cap:
        raise ValueError("splice: out holds %d bytes, out_cap is %d" % (out.numel(), out_cap))
    out_start = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    info = torch.empty(INFO_WORDS, dtype=torch.int64, device=dev)
    need = int(lib.rd_bam_tag_splice_workspace_bytes(n_rec, len(tags)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    if n_rec == 0:
        out_start.zero_()
    args = (N.ptr(text), int(text.numel()), N.ptr(rec_start), N.ptr(raw), int(raw.numel()), N.ptr(raw_start), n_rec, b"".join(tags), len(tags), N.ptr(out),
            out_cap, N.ptr(out_start), N.ptr(info), N.ptr(ws), ws.numel())
    with torch.cuda.device(dev):
        if floats:
            N.check(lib.rd_bam_tag_splice_ex(*args, N.BAM_TAGS_FLOATS, N.stream_ptr(dev)), "rd_bam_tag_splice_ex")
        else:
            N.check(lib.rd_bam_tag_splice(*args, N.stream_ptr(dev)), "rd_bam_tag_splice")
    return out, out_start, info


class DeviceBamTags:
    """splice(chunk) -> (text, out_start, info): the tagged view of a DeviceChunk that carries its raw records (the reader ran with
    keep_raw). text: uint8 on the device, cut behind the tagged bytes (with the slack of 256 bytes a chunk's text has); out_start int64[n + 1] on the device; info: the call's int64[8 + TAGS_MAX]
    as a numpy array - the host waits for it (the splice depends on nothing but the chunk, so it runs on a stream that is not behind
    the recurrences), which is where a chunk that did not fit its hint is spliced again. The counters of every call are added up in
    `copied`, `malformed_records`, `float_values_skipped`; `repeats` counts the second calls. floats: f and B:f values are written
    (bam.float_g) instead of skipped."""

    def __init__(self, device, tags, floats=False):
        self.device = torch.device(device)
        self.tags = [bytes(t) for t in tags]
        self.floats = bool(floats)
        self.copied = [0] * len(self.tags)
        self.malformed_records = 0
        self.float_values_skipped = 0
        self.repeats = 0

    def _call(self, text, rs, raw, raw_start, n, cap):
        out, out_start, info = splice(text, rs, raw, raw_start, n, self.tags, cap, floats=self.floats)
        host = torch.empty(INFO_WORDS, dtype=torch.int64, pin_memory=True)
        host.copy_(info, non_blocking=True)
        ev = N.new_event()
        ev.record(torch.cuda.current_stream(self.device))
        N.wait_event(ev)
        return out, out_start, host.numpy().copy()

    def splice(self, chunk):
        if chunk.raw is None:
            raise RuntimeError("DeviceBamTags.splice: the chunk carries no raw records (the reader must run with keep_raw)")
        text, rs = chunk.dev[0], chunk.dev[3]
        raw, raw_start = chunk.raw
        n = int(rs.numel()) - 1
        if int(raw_start.numel()) - 1 != n:
            raise RuntimeError("DeviceBamTags.splice: the chunk holds %d raw records for %d FASTQ records" % (int(raw_start.numel()) - 1, n))
        out, out_start, info = self._call(text, rs, raw, raw_start, n, default_hint(text.numel(), raw.numel()))
        if int(info[3]) == 1:
            self.repeats += 1
            del out
            out, out_start, info = self._call(text, rs, raw, raw_start, n, int(info[1]))
        if int(info[3]):
            raise RuntimeError("device BAM tags: the chunk's record tables do not describe its text and raw records (fault %d)" % int(info[3]))
        for j in range(len(self.tags)):
            self.copied[j] += int(info[8 + j])
        self.malformed_records += int(info[4])
        self.float_values_skipped += int(info[5])
        size = int(info[1])
        return out[:min(out.numel(), ((size + 255) // 256) * 256 + 256)], out_start, info

    def counts(self):
        return {"copied": list(self.copied), "malformed_records": self.malformed_records, "float_values_skipped": self.float_values_skipped}


def to_json(tags, counts_per_mate, floats=False):
    """the "bam_tags" object of the summary: counts_per_mate = [counts()] of a single-end or interleaved run, [mate 1's, mate 2's] of
    a two-file run (every count is then a pair). floats (--bam_tag_floats): "float_format": "%g" as the last key"""
    names = [bytes(t).decode() for t in tags]
    if len(counts_per_mate) == 1:
        c = counts_per_mate[0]
        doc = {"tags": names, "copied": [int(x) for x in c["copied"]], "malformed_records": int(c["malformed_records"]),
               "float_values_skipped": int(c["float_values_skipped"])}
    else:
        doc = {"tags": names, "copied": [[int(c["copied"][j]) for c in counts_per_mate] for j in range(len(names))],
               "malformed_records": [int(c["malformed_records"]) for c in counts_per_mate],
               "float_values_skipped": [int(c["float_values_skipped"]) for c in counts_per_mate]}
    if floats:
        doc["float_format"] = "%g"
    return doc


def log_line(tags, counts_per_mate):
    """'BAM tags: MM N, ML N, RG N copied; X records with malformed tags, Y float values skipped' - the mates' counts summed"""
    names = [bytes(t).decode() for t in tags]
    copied = [sum(int(c["copied"][j]) for c in counts_per_mate) for j in range(len(names))]
    return "BAM tags: {} copied; {} records with malformed tags, {} float values skipped".format(
        ", ".join("{} {}".format(t, n) for t, n in zip(names, copied)), sum(int(c["malformed_records"]) for c in counts_per_mate),
        sum(int(c["float_values_skipped"]) for c in counts_per_mate))


def as_vector(counts_per_mate, n_tags):
    """the counters as one int64 vector (what the ranks of a --bam_shard run sum): per mate n_tags + 2 words"""
    v = []
    for c in counts_per_mate:
        v += [int(x) for x in c["copied"]] + [int(c["malformed_records"]), int(c["float_values_skipped"])]
    return np.asarray(v, dtype=np.int64)


def from_vector(v, n_tags, mates):
    v = [int(x) for x in v]
    w = n_tags + 2
    return [{"copied": v[m * w:m * w + n_tags], "malformed_records": v[m * w + n_tags], "float_values_skipped": v[m * w + n_tags + 1]}
            for m in range(mates)]
