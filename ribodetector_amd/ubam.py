"""FASTQ / FASTA input written as unaligned BAM (`--ubam_output`): the RAW view of a chunk that did not come from a BAM file - its
records as BAM records, made on the device from the chunk's text and tables (DeviceChunk.dev): C ABI rd_bam_encode,
csrc/rd_bam_encode.hpp. The rule is bam.py (from_fastq, ubam_name, UBAM_HEADER_TEXT). The raw bytes have a bound linear in the text
(bam.ubam_bound), so the buffer is sized without a hint, the call is made once and nothing waits for it.

`--ubam_tags LIST`: the records carry the listed tags of their header lines' comments (C ABI rd_bam_encode_ex; the rule is
bam.tags_from_comment). A tag takes at most twice its text and real comments shrink, so the buffer keeps the same size
(RD_UBAM_TAGS_HINT overrides it); the call reports the exact need with fault 1, and a chunk that needs more is encoded once more at
that size - the host waits for the verdict of every call, as it does under --bam_tags.

`--ubam_tag_floats`: the f and B:f values of the listed tags become float32 tags (flag RD_UBAM_TAG_FLOATS; the rule is
bam.float_from_text, csrc/rd_float_parse.hpp) instead of being left out; float_parse is the converter alone (C ABI rd_float_parse).
"""
import os

import torch

from . import _native as N
from . import bam

INFO_WORDS = 8
COUNTERS = ("bases_changed", "quals_clamped", "names_starred")      # info[4], [5], [6]
HINT_ENV = "RD_UBAM_TAGS_HINT"
TAG_INFO = 10           # with listed names: info[8] malformed records, [9] float values skipped, [10 + j] records in which name j was copied


def parse_list(text):
    """the names of --ubam_tags LIST (bam.parse_tag_list); RuntimeError names the flag"""
    try:
        return bam.parse_tag_list(text)
    except ValueError as e:
        raise RuntimeError("--ubam_tags: {} (checked before anything touches a device)".format(e))


def flags_word(n_mates=1, mate=0, fasta=False):
    """the flags of rd_bam_encode: single-end (4, 4); a mate's file (77, 77) / (141, 141); mate = bam.INTERLEAVED: (77, 141)"""
    if mate == bam.INTERLEAVED:
        even, odd = bam.UBAM_FLAGS[(2, 0)], bam.UBAM_FLAGS[(2, 1)]
    else:
        even = odd = bam.UBAM_FLAGS[(int(n_mates), int(mate))]
    return (N.UBAM_FASTA if fasta else 0) | (even << N.UBAM_EVEN_SHIFT) | (odd << N.UBAM_ODD_SHIFT)


def encode(text, rec_start, seq_off, seq_len, n_rec, flags, raw_cap=None, raw=None, rec_first=0, rec_stride=1, text_bytes=None, tags=(), floats=False):
    """one call of rd_bam_encode on the current stream: (raw, raw_start int64[n_rec + 1], info int64[8]), all on the device. raw: a
    uint8 buffer of at least raw_cap bytes (made here when None; raw_cap None: the bound of bam.ubam_bound). Asynchronous.
    tags (names of 2 bytes): one call of rd_bam_encode_ex - the records carry the listed tags of their header lines' comments, and info
    is int64[10 + len(tags)]; fault 1 then leaves the bytes the records need in info[1]. floats (with tags): RD_UBAM_TAG_FLOATS - f and
    B:f values become float32 tags."""
    n_rec, tags = int(n_rec), [bytes(t) for t in tags]
    if any(len(t) != 2 for t in tags):
        raise ValueError("encode: a tag has 2 bytes")
    if floats and not tags:
        raise ValueError("encode: floats says how the listed tags' float values are read: it needs tags")
    if text.dtype != torch.uint8 or not text.is_contiguous():
        raise TypeError("encode: text must be a contiguous uint8 tensor")
    for t, name, dt in ((rec_start, "rec_start", torch.int64), (seq_off, "seq_off", torch.int64), (seq_len, "seq_len", torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError("encode: %s must be a contiguous %s tensor" % (name, dt))
    last = int(rec_first) + (n_rec - 1) * int(rec_stride) if n_rec else -1
    if rec_start.numel() < last + 2 or seq_off.numel() < last + 1 or seq_len.numel() < last + 1:
        raise ValueError("encode: the tables do not hold entry %d" % last)
    dev, lib = text.device, N.lib()
    text_bytes = int(text.numel()) if text_bytes is None else int(text_bytes)
    if raw_cap is None:
        raw_cap = bam.ubam_bound(text_bytes, n_rec, bool(flags & N.UBAM_FASTA))
    raw_cap = int(raw_cap)
    if raw is None:
        raw = torch.empty(((max(raw_cap, 0) + 255) // 256) * 256 + 256, dtype=torch.uint8, device=dev)
    if raw.numel() < raw_cap:
        raise ValueError("encode: raw holds %d bytes, raw_cap is %d" % (raw.numel(), raw_cap))
    raw_start = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    if not tags:
        info = torch.empty(INFO_WORDS, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(lib.rd_bam_encode_workspace_bytes(n_rec)), 256), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            N.check(lib.rd_bam_encode(N.ptr(text), text_bytes, N.ptr(rec_start), N.ptr(seq_off), N.ptr(seq_len), n_rec, int(rec_first), int(rec_stride),
                                      int(flags), N.ptr(raw), raw_cap, N.ptr(raw_start), N.ptr(info), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "rd_bam_encode")
        return raw, raw_start, info
    info = torch.empty(TAG_INFO + len(tags), dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.rd_bam_encode_tags_workspace_bytes(n_rec, len(tags))), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.rd_bam_encode_ex(N.ptr(text), text_bytes, N.ptr(rec_start), N.ptr(seq_off), N.ptr(seq_len), n_rec, int(rec_first), int(rec_stride),
                                     int(flags) | (N.UBAM_TAG_FLOATS if floats else 0), b"".join(tags), len(tags), N.ptr(raw), raw_cap, N.ptr(raw_start), N.ptr(info), N.ptr(ws), ws.numel(),
                                     N.stream_ptr(dev)), "rd_bam_encode_ex")
    return raw, raw_start, info


def tags_hint(text_bytes, n_rec, fasta=False):
    """bytes reserved for a chunk's records under --ubam_tags when RD_UBAM_TAGS_HINT is not set: bam.ubam_bound - the tags of real
    comments take fewer bytes than their text (csrc/rd_bam_encode.hpp has the bound)"""
    env = os.environ.get(HINT_ENV)
    if env:
        return max(16, int(env))
    return bam.ubam_bound(text_bytes, n_rec, fasta)


def float_parse(texts):
    """(bits uint32[n], status uint8[n]) of the texts of n float values (bytes each), both on the host: one call of rd_float_parse on
    the current device's stream - bam.float_from_text on the device. status 0: converted; 1: not of the syntax; 2: more than 17
    significant digits (bits is 0 for 1 and 2)."""
    import numpy as np
    texts = [bytes(t) for t in texts]
    n = len(texts)
    start = np.zeros(n + 1, np.int64)
    start[1:] = np.cumsum(np.fromiter((len(t) for t in texts), np.int64, n))
    dev = torch.device("cuda", torch.cuda.current_device())
    text = torch.from_numpy(np.frombuffer(b"".join(texts) or b"\0", np.uint8).copy()).to(dev)
    st = torch.from_numpy(start).to(dev)
    bits = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().rd_float_parse(N.ptr(text), N.ptr(st), n, N.ptr(bits), N.ptr(status), N.stream_ptr(dev)), "rd_float_parse")
    return bits[:n].cpu().numpy().view(np.uint32), status[:n].cpu().numpy()


class DeviceUbam:
    """encode(chunk, mate, n_mates) -> (raw, raw_start, info): the raw view of a DeviceChunk of FASTQ (fasta: FASTA) records, all
    three on the device; mate = bam.INTERLEAVED for an interleaved chunk. Nothing waits: info (rd_bam_encode's int64[8]) is read by
    whoever has waited for an event behind the call - add(info) then sums its counters and says which record, if any, cannot be a
    BAM record.
    tags (--ubam_tags): the records carry the listed tags of their comments. The host then WAITS for the verdict of the call, behind
    it on the current stream - a chunk whose records need more than their hint is encoded once more at the exact size (`repeats`
    counts them) - and info is rd_bam_encode_ex's int64[10 + len(tags)] as a host tensor; add(info) sums its tag counters too."""

    def __init__(self, device, fasta=False, tags=(), floats=False):
        self.device = torch.device(device)
        self.fasta = bool(fasta)
        self.tags = [bytes(t) for t in tags]
        self.floats = bool(floats)               # --ubam_tag_floats: f and B:f values become float32 tags
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.copied = [0] * len(self.tags)
        self.malformed_records = 0
        self.float_values_skipped = 0
        self.repeats = 0

    def _call(self, chunk, flags, cap):
        text, so, sl, rs = chunk.dev
        raw, raw_start, info = encode(text, rs, so, sl, int(rs.numel()) - 1, flags, raw_cap=cap, tags=self.tags, floats=self.floats)
        host = torch.empty(info.numel(), dtype=torch.int64, pin_memory=True)
        host.copy_(info, non_blocking=True)
        ev = N.new_event()
        ev.record(torch.cuda.current_stream(self.device))
        N.wait_event(ev)
        return raw, raw_start, host

    def encode(self, chunk, mate=0, n_mates=1):
        text, so, sl, rs = chunk.dev
        flags = flags_word(n_mates, mate, self.fasta)
        if not self.tags:
            return encode(text, rs, so, sl, int(rs.numel()) - 1, flags)
        raw, raw_start, info = self._call(chunk, flags, tags_hint(int(text.numel()), int(rs.numel()) - 1, self.fasta))
        if int(info[3]) == 1:
            self.repeats += 1
            del raw
            raw, raw_start, info = self._call(chunk, flags, int(info[1]))
        return raw, raw_start, info

    def add(self, info):
        """the verdict of one call from its info on the host: RuntimeError on a fault; the counters are added; returns (index of the
        first record of the call whose name is too long or -1, the same for a quality line that is not as long as its sequence)"""
        if int(info[3]):
            raise RuntimeError("device BAM encode: the chunk's record tables do not describe its text, or the records do not fit their "
                               "bound (fault %d)" % int(info[3]))
        for j, k in enumerate(COUNTERS):
            self.counts[k] += int(info[4 + j])
        if self.tags:
            self.malformed_records += int(info[8])
            self.float_values_skipped += int(info[9])
            for j in range(len(self.tags)):
                self.copied[j] += int(info[TAG_INFO + j])
        return int(info[2]), int(info[7])

    def tag_counts(self):
        return {"copied": list(self.copied), "malformed_records": self.malformed_records, "float_values_skipped": self.float_values_skipped}


def to_json(counts_per_mate):
    """the "ubam_output" object of the summary: the counters summed over the mates' files"""
    return {k: sum(int(c[k]) for c in counts_per_mate) for k in COUNTERS}


def log_line(counts_per_mate):
    doc = to_json(counts_per_mate)
    return "BAM records from text: {} bases changed, {} qualities clamped, {} names starred".format(*(doc[k] for k in COUNTERS))


def to_json_tags(tags, counts_per_mate, floats=False):
    """the "ubam_tags" object of the summary: counts_per_mate = [tag_counts()] of a single-end or interleaved run, [mate 1's, mate
    2's] of a two-file run (every count is then a pair). floats (--ubam_tag_floats): "float_rounding" as the last key"""
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
        doc["float_rounding"] = "nearest-even"
    return doc


def log_line_tags(tags, counts_per_mate):
    """'BAM tags from text: MM N, ML N copied; X records with malformed tags, Y float values skipped' - the mates' counts summed"""
    names = [bytes(t).decode() for t in tags]
    copied = [sum(int(c["copied"][j]) for c in counts_per_mate) for j in range(len(names))]
    return "BAM tags from text: {} copied; {} records with malformed tags, {} float values skipped".format(
        ", ".join("{} {}".format(t, n) for t, n in zip(names, copied)), sum(int(c["malformed_records"]) for c in counts_per_mate),
        sum(int(c["float_values_skipped"]) for c in counts_per_mate))
