"""FASTQ / FASTA input written as unaligned BAM (`--ubam_output`): the RAW view of a chunk that did not come from a BAM file - its
records as BAM records, made on the device from the chunk's text and tables (DeviceChunk.dev): C ABI rd_bam_encode,
csrc/rd_bam_encode.hpp. The rule is bam.py (from_fastq, ubam_name, UBAM_HEADER_TEXT). The raw bytes have a bound linear in the text
(bam.ubam_bound), so the buffer is sized without a hint, the call is made once and nothing waits for it.
"""
import torch

from . import _native as N
from . import bam

INFO_WORDS = 8
COUNTERS = ("bases_changed", "quals_clamped", "names_starred")      # info[4], [5], [6]


def flags_word(n_mates=1, mate=0, fasta=False):
    """the flags of rd_bam_encode: single-end (4, 4); a mate's file (77, 77) / (141, 141); mate = bam.INTERLEAVED: (77, 141)"""
    if mate == bam.INTERLEAVED:
        even, odd = bam.UBAM_FLAGS[(2, 0)], bam.UBAM_FLAGS[(2, 1)]
    else:
        even = odd = bam.UBAM_FLAGS[(int(n_mates), int(mate))]
    return (N.UBAM_FASTA if fasta else 0) | (even << N.UBAM_EVEN_SHIFT) | (odd << N.UBAM_ODD_SHIFT)


def encode(text, rec_start, seq_off, seq_len, n_rec, flags, raw_cap=None, raw=None, rec_first=0, rec_stride=1, text_bytes=None):
    """one call of rd_bam_encode on the current stream: (raw, raw_start int64[n_rec + 1], info int64[8]), all on the device. raw: a
    uint8 buffer of at least raw_cap bytes (made here when None; raw_cap None: the bound of bam.ubam_bound). Asynchronous."""
    n_rec = int(n_rec)
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
    info = torch.empty(INFO_WORDS, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.rd_bam_encode_workspace_bytes(n_rec)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.rd_bam_encode(N.ptr(text), text_bytes, N.ptr(rec_start), N.ptr(seq_off), N.ptr(seq_len), n_rec, int(rec_first), int(rec_stride),
                                  int(flags), N.ptr(raw), raw_cap, N.ptr(raw_start), N.ptr(info), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "rd_bam_encode")
    return raw, raw_start, info


class DeviceUbam:
    """encode(chunk, mate, n_mates) -> (raw, raw_start, info): the raw view of a DeviceChunk of FASTQ (fasta: FASTA) records, all
    three on the device; mate = bam.INTERLEAVED for an interleaved chunk. Nothing waits: info (rd_bam_encode's int64[8]) is read by
    whoever has waited for an event behind the call - add(info) then sums its counters and says which record, if any, cannot be a
    BAM record."""

    def __init__(self, device, fasta=False):
        self.device = torch.device(device)
        self.fasta = bool(fasta)
        self.counts = dict.fromkeys(COUNTERS, 0)

    def encode(self, chunk, mate=0, n_mates=1):
        text, so, sl, rs = chunk.dev
        return encode(text, rs, so, sl, int(rs.numel()) - 1, flags_word(n_mates, mate, self.fasta))

    def add(self, info):
        """the verdict of one call from its info on the host: RuntimeError on a fault; the counters are added; returns (index of the
        first record of the call whose name is too long or -1, the same for a quality line that is not as long as its sequence)"""
        if int(info[3]):
            raise RuntimeError("device BAM encode: the chunk's record tables do not describe its text, or the records do not fit their "
                               "bound (fault %d)" % int(info[3]))
        for j, k in enumerate(COUNTERS):
            self.counts[k] += int(info[4 + j])
        return int(info[2]), int(info[7])


def to_json(counts_per_mate):
    """the "ubam_output" object of the summary: the counters summed over the mates' files"""
    return {k: sum(int(c[k]) for c in counts_per_mate) for k in COUNTERS}


def log_line(counts_per_mate):
    doc = to_json(counts_per_mate)
    return "BAM records from text: {} bases changed, {} qualities clamped, {} names starred".format(*(doc[k] for k in COUNTERS))
