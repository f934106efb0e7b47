"""The run summary (`--summary`): per-run QC counters accumulated on the device chunk by chunk (C ABI rd_summary_accumulate,
csrc/rd_summary.hpp) and written by rank 0 as one JSON file when the run has ended well.

A unit is a read (single-end) or a pair; class c = label + 1 (0 unclassified, 1 nonrRNA, 2 rRNA) of the unit; mate m = 0 / 1. The
accumulator is ONE int64 array whose sections LAYOUT names (the RD_SUM_* constants of include/ribodetector_amd.h); integer sums, so
the result does not depend on the chunking, the ingest path or the number of ranks.
"""
import json

import numpy as np
import torch

from . import _native as N

FORMAT = "ribodetector-summary/1"
LEN_BINS, P_BINS, GC_BINS = 513, 100, 101            # RD_SUM_LEN_BINS / RD_SUM_P_BINS / RD_SUM_GC_BINS
# section -> (offset, shape) in the int64 accumulator: RD_SUM_<SECTION>, and RD_SUM_WORDS behind the last one
LAYOUT = {
    "units": (0, (3,)),                              # units per final label
    "mate_labels": (3, (3, 2, 2)),                   # pairs by class, argmax of mate 1's logits, of mate 2's
    "length": (15, (2, 3, LEN_BINS)),                # reads by mate, class, min(seq_len, 512)
    "p_rrna": (3093, (3, 3, P_BINS)),                # source (mate 1, mate 2, pair) x class x min(q / 100, 99)
    "bases": (3993, (2, 3, 5)),                      # bases by mate, class, code: A C G T(U) other
    "gc": (4023, (2, 3, GC_BINS)),                   # reads by mate, class, 100 (C + G) / (A + C + G + T)
}
WORDS = 4629
CLASSES = ("unclassified", "nonrRNA", "rRNA")        # class 0, 1, 2 = label -1, 0, 1
BASES = ("A", "C", "G", "T", "other")


def sections(acc):
    """{section: view of acc with the section's shape}"""
    acc = np.asarray(acc)
    if acc.shape != (WORDS,):
        raise ValueError("a summary accumulator has %d words; got shape %r" % (WORDS, acc.shape))
    return {k: acc[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in LAYOUT.items()}


class DeviceSummary:
    """add(dev_in_a, logits_a, dev_in_b, logits_b, labels): acc += the counters of one chunk. dev_in_x = (text uint8[*], seq_off
    int64[n], seq_len int32[n]) of one mate as rd_classify takes them, logits_x fp32[n, 2], labels int8[n]; dev_in_b / logits_b None =
    single-end. Returns info int64[4] on the device: info[0] != 0 = the chunk's tables were bad and NOTHING was added. Asynchronous on
    the current stream; the caller keeps the tensors alive until the stream has passed the call. result(): the int64 numpy array."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.acc = torch.zeros(int(N.lib().rd_summary_words()), dtype=torch.int64, device=self.device)

    def add(self, dev_in_a, logits_a, dev_in_b, logits_b, labels):
        n = int(labels.numel())
        if labels.dtype not in (torch.int8, torch.uint8) or not labels.is_contiguous():
            raise TypeError("DeviceSummary.add: labels must be a contiguous int8 / uint8 tensor")
        if (dev_in_b is None) != (logits_b is None):
            raise TypeError("DeviceSummary.add: mate 2 takes both its tables and its logits, or neither")
        for din, lg in ((dev_in_a, logits_a), (dev_in_b, logits_b)):
            if din is None:
                continue
            text, off, ln = din
            if text.dtype != torch.uint8 or not text.is_contiguous():
                raise TypeError("DeviceSummary.add: text must be a contiguous uint8 tensor")
            if off.dtype != torch.int64 or ln.dtype != torch.int32 or min(off.numel(), ln.numel()) < n or not off.is_contiguous() or not ln.is_contiguous():
                raise TypeError("DeviceSummary.add: seq_off int64[n] and seq_len int32[n], contiguous")
            if lg.dtype != torch.float32 or not lg.is_contiguous() or lg.numel() < 2 * n:
                raise TypeError("DeviceSummary.add: logits must be contiguous fp32 [n, 2] tensors")
        info = torch.empty(4, dtype=torch.int64, device=self.device)       # (zeroed by the call)
        ta, oa, la = dev_in_a
        tb, ob, lb = dev_in_b if dev_in_b is not None else (None, None, None)
        with torch.cuda.device(self.device):
            N.check(N.lib().rd_summary_accumulate(N.ptr(ta), int(ta.numel()), N.ptr(oa), N.ptr(la), N.ptr(logits_a),
                                                  N.ptr(tb), 0 if tb is None else int(tb.numel()), N.ptr(ob), N.ptr(lb), N.ptr(logits_b),
                                                  N.ptr(labels), n, N.ptr(self.acc), N.ptr(info), N.stream_ptr(self.device)), "rd_summary_accumulate")
        return info

    def result(self):
        return self.acc.cpu().numpy()


def to_json(acc, meta):
    """the summary document (a dict) of an accumulator; meta: version, paired, interleaved, len, ensure, model, inputs
    and, under --windows, windows = {stride, max_per_read, fuse, classified}. Pure host code."""
    s = sections(np.asarray(acc, dtype=np.int64))
    paired = bool(meta["paired"])
    units = [int(x) for x in s["units"]]
    total = sum(units)
    sources = ["mate1", "mate2", "pair"] if paired else ["mate1"]
    mates = sources[:2]

    def by_class(a):
        return {c: [int(x) for x in a[k]] for k, c in enumerate(CLASSES)}
    doc = {"format": FORMAT}
    for k in ("version", "paired", "interleaved", "len", "ensure", "model", "inputs"):
        doc[k] = meta[k]
    doc["reads"] = {"total": total, "nonrRNA": units[1], "rRNA": units[2], "unclassified": units[0],
                    "rRNA_fraction": round(units[2] / total, 6) if total else None}
    if paired:
        doc["mate_labels"] = {c: s["mate_labels"][k].tolist() for k, c in enumerate(CLASSES)}
    doc["length"] = dict({"overflow_from": LEN_BINS - 1}, **{m: by_class(s["length"][e]) for e, m in enumerate(mates)})
    doc["p_rrna"] = dict({"bin_width": 1.0 / P_BINS}, **{m: by_class(s["p_rrna"][e]) for e, m in enumerate(sources)})
    doc["bases"] = {m: {c: dict(zip(BASES, (int(x) for x in s["bases"][e][k]))) for k, c in enumerate(CLASSES)} for e, m in enumerate(mates)}
    doc["gc"] = {m: by_class(s["gc"][e]) for e, m in enumerate(mates)}
    # reads longer than -l, which the model saw truncated. Bin 512 holds the reads of 512 bases AND longer, so the count can be told
    # from the histogram only while -l lies below that bin
    ln = int(meta["len"])
    doc["truncated_reads"] = int(s["length"][:len(mates), :, ln + 1:].sum()) if 0 <= ln < LEN_BINS - 1 else None
    # --windows only: the settings, and the windows classified per mate (the reads above were then classified over their whole length;
    # truncated_reads keeps its meaning, the reads longer than -l)
    if meta.get("windows") is not None:
        doc["windows"] = dict(meta["windows"])
    return doc


def write_json(path, doc):
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
