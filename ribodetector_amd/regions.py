"""The rRNA stretches of reads classified over windows (`--regions`, with `--windows`): the rule in pure Python / numpy - what the
tests compare the device's file with, and what the host side of the run needs (the header, the buffer hint). The device side is
csrc/rd_regions.hpp behind the C ABI rd_region_format; include/ribodetector_amd.h states the rule.

L = -l; W and start(j) = j (len - L) // (W - 1) are the window rule's (windows.py). Window j of a read is an rRNA window when its final
fp32 logits have l1 > l0 (a tie is not). It covers [start(j), start(j) + L) when W > 1 and [0, min(len, L)) when W == 1. A region is a
maximal run a..b of rRNA windows of one read: [start(a), start(b) + L) in 0-based bases of the read - when --max_windows caps the
windows, the unsampled bases between two rRNA windows belong to it; with a stride below L / 2 two regions of a read may overlap (they are
still in ascending start). A region of no bases (a read of 0 bases) is not written."""
import os

import numpy as np

from . import windows as W

HEADER = b"#read_id\tstart\tend\tmate\twindows\tp_rrna_max\n"
HINT_ENV = "RD_REGIONS_HINT"


def q_of(l0, l1):
    """q = rint(softmax([l0, l1])[1] * 1e4) in float64 from d = l1 - l0 taken in fp32: rp_q of csrc/rd_common.hpp, the value the
    per-read report prints (the package's one Python statement of it; the report's host test has the same for its own formatter)"""
    d = float(np.float32(l1) - np.float32(l0))
    e = np.exp(-abs(d))
    p = 1.0 / (1.0 + e) if d >= 0 else e / (1.0 + e)
    return int(np.rint(p * 1e4))


def fmt_q(q):
    """q as the report prints it: 0.dddd or 1.0000"""
    return b"1.0000" if q >= 10000 else b"0.%04d" % q


def regions_of(length, L, w_labels):
    """[(start, end, first window, last window)] of a read of `length` bases whose windows have the truth values w_labels (rRNA or
    not), in ascending start; Python integers"""
    length, L, n = int(length), int(L), len(w_labels)
    if n == 1:
        end = min(length, L)
        return [(0, end, 0, 0)] if w_labels[0] and end > 0 else []
    starts = W.starts(length, L, n)
    out, a = [], None
    for j in range(n + 1):
        if j < n and w_labels[j]:
            a = j if a is None else a
        elif a is not None:
            out.append((starts[a], starts[j - 1] + L, a, j - 1))
            a = None
    return out


def format_lines(ids, lens, win_first, win_logits, L, mate):
    """the lines (no header) of one mate's reads: a list with the bytes of every read's lines (b"" for a read without a region), so that
    the caller can interleave the mates of a pair. ids: the reads' id bytes; lens: their lengths; win_first int64[n + 1] and win_logits
    fp32[total, 2]: the window plan and the windows' final logits; mate: 1 or 2."""
    wl = np.asarray(win_logits, dtype=np.float32).reshape(-1, 2)
    first = np.asarray(win_first, dtype=np.int64)
    out = []
    for i, rid in enumerate(ids):
        f, e = int(first[i]), int(first[i + 1])
        w = wl[f:e]
        lines = []
        for s, t, a, b in regions_of(lens[i], L, (w[:, 1] > w[:, 0]).tolist()):
            q = max(q_of(w[j, 0], w[j, 1]) for j in range(a, b + 1))
            lines.append(b"%s\t%d\t%d\t%d\t%d\t%s\n" % (bytes(rid), s, t, int(mate), b - a + 1, fmt_q(q)))
        out.append(b"".join(lines))
    return out


def default_hint(text_bytes, n, total_windows, mates=1):
    """bytes reserved for a chunk's lines when RD_REGIONS_HINT is not set: a sixteenth of the text (rRNA is a minority of most inputs, and
    a line is shorter than a 100 bp record) plus 64 bytes per unit and 16 per window beyond one per unit - room for a line per read of
    short ids and for a good share of the windows of long reads. A chunk that needs more is formatted a second time with the exact size
    (fault 1 of rd_region_format)."""
    env = os.environ.get(HINT_ENV)
    if env:
        return max(16, int(env))
    units = int(n) * int(mates)
    return int(text_bytes) // 16 + 64 * units + 16 * max(0, int(total_windows) - units) + 4096
