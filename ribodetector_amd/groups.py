"""Counters per BAM read group (`--summary PATH --read_groups`): units and bases per class for every '@RG' the header of mate 1's BAM
declares, plus three rows for the records without an RG tag, with an RG no line declares and with malformed tags. Counted on the device
chunk by chunk over the chunks' raw records (DeviceChunk.raw): C ABI rd_bam_tag_find / rd_bam_group_rows / rd_bam_group_accumulate,
csrc/rd_bam_tags.hpp; the rule is bam.py (find_tag, read_groups, group_row).

The device's dictionary holds the declared ids SORTED as unsigned bytes (bam.sorted_ids), so the accumulator's rows are in sorted order:
acc = int64[(G + 3) * 6 + 1] = [row][class][units, bases] and one last word, the pairs whose mate 2 lands in another row than mate 1.
Rows G, G + 1, G + 2 = none / undeclared / malformed. to_json maps the rows back to header order. A pair is counted in MATE 1's row.
"""
import numpy as np
import torch

from . import _native as N
from . import bam

TAG = b"RG"
CLASSES = ("unclassified", "nonrRNA", "rRNA")        # class 0, 1, 2 = label -1, 0, 1
FIELDS = ("SM", "BC", "LB", "PL")                    # the @RG fields a group's entry repeats (null when the line has none)


def acc_words(G):
    return (int(G) + 3) * 6 + 1


def check_groups(header_bytes):
    """bam.read_groups(header_bytes) with the limits of a run: RuntimeError for a header whose @RG lines are not a dictionary (no ID, an
    empty or a duplicate ID) or that declares more than 65,536 groups. Pure host code."""
    try:
        groups = bam.read_groups(header_bytes)
    except ValueError as e:
        raise RuntimeError("--read_groups: {} (checked before anything touches a device)".format(e))
    if len(groups) > N.GROUPS_MAX:
        raise RuntimeError("--read_groups: the header declares {} read groups, more than {} (checked before anything touches a "
                           "device)".format(len(groups), N.GROUPS_MAX))
    return groups


def tag_find(raw, raw_start, n_rec, tag):
    """(val_off int64[n_rec], val_len int32[n_rec], val_type uint8[n_rec]) of the first tag `tag` of every record of a raw view (raw
    uint8 device tensor, raw_start int64[n_rec + 1]): bam.find_tag of every record, on the current stream"""
    tag, n_rec = bytes(tag), int(n_rec)
    if len(tag) != 2:
        raise ValueError("tag_find: a tag has 2 bytes")
    if raw.dtype != torch.uint8 or raw_start.dtype != torch.int64 or not raw.is_contiguous() or not raw_start.is_contiguous() or raw_start.numel() < n_rec + 1:
        raise TypeError("tag_find: raw uint8[*] and raw_start int64[n_rec + 1], contiguous")
    dev = raw.device
    vo = torch.empty(n_rec, dtype=torch.int64, device=dev)
    vl = torch.empty(n_rec, dtype=torch.int32, device=dev)
    vt = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().rd_bam_tag_find(N.ptr(raw), int(raw.numel()), N.ptr(raw_start), n_rec, tag, N.ptr(vo), N.ptr(vl), N.ptr(vt), N.stream_ptr(dev)),
                "rd_bam_tag_find")
    return vo, vl, vt


class Dictionary:
    """the declared ids on the device: sorted (bam.sorted_ids), behind one another, with the table of their starts"""

    def __init__(self, device, ids):
        self.device = torch.device(device)
        self.sorted, self.order = bam.sorted_ids(ids)
        self.G = len(self.sorted)
        if self.G > N.GROUPS_MAX:
            raise ValueError("a dictionary holds at most %d read groups" % N.GROUPS_MAX)
        off = np.zeros(self.G + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(s) for s in self.sorted], dtype=np.int64)
        data = np.frombuffer(b"".join(self.sorted) + b"\0", dtype=np.uint8).copy()          # (never empty: a tensor of no bytes has no pointer)
        self.bytes = torch.from_numpy(data).to(self.device)
        self.off = torch.from_numpy(off).to(self.device)

    def rows(self, raw, val_off, val_len, val_type):
        """rows int32[n_rec] (bam.group_row over the SORTED ids) from the tables of tag_find(raw, ..., b"RG")"""
        n_rec = int(val_off.numel())
        rows = torch.empty(n_rec, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().rd_bam_group_rows(N.ptr(raw), N.ptr(val_off), N.ptr(val_len), N.ptr(val_type), n_rec, N.ptr(self.bytes), N.ptr(self.off), self.G,
                                              N.ptr(rows), N.stream_ptr(self.device)), "rd_bam_group_rows")
        return rows


def accumulate(acc, G, labels, view_a, view_b=None):
    """acc += the units of one chunk (C ABI rd_bam_group_accumulate). view_x = (raw, raw_start, rows, first, stride) of a mate; view_b
    None: single-end. labels int8[n]. Returns info int64[4] on the device: info[0] != 0 = NOTHING was added."""
    n = int(labels.numel())
    if labels.dtype not in (torch.int8, torch.uint8) or not labels.is_contiguous():
        raise TypeError("groups.accumulate: labels must be a contiguous int8 / uint8 tensor")
    if acc.dtype != torch.int64 or acc.numel() != acc_words(G) or not acc.is_contiguous():
        raise TypeError("groups.accumulate: acc is int64[(G + 3) * 6 + 1]")
    for v in (view_a, view_b):
        if v is None:
            continue
        raw, rs, rows, first, stride = v
        need = 0 if n == 0 else int(first) + int(stride) * (n - 1) + 1
        if raw.dtype != torch.uint8 or rs.dtype != torch.int64 or rows.dtype != torch.int32 or not rs.is_contiguous() or not rows.is_contiguous() or \
                first < 0 or stride < 1 or rs.numel() < need or rows.numel() < need:
            raise TypeError("groups.accumulate: a mate is (raw uint8[*], raw_start int64[>= records], rows int32[>= records], first >= 0, stride >= 1)")
    dev = acc.device
    info = torch.empty(4, dtype=torch.int64, device=dev)       # (zeroed by the call)
    ra, sa, wa, fa, ta = view_a
    rb, sb, wb, fb, tb = view_b if view_b is not None else (None, None, None, 0, 1)
    with torch.cuda.device(dev):
        N.check(N.lib().rd_bam_group_accumulate(N.ptr(ra), N.ptr(sa), N.ptr(wa), int(fa), int(ta), N.ptr(rb), N.ptr(sb), N.ptr(wb), int(fb), int(tb),
                                                N.ptr(labels), n, int(G), N.ptr(acc), N.ptr(info), N.stream_ptr(dev)), "rd_bam_group_accumulate")
    return info


class DeviceGroups:
    """add(chunks, labels, interleaved): acc += the units of one chunk, counted per read group. chunks = the chunk of every input file
    (DeviceChunk with .raw: the reader ran with keep_raw), labels int8[n] of the units; interleaved: ONE chunk whose records 2 u and
    2 u + 1 are unit u's mates. Two files: mate 2's values are looked up in mate 1's dictionary. Returns info int64[4] on the device
    (info[0] != 0: nothing was added). Asynchronous on the current stream; the caller keeps the chunks alive until the stream has passed
    the call. result(): the int64 numpy array, rows in SORTED order (to_json maps them back)."""

    def __init__(self, device, header_bytes):
        self.device = torch.device(device)
        self.groups = check_groups(header_bytes)
        self.dict = Dictionary(self.device, [g[0] for g in self.groups])
        self.G = self.dict.G
        self.acc = torch.zeros(acc_words(self.G), dtype=torch.int64, device=self.device)

    def rows(self, raw, raw_start, n_rec):
        return self.dict.rows(raw, *tag_find(raw, raw_start, n_rec, TAG))

    def add(self, chunks, labels, interleaved=False, rows_a=None):
        """rows_a: the rows of mate 1's chunk where the caller has them already (rows(*chunks[0].raw, records))"""
        n = int(labels.numel())
        views = []
        for k, c in enumerate(chunks):
            if c.raw is None:
                raise RuntimeError("DeviceGroups.add: the chunk carries no raw records (the reader must run with keep_raw)")
            raw, rs = c.raw
            n_rec = int(rs.numel()) - 1
            if n_rec < (2 * n if interleaved else n):
                raise RuntimeError("DeviceGroups.add: the chunk holds %d raw records for %d units" % (n_rec, n))
            views.append((raw, rs, rows_a if k == 0 and rows_a is not None else self.rows(raw, rs, n_rec)))
        if interleaved:
            a, b = views[0] + (0, 2), views[0] + (1, 2)
        else:
            a, b = views[0] + (0, 1), (views[1] + (0, 1) if len(views) > 1 else None)
        return accumulate(self.acc, self.G, labels, a, b)

    def result(self):
        return self.acc.cpu().numpy()


def _counts(a):
    total = int(a[0] + a[1] + a[2])
    return {"total": total, "nonrRNA": int(a[1]), "rRNA": int(a[2]), "unclassified": int(a[0]),
            "rRNA_fraction": round(int(a[2]) / total, 6) if total else None}


def to_json(acc, groups, paired, input=None):
    """the "read_groups" object of the summary from an accumulator (rows in sorted order) and groups = bam.read_groups(header), which
    gives the order of the entries. Pure host code."""
    ids = [g[0] for g in groups]
    G = len(ids)
    acc = np.asarray(acc, dtype=np.int64)
    if acc.shape != (acc_words(G),):
        raise ValueError("the accumulator of %d read groups has %d words; got shape %r" % (G, acc_words(G), acc.shape))
    rows = acc[:-1].reshape(G + 3, 3, 2)
    _, order = bam.sorted_ids(ids)
    where = {h: j for j, h in enumerate(order)}      # header index -> sorted row

    def row(j):
        return {"units": _counts(rows[j, :, 0]), "bases": _counts(rows[j, :, 1])}
    doc = {"tag": TAG.decode(), "input": input, "groups": []}
    for h, (rid, fields) in enumerate(groups):
        entry = {"id": rid.decode("latin-1")}
        for f in FIELDS:
            entry[f] = fields.get(f)
        entry.update(row(where[h]))
        doc["groups"].append(entry)
    doc["none"], doc["undeclared"], doc["malformed_tags"] = row(G), row(G + 1), row(G + 2)
    if paired:
        doc["mate2_differs"] = int(acc[-1])
    return doc


def units_per_class(acc, G):
    """[unclassified, nonrRNA, rRNA] units summed over all rows: what the run's own counts must equal"""
    return [int(x) for x in np.asarray(acc, dtype=np.int64)[:-1].reshape(int(G) + 3, 3, 2)[:, :, 0].sum(0)]
