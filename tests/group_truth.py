"""Outputs per read group, stated plainly: what rd_group_keys, rd_group_pack and rd_gz_compress_grouped (csrc/rd_group_pack.hpp) and
the CLI's --split_groups have to produce, in loops a reader can check by eye. The tests hold the device and the run to this file,
and tests/test_split_groups_host.py holds this file to itself."""
from ribodetector_amd import bam


def keys(rows, labels, class_slot, G, first=0, stride=1, mate=-1):
    """rd_group_keys: unit u is entry first + stride * u of `rows` (0 .. G + 2) with label labels[u] (-1, 0, 1); class_slot[label + 1] is
    the index of that class's family among the mate's file sets, or -1. key = slot * (G + 1) + min(row, G), or -1. mate = -1: a key per
    unit; mate = 0 / 1: a key per RECORD of an interleaved chunk - record 2u + mate gets the unit's, the other mate's record -1.
    Returns (keys, flags): flags bit 0 = a label outside -1..1, bit 1 = a row outside 0..G + 2 (such units get -1)."""
    out, flags = [], 0
    for u, lab in enumerate(labels):
        row, key = int(rows[first + stride * u]), -1
        bad = (1 if lab < -1 or lab > 1 else 0) | (2 if row < 0 or row > G + 2 else 0)
        flags |= bad
        if not bad and class_slot[lab + 1] >= 0:
            key = class_slot[lab + 1] * (G + 1) + min(row, G)
        if mate < 0:
            out.append(key)
        else:
            pair = [-1, -1]
            pair[mate] = key
            out.extend(pair)
    return out, flags


def partition(text, rec_start, keys, K):
    """rd_group_pack: for every key 0 .. K - 1 the records that carry it, in input order, joined: [(bytes, records)] of K entries"""
    text = bytes(text)
    runs = [[] for _ in range(K)]
    for i, k in enumerate(keys):
        if k >= 0:
            runs[k].append(text[rec_start[i]:rec_start[i + 1]])
    return [(b"".join(r), len(r)) for r in runs]


def layout(runs, align=16):
    """where rd_group_pack puts the runs: every run starts on the next multiple of `align` behind the run before it. Returns
    ([offset per key], bytes of `out` in use = the end of the last run that holds a byte)"""
    offs, at, need = [], 0, 0
    for data, _ in runs:
        offs.append(at)
        if data:
            need = at + len(data)
        at += -(-len(data) // align) * align
    return offs, need


def group_rows(data, ids, start=None):
    """the row of every delivered record of `data` among the ids of its header, SORTED as the device's dictionary is (bam.sorted_ids)"""
    data = bytes(data)
    srt, _ = bam.sorted_ids(ids)
    rows = []
    for r in bam.records(data, start):
        if not r.skipped:
            rows.append(bam.group_row(data, *bam.find_tag(data, r.offset, b"RG"), srt))
    return rows


def split_select(data, labels, ids, label, source="fastq", tags=None, floats=False, first=0, stride=1, mate=None, rows=None):
    """--split_groups: the bytes of every member of ONE family - the file of class `label` - for the BAM file `data` (inflated) and the
    unit labels. Unit u is delivered record first + stride * u; its member is the row of THAT record (mate 1's) with rows G .. G + 2
    folded into the last one. mate = None: a unit's bytes are its stride consecutive records (one file for both mates, or single-end);
    mate = m: only record first + stride * u + m (the file of one mate of an interleaved input). source: "fastq" (verbatim text),
    "tagged" (--bam_tags: `tags`, `floats`) or "raw" (--bam_output). rows: the rows of MATE 1's file where `data` is mate 2's (two input
    files: mate 2's own RG is not consulted). Returns G + 1 byte strings in SORTED-id order, unassigned last."""
    data = bytes(data)
    G = len(ids)
    delivered = [r for r in bam.records(data) if not r.skipped]
    rows = group_rows(data, ids) if rows is None else rows
    if source == "raw":
        rec = [data[r.offset:r.offset + r.size] for r in delivered]
    elif source == "tagged":
        rec = []
        for r in delivered:
            text = r.fastq()
            at = text.index(b"\n")
            rec.append(text[:at] + bam.tag_comment(data, r.offset, tags, floats)[0] + text[at:])
    else:
        rec = [r.fastq() for r in delivered]
    members = [[] for _ in range(G + 1)]
    for u, lab in enumerate(labels):
        if lab != label:
            continue
        at = first + stride * u
        piece = rec[at + mate] if mate is not None else b"".join(rec[at:at + stride])
        members[min(rows[at], G)].append(piece)
    return [b"".join(m) for m in members]
