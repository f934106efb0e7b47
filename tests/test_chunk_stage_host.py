"""The per-chunk stage of the CLI on the host (no GPU, no model): the record-view rule of detect.record_view against the selection
written out directly, in every layout and for both kinds of source, the order in which collect_chunk runs a ticket's checks, and the
jobs a mate's writer makes of a chunk's pieces."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from ribodetector_amd import detect
from ribodetector_amd.data_loader import fastx_parser as fx
from ribodetector_amd.ticket import CHECK_ORDER, Ticket

PAIRS = 5
PAIR_LABELS = np.array([0, 1, -1, 1, 0], dtype=np.int8)                  # one label per pair (interleaved layouts)
RECORD_LABELS = np.array([1, 0, 0, -1, 1, -1, 0, 1, 1, 0], dtype=np.int8)     # one label per record (two input files)
LABELS = (0, 1, -1, 3)                                                    # 3: the label of no unit - the empty selection


def _source(lengths, seed):
    """records of the given lengths (distinct bytes, so that no two selections are equal by chance), their text and record table"""
    rng = np.random.default_rng(seed)
    recs = [rng.integers(33, 127, size=n, dtype=np.uint8).tobytes() for n in lengths]
    table = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return recs, (torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()), torch.from_numpy(table))


# the FASTQ text of 5 pairs and a raw text over the same 10 records whose records have other lengths (BAM records, tagged text)
SOURCES = {"fastq": _source([41, 44, 47, 53, 59, 62, 68, 71, 77, 83], 1), "raw": _source([90, 31, 36, 72, 55, 97, 34, 64, 49, 80], 2)}


def _select(text, table, labels, lab):
    """what compress_selected / pack_selected take of (text, table, labels) for one label"""
    text, table, labels = (np.asarray(x) for x in (text, table, labels))
    keep = np.flatnonzero(labels == lab)
    return b"".join(text[table[k]:table[k + 1]].tobytes() for k in keep)


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_record_view_two_files(name):
    recs, source = SOURCES[name]
    labels = torch.from_numpy(RECORD_LABELS)
    text, table, sel = detect.record_view(source, len(recs), labels, 0)
    assert text is source[0] and table is source[1] and sel is labels          # nothing is copied
    for lab in LABELS:
        assert _select(text, table, sel, lab) == b"".join(recs[k] for k in range(len(recs)) if RECORD_LABELS[k] == lab)
    assert _select(text, table, sel, 3) == b""


@pytest.mark.parametrize("precomputed", [False, True])
@pytest.mark.parametrize("name", sorted(SOURCES))
def test_record_view_interleaved_one_output(name, precomputed):
    """pair k = records 2 k and 2 k + 1 together; the table of the pairs is the one the source has already, where it has one"""
    recs, source = SOURCES[name]
    labels = torch.from_numpy(PAIR_LABELS)
    pair_table = source[1][0:2 * PAIRS + 1:2].contiguous() if precomputed else None
    text, table, sel = detect.record_view(source, PAIRS, labels, 0, interleaved=True, outs=1, pair_table=pair_table)
    assert text is source[0] and sel is labels and table.numel() == PAIRS + 1 and table.is_contiguous()
    assert not precomputed or table is pair_table
    for lab in LABELS:
        assert _select(text, table, sel, lab) == b"".join(recs[2 * k] + recs[2 * k + 1] for k in range(PAIRS) if PAIR_LABELS[k] == lab)
    assert _select(text, table, sel, 3) == b""


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_record_view_interleaved_two_outputs(name):
    """mate e's file: records 2 k + e of the pairs with the label, over the full table, by the host's own label expansion"""
    recs, source = SOURCES[name]
    labels = torch.from_numpy(PAIR_LABELS)
    for e in (0, 1):
        text, table, sel = detect.record_view(source, PAIRS, labels, e, interleaved=True, outs=2, expand=fx.expand_pair_labels)
        assert text is source[0] and table is source[1] and len(sel) == 2 * PAIRS
        for lab in LABELS:
            assert _select(text, table, sel, lab) == b"".join(recs[2 * k + e] for k in range(PAIRS) if PAIR_LABELS[k] == lab)
        assert _select(text, table, sel, 3) == b""


def test_labels_cover_the_cases():
    assert {0, 1, -1} <= set(PAIR_LABELS.tolist()) and {0, 1, -1} <= set(RECORD_LABELS.tolist())
    assert 3 not in PAIR_LABELS and 3 not in RECORD_LABELS


class _Fault(RuntimeError):
    pass


def _predictor(gathers):
    pred = detect.Predictor.__new__(detect.Predictor)          # (collect_chunk reads the layout and the rank, nothing else)
    pred.multi, pred.sharded_parse, pred.rank = gathers, False, 0
    assert pred.gathers_labels == gathers
    return pred


@pytest.mark.parametrize("gathers", [False, True])
@pytest.mark.parametrize("first, second", list(itertools.combinations(CHECK_ORDER, 2)))
def test_checks_run_in_one_order(monkeypatch, gathers, first, second):
    """two faults coincide: the one that comes first in totals, pairs, summary, groups, regions ends the run, in both layouts and
    whatever the order the side products registered in - and only after the chunk's event has been waited for"""
    assert CHECK_ORDER == ("totals", "pairs", "summary", "groups", "regions")
    waited = []
    monkeypatch.setattr(detect._native_mod, "wait_event", waited.append)

    def fail(name):
        assert waited == ["done"]
        raise _Fault(name)
    tk = Ticket(4, None, None, done="done", host=torch.zeros(4, dtype=torch.int8), finish=lambda: torch.zeros(4, dtype=torch.int8))
    for name in (second, first):
        tk.checks[name] = lambda name=name: fail(name)
    with pytest.raises(_Fault, match="^%s$" % first):
        _predictor(gathers).collect_chunk(tk)


@pytest.mark.parametrize("gathers", [False, True])
def test_collect_waits_where_it_must(monkeypatch, gathers):
    """no side product: the label gather's path has no host wait of its own; every other path waits once, and a passing check under
    the gather waits once too"""
    waited = []
    monkeypatch.setattr(detect._native_mod, "wait_event", waited.append)
    labels = torch.tensor([0, 1, -1, 1], dtype=torch.int8)
    tk = Ticket(4, None, None, done="done", host=labels, finish=lambda: labels)
    assert _predictor(gathers).collect_chunk(tk).tolist() == [0, 1, -1, 1]
    assert waited == ([] if gathers else ["done"])
    ran = []
    tk.checks["summary"] = lambda: ran.append("summary")
    assert _predictor(gathers).collect_chunk(tk).tolist() == [0, 1, -1, 1]
    assert ran == ["summary"] and waited == (["done"] if gathers else ["done", "done"])


class _File:
    """a writer's file handle that records (file key, method, what it was given): the bytes at the pointer, or the label"""

    def __init__(self, key, log):
        self.key, self.log = key, log

    def write_text(self, ptr, nb):
        self.log.append((self.key, "write_text", ctypes.string_at(ptr, nb)))

    def write_members(self, ptr, nb):
        self.log.append((self.key, "write_members", ctypes.string_at(ptr, nb)))

    def write_selected(self, chunk, labels, label):
        self.log.append((self.key, "write_selected", (chunk, labels, label)))


def _info(gz_bytes, text_bytes, fault=0):
    return torch.tensor([gz_bytes, text_bytes, 0, fault], dtype=torch.int64)


def _bytes(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8)


def _writer(keys):
    """mate 1's writer over files `keys` (no thread, no stream), the log its handles write, and its predictor's split counters"""
    log = []
    pred = detect.Predictor.__new__(detect.Predictor)
    pred._split_ids = ["rg1", "rg2"]                                # (two declared groups + the unassigned: three members per family)
    pred._split_recs = {(0, lab): np.zeros(3, dtype=np.int64) for lab in (0, 1)}
    w = detect._MateWriter.__new__(detect._MateWriter)
    w.pred, w.e, w.files = pred, 0, [(key, _File(key, log)) for key in keys]
    w.keys, w.handles = w._file_index(0, w.files)
    return w, log, pred


FAMILY = [(0, lab, g) for lab in (0, 1) for g in range(3)]
LABEL_FILES = [(0, 10), (0, 11), (0, 12), (0, 13)]
# a grouped call's text over 2 labels x 3 members: runs on multiples of 16, keys 1 and 4 without a record
GROUP_BUF = b"key0 bytes......" + b"key two" + b"." * 9 + b"k3" + b"." * 14 + b"the last key"
GROUP_TAB = [[0, 16, 2, 0], [16, 0, 0, 0], [16, 7, 1, 0], [32, 2, 1, 0], [48, 0, 0, 0], [48, 12, 3, 0]]


def _grouped(kinfo=0, fault=0):
    return detect.Piece(_bytes(GROUP_BUF), _info(0, 60, fault), True, key_tab=torch.tensor(GROUP_TAB, dtype=torch.int64), kinfo=_info(kinfo, 8),
                        labels=(0, 1))


def test_the_writers_jobs_for_a_chunk():
    """one mate, one item: a label piece that fits; gzip members that do not fit their buffer, with the text as fallback; the same
    without a fallback and a file without a piece, whose records the host writes; a grouped piece over 2 labels x 3 members with two
    empty keys. The jobs are the grouped piece's runs, then the files' in file order; the grouped table's records reach the counters."""
    w, log, pred = _writer(FAMILY + LABEL_FILES)
    fits = _info(0, 9)
    fallback = detect.Piece(_bytes(b"the text of the chunk's report"), _info(0, 30), True, _info(0, 30), "report")
    too_big = _info(70, 0)
    pieces = {(0, detect.SPLIT): [_grouped()],
              (0, 10): [detect.Piece(_bytes(b"nine byte + slack"), fits, True, fits, "select")],
              (0, 11): [detect.Piece(_bytes(b"x" * 64), too_big, False, too_big, "report", fallback=fallback)],
              (0, 12): [detect.Piece(_bytes(b"x" * 64), too_big, False, too_big, "gzip")]}
    jobs = w._issue(("chunk", "labels", pieces), 0)
    assert log == [] and all(done is None for done, _ in jobs)      # (host buffers: nothing to fetch, nothing written yet)
    for _, write in jobs:
        write()
    host = ("chunk", "labels")
    assert log == [((0, 0, 0), "write_text", b"key0 bytes......"), ((0, 0, 2), "write_text", b"key two"), ((0, 1, 0), "write_text", b"k3"),
                   ((0, 1, 2), "write_text", b"the last key"),
                   ((0, 10), "write_text", b"nine byte"), ((0, 11), "write_text", b"the text of the chunk's report"),
                   ((0, 12), "write_selected", host + (12,)), ((0, 13), "write_selected", host + (13,))]
    records = np.array(GROUP_TAB)[:, 2]
    assert pred._split_recs[(0, 0)].tolist() == records[:3].tolist() and pred._split_recs[(0, 1)].tolist() == records[3:].tolist()
    # members instead of text: the same runs through write_members
    w, log, _ = _writer(FAMILY)
    for _, write in w._issue(("chunk", "labels", {(0, detect.SPLIT): [_grouped()._replace(text=False, info=_info(60, 0))]}), 0):
        write()
    assert [(key, how) for key, how, _ in log] == [(key, "write_members") for key in ((0, 0, 0), (0, 0, 2), (0, 1, 0), (0, 1, 2))]


@pytest.mark.parametrize("bad, message", [
    ({(0, detect.SPLIT): [_grouped(kinfo=2)]}, r"device group keys: a label or a read-group row of the chunk is outside its range \(flags 2\)"),
    ({(0, detect.SPLIT): [_grouped(fault=4)]},
     r"device group pack: the chunk's keys or record table do not describe its text, or the output did not fit \(fault 4\)"),
    ({(0, detect.SPLIT): [_grouped()._replace(text=False, info=_info(60, 0, 1))]},
     r"device group gzip: the chunk's keys or record table do not describe its text, or the output did not fit \(fault 1\)"),
    ({(0, 13): [detect.Piece(_bytes(b"x" * 64), _info(0, 9, 1), True, _info(0, 9, 1), "select")]},
     "device select: the chunk's record table does not describe its text")])
def test_a_faulty_piece_ends_the_item_before_any_write(bad, message):
    """the fault of a grouped call, of its keys, or of a label file's selection - the LAST file's, behind pieces that are fine - raises
    while the jobs are made: nothing of the item has been queued or written"""
    w, log, pred = _writer(FAMILY + LABEL_FILES)
    fine = _info(0, 9)
    pieces = {key: [detect.Piece(_bytes(b"nine byte + slack"), fine, True, fine, "select")] for key in LABEL_FILES[:3]}
    pieces.update(bad)
    with pytest.raises(RuntimeError, match="^%s$" % message):
        w._issue(("chunk", "labels", pieces), 0)
    assert log == [] and not any(r.any() for r in pred._split_recs.values())
