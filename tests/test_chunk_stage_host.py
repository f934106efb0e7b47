"""The per-chunk stage of the CLI on the host (no GPU, no model): the record-view rule of detect.record_view against the selection
written out directly, in every layout and for both kinds of source, and the order in which collect_chunk runs a ticket's checks."""
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
