"""--summary on the GPU: the accumulate kernels (rd_summary_accumulate through summary.DeviceSummary) against the numpy reference of
tests/test_summary_host.py and against the report kernel's q values, and the CLI's JSON against its own output files, its per-read
report, the input, the other ingest paths, chunk sizes and two ranks."""
import gzip
import json
import logging
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_read_report as R  # noqa: E402
import test_read_report_host as H  # noqa: E402
import test_summary_host as S  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("reads", "mate_labels", "length", "p_rrna", "bases", "gc", "truncated_reads")     # what of the JSON the counters decide


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
def _dev(text, off, lens):
    import torch
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    return t, torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to("cuda:0")


def _add(ds, mate_a, la, mate_b, lb, labels):
    """one DeviceSummary.add of host inputs; returns the host copy of info"""
    import torch
    info = ds.add(mate_a, torch.from_numpy(la).to("cuda:0"), mate_b, None if lb is None else torch.from_numpy(lb).to("cuda:0"),
                  torch.from_numpy(np.asarray(labels, dtype=np.int8)).to("cuda:0"))
    torch.cuda.synchronize()
    return info.cpu().numpy()


def _diff(got, want):
    """which sections differ (for the assertion message)"""
    return [k for k in S.views(got) if not (S.views(got)[k] == S.views(want)[k]).all()]


def _case(n, seed, paired, redraw=True, tails=(1, 15, 16, 17, 33, 600)):
    ta = S.make_text(n, seed, tails)
    tb = S.make_text(n, seed + 100, tails) if paired else None
    m = len(ta[2])
    la, lb = S.make_logits(m, seed + 7, paired, redraw)
    labels = np.random.default_rng(seed).integers(-1 if paired else 0, 2, m)
    return ta, tb, la, lb, labels


@pytest.mark.parametrize("paired", [False, True])
def test_kernel_against_reference(paired):
    from ribodetector_amd.summary import DeviceSummary
    ta, tb, la, lb, labels = _case(5000, 31 + paired, paired)
    for a, b in zip(S.bins_fp32(la, lb), S.bins_fp64(la, lb)):      # the chosen logits: fp32 and float64 give the same bins
        assert (a == b).all()
    assert ((ta[2] + ta[3]) == len(ta[0])).sum() >= 7                  # sequences that end on the text's last byte
    want = S.accumulate(S.seqs_of(ta[0], ta[2], ta[3]), la, S.seqs_of(tb[0], tb[2], tb[3]) if paired else None, lb, labels)
    ds = DeviceSummary("cuda:0")
    info = _add(ds, _dev(ta[0], ta[2], ta[3]), la, _dev(tb[0], tb[2], tb[3]) if paired else None, lb, labels)
    assert int(info[0]) == 0 and int(info[1]) == len(labels)
    got = ds.result()
    assert got.dtype == np.int64 and got.shape == (S.WORDS,)
    assert (got == want).all(), _diff(got, want)


@pytest.mark.parametrize("paired", [False, True])
def test_p_bins_against_the_report_kernel(paired):
    """the same inputs WITHOUT the redraw: the q values that rd_report_format prints, binned on the host, are the p_rrna section"""
    import torch
    from ribodetector_amd.gz import DeviceReport
    from ribodetector_amd.summary import DeviceSummary
    ta, tb, la, lb, labels = _case(5000, 41 + paired, paired, redraw=False, tails=())
    mate_a = _dev(ta[0], ta[2], ta[3])
    out, _, rinfo = DeviceReport("cuda:0").format(mate_a[0], torch.from_numpy(ta[1]).to("cuda:0"), torch.from_numpy(la).to("cuda:0"),
                                                  None if lb is None else torch.from_numpy(lb).to("cuda:0"), torch.from_numpy(labels.astype(np.int8)).to("cuda:0"))
    torch.cuda.synchronize()
    assert int(rinfo[3]) == 0
    _, rows = H.parse(b"#\n" + out[: int(rinfo[1])].cpu().numpy().tobytes())
    assert len(rows) == 5000
    want = np.zeros((3, 3, 100), dtype=np.int64)
    for (_, _, qs), lab in zip(rows, labels):
        for src, q in enumerate(qs):
            want[src, lab + 1, S.p_bin(q)] += 1
    ds = DeviceSummary("cuda:0")
    info = _add(ds, mate_a, la, _dev(tb[0], tb[2], tb[3]) if paired else None, lb, labels)
    assert int(info[0]) == 0
    assert (S.views(ds.result())["p_rrna"] == want).all()


def test_accumulation_and_shapes():
    import torch
    from ribodetector_amd.summary import DeviceSummary
    ds = DeviceSummary("cuda:0")
    total = np.zeros(S.WORDS, dtype=np.int64)
    for n, seed in ((1300, 51), (700, 52), (1, 53)):                   # two calls give the sum of two references; n = 1 works
        ta, tb, la, lb, labels = _case(n, seed, True, tails=(16,) if n > 1 else ())
        total += S.accumulate(S.seqs_of(ta[0], ta[2], ta[3]), la, S.seqs_of(tb[0], tb[2], tb[3]), lb, labels)
        info = _add(ds, _dev(ta[0], ta[2], ta[3]), la, _dev(tb[0], tb[2], tb[3]), lb, labels)
        assert int(info[0]) == 0 and int(info[1]) == len(labels)
        assert (ds.result() == total).all(), (n, _diff(ds.result(), total))
    # n = 0 changes nothing
    e64, e32 = torch.empty(0, dtype=torch.int64, device="cuda:0"), torch.empty(0, dtype=torch.int32, device="cuda:0")
    text = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    info = ds.add((text, e64, e32), torch.empty((0, 2), device="cuda:0"), None, None, torch.empty(0, dtype=torch.int8, device="cuda:0"))
    torch.cuda.synchronize()
    assert int(info[0]) == 0 and (ds.result() == total).all()


@pytest.mark.parametrize("n", [257, 70001])
def test_identical_reads_land_in_one_bin(n):
    """n identical pairs: every section gets all of them in ONE bin per mate / source - no narrow LDS counter may wrap"""
    from ribodetector_amd.summary import DeviceSummary
    s1, s2 = b"ACGTTGCANNACGGGCTTAACCGGTTAGCATCGA", b"TTTTUACGCGCGATATATAGCGCGCTAGCTAGCTAGCTAGCTAGGATC"
    text = b"@p/1\n" + s1 + b"\n+\n@p/2\n" + s2                        # (mate 2's sequence ends on the text's last byte)
    offs, lens = (5, len(text) - len(s2)), (len(s1), len(s2))
    la, lb = np.tile(np.float32([0.25, 1.75]), (n, 1)), np.tile(np.float32([-2.0, 0.5]), (n, 1))
    one = S.accumulate([s1], la[:1], [s2], lb[:1], [1])
    ds = DeviceSummary("cuda:0")
    info = _add(ds, _dev(text, np.full(n, offs[0]), np.full(n, lens[0])), la, _dev(text, np.full(n, offs[1]), np.full(n, lens[1])), lb, np.ones(n))
    assert int(info[0]) == 0
    got = ds.result()
    assert (got == n * one).all(), _diff(got, n * one)
    v = S.views(got)
    assert v["units"][2] == n and v["mate_labels"][2, 1, 1] == n and (v["length"] == n).sum() == 2 and (v["p_rrna"] == n).sum() == 3 and (v["gc"] == n).sum() == 2


def test_faulty_chunks_add_nothing():
    """bad table entries that the check pass must reject: the accumulate pass then reads nothing, and acc stays bit-identical"""
    from ribodetector_amd.summary import DeviceSummary
    ta, tb, la, lb, labels = _case(3000, 61, True, tails=())
    text, _, off, lens = ta
    ds = DeviceSummary("cuda:0")
    mate_b = _dev(tb[0], tb[2], tb[3])
    assert int(_add(ds, _dev(text, off, lens), la, mate_b, lb, labels)[0]) == 0
    before = ds.result().copy()
    assert before[:3].sum() == 3000
    bad_label = labels.copy()
    bad_label[1234] = 2
    neg_len = lens.copy()
    neg_len[77] = -1
    past = off.copy()
    past[2999] = len(text) - int(lens[2999]) + 1                       # the last sequence, moved one byte past the text's end
    for o, ln, lab in ((off, lens, bad_label), (off, neg_len, labels), (past, lens, labels)):
        info = _add(ds, _dev(text, o, ln), la, mate_b, lb, lab)
        assert int(info[0]) != 0
        assert (ds.result() == before).all()
    # ... in mate 2's table just as well, and single-end
    info = _add(ds, mate_b, lb, _dev(text, past, lens), la, labels)
    assert int(info[0]) != 0 and (ds.result() == before).all()
    info = _add(ds, _dev(text, off, neg_len), la, None, None, np.abs(labels))
    assert int(info[0]) != 0 and (ds.result() == before).all()
    assert int(_add(ds, _dev(text, off, lens), la, mate_b, lb, labels)[0]) == 0
    assert (ds.result() == 2 * before).all()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------------
N_PAIRS = 3000


def _records(path):
    with (gzip.open(path, "rb") if path.endswith("gz") else open(path, "rb")) as fh:
        return fh.read().count(b"\n") // 4


def _counters(path):
    doc = json.load(open(path))
    assert doc["format"] == "ribodetector-summary/1"
    return {k: doc[k] for k in COUNTERS if k in doc}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """3,000 pairs of 40-160 bp, some with N, and the run every other run is compared with: two plain files, 6 chunks, -e both, with
    --read_report and --summary"""
    from ribodetector_amd import detect, synth
    d = tmp_path_factory.mktemp("summary_cli")
    reads = [synth.reads_numpy(N_PAIRS, (40, 160), seed=71 + e, rrna_frac=0.3, n_rate=0.01) for e in (0, 1)]
    inputs = [str(d / ("p_%d.fq" % (e + 1))) for e in (0, 1)]
    for e in (0, 1):
        synth.write_fastq(inputs[e], reads[e][0], reads[e][1], e + 1)
    seqs = [[reads[e][0].tobytes()[reads[e][1][i]:reads[e][1][i + 1]] for i in range(N_PAIRS)] for e in (0, 1)]
    assert any(b"N" in s for s in seqs[0])

    def run(tag, inp, extra=(), summary=True, chunk="1", paired_out=True):
        outs = [str(d / ("%s_n%d.fq" % (tag, e))) for e in (1, 2)][:2 if paired_out else 1]
        rrs = [str(d / ("%s_r%d.fq" % (tag, e))) for e in (1, 2)][:2 if paired_out else 1]
        rep, js = str(d / (tag + ".tsv")), str(d / (tag + ".json"))
        p = detect.main(["-l", "100", "-i", *inp, "-o", *outs, "-r", *rrs, "-e", "both", "--chunk_size", chunk, "-m", "3", "--read_report", rep]
                        + (["--summary", js] if summary else []) + list(extra))
        return {"p": p, "outs": outs, "rrs": rrs, "rep": rep, "json": js, "files": outs + rrs + [o + ".unclassified.gz" for o in outs] + [rep]}
    base = run("base", inputs)
    return {"dir": d, "inputs": inputs, "seqs": seqs, "run": run, "base": base, "doc": json.load(open(base["json"]))}


def test_cli_summary_against_outputs_report_and_input(cli):
    base, doc = cli["base"], cli["doc"]
    p = base["p"]
    assert (doc["paired"], doc["interleaved"], doc["len"], doc["ensure"], doc["model"], doc["inputs"]) == (True, False, 100, "both", "mcc", cli["inputs"])
    reads = doc["reads"]
    assert reads["total"] == N_PAIRS == p.num_read
    assert reads["nonrRNA"] == _records(base["outs"][0]) == _records(base["outs"][1]) == p.num_nonrrna
    assert reads["rRNA"] == _records(base["rrs"][0]) == p.num_rrna
    assert reads["unclassified"] == _records(base["outs"][0] + ".unclassified.gz") == p.num_unknown > 0
    assert reads["rRNA_fraction"] == round(p.num_rrna / N_PAIRS, 6)
    hdr, rows = H.parse(H.read_report(base["rep"]))
    assert len(rows) == N_PAIRS
    labels = np.array([{b"unclassified": -1, b"nonrRNA": 0, b"rRNA": 1}[r[1]] for r in rows])
    # p_rrna = the report's three columns aggregated by its label column
    want = np.zeros((3, 3, 100), dtype=np.int64)
    for (_, _, qs), lab in zip(rows, labels):
        for src, q in enumerate(qs):
            want[src, lab + 1, S.p_bin(q)] += 1
    for src, name in enumerate(("mate1", "mate2", "pair")):
        for c, cname in enumerate(S.CLASSES):
            assert doc["p_rrna"][name][cname] == want[src, c].tolist()
    # length / bases / gc = the reference over the input, grouped by the report's labels
    ref = S.views(S.accumulate(cli["seqs"][0], np.zeros((N_PAIRS, 2), np.float32), cli["seqs"][1], np.zeros((N_PAIRS, 2), np.float32), labels))
    for e, name in enumerate(("mate1", "mate2")):
        for c, cname in enumerate(S.CLASSES):
            assert doc["length"][name][cname] == ref["length"][e, c].tolist()
            assert doc["gc"][name][cname] == ref["gc"][e, c].tolist()
            assert list(doc["bases"][name][cname].values()) == ref["bases"][e, c].tolist()
    for cname in S.CLASSES:
        assert np.sum(doc["mate_labels"][cname]) == reads[cname]
    assert doc["truncated_reads"] == sum(len(s) > 100 for s in cli["seqs"][0] + cli["seqs"][1]) > 0


def test_cli_counters_do_not_depend_on_chunks_or_ingest(cli):
    d, want = cli["dir"], _counters(cli["base"]["json"])
    assert _counters(cli["run"]("chunk3", cli["inputs"], chunk="3")["json"]) == want
    gz = [str(d / ("g_%d.fq.gz" % (e + 1))) for e in (0, 1)]
    for src, dst in zip(cli["inputs"], gz):
        open(dst, "wb").write(gzip.compress(open(src, "rb").read(), 6))
    assert _counters(cli["run"]("gz", gz)["json"]) == want
    # the same pairs as ONE interleaved file
    recs = [open(p, "rb").read().split(b"\n") for p in cli["inputs"]]
    il = str(d / "il.fq")
    with open(il, "wb") as fh:
        for i in range(N_PAIRS):
            for e in (0, 1):
                fh.write(b"\n".join(recs[e][4 * i:4 * i + 4]) + b"\n")
    r = cli["run"]("il", [il], extra=["--interleaved"])
    assert _counters(r["json"]) == want and json.load(open(r["json"]))["interleaved"] is True
    cli["interleaved"] = il


def test_cli_single_end_fasta_and_fastq(cli):
    from ribodetector_amd import detect
    d = cli["dir"]
    fa = str(d / "m1.fa")
    with open(fa, "wb") as fh:
        for i, s in enumerate(cli["seqs"][0]):
            fh.write(b">syn.%d/1\n%s\n" % (i, s))
    docs = []
    for tag, inp in (("se_fq", cli["inputs"][0]), ("se_fa", fa)):
        js = str(d / (tag + ".json"))
        p = detect.main(["-l", "100", "-i", inp, "-o", str(d / (tag + "_n.out")), "--chunk_size", "1", "-m", "3", "--summary", js])
        docs.append(json.load(open(js)))
        assert docs[-1]["paired"] is False and docs[-1]["reads"]["total"] == N_PAIRS and docs[-1]["reads"]["rRNA"] == p.num_rrna
    assert {k: docs[0][k] for k in COUNTERS if k in docs[0]} == {k: docs[1][k] for k in COUNTERS if k in docs[1]}
    one, two = docs[0], cli["doc"]
    assert "mate_labels" not in one and "mate2" not in one["length"] and "pair" not in one["p_rrna"] and one["reads"]["unclassified"] == 0
    # what does not depend on the label: mate 1's histograms summed over the classes are those of the paired run
    for sec in ("length", "gc", "p_rrna"):
        assert np.sum(list(one[sec]["mate1"].values()), axis=0).tolist() == np.sum(list(two[sec]["mate1"].values()), axis=0).tolist()


def test_cli_outputs_unchanged_by_the_flag(cli, caplog):
    caplog.set_level(logging.INFO)
    with_flag = cli["run"]("with", cli["inputs"])
    assert "rRNA fraction: %.6f (summary: %s)" % (cli["doc"]["reads"]["rRNA_fraction"], with_flag["json"]) in caplog.text
    caplog.clear()
    without = cli["run"]("without", cli["inputs"], summary=False)
    assert "rRNA fraction" not in caplog.text and not os.path.exists(without["json"])
    for a, b in zip(with_flag["files"], without["files"]):
        assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


def test_cli_no_summary_of_a_failed_run(cli):
    from ribodetector_amd import detect
    d = cli["dir"]
    odd = str(d / "odd.fq")
    with open(odd, "wb") as fh:                                        # three records: one pair and a lone read
        fh.write(b"\n".join(open(cli["inputs"][0], "rb").read().split(b"\n")[:12]) + b"\n")
    js = str(d / "odd.json")
    with pytest.raises(Exception):
        detect.main(["-l", "100", "-i", odd, "-o", str(d / "odd_n.fq"), "--interleaved", "--no_mate_check", "--summary", js])
    assert not os.path.exists(js)


def test_cli_two_ranks(cli):
    """both rank layouts: the sharded parse (plain mate files: every rank counts its own byte range) and the label gather (an
    interleaved file: every rank counts its shard of each chunk's pairs); the ranks' counters are summed before rank 0 writes"""
    d, want = cli["dir"], _counters(cli["base"]["json"])
    il = cli.get("interleaved")
    if il is None:
        il = str(d / "il2.fq")
        recs = [open(p, "rb").read().split(b"\n") for p in cli["inputs"]]
        with open(il, "wb") as fh:
            for i in range(N_PAIRS):
                for e in (0, 1):
                    fh.write(b"\n".join(recs[e][4 * i:4 * i + 4]) + b"\n")
    common = ["-l", "100", "-e", "both", "--chunk_size", "1", "-m", "3"]
    js = str(d / "two_sharded.json")
    r, _ = R._torchrun(2, common + ["-i", *cli["inputs"], "-o", str(d / "t1.fq"), str(d / "t2.fq"), "--summary", js])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Rank 1 parses" in r.stdout + r.stderr and (r.stdout + r.stderr).count("rRNA fraction:") == 1
    assert _counters(js) == want
    js = str(d / "two_gather.json")
    r, _ = R._torchrun(2, common + ["-i", il, "--interleaved", "-o", str(d / "u1.fq"), str(d / "u2.fq"), "--summary", js])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "label-gather layout" in r.stdout + r.stderr
    assert _counters(js) == want
