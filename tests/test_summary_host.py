"""--summary without a GPU: a numpy reference of the counters (include/ribodetector_amd.h RD_SUM_*, README "Run summary") that
tests/test_gpu_summary.py compares the device's accumulator against, the inputs both files use, the argument checks, the layout table
and the JSON document."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_read_report_host as H  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# the accumulator as the issue's table gives it: section -> shape, in this order, without gaps
SECTIONS = [("units", (3,)), ("mate_labels", (3, 2, 2)), ("length", (2, 3, 513)), ("p_rrna", (3, 3, 100)), ("bases", (2, 3, 5)), ("gc", (2, 3, 101))]
WORDS = sum(int(np.prod(s)) for _, s in SECTIONS)
CLASSES = ("unclassified", "nonrRNA", "rRNA")


def views(acc):
    out, o = {}, 0
    for name, shape in SECTIONS:
        k = int(np.prod(shape))
        out[name] = acc[o:o + k].reshape(shape)
        o += k
    return out


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def code_counts(seq):
    """[A, C, G, T (with U), other] of a sequence (bytes): rd_code - lowercase counts as other"""
    a = np.frombuffer(seq, dtype=np.uint8)
    c = [int((a == ord(ch)).sum()) for ch in "ACG"] + [int(((a == ord("T")) | (a == ord("U"))).sum())]
    return c + [len(a) - sum(c)]


def x_of(l0, l1):
    """softmax([l0, l1])[1] * 1e4 in float64"""
    d = float(l1) - float(l0)
    e = np.exp(-abs(d))
    return (1.0 / (1.0 + e) if d >= 0 else e / (1.0 + e)) * 1e4


def p_bin(q):
    return min(int(q) // 100, 99)


def pair_sums(la, lb):
    """the fp32 sums of the pair rule, as the report forms them"""
    return np.float32(la[0] + lb[0]), np.float32(la[1] + lb[1])


def accumulate(seqs_a, logits_a, seqs_b, logits_b, labels):
    """int64[WORDS]: the counters of units whose mates' sequences are seqs_a / seqs_b (lists of bytes; seqs_b None = single-end),
    logits fp32 [n, 2], labels in {-1, 0, 1}; q is binned in float64 (H.q_of)"""
    acc = np.zeros(WORDS, dtype=np.int64)
    s = views(acc)
    la = np.asarray(logits_a, dtype=np.float32)
    lb = None if seqs_b is None else np.asarray(logits_b, dtype=np.float32)
    for i, lab in enumerate(labels):
        c = int(lab) + 1
        assert 0 <= c <= 2
        s["units"][c] += 1
        for m, (seqs, lg) in enumerate(((seqs_a, la), (seqs_b, lb))[:1 if seqs_b is None else 2]):
            cnt = code_counts(seqs[i])
            s["length"][m, c, min(len(seqs[i]), 512)] += 1
            s["bases"][m, c] += cnt
            acgt = sum(cnt[:4])
            if acgt:
                s["gc"][m, c, 100 * (cnt[1] + cnt[2]) // acgt] += 1
            s["p_rrna"][m, c, p_bin(H.q_of(lg[i, 0], lg[i, 1]))] += 1
        if seqs_b is not None:
            s["mate_labels"][c, int(la[i, 1] > la[i, 0]), int(lb[i, 1] > lb[i, 0])] += 1
            s["p_rrna"][2, c, p_bin(H.q_of(*pair_sums(la[i], lb[i])))] += 1
    return acc


# ---- inputs shared with the GPU file ----------------------------------------------------------------------------------------------------------
SPECIAL_LENS = [0, 1, 15, 16, 17, 511, 512, 513, 600]
ALPHABET = np.frombuffer(b"ACGTUNacgtRY-", dtype=np.uint8)


def make_text(n, seed, tails=(1, 15, 16, 17, 33, 600)):
    """n records as one text: FASTQ records, the last one FASTA without a final newline, so that its sequence ends on the text's last
    byte. Returns (text bytes, rec_start int64[n + 1], seq_off int64[n + len(tails)], seq_len int32[...]): the sequence table has one
    more entry per `tails` value L, the last L bytes of the text - more sequences that end on its last byte (the tables may alias)."""
    rng = np.random.default_rng(seed)
    lens = [SPECIAL_LENS[i % len(SPECIAL_LENS)] if i < 10 * len(SPECIAL_LENS) else int(rng.integers(1, 301)) for i in range(n)]
    rng.shuffle(lens)
    if lens[-1] < 17:
        lens[-1] = 117
    parts, rs, off, pos = [], [0], [], 0
    for i, ln in enumerate(lens):
        alpha = ALPHABET[:4] if rng.integers(0, 2) else ALPHABET
        seq = alpha[rng.integers(0, len(alpha), ln)].tobytes()
        hdr = b"%sr%d x\n" % (b">" if i == n - 1 else b"@", i)
        rec = hdr + seq + (b"" if i == n - 1 else b"\n+\n" + b"I" * ln + b"\n")
        off.append(pos + len(hdr))
        parts.append(rec)
        pos += len(rec)
        rs.append(pos)
    for t in tails:
        off.append(pos - t)
        lens.append(t)
    return b"".join(parts), np.array(rs, dtype=np.int64), np.array(off, dtype=np.int64), np.array(lens, dtype=np.int32)


def seqs_of(text, off, lens):
    return [text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)]


def bin_safe(x):
    """is x = p * 1e4 more than 0.05 away from every 100 k - 0.5, where the bin of rint(x) changes?"""
    t = (x + 0.5) % 100.0
    return min(t, 100.0 - t) > 0.05


def draw_logits(n, rng):
    """logits in the style of test_gpu_read_report._logits: ties, +-40, tiny margins"""
    lg = rng.normal(0, 4, (n, 2)).astype(np.float32)
    k = rng.integers(0, 5, n)
    lg[k == 0, 1] = lg[k == 0, 0]
    lg[k == 1] = np.array([[-40, 40], [40, -40]], dtype=np.float32)[rng.integers(0, 2, int((k == 1).sum()))]
    lg[k == 2, 1] = lg[k == 2, 0] + rng.choice([1e-6, -1e-6, 3e-5, -2e-4], int((k == 2).sum())).astype(np.float32)
    return lg


def make_logits(n, seed, paired, redraw=True):
    """(logits_a, logits_b | None). redraw: a unit whose p of a mate (or of the pair) lies within 0.05 of a bin boundary in x = p * 1e4
    is drawn again, not dropped, until none does - fp32 rp_q is within about 2e-3 in x of float64, so both then give the same bins"""
    rng = np.random.default_rng(seed)
    la = draw_logits(n, rng)
    lb = draw_logits(n, rng) if paired else None

    def safe(i):
        ok = bin_safe(x_of(la[i, 0], la[i, 1]))
        if paired:
            ok = ok and bin_safe(x_of(lb[i, 0], lb[i, 1])) and bin_safe(x_of(*pair_sums(la[i], lb[i])))
        return ok
    if redraw:
        for i in range(n):
            while not safe(i):
                la[i] = draw_logits(1, rng)[0]
                if paired:
                    lb[i] = draw_logits(1, rng)[0]
    return la, lb


def q_fp32(l0, l1):
    """rp_q of csrc/rd_common.hpp evaluated with numpy float32 (l0, l1: float32 arrays)"""
    d = (l1 - l0).astype(np.float32)
    e = np.exp(-np.abs(d)).astype(np.float32)
    one = np.float32(1.0)
    p = np.where(d >= 0, one / (one + e), e / (one + e)).astype(np.float32)
    return np.clip(np.rint(p * np.float32(10000.0)), 0, 10000).astype(np.int64)


def bins_fp32(la, lb):
    """[sources][n] p bins of the inputs by the fp32 evaluation"""
    out = [np.minimum(q_fp32(la[:, 0], la[:, 1]) // 100, 99)]
    if lb is not None:
        out.append(np.minimum(q_fp32(lb[:, 0], lb[:, 1]) // 100, 99))
        out.append(np.minimum(q_fp32((la[:, 0] + lb[:, 0]).astype(np.float32), (la[:, 1] + lb[:, 1]).astype(np.float32)) // 100, 99))
    return out


def bins_fp64(la, lb):
    out = [np.array([p_bin(H.q_of(a[0], a[1])) for a in la])]
    if lb is not None:
        out.append(np.array([p_bin(H.q_of(b[0], b[1])) for b in lb]))
        out.append(np.array([p_bin(H.q_of(*pair_sums(a, b))) for a, b in zip(la, lb)]))
    return out


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_follows_the_table():
    seqs = [b"ACGT", b"", b"acgtNNUU", b"G" * 600, b"CCGA-"]
    la = np.array([[0, 0], [0, 40], [40, 0], [1.0, 1.00001], [-3, 2]], dtype=np.float32)
    s = views(accumulate(seqs, la, None, None, [0, 1, 0, 1, 1]))
    assert s["units"].tolist() == [0, 2, 3] and s["mate_labels"].sum() == 0
    assert s["length"][0, 1, 4] == 1 and s["length"][0, 2, 0] == 1 and s["length"][0, 1, 8] == 1 and s["length"][0, 2, 512] == 1 and s["length"][0, 2, 5] == 1
    assert s["length"][1].sum() == 0
    assert s["bases"][0, 1].tolist() == [1, 1, 1, 3, 6]          # ACGT + (UU as T, acgt and NN as other)
    assert s["bases"][0, 2].tolist() == [1, 2, 601, 0, 1]
    assert s["gc"][0, 1, 50] == 1 and s["gc"][0, 1, 0] == 1 and s["gc"][0, 2, 100] == 1 and s["gc"][0, 2, 75] == 1 and s["gc"].sum() == 4   # the empty read: no bin
    assert s["p_rrna"][0, 1, 50] == 1 and s["p_rrna"][0, 2, 99] == 2 and s["p_rrna"][0, 1, 0] == 1 and s["p_rrna"][0, 2, 50] == 1
    lb = la[::-1].copy()
    s = views(accumulate(seqs, la, seqs[::-1], lb, [-1, 1, 0, 1, -1]))
    assert s["units"].tolist() == [2, 1, 2]
    assert s["mate_labels"].sum(axis=(1, 2)).tolist() == [2, 1, 2]
    assert s["mate_labels"][0].tolist() == [[0, 1], [1, 0]]      # units 0 and 4: (tie, l1 > l0) and (l1 > l0, tie)
    assert s["p_rrna"].sum(axis=(1, 2)).tolist() == [5, 5, 5] and s["length"][1].sum() == 5


def test_chosen_logits_bin_alike_in_fp32():
    """the inputs of the GPU comparison: after the redraw the float64 reference and an fp32 evaluation of rp_q agree on every bin"""
    for paired in (False, True):
        la, lb = make_logits(5000, 21 + paired, paired)
        for a, b in zip(bins_fp32(la, lb), bins_fp64(la, lb)):
            assert (a == b).all()
        assert (la[:, 0] == la[:, 1]).sum() > 500                # the ties stay


def test_make_text_places_sequences_on_the_last_byte():
    text, rs, off, lens = make_text(300, 4)
    assert rs[-1] == len(text) and len(off) == len(lens) == 306
    assert ((off + lens) == len(text)).sum() >= 7 and (off + lens).max() == len(text)
    assert set(SPECIAL_LENS) <= set(lens.tolist())
    for i in (0, 150, 299):
        assert text[rs[i]:rs[i] + 1] in (b"@", b">") and text[off[i] - 1:off[i]] == b"\n"


def test_layout_table_covers_the_accumulator():
    from ribodetector_amd import summary as S
    hdr = open(os.path.join(ROOT, "include", "ribodetector_amd.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define RD_SUM_([A-Z_]+) (\d+)", hdr)}
    words = const["WORDS"]
    from ribodetector_amd import _native as N
    if os.path.exists(N.LIB_PATH):
        assert int(N.lib().rd_summary_words()) == words
    assert words == WORDS == S.WORDS
    assert [(k, tuple(s)) for k, (_, s) in S.LAYOUT.items()] == SECTIONS
    covered = np.zeros(words, dtype=np.int64)
    for name, (o, shape) in S.LAYOUT.items():
        assert const[name.upper()] == o
        covered[o:o + int(np.prod(shape))] += 1
    assert (covered == 1).all()                                   # no gap, no overlap
    assert (const["LEN_BINS"], const["P_BINS"], const["GC_BINS"]) == (513, 100, 101) == (S.LEN_BINS, S.P_BINS, S.GC_BINS)
    acc = np.arange(words, dtype=np.int64)
    for name, v in S.sections(acc).items():
        assert (v == views(acc)[name]).all()


@pytest.mark.parametrize("case", ["o", "r", "o2", "unclassified", "report", "relative"])
def test_argument_errors(tmp_path, case, monkeypatch):
    monkeypatch.chdir(tmp_path)
    i1, i2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    o1, o2, r1, r2, rep = (str(tmp_path / x) for x in ("o1.fq", "o2.fq.gz", "r1.fq", "r2.fq", "rep.tsv"))
    bad = {"o": o1, "r": r2, "o2": o2, "unclassified": o2 + ".unclassified.gz", "report": rep, "relative": "r1.fq"}[case]
    p, ran = H._predictor(tmp_path, ["-l", "100", "-i", i1, i2, "-o", o1, o2, "-r", r1, r2, "-e", "both", "--read_report", rep, "--summary", bad])
    with pytest.raises(RuntimeError, match="--summary"):
        p.detect()
    assert ran == [] and not os.path.exists(bad)


def test_argument_accepted(tmp_path):
    from ribodetector_amd import detect
    i1, o1 = str(tmp_path / "a.fq"), str(tmp_path / "o.fq")
    p, ran = H._predictor(tmp_path, ["-l", "100", "-i", i1, "-o", o1, "--summary", o1 + ".unclassified.gz"])     # single-end: that name is free
    p.detect()
    assert ran == ["run"]
    a = detect.build_parser().parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq"])
    assert a.summary is None and "--summary" in detect.build_parser().format_help()
    detect.check_summary(None, ["a"], None, False, "none", "a")
    with pytest.raises(RuntimeError):
        detect.check_summary("rep", ["a"], None, False, "none", "./rep")


def _meta(paired, ln=100):
    return {"version": "0", "paired": paired, "interleaved": False, "len": ln, "ensure": "both", "model": "mcc", "inputs": ["a", "b"][:1 + paired]}


def test_to_json_of_a_reference_accumulator():
    import json
    from ribodetector_amd import summary as S
    text, _, off, lens = make_text(400, 9)
    text2, _, off2, lens2 = make_text(400, 10)
    sa, sb = seqs_of(text, off, lens), seqs_of(text2, off2, lens2)
    n = len(sa)
    la, lb = make_logits(n, 3, True)
    labels = np.random.default_rng(1).integers(-1, 2, n)
    acc = accumulate(sa, la, sb, lb, labels)
    doc = json.loads(json.dumps(S.to_json(acc, _meta(True))))      # (plain JSON types only)
    assert doc["format"] == "ribodetector-summary/1" and doc["paired"] is True and doc["len"] == 100 and doc["model"] == "mcc"
    units = {c: int((labels == k - 1).sum()) for k, c in enumerate(CLASSES)}
    assert doc["reads"] == {"total": n, "nonrRNA": units["nonrRNA"], "rRNA": units["rRNA"], "unclassified": units["unclassified"],
                            "rRNA_fraction": round(units["rRNA"] / n, 6)}
    for c in CLASSES:
        assert np.sum(doc["mate_labels"][c]) == units[c] and np.shape(doc["mate_labels"][c]) == (2, 2)
        for m, seqs in (("mate1", sa), ("mate2", sb)):
            assert len(doc["length"][m][c]) == 513 and sum(doc["length"][m][c]) == units[c]
            assert len(doc["gc"][m][c]) == 101 and sum(doc["gc"][m][c]) <= units[c]
            assert list(doc["bases"][m][c]) == ["A", "C", "G", "T", "other"]
            assert sum(doc["bases"][m][c].values()) == sum(len(s) for s, lab in zip(seqs, labels) if CLASSES[lab + 1] == c)
        for src in ("mate1", "mate2", "pair"):
            assert len(doc["p_rrna"][src][c]) == 100 and sum(doc["p_rrna"][src][c]) == units[c]
    assert doc["length"]["overflow_from"] == 512 and doc["p_rrna"]["bin_width"] == 0.01
    assert doc["truncated_reads"] == sum(len(s) > 100 for s in sa + sb)
    assert S.to_json(acc, _meta(True, 600))["truncated_reads"] is None
    # single-end: no second mate, no pair
    acc1 = accumulate(sa, la, None, None, np.abs(labels))
    one = S.to_json(acc1, _meta(False))
    assert "mate_labels" not in one
    for sec in ("length", "p_rrna", "bases", "gc"):
        assert "mate1" in one[sec] and "mate2" not in one[sec] and "pair" not in one[sec]
        assert set(one[sec]["mate1"]) == set(CLASSES)
    assert one["reads"]["unclassified"] == 0 and one["reads"]["total"] == n
    # nothing read
    zero = S.to_json(np.zeros(WORDS, dtype=np.int64), _meta(False))
    assert zero["reads"] == {"total": 0, "nonrRNA": 0, "rRNA": 0, "unclassified": 0, "rRNA_fraction": None} and zero["truncated_reads"] == 0
    with pytest.raises(ValueError):
        S.to_json(np.zeros(WORDS - 1, dtype=np.int64), _meta(False))


def test_exports_declared():
    from ribodetector_amd import _native as N
    src = open(os.path.join(ROOT, "include", "ribodetector_amd.h")).read()
    for name in ("rd_summary_words", "rd_summary_accumulate"):
        assert name in src and name in N.SYMBOLS
    L = N.lib()
    assert int(L.rd_summary_words()) == WORDS
    assert L.rd_summary_accumulate(None, 0, None, None, None, None, 0, None, None, None, None, 0, None, None, None) == 0      # n = 0: a no-op
    assert L.rd_summary_accumulate(None, 0, None, None, None, None, 0, None, None, None, None, -1, None, None, None) != 0
