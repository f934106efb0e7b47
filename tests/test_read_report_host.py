"""--read_report without a GPU: the argument checks, the header lines, and a pure-Python formatter of the report format (README
"Per-read report") that tests/test_gpu_read_report.py compares the device's report against."""
import gzip
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

LABEL_NAMES = {1: b"rRNA", 0: b"nonrRNA", -1: b"unclassified"}
_WS = b" \t\r\n\x0b\x0c"


# ---- the reference formatter --------------------------------------------------------------------------------------------------------
def read_id(record):
    """the bytes of the header line after '@' / '>' up to the first of {space, \\t, \\r, \\n, \\v, \\f}"""
    assert record[:1] in (b"@", b">")
    end = 1
    while end < len(record) and record[end] not in _WS:
        end += 1
    return record[1:end]


def q_of(l0, l1):
    """rint(softmax([l0, l1])[1] * 1e4) in float64"""
    d = float(l1) - float(l0)
    e = np.exp(-abs(d))
    p = 1.0 / (1.0 + e) if d >= 0 else e / (1.0 + e)
    return int(np.rint(p * 1e4))


def fmt_q(q):
    return b"1.0000" if q >= 10000 else b"0.%04d" % q


def header(paired):
    return b"#read_id\tlabel\tp_rrna_1\tp_rrna_2\tp_rrna_pair\n" if paired else b"#read_id\tlabel\tp_rrna\n"


def format_lines(records, labels, logits_a, logits_b=None):
    """the report lines (no header) of records (bytes each, header line first), int labels, fp32 [n, 2] logits of mate 1 (and 2)"""
    out = []
    la = np.asarray(logits_a, dtype=np.float32)
    lb = None if logits_b is None else np.asarray(logits_b, dtype=np.float32)
    for i, rec in enumerate(records):
        fields = [read_id(rec), LABEL_NAMES[int(labels[i])], fmt_q(q_of(la[i, 0], la[i, 1]))]
        if lb is not None:
            s0, s1 = np.float32(la[i, 0] + lb[i, 0]), np.float32(la[i, 1] + lb[i, 1])     # the fp32 sums of the pair rule
            fields += [fmt_q(q_of(lb[i, 0], lb[i, 1])), fmt_q(q_of(s0, s1))]
        out.append(b"\t".join(fields) + b"\n")
    return b"".join(out)


def parse(text):
    """report text -> (header line, [(id, label, [q, ...]), ...]) with q as integers"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    rows = []
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        rows.append((f[0], f[1], [int(round(float(x) * 1e4)) for x in f[2:]]))
    return lines[0] + b"\n", rows


def read_report(path):
    with (gzip.open(path, "rb") if path.endswith("gz") else open(path, "rb")) as fh:
        return fh.read()


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_formatter_follows_the_spec():
    recs = [b"@a b\nAC\n+\nII\n", b"@\tx\nA\n+\nI\n", b">r\r\nACGT\n", b"@" + b"x" * 300 + b"\nA\n+\nI\n", b"@id\x0bq\nA\n+\nI\n"]
    la = np.array([[0, 0], [0, 40], [40, 0], [1.0, 1.00001], [-3, 2]], dtype=np.float32)
    txt = format_lines(recs, [0, 1, 0, 1, 1], la)
    lines = txt.split(b"\n")
    assert lines[0] == b"a\tnonrRNA\t0.5000"
    assert lines[1] == b"\trRNA\t1.0000"                 # empty id; p = 1 - 4e-18
    assert lines[2] == b"r\tnonrRNA\t0.0000"
    assert lines[3] == b"x" * 300 + b"\trRNA\t0.5000"
    assert lines[4] == b"id\trRNA\t%s" % fmt_q(q_of(-3, 2))
    assert fmt_q(q_of(-3, 2)) == b"0.9933"
    pl = format_lines(recs[:2], [-1, 0], la[:2], la[:2][:, ::-1])
    assert pl.split(b"\n")[0] == b"a\tunclassified\t0.5000\t0.5000\t0.5000"
    assert pl.split(b"\n")[1] == b"\tnonrRNA\t1.0000\t0.0000\t0.5000"
    hdr, rows = parse(header(False) + txt)
    assert hdr == b"#read_id\tlabel\tp_rrna\n" and rows[0] == (b"a", b"nonrRNA", [5000]) and len(rows) == 5


def test_header_lines():
    from ribodetector_amd import gz
    assert gz.REPORT_HEADER_SE == b"#read_id\tlabel\tp_rrna\n" == header(False)
    assert gz.REPORT_HEADER_PE == b"#read_id\tlabel\tp_rrna_1\tp_rrna_2\tp_rrna_pair\n" == header(True)


def test_flag_and_help():
    from ribodetector_amd import detect
    p = detect.build_parser()
    a = p.parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq", "--read_report", "rep.tsv.gz"])
    assert a.read_report == "rep.tsv.gz"
    assert p.parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq"]).read_report is None
    h = p.format_help()
    assert "--read_report" in h and "#read_id<TAB>label<TAB>p_rrna" in h and "p_rrna_pair" in h


def _predictor(tmp_path, argv):
    from ribodetector_amd import detect
    from ribodetector_amd.parse_config import ConfigParser
    args = detect.build_parser().parse_args(argv)
    cfg = ConfigParser.from_json(os.path.join(ROOT, "ribodetector_amd", "config.json"))
    p = detect.Predictor(cfg, args)
    p.len = args.len                       # (load_model sets it; no model is loaded here)
    ran = []
    p.run = lambda: ran.append("run")
    p.run_with_chunks = lambda *a, **k: ran.append("chunks")
    return p, ran


@pytest.mark.parametrize("case", ["o", "r", "o2", "unclassified", "relative"])
def test_argument_errors(tmp_path, case, monkeypatch):
    monkeypatch.chdir(tmp_path)
    i1, i2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    o1, o2, r1, r2 = (str(tmp_path / x) for x in ("o1.fq", "o2.fq.gz", "r1.fq", "r2.fq"))
    bad = {"o": o1, "r": r2, "o2": o2, "unclassified": o1 + ".unclassified.gz", "relative": "o1.fq"}[case]
    p, ran = _predictor(tmp_path, ["-l", "100", "-i", i1, i2, "-o", o1, o2, "-r", r1, r2, "-e", "both", "--read_report", bad])
    with pytest.raises(RuntimeError, match="--read_report"):
        p.detect()
    assert ran == []


def test_argument_accepted(tmp_path):
    i1, i2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    o1, o2 = str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq")
    # no unclassified files without -e both: that name is free
    p, ran = _predictor(tmp_path, ["-l", "100", "-i", i1, i2, "-o", o1, o2, "-e", "none", "--read_report", o1 + ".unclassified.gz"])
    p.detect()
    assert ran == ["run"]
    p, ran = _predictor(tmp_path, ["-l", "100", "-i", i1, "-o", o1, "--read_report", str(tmp_path / "rep.tsv"), "--chunk_size", "1"])
    p.detect()
    assert ran == ["chunks"]


def test_check_read_report_function():
    from ribodetector_amd.detect import check_read_report
    check_read_report(None, ["a"], None, False, "none")
    check_read_report("rep", ["a"], None, False, "none")
    with pytest.raises(RuntimeError):
        check_read_report("a", ["a"], None, False, "none")
    with pytest.raises(RuntimeError):
        check_read_report("b.unclassified.gz", ["a", "b"], None, True, "both")
    check_read_report("b.unclassified.gz", ["b"], None, False, "both")


def test_exports_declared():
    """the three entry points are in the header, the binding list and the library (no GPU needed to load it)"""
    from ribodetector_amd import _native as N
    src = open(os.path.join(ROOT, "include", "ribodetector_amd.h")).read()
    for name in ("rd_report_workspace_bytes", "rd_report_out_bound", "rd_report_format"):
        assert name in src and name in N.SYMBOLS
    lib = N.lib()
    assert int(lib.rd_report_out_bound(10, 1000)) >= 1000 + 10 * 35
    assert int(lib.rd_report_workspace_bytes(1 << 20)) >= 12 << 20
