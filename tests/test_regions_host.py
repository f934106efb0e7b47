"""--regions on the host: the region rule (ribodetector_amd/regions.py, what tests/test_gpu_regions.py compares the device's lines with)
on hand-written cases, the line format byte for byte, the CLI's argument errors and the refusals of rd_region_format. No GPU is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_read_report_host as RH  # noqa: E402
import test_windows_host as WH  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R, N = 1, 0                     # an rRNA window, a window that is not


def _regions(length, L, labels):
    from ribodetector_amd import regions
    return [(s, e, b - a + 1) for s, e, a, b in regions.regions_of(length, L, labels)]


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def test_one_window():
    assert _regions(60, 100, [R]) == [(0, 60, 1)]                 # len < L: the read itself
    assert _regions(100, 100, [R]) == [(0, 100, 1)]               # len == L
    assert _regions(5000, 100, [R]) == [(0, 100, 1)]              # K == 1 on a long read: the window is its first L bases
    assert _regions(60, 100, [N]) == [] and _regions(5000, 100, [N]) == []
    assert _regions(0, 100, [R]) == []                            # a read of 0 bases: end == start, no line
    assert _regions(1, 100, [R]) == [(0, 1, 1)]


def test_all_none_alternating():
    # 300 bases, L = S = 100: windows at 0, 100, 200
    assert WH.n_windows(300, 100, 100, 32) == 3
    assert _regions(300, 100, [R, R, R]) == [(0, 300, 3)]
    assert _regions(300, 100, [N, N, N]) == []
    assert _regions(300, 100, [R, N, R]) == [(0, 100, 1), (200, 300, 1)]
    assert _regions(300, 100, [N, R, N]) == [(100, 200, 1)]
    # 201 bases: windows at 0, 50, 101 (the rule's integer division)
    assert _regions(201, 100, [N, R, R]) == [(50, 201, 2)]
    assert _regions(201, 100, [R, R, N]) == [(0, 150, 2)]


def test_runs_at_the_first_and_last_window():
    lab = [R, R, N, N, N, N, R, R, R, N]
    assert WH.n_windows(1000, 100, 100, 32) == 10
    assert _regions(1000, 100, lab) == [(0, 200, 2), (600, 900, 3)]
    assert _regions(1000, 100, lab[::-1]) == [(100, 400, 3), (800, 1000, 2)]
    assert _regions(1000, 100, [N] * 9 + [R]) == [(900, 1000, 1)]
    assert _regions(1000, 100, [R] + [N] * 9) == [(0, 100, 1)]


def test_capped_windows_keep_the_gaps_inside_a_region():
    # 3301 bases at K = 32: windows 0, 103, 206, ... (tests/test_windows_host.py HAND): between two windows 3 bases are in no window
    w, starts = WH.HAND[3301]
    assert w == 32 and starts[1] == 103 and starts[2] == 206 and starts[30] == 3097 and starts[31] == 3201
    lab = [N] + [R, R] + [N] * 27 + [R, R]
    assert _regions(3301, 100, lab) == [(103, 306, 2), (3097, 3301, 2)]       # 203 bases: the gap 203..206 belongs to the region
    # a contig far beyond K windows: 5 windows over 1,000,100 bases are 250,000 bases apart
    assert _regions(1000100, 100, [N, R, R, N, R]) == [(250000, 500100, 2), (1000000, 1000100, 1)]


def test_small_stride_regions_overlap():
    # L = 100, S = 30 on 250 bases: W = 6 windows at 0, 30, 60, 90, 120, 150 - a window between two regions is shorter than their reach
    assert WH.n_windows(250, 100, 30, 32) == 6
    got = _regions(250, 100, [R, N, R, N, N, R])
    assert got == [(0, 100, 1), (60, 160, 1), (150, 250, 1)]
    assert got[1][0] < got[0][1] and got == sorted(got)             # they overlap and are in ascending start


def test_tie_is_not_rrna():
    from ribodetector_amd import regions
    first = np.array([0, 3], dtype=np.int64)
    wl = np.array([[1.5, 1.5], [0.25, 0.5], [-2.0, -2.0]], dtype=np.float32)
    assert regions.format_lines([b"r"], [300], first, wl, 100, 1) == [b"r\t100\t200\t1\t1\t0.5622\n"]
    wl[1] = [0.5, 0.5]
    assert regions.format_lines([b"r"], [300], first, wl, 100, 1) == [b""]


# ---- the lines ------------------------------------------------------------------------------------------------------------------------
def test_format_lines_byte_for_byte():
    from ribodetector_amd import regions
    assert regions.HEADER == b"#read_id\tstart\tend\tmate\twindows\tp_rrna_max\n"
    ids = [b"short", b"", b"contig/1 ", b"none", b"empty"]
    lens = [80, 100, 1000, 300, 0]
    first = np.array([0, 1, 2, 12, 15, 16], dtype=np.int64)
    wl = np.zeros((16, 2), dtype=np.float32)
    wl[0] = [0, 40]                                 # p = 1 - 4e-18
    wl[1] = [-3, 2]                                 # 0.9933 (the report's own example)
    wl[2:12] = [[2, 0]] * 10
    wl[4], wl[5], wl[6] = [0, 1], [0, 3], [0, 2]    # a run of three: the largest p is the middle window's
    wl[11] = [0, 0.5]                               # a run at the last window
    wl[12:15] = [[1, 0]] * 3
    wl[15] = [0, 9]                                 # rRNA, but the read has no bases
    got = regions.format_lines(ids, lens, first, wl, 100, 2)
    assert got == [b"short\t0\t80\t2\t1\t1.0000\n", b"\t0\t100\t2\t1\t0.9933\n",
                   b"contig/1 \t200\t500\t2\t3\t0.9526\ncontig/1 \t900\t1000\t2\t1\t0.6225\n", b"", b""]
    assert regions.format_lines(ids[:1], lens[:1], first[:2], wl[:1], 100, 1) == [b"short\t0\t80\t1\t1\t1.0000\n"]


def test_q_is_the_reports():
    """one statement of q in the package; it is the report's formatter's (tests/test_read_report_host.py) wherever fp32 and float64 agree"""
    from ribodetector_amd import regions
    rng = np.random.default_rng(5)
    lg = (rng.standard_normal((2000, 2)) * 5).astype(np.float32)
    assert [regions.q_of(a, b) for a, b in lg] == [RH.q_of(a, b) for a, b in lg]
    assert [regions.fmt_q(q) for q in (0, 7, 9999, 10000)] == [RH.fmt_q(q) for q in (0, 7, 9999, 10000)] == [b"0.0000", b"0.0007", b"0.9999", b"1.0000"]


# ---- the CLI's arguments --------------------------------------------------------------------------------------------------------------
def test_flag_and_help():
    from ribodetector_amd import detect
    p = detect.build_parser()
    a = p.parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq", "--windows", "--regions", "r.bed.gz"])
    assert a.regions == "r.bed.gz" and a.windows
    assert p.parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq"]).regions is None
    h = p.format_help()
    assert "--regions" in h and "#read_id<TAB>start<TAB>end<TAB>mate<TAB>windows<TAB>p_rrna_max" in h


def test_check_regions_function():
    from ribodetector_amd.detect import check_regions
    check_regions(None, False)
    check_regions("r.bed", True, ["a"], None, False, "none")
    with pytest.raises(RuntimeError, match="--regions needs --windows"):
        check_regions("r.bed", False)
    for kw in (dict(output=["a", "r.bed"]), dict(output=["a"], rrna=["./r.bed"]), dict(output=["a"], read_report="r.bed"),
               dict(output=["a"], summary="r.bed")):
        with pytest.raises(RuntimeError, match="--regions r.bed is also"):
            check_regions("r.bed", True, **kw)
    with pytest.raises(RuntimeError, match="unclassified"):
        check_regions("b.unclassified.gz", True, ["a", "b"], None, True, "both")
    check_regions("b.unclassified.gz", True, ["b"], None, False, "both")
    check_regions("b.unclassified.gz", True, ["a", "b"], None, True, "none")


@pytest.mark.parametrize("case", ["no_windows", "o", "r", "unclassified", "report", "summary"])
def test_argument_errors_before_anything_runs(tmp_path, case, monkeypatch):
    monkeypatch.chdir(tmp_path)
    i1, i2 = str(tmp_path / "a_1.fq"), str(tmp_path / "a_2.fq")
    o1, o2, r1, r2 = (str(tmp_path / x) for x in ("o1.fq", "o2.fq.gz", "r1.fq", "r2.fq"))
    rep, summ = str(tmp_path / "rep.tsv"), str(tmp_path / "s.json")
    bad = {"no_windows": "reg.bed", "o": "o1.fq", "r": r2, "unclassified": o2 + ".unclassified.gz", "report": rep, "summary": summ}[case]
    argv = ["-l", "100", "-i", i1, i2, "-o", o1, o2, "-r", r1, r2, "-e", "both", "--read_report", rep, "--summary", summ, "--regions", bad]
    p, ran = RH._predictor(tmp_path, argv + ([] if case == "no_windows" else ["--windows"]))
    with pytest.raises(RuntimeError, match="--regions"):
        p.detect()
    assert ran == []
    if case == "no_windows":                        # main() refuses before the model is loaded
        from ribodetector_amd import detect
        monkeypatch.setattr(detect.Predictor, "load_model", lambda self: pytest.fail("the model was loaded"))
        with pytest.raises(RuntimeError, match="--regions needs --windows"):
            detect.main(argv)


def test_argument_accepted(tmp_path):
    i1, o1 = str(tmp_path / "a.fq"), str(tmp_path / "o.fq")
    p, ran = RH._predictor(tmp_path, ["-l", "100", "-i", i1, "-o", o1, "--windows", "--regions", str(tmp_path / "r.bed")])
    p.detect()
    assert ran == ["run"]


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def test_exports_declared_and_refusals():
    """both entry points are in the header, the binding list and the library; bad arguments are refused before any HIP call"""
    from ribodetector_amd import _native as NV
    src = open(os.path.join(ROOT, "include", "ribodetector_amd.h")).read()
    for name in ("rd_region_workspace_bytes", "rd_region_format"):
        assert name in src and name in NV.SYMBOLS
    lib = NV.lib()
    wb = lib.rd_region_workspace_bytes
    assert wb(-1, 0) == 0 and wb(10, -1) == 0 and wb(1 << 30, 0) == 0
    # room for (windows + units) / 2 line entries of 24 bytes, whatever the number of mates
    assert wb(1000, 2000 + 8192) - wb(1000, 2000) == 24 * 4096 and wb(0, 0) > 0 and wb(1000, 2000) > 2000 * 20
    P, big = 0x10000, 1 << 40

    def fmt(text_a=P, bytes_a=100, rs_a=P, len_a=P, first_a=P, wl_a=P, text_b=None, bytes_b=0, rs_b=None, len_b=None, first_b=None, wl_b=None,
            stride=1, n=10, max_len=100, out=P, cap=1000, info=P, ws=P, ws_bytes=big):
        return lib.rd_region_format(text_a, bytes_a, rs_a, len_a, first_a, wl_a, text_b, bytes_b, rs_b, len_b, first_b, wl_b, stride, n, max_len, out,
                                    cap, info, ws, ws_bytes, None)
    for kw in (dict(n=-1), dict(n=1 << 30), dict(bytes_a=-1), dict(stride=0), dict(stride=3), dict(max_len=0), dict(info=None), dict(text_a=None),
               dict(rs_a=None), dict(len_a=None), dict(first_a=None), dict(wl_a=None), dict(out=None), dict(ws=None), dict(ws=P + 8), dict(out=P + 8),
               dict(wl_a=P + 4), dict(text_b=P, rs_b=None), dict(text_b=P, rs_b=P, len_b=P, first_b=P, wl_b=None), dict(ws_bytes=100)):
        assert fmt(**kw) != 0, kw
