"""--windows on the host: the window rule and both fusions as a pure-numpy reference (what tests/test_gpu_windows.py compares the
kernels with, bit for bit), hand cases of the rule, the CLI's argument errors and the refusals of the rd_window_* entry points.
No GPU is needed."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the reference: integers for the rule (Python ints, so nothing can overflow), np.float32 one operation at a time for the fusions
def n_windows(length, L, S, K):
    length = int(length)
    if length <= L:
        return 1
    return min(K, -(-(length - L) // S) + 1)


def plan(lens, L, S, K):
    """win_first int64[n + 1]: the exclusive scan of W, entry n = the total"""
    w = np.array([n_windows(x, L, S, K) for x in np.asarray(lens).tolist()], dtype=np.int64)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(w, dtype=np.int64)])


def fill(offs, lens, L, S, K):
    """(win_off int64[total], win_len int32[total])"""
    wo, wl = [], []
    for off, length in zip(np.asarray(offs).tolist(), np.asarray(lens).tolist()):
        w = n_windows(length, L, S, K)
        if w == 1:
            wo.append(off)
            wl.append(length)
        else:
            wo += [off + j * (length - L) // (w - 1) for j in range(w)]
            wl += [L] * w
    return np.array(wo, dtype=np.int64), np.array(wl, dtype=np.int32)


def fuse(win_logits, win_first, mode, only_multi=False, into=None):
    """fp32[n, 2] (and uint8[n] labels) from fp32[total, 2]; rows that only_multi skips keep the values of `into` = (logits, labels)"""
    win_logits = np.asarray(win_logits, dtype=np.float32)
    n = len(win_first) - 1
    out = np.zeros((n, 2), dtype=np.float32) if into is None else into[0].copy()
    lab = np.zeros(n, dtype=np.uint8) if into is None else into[1].copy()
    for i in range(n):
        f, w = int(win_first[i]), int(win_first[i + 1] - win_first[i])
        if only_multi and w == 1:
            continue
        r = win_logits[f].copy()
        if mode == "mean":
            for j in range(1, w):
                r = np.array([np.float32(r[0] + win_logits[f + j][0]), np.float32(r[1] + win_logits[f + j][1])], dtype=np.float32)
            r = np.array([np.float32(r[0] / np.float32(w)), np.float32(r[1] / np.float32(w))], dtype=np.float32)
        else:
            best = np.float32(r[1] - r[0])
            for j in range(1, w):
                d = np.float32(win_logits[f + j][1] - win_logits[f + j][0])
                if d > best:
                    best, r = d, win_logits[f + j].copy()
        out[i] = r
        lab[i] = 1 if r[1] > r[0] else 0
    return out, lab


# ---- hand cases: L = 100, S = 100, K = 32 -> (W, starts); "..." entries are checked at the listed positions
HAND = {
    0: (1, None), 1: (1, None), 99: (1, None), 100: (1, None),
    101: (2, [0, 1]),
    199: (2, [0, 99]),
    200: (2, [0, 100]),
    201: (3, [0, 50, 101]),
    300: (3, [0, 100, 200]),
    3199: (32, {0: 0, 1: 99, 2: 199, 30: 2999, 31: 3099}),
    3200: (32, {j: 100 * j for j in range(32)}),
    3201: (32, {0: 0, 1: 100, 2: 200, 30: 3000, 31: 3101}),           # ceil(3101 / 100) + 1 = 33 > K
    3301: (32, {0: 0, 1: 103, 2: 206, 30: 3097, 31: 3201}),
    2 ** 31 - 1: (32, {0: 0, 1: 69273662, 2: 138547325, 30: 2078209884, 31: 2147483547}),     # 31 (len - L) does not fit 32 bits
}
HAND_LENS = sorted(HAND)


def _check_shape(offs, lens, L, S, K):
    """what holds for every case: first start 0, last start len - L, starts non-decreasing, full windows inside the read"""
    first = plan(lens, L, S, K)
    wo, wl = fill(offs, lens, L, S, K)
    assert first[-1] == len(wo) == len(wl)
    for i, (off, length) in enumerate(zip(offs, lens)):
        f, w = int(first[i]), int(first[i + 1] - first[i])
        st = wo[f:f + w] - off
        assert st[0] == 0 and (np.diff(st) >= 0).all()
        if w == 1:
            assert wl[f] == length
        else:
            assert st[-1] == length - L and (wl[f:f + w] == L).all() and length > L
    return first, wo, wl


def test_hand_cases():
    L, S, K = 100, 100, 32
    offs = np.arange(len(HAND_LENS), dtype=np.int64) * 7 + 3
    first, wo, wl = _check_shape(offs, HAND_LENS, L, S, K)
    for i, length in enumerate(HAND_LENS):
        w, starts = HAND[length]
        f = int(first[i])
        assert first[i + 1] - f == w, length
        if starts is None:
            assert (wo[f], wl[f]) == (offs[i], length)
            continue
        for j, s in (enumerate(starts) if isinstance(starts, list) else starts.items()):
            assert wo[f + j] == offs[i] + s, (length, j)


def test_stride_one_and_window_cap():
    first, wo, wl = _check_shape([5], [20], 4, 1, 4096)
    assert first[-1] == 17 and (wo == 5 + np.arange(17)).all() and (wl == 4).all()
    # the cap spreads K windows over the read
    first, wo, wl = _check_shape([0], [20], 4, 1, 5)
    assert wo.tolist() == [0, 4, 8, 12, 16]
    first, wo, wl = _check_shape([0], [21], 4, 1, 5)
    assert wo.tolist() == [0, 4, 8, 12, 17]


def test_one_window_per_read_is_the_read_table():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 1000, 300).astype(np.int32)
    offs = np.cumsum(lens, dtype=np.int64) - lens
    first, wo, wl = _check_shape(offs, lens, 100, 100, 1)
    assert (first == np.arange(301)).all() and (wo == offs).all() and (wl == lens).all()


def test_package_rule_agrees_with_the_reference():
    """ribodetector_amd/windows.py (the shard bounds of the label gather) is the same rule"""
    from ribodetector_amd import windows as W
    rng = np.random.default_rng(11)
    for L, S, K in ((100, 100, 32), (100, 37, 4096), (4, 1, 4096), (100, 100, 1), (70, 2 ** 31 - 1, 32), (100, 1000, 2)):
        lens = np.concatenate([rng.integers(0, 5000, 500), np.array(HAND_LENS)]).astype(np.int64)
        want = np.diff(plan(lens, L, S, K))
        assert (W.counts(lens, L, S, K) == want).all()
        for length, w in zip(lens.tolist(), want.tolist()):
            if w > 1:
                assert W.starts(length, L, w) == (fill([0], [length], L, S, K)[0]).tolist()
    assert W.check_params(100) == (100, 32) and W.check_params(100, 7, 4096) == (7, 4096)
    for bad in ((100, 0, 32), (100, 2 ** 31, 32), (100, 100, 0), (100, 100, 4097)):
        with pytest.raises(RuntimeError, match="windows"):
            W.check_params(*bad)


def test_fusions_of_the_reference():
    w = np.array([[1.0, 2.0], [0.5, 0.25], [3.0, 3.0], [1.0, 2.0], [-1.0, 0.0], [7.0, 7.5]], dtype=np.float32)
    first = np.array([0, 1, 3, 6])
    out, lab = fuse(w, first, "mean")
    assert out[0].tobytes() == w[0].tobytes()                      # W == 1: bit for bit
    assert out[1].tolist() == [1.75, 1.625] and lab.tolist() == [1, 0, 1]
    assert out[2].tolist() == [np.float32(np.float32(7.0) / np.float32(3)), np.float32(np.float32(9.5) / np.float32(3))]
    out, lab = fuse(w, first, "max")
    assert out[1].tolist() == [3.0, 3.0] and lab[1] == 0           # d = -0.25, 0: the second window; a tie of the logits is label 0
    assert out[2].tolist() == [1.0, 2.0]                           # d = 1, 1, 0.5: the lowest window of the tie
    sent = (np.full((3, 2), -9.0, dtype=np.float32), np.full(3, 7, dtype=np.uint8))
    out, lab = fuse(w, first, "mean", only_multi=True, into=sent)
    assert out[0].tolist() == [-9.0, -9.0] and lab.tolist() == [7, 0, 1] and out[1].tolist() == [1.75, 1.625]


# ---- the CLI's argument errors: before anything touches a device ---------------------------------------------------------------------------
def _predictor(argv):
    from ribodetector_amd import detect
    from ribodetector_amd.parse_config import ConfigParser
    args = detect.build_parser().parse_args(argv)
    p = detect.Predictor(ConfigParser.from_json(os.path.join(ROOT, "ribodetector_amd", "config.json")), args)
    p.len = args.len                       # (load_model sets it; no model is loaded here)
    ran = []
    p.run = lambda: ran.append("run")
    p.run_with_chunks = lambda *a, **k: ran.append("chunks")
    return p, ran


BAD_ARGS = [
    (["--window_stride", "50"], "--window_stride needs --windows"),
    (["--max_windows", "4"], "--max_windows needs --windows"),
    (["--window_fuse", "max"], "--window_fuse needs --windows"),
    (["--windows", "--window_stride", "0"], "--window_stride must be in"),
    (["--windows", "--window_stride", "-3"], "--window_stride must be in"),
    (["--windows", "--window_stride", str(2 ** 31)], "--window_stride must be in"),
    (["--windows", "--max_windows", "0"], "--max_windows must be in"),
    (["--windows", "--max_windows", "4097"], "--max_windows must be in"),
]


@pytest.mark.parametrize("extra,msg", BAD_ARGS)
def test_argument_errors(tmp_path, extra, msg, monkeypatch):
    from ribodetector_amd import detect
    base = ["-l", "100", "-i", str(tmp_path / "a.fq"), "-o", str(tmp_path / "o.fq")]
    with pytest.raises(RuntimeError, match=msg):
        detect.check_windows(detect.build_parser().parse_args(base + extra))
    p, ran = _predictor(base + extra)
    with pytest.raises(RuntimeError, match=msg):
        p.detect()
    assert ran == []
    # main() refuses before it loads a model: a load would raise its own error on a machine without a GPU, or initialise one
    monkeypatch.setattr(detect.Predictor, "load_model", lambda self: (_ for _ in ()).throw(AssertionError("load_model was reached")))
    with pytest.raises(RuntimeError, match=msg):
        detect.main(base + extra)


def test_arguments_accepted(tmp_path):
    from ribodetector_amd import detect
    base = ["-l", "100", "-i", str(tmp_path / "a.fq"), "-o", str(tmp_path / "o.fq")]
    assert detect.check_windows(detect.build_parser().parse_args(base)) is None
    assert detect.check_windows(detect.build_parser().parse_args(base + ["--windows"])) == {"stride": None, "max_per_read": 32, "fuse": "mean"}
    got = detect.check_windows(detect.build_parser().parse_args(base + ["--windows", "--window_stride", str(2 ** 31 - 1), "--max_windows", "4096",
                                                                        "--window_fuse", "max"]))
    assert got == {"stride": 2 ** 31 - 1, "max_per_read": 4096, "fuse": "max"}
    with pytest.raises(SystemExit):
        detect.build_parser().parse_args(base + ["--windows", "--window_fuse", "sum"])
    p, ran = _predictor(base + ["--windows", "--max_windows", "1"])
    p.detect()
    assert ran == ["run"] and p._windows["max_per_read"] == 1
    help_ = detect.build_parser().format_help()
    assert all(f in help_ for f in ("--windows", "--window_stride", "--max_windows", "--window_fuse"))


def test_summary_document_gains_windows_only_under_the_flag():
    from ribodetector_amd import summary as S
    acc = np.zeros(S.WORDS, dtype=np.int64)
    meta = {"version": "x", "paired": False, "interleaved": False, "len": 100, "ensure": "none", "model": "mcc", "inputs": ["a.fq"]}
    assert "windows" not in S.to_json(acc, meta) and "windows" not in S.to_json(acc, dict(meta, windows=None))
    w = {"stride": 100, "max_per_read": 32, "fuse": "mean", "classified": [12]}
    doc = S.to_json(acc, dict(meta, windows=w))
    assert doc["windows"] == w and {k: v for k, v in doc.items() if k != "windows"} == S.to_json(acc, meta)


# ---- the entry points' refusals: no pointer is dereferenced and nothing is launched ------------------------------------------------------
def test_window_entry_points_refuse_bad_arguments_without_gpu():
    from ribodetector_amd import _native as N
    L = N.lib()
    P, Q, big = 0x10000, 0x10001, 1 << 40

    def refused(name, args, code, word):
        rc = getattr(L, name)(*args)
        msg = L.rd_last_error()
        assert rc == code and msg.startswith(name.encode() + b":") and word in msg, (name, args, rc, msg)

    def plan_(seq_len=P, n=10, max_len=100, stride=100, most=32, first=P, info=P, ws=P, ws_bytes=big):
        return (seq_len, n, max_len, stride, most, first, info, ws, ws_bytes, None)

    def fill_(off=P, seq_len=P, first=P, n=10, max_len=100, stride=100, most=32, total=10, wo=P, wl=P):
        return (off, seq_len, first, n, max_len, stride, most, total, wo, wl, None)

    for name, mk in (("rd_window_plan", plan_), ("rd_window_fill", fill_)):
        refused(name, mk(n=-1), -1, b"n=-1 out of range")
        refused(name, mk(n=1 << 31), -1, b"out of range")
        refused(name, mk(max_len=0), -1, b"max_len=0")
        refused(name, mk(stride=0), -1, b"stride=0")
        refused(name, mk(stride=1 << 31), -1, b"stride=2147483648")
        refused(name, mk(most=0), -1, b"max_windows=0")
        refused(name, mk(most=4097), -1, b"max_windows=4097")
        refused(name, mk(seq_len=None), -1, b"null")
        refused(name, mk(first=None), -1, b"null")
    refused("rd_window_plan", plan_(info=None), -1, b"null")
    refused("rd_window_plan", plan_(ws=None), -1, b"null")
    refused("rd_window_plan", plan_(ws=Q), -1, b"aligned")
    refused("rd_window_plan", plan_(ws_bytes=0), -4, b"workspace too small")
    refused("rd_window_plan", plan_(n=4096, ws_bytes=int(L.rd_window_workspace_bytes(4096)) - 1), -4, b"workspace too small")
    refused("rd_window_fill", fill_(off=None), -1, b"null")
    refused("rd_window_fill", fill_(wo=None), -1, b"null")
    refused("rd_window_fill", fill_(wl=None), -1, b"null")
    refused("rd_window_fill", fill_(total=9), -1, b"total=9")            # fewer windows than reads
    refused("rd_window_fill", fill_(total=321), -1, b"total=321")        # more than max_windows per read

    def fuse_(wl=P, first=P, n=10, mode=0, only=0, logits=P, labels=None):
        return (wl, first, n, mode, only, logits, labels, None)
    refused("rd_window_fuse", fuse_(n=-1), -1, b"out of range")
    refused("rd_window_fuse", fuse_(mode=2), -1, b"unknown mode 2")
    refused("rd_window_fuse", fuse_(mode=-1), -1, b"unknown mode")
    refused("rd_window_fuse", fuse_(wl=None), -1, b"null")
    refused("rd_window_fuse", fuse_(first=None), -1, b"null")
    refused("rd_window_fuse", fuse_(logits=None), -1, b"null")
    refused("rd_window_fuse", fuse_(logits=P + 4), -1, b"aligned")
    # the sizing function: a block sum per 2,048 entries of the scan (n + 1 entries) and the fault word, each a 256-byte piece
    assert [int(L.rd_window_workspace_bytes(n)) for n in (-1, 0, 1, 2047, 2048, 65535, 65536, 1 << 20)] == [0, 512, 512, 512, 512, 512, 768, 4608]
    assert int(L.rd_window_workspace_bytes(1 << 31)) == 0
    assert (N.WINDOW_MAX, N.WINDOW_FUSE) == (4096, {"mean": 0, "max": 1})
