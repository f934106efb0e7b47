"""--windows on the GPU: rd_window_plan / rd_window_fill / rd_window_fuse bit for bit against the numpy reference of
tests/test_windows_host.py, SeqModel.classify_windows against the CPU oracle over the reference window table, and the CLI with the
flag against the CLI without it (where no read is longer than -l) and against classify_windows (where reads are)."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_interleaved as I  # noqa: E402
import test_interleaved_host as IH  # noqa: E402
import test_windows_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["none", "rrna", "norrna", "both"]
SMALL = I.SMALL                 # chunks of 1,024 reads / 512 pairs at -l 100


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _plan_fill(offs, lens, L, S, K):
    """rd_window_plan and rd_window_fill through the C ABI -> (win_first, win_off, win_len as numpy, info as a list)"""
    import torch
    from ribodetector_amd import _native as N
    lib = N.lib()
    n = len(lens)
    d_off, d_len = _dev(np.asarray(offs, dtype=np.int64)), _dev(np.asarray(lens, dtype=np.int32))
    first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    info = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(int(lib.rd_window_workspace_bytes(n)), dtype=torch.uint8, device="cuda:0")
    st = N.stream_ptr(torch.device("cuda:0"))
    N.check(lib.rd_window_plan(N.ptr(d_len), n, L, S, K, N.ptr(first), N.ptr(info), N.ptr(ws), ws.numel(), st), "rd_window_plan")
    info = [int(x) for x in info.cpu()]
    if info[3]:
        return first.cpu().numpy(), None, None, info
    total = info[1]
    wo = torch.full((total + 1,), -7, dtype=torch.int64, device="cuda:0")          # (one entry more: it must stay untouched)
    wl = torch.full((total + 1,), -7, dtype=torch.int32, device="cuda:0")
    N.check(lib.rd_window_fill(N.ptr(d_off), N.ptr(d_len), N.ptr(first), n, L, S, K, total, N.ptr(wo), N.ptr(wl), st), "rd_window_fill")
    torch.cuda.synchronize()
    wo, wl = wo.cpu().numpy(), wl.cpu().numpy()
    assert wo[total] == -7 and wl[total] == -7
    return first.cpu().numpy(), wo[:total], wl[:total], info


def _lengths(n, seed, L=100):
    """about 5 % of the reads longer than L, and the hand cases of the host test planted at random rows"""
    rng = np.random.default_rng(seed)
    lens = np.where(rng.random(n) < 0.05, rng.integers(L + 1, 40 * L, n), rng.integers(0, L + 1, n)).astype(np.int64)
    if n >= 4 * len(H.HAND_LENS):
        lens[rng.choice(n, len(H.HAND_LENS), replace=False)] = H.HAND_LENS
    offs = rng.integers(0, 1 << 40, n).astype(np.int64)         # (no text is read: any offsets will do)
    return offs, lens


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, (1 << 17) + 3, 256 * 2048 + 1])      # (the last: 257 scan blocks, a second trip of the base pass)
def test_plan_and_fill_against_the_reference(n):
    for L, S, K in ((100, 100, 32), (100, 37, 4096)) + (((4, 1, 5),) if n <= 2049 else ()):
        offs, lens = _lengths(n, 1000 + n, L)
        if n == 1:
            lens[0] = 2 ** 31 - 1
        first, wo, wl, info = _plan_fill(offs, lens, L, S, K)
        want_first = H.plan(lens, L, S, K)
        want_wo, want_wl = H.fill(offs, lens, L, S, K)
        assert info == [n, int(want_first[-1]), 0, 0]
        assert first.dtype == np.int64 and np.array_equal(first, want_first)
        if n:
            assert wo.dtype == np.int64 and wl.dtype == np.int32 and np.array_equal(wo, want_wo) and np.array_equal(wl, want_wl)
    if n >= 2048:
        assert (np.diff(want_first) > 1).sum() > 20 and (np.diff(want_first) == 1).sum() > n // 2


def test_plan_reports_a_negative_length():
    offs, lens = _lengths(5000, 3)
    for row in (0, 2047, 4999):
        bad = lens.copy()
        bad[row] = -1
        _, _, _, info = _plan_fill(offs, bad, 100, 100, 32)
        assert info[3] != 0 and info[0] == 5000, row
    assert _plan_fill(offs, lens, 100, 100, 32)[3][3] == 0


def _fuse(win_logits, first, mode, only_multi=False, into=None, want_labels=True):
    import torch
    from ribodetector_amd import _native as N
    n = len(first) - 1
    wl = _dev(np.asarray(win_logits, dtype=np.float32).reshape(-1, 2)) if len(win_logits) else torch.empty((1, 2), dtype=torch.float32, device="cuda:0")
    out = _dev(into[0]) if into is not None else torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda:0")
    lab = _dev(into[1]) if into is not None else torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    N.check(N.lib().rd_window_fuse(N.ptr(wl), N.ptr(_dev(np.asarray(first, dtype=np.int64))), n, N.WINDOW_FUSE[mode], 1 if only_multi else 0, N.ptr(out),
                                   N.ptr(lab if want_labels else None), N.stream_ptr(torch.device("cuda:0"))), "rd_window_fuse")
    torch.cuda.synchronize()
    return out.cpu().numpy(), lab.cpu().numpy()


def _fuse_case(n, seed):
    """window counts (most reads 1; some 2..40; a read of 4,096 windows when there is room) and fp32 window logits with exact ties in d"""
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(n) < 0.3, rng.integers(2, 41, n), 1).astype(np.int64)
    if n >= 1:
        w[n // 2] = 4096
    first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(w)])
    total = int(first[-1])
    wl = (rng.standard_normal((total, 2)) * 4).astype(np.float32)
    for i in np.flatnonzero(w > 1)[::3]:                    # ties of the largest d: a window repeated, and another pair of logits with the same d
        f, k = int(first[i]), int(w[i])
        wl[f:f + k] = np.round(wl[f:f + k] * 8) / 8         # (eighths: the differences are exact)
        j = f + int(np.argmax(wl[f:f + k, 1] - wl[f:f + k, 0]))
        t = f + (j - f + 1) % k
        wl[t] = wl[j] + np.float32(2.0)
    return first, wl


@pytest.mark.parametrize("n", [0, 1, 2049])
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_fuse_against_the_reference(n, mode):
    first, wl = _fuse_case(n, 50 + n)
    want, want_lab = H.fuse(wl, first, mode)
    got, got_lab = _fuse(wl, first, mode)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_lab, want_lab)
    if n > 1:
        d = wl[:, 1] - wl[:, 0]
        ties = sum(1 for i in range(n) if first[i + 1] - first[i] > 1 and (d[first[i]:first[i + 1]] == d[first[i]:first[i + 1]].max()).sum() > 1)
        assert ties > 50 and (np.diff(first) == 4096).any()
    # only_multi: the rows of one-window reads keep what they held, logits and labels
    sent = (np.full((n, 2), -9.5, dtype=np.float32), np.full(n, 7, dtype=np.uint8))
    want, want_lab = H.fuse(wl, first, mode, only_multi=True, into=sent)
    got, got_lab = _fuse(wl, first, mode, only_multi=True, into=sent)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_lab, want_lab)
    one = np.diff(first) == 1
    assert (got[one] == -9.5).all() and (got_lab[one] == 7).all() and (got[~one] != -9.5).any(axis=1).all()
    # no labels wanted: the logits alone
    got, got_lab = _fuse(wl, first, mode, want_labels=False)
    assert got.tobytes() == H.fuse(wl, first, mode)[0].tobytes() and (got_lab == 9).all()


# ---- SeqModel.classify_windows against the oracle ------------------------------------------------------------------------------------------
def mixed_reads(n_short, n_long, seed, short=(30, 100), long_=(101, 1000)):
    """synthetic reads, n_long of them longer than 100 bases, in a seeded random order: (arena, offsets int64[n + 1], lens int32[n])"""
    from ribodetector_amd import synth
    a1, o1, l1 = synth.reads_numpy(n_short, short, seed=seed, rrna_frac=0.3)
    a2, o2, l2 = synth.reads_numpy(n_long, long_, seed=seed + 1, rrna_frac=0.3)
    order = np.random.default_rng(seed + 2).permutation(n_short + n_long)
    seqs = [a1[o1[i]:o1[i + 1]] for i in range(n_short)] + [a2[o2[i]:o2[i + 1]] for i in range(n_long)]
    seqs = [seqs[i] for i in order]
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    offs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens, dtype=np.int64)])
    return np.concatenate(seqs), offs, lens


ORACLE_SEED = 2024


def oracle_windows(oracle, arena, offs, lens, L=100, S=100, K=32):
    """the oracle's logits of every window of the reference window table: (win_first, fp32[total, 2])"""
    first = H.plan(lens, L, S, K)
    wo, wl = H.fill(offs[:-1], lens, L, S, K)
    return first, oracle.forward_packed(arena, wo, wl, L)


@pytest.fixture(scope="module")
def oracle_case(oracle):
    """2,048 reads of 30..1,000 bases, one in three longer than -l 100, and the oracle's window logits (computed once, read only)"""
    arena, offs, lens = mixed_reads(1365, 683, ORACLE_SEED)
    first, wl = oracle_windows(oracle, arena, offs, lens)
    wl.setflags(write=False)
    return {"arena": arena, "offs": offs, "lens": lens, "first": first, "win_logits": wl}


def _batch(arena, offs, lens):
    return _dev(arena), _dev(np.asarray(offs[:len(lens)], dtype=np.int64)), _dev(np.asarray(lens, dtype=np.int32))


def test_classify_windows_mean_against_the_oracle(gpu_model, oracle_case):
    import torch
    c = oracle_case
    assert len(c["lens"]) == 2048 and 600 < (c["lens"] > 100).sum() < 760
    want, _ = H.fuse(c["win_logits"], c["first"], "mean")
    margin = np.abs(want[:, 1] - want[:, 0])
    assert (margin < 2e-4).sum() <= 1                       # the seed: the oracle alone leaves at most one read inside the band
    logits, labels, total = gpu_model.classify_windows(*_batch(c["arena"], c["offs"], c["lens"]), 100)
    torch.cuda.synchronize()
    got, lab = logits.cpu().numpy(), labels.cpu().numpy()
    assert total == c["first"][-1] and got.shape == (2048, 2) and got.dtype == np.float32
    err = float(np.abs(got - want).max())
    print("classify_windows mean: max |fused - oracle| = %.3g over %d windows" % (err, total))
    assert err <= 1e-4
    sure = margin >= 2e-4
    assert np.array_equal(lab[sure], (want[sure, 1] > want[sure, 0]).astype(np.uint8))
    assert np.array_equal(lab, (got[:, 1] > got[:, 0]).astype(np.uint8))


def test_classify_windows_max_against_the_oracle(gpu_model, oracle_case):
    import torch
    c = oracle_case
    logits, labels, _ = gpu_model.classify_windows(*_batch(c["arena"], c["offs"], c["lens"]), 100, fuse="max")
    torch.cuda.synchronize()
    got, wl, first = logits.cpu().numpy(), c["win_logits"], c["first"]
    d = wl[:, 1] - wl[:, 0]
    for i in range(len(c["lens"])):
        f, e = int(first[i]), int(first[i + 1])
        near = [j for j in range(f, e) if d[j] >= d[f:e].max() - 2e-4]
        assert min(float(np.abs(got[i] - wl[j]).max()) for j in near) <= 1e-4, i
    assert np.array_equal(labels.cpu().numpy(), (got[:, 1] > got[:, 0]).astype(np.uint8))


def test_one_window_reads_are_classify_bytes_bit_for_bit(gpu_model, oracle_case):
    import torch
    c = oracle_case
    b = _batch(c["arena"], c["offs"], c["lens"])
    ref, ref_lab = gpu_model.classify_bytes(*b, 100)
    gpu_model.sync_results()
    torch.cuda.synchronize()
    ref, ref_lab = ref.cpu().numpy(), ref_lab.cpu().numpy()
    one = c["lens"] <= 100
    for fuse in ("mean", "max"):
        logits, labels, total = gpu_model.classify_windows(*b, 100, fuse=fuse)
        torch.cuda.synchronize()
        assert total > 2048 and logits.cpu().numpy()[one].tobytes() == ref[one].tobytes()
        assert np.array_equal(labels.cpu().numpy()[one], ref_lab[one])
        # the long reads are not the truncated reads (under "max" they are where the read's first window wins: one read in W)
        assert (logits.cpu().numpy()[~one] != ref[~one]).any(axis=1).mean() > (0.9 if fuse == "mean" else 0.5)
        # max_windows = 1: every read is its own entry
        logits, labels, total = gpu_model.classify_windows(*b, 100, max_windows=1, fuse=fuse)
        torch.cuda.synchronize()
        assert total == 2048 and logits.cpu().numpy().tobytes() == ref.tobytes() and np.array_equal(labels.cpu().numpy(), ref_lab)
    # a stride of its own, sliced classify calls: the fused logits do not depend on the slicing
    full = gpu_model.classify_windows(*b, 100, stride=37, max_windows=4096)
    torch.cuda.synchronize()
    old = gpu_model.WINDOW_SLICE
    gpu_model.WINDOW_SLICE = 1000
    try:
        sliced = gpu_model.classify_windows(*b, 100, stride=37, max_windows=4096)
        torch.cuda.synchronize()
    finally:
        gpu_model.WINDOW_SLICE = old
    assert full[2] == sliced[2] == H.plan(c["lens"], 100, 37, 4096)[-1] and full[0].cpu().numpy().tobytes() == sliced[0].cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="windows"):
        gpu_model.classify_windows(*b, 100, max_windows=4097)
    with pytest.raises(RuntimeError, match="fuse"):
        gpu_model.classify_windows(*b, 100, fuse="sum")


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
def _records(arena, offs, mate=None):
    b = arena.tobytes()
    out = []
    for i in range(len(offs) - 1):
        s = b[offs[i]:offs[i + 1]]
        out.append(b"@syn.%d%s\n%s\n+\n%s\n" % (i, b"/%d" % mate if mate else b"", s, b"I" * len(s)))
    return out


def _run_set(tmp, tag, inputs, ensure, extra=(), env=None, paired=None, gz=False, report=True, summary=True):
    """one CLI run with -o / -r (one file per input, or per mate), report and summary; returns (Predictor, {name: bytes}, summary dict)"""
    paired = len(inputs) == 2 if paired is None else paired
    ext = ".fq.gz" if gz else ".fq"
    names = ["o1", "o2", "r1", "r2"] if paired else ["o1", "r1"]
    f = {k: str(tmp / ("%s_%s%s" % (tag, k, ext))) for k in names}
    rep, summ = str(tmp / (tag + "_rep.tsv")), str(tmp / (tag + "_sum.json"))
    o, r = [f[k] for k in names if k[0] == "o"], [f[k] for k in names if k[0] == "r"]
    args = ["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "-e", ensure] + (["--read_report", rep] if report else []) + \
           (["--summary", summ] if summary else []) + list(extra) + SMALL
    p = I._run(args, env)
    files = {k: I._read(v) for k, v in f.items()}
    for k in [x for x in names if x[0] == "o"]:
        files["u" + k[1]] = I._read(f[k] + ".unclassified.gz")
    files["rep"] = I._read(rep) if report else None
    return p, files, (json.load(open(summ)) if summary else None)


def _minus_windows(doc):
    return {k: v for k, v in doc.items() if k != "windows"}


@pytest.fixture(scope="module")
def short_pairs(tmp_path_factory):
    """3,000 pairs of 60..100 bases: nothing is longer than -l 100"""
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("wshort")
    out = []
    for mate, seed in ((1, 61), (2, 62)):
        a, o, _ = synth.reads_numpy(3000, (60, 100), seed=seed, rrna_frac=0.3)
        out.append(str(d / ("s_%d.fq" % mate)))
        synth.write_fastq(out[-1], a, o, mate)
    return out


@pytest.mark.parametrize("ensure", MODES)
def test_cli_without_long_reads_the_flag_changes_nothing(tmp_path, short_pairs, ensure):
    p0, f0, s0 = _run_set(tmp_path, "plain", short_pairs, ensure)
    p1, f1, s1 = _run_set(tmp_path, "win", short_pairs, ensure, ["--windows"])
    assert p0.num_read == p1.num_read == 3000 and I._counters(p0) == I._counters(p1)
    assert f0 == f1 and len(f0["o1"]) > 0 and len(f0["r1"]) > 0 and len(f0["rep"]) > 0
    assert "windows" not in s0 and _minus_windows(s1) == s0
    assert s1["windows"] == {"stride": 100, "max_per_read": 32, "fuse": "mean", "classified": [3000, 3000]}
    if ensure == "rrna":                                    # ... and under the reference's CPU semantics (zero-padded input)
        p3, f3, s3 = _run_set(tmp_path, "cpu", short_pairs, ensure, ["--semantics", "cpu"])
        p4, f4, s4 = _run_set(tmp_path, "cpuwin", short_pairs, ensure, ["--semantics", "cpu", "--windows"])
        assert f3 == f4 and _minus_windows(s4) == s3 and f3 != f0          # (reads shorter than -l: the two semantics differ)
    if ensure == "none":                                    # ... and under the other fusion, and from the host's parser
        p2, f2, s2 = _run_set(tmp_path, "winmax", short_pairs, ensure, ["--windows", "--window_fuse", "max", "--window_stride", "10"], env={"RD_INGEST": "host"})
        assert f2 == f0 and _minus_windows(s2) == s0 and s2["windows"]["fuse"] == "max" and s2["windows"]["stride"] == 10


SE_SEED, PE_SEED = 71, 81


def se_mixed():
    """3,000 single-end reads of 50..700 bases, about one in three longer than 100"""
    return mixed_reads(2000, 1000, SE_SEED, short=(50, 100), long_=(101, 700))


def pe_250():
    """1,500 pairs of 250 bp mates"""
    from ribodetector_amd import synth
    return [synth.reads_numpy(1500, 250, seed=PE_SEED + m, rrna_frac=0.3) for m in (0, 1)]


@pytest.fixture(scope="module")
def se_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wse")
    arena, offs, lens = se_mixed()
    recs = _records(arena, offs)
    path = str(d / "mixed.fq")
    open(path, "wb").write(b"".join(recs))
    open(path + ".gz", "wb").write(gzip.compress(b"".join(recs), 6))
    return {"path": path, "recs": recs, "arrays": (arena, offs, lens)}


def _report_rows(blob):
    lines = blob.decode().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#read_id")
    return [ln.split("\t") for ln in lines[1:-1]]


def _p(logits):
    d = logits[:, 1].astype(np.float64) - logits[:, 0].astype(np.float64)
    return 1.0 / (1.0 + np.exp(-d))


def test_cli_max_windows_one_is_the_run_without_the_flag(tmp_path, se_files):
    p0, f0, s0 = _run_set(tmp_path, "plain", [se_files["path"]], "none")
    p1, f1, s1 = _run_set(tmp_path, "k1", [se_files["path"]], "none", ["--windows", "--max_windows", "1"])
    assert f0 == f1 and _minus_windows(s1) == s0 and s1["windows"]["classified"] == [3000] and s0["truncated_reads"] == 1000


@pytest.mark.parametrize("fuse", ["mean", "max"])
def test_cli_single_end_mixed_lengths(tmp_path, se_files, gpu_model, fuse):
    import torch
    arena, offs, lens = se_files["arrays"]
    recs = se_files["recs"]
    logits, labels, total = gpu_model.classify_windows(*_batch(arena, offs, lens), 100, fuse=fuse)
    trunc, _ = gpu_model.classify_bytes(*_batch(arena, offs, lens), 100)
    gpu_model.sync_results()
    torch.cuda.synchronize()
    logits, labels, trunc = logits.cpu().numpy(), labels.cpu().numpy(), trunc.cpu().numpy()
    assert total == H.plan(lens, 100, 100, 32)[-1] > 3000
    assert np.abs(logits[:, 1] - logits[:, 0]).min() > 2e-4             # the seed: no read of this file is inside the noise band
    extra = ["--windows"] + (["--window_fuse", "max"] if fuse == "max" else [])
    p, f, s = _run_set(tmp_path, "dev", [se_files["path"]], "none", extra)
    assert p.ingest["mixed.fq"]["path"] == "device"
    assert f["o1"] == b"".join(r for r, lab in zip(recs, labels) if lab == 0) and f["r1"] == b"".join(r for r, lab in zip(recs, labels) if lab == 1)
    assert (p.num_read, p.num_nonrrna, p.num_rrna) == (3000, int((labels == 0).sum()), int((labels == 1).sum())) and p.num_rrna > 300
    rows = _report_rows(f["rep"])
    assert [r[0] for r in rows] == ["syn.%d" % i for i in range(3000)] and [r[1] for r in rows] == [("rRNA" if lab else "nonrRNA") for lab in labels]
    got_p = np.array([float(r[2]) for r in rows])
    assert np.abs(got_p - _p(logits)).max() <= 0.51e-4                  # the fused logits' p_rrna (four decimals) ...
    assert (np.abs(got_p - _p(trunc)) > 1e-3).sum() > 100                # ... not the truncated reads'
    assert s["reads"] == {"total": 3000, "nonrRNA": int((labels == 0).sum()), "rRNA": int((labels == 1).sum()), "unclassified": 0,
                          "rRNA_fraction": round(int((labels == 1).sum()) / 3000, 6)}
    assert s["windows"] == {"stride": 100, "max_per_read": 32, "fuse": fuse, "classified": [int(total)]}
    assert s["truncated_reads"] == int((lens > 100).sum()) == 1000
    bins = np.minimum((np.rint(_p(logits) * 1e4) // 100).astype(int), 99)
    # (p_rrna bins of the summary: of the fused logits; a value on a bin's edge may fall either side of it in fp32)
    got_bins = np.array(s["p_rrna"]["mate1"]["rRNA"]) + np.array(s["p_rrna"]["mate1"]["nonrRNA"])
    assert got_bins.sum() == 3000 and np.abs(np.cumsum(got_bins) - np.cumsum(np.bincount(bins, minlength=100))).max() <= 2
    # the same files from the host's parser and from the .gz input
    for tag, inp, env in (("host", se_files["path"], {"RD_INGEST": "host"}), ("gz", se_files["path"] + ".gz", None), ("hostgz", se_files["path"] + ".gz", {"RD_INGEST": "host"})):
        p2, f2, s2 = _run_set(tmp_path, tag, [inp], "none", extra, env=env)
        assert f2 == f and {k: v for k, v in s2.items() if k != "inputs"} == {k: v for k, v in s.items() if k != "inputs"}, tag
        if env:
            assert p2.ingest.get(os.path.basename(inp), {}).get("path") != "device"


@pytest.fixture(scope="module")
def pe_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wpe")
    (a1, o1, l1), (a2, o2, l2) = pe_250()
    r1, r2 = _records(a1, o1, 1), _records(a2, o2, 2)
    i1, i2, il = str(d / "p_1.fq"), str(d / "p_2.fq"), str(d / "p_il.fq")
    open(i1, "wb").write(b"".join(r1))
    open(i2, "wb").write(b"".join(r2))
    open(il, "wb").write(b"".join(IH.interleave(r1, r2)))
    open(il + ".gz", "wb").write(gzip.compress(open(il, "rb").read(), 6))
    return {"i": [i1, i2], "il": il, "r": (r1, r2), "arrays": ((a1, o1, l1), (a2, o2, l2))}


@pytest.mark.parametrize("ensure", MODES)
def test_cli_pairs_of_250_bp_mates(tmp_path, pe_files, gpu_model, ensure):
    import torch
    from ribodetector_amd.model import model as M
    (a1, o1, l1), (a2, o2, l2) = pe_files["arrays"]
    r1, r2 = pe_files["r"]
    g1, _, t1 = gpu_model.classify_windows(*_batch(a1, o1, l1), 100, want_labels=False)
    g2, _, t2 = gpu_model.classify_windows(*_batch(a2, o2, l2), 100, want_labels=False)
    lab = M.pair_fuse(g1, g2, ensure)
    torch.cuda.synchronize()
    assert t1 == t2 == 4500
    g1, g2, lab = g1.cpu().numpy(), g2.cpu().numpy(), lab.cpu().numpy()
    m = [np.abs(g[:, 1] - g[:, 0]) for g in (g1, g2)] + [np.abs((g1[:, 1] + g2[:, 1]) - (g1[:, 0] + g2[:, 0]))]
    assert min(x.min() for x in m) > 2e-4                                # the seed: no mate and no pair inside the noise band
    p, f, s = _run_set(tmp_path, "two", pe_files["i"], ensure, ["--windows"])
    sel = lambda recs, want: b"".join(r for r, x in zip(recs, lab) if x == want)      # noqa: E731
    assert (f["o1"], f["o2"], f["r1"], f["r2"]) == (sel(r1, 0), sel(r2, 0), sel(r1, 1), sel(r2, 1))
    assert (p.num_read, p.num_nonrrna, p.num_rrna, p.num_unknown) == (1500, int((lab == 0).sum()), int((lab == 1).sum()), int((lab == -1).sum()))
    if ensure == "both":
        assert p.num_unknown > 0 and f["u1"] == sel(r1, -1) and f["u2"] == sel(r2, -1)
    rows = _report_rows(f["rep"])
    assert [r[1] for r in rows] == [{1: "rRNA", 0: "nonrRNA", -1: "unclassified"}[int(x)] for x in lab]
    for col, g in ((2, g1), (3, g2), (4, g1 + g2)):
        assert np.abs(np.array([float(r[col]) for r in rows]) - _p(g)).max() <= 0.51e-4
    assert s["windows"]["classified"] == [4500, 4500] and s["truncated_reads"] == 3000 and s["reads"]["total"] == 1500
    # host ingest, and the same pairs from one interleaved file (plain and .gz; device and host ingest): the same files
    same = lambda a, b: {k: v for k, v in a.items() if k != "inputs" and k != "interleaved"} == {k: v for k, v in b.items() if k != "inputs" and k != "interleaved"}      # noqa: E731
    # (-e none, whose float64 pass over the pairs is followed by the second fusion, takes every path; the other modes one each)
    if ensure in ("none", "both"):
        p2, f2, s2 = _run_set(tmp_path, "twohost", pe_files["i"], ensure, ["--windows"], env={"RD_INGEST": "host"})
        assert f2 == f and same(s2, s)
    runs = {"none": [("il", pe_files["il"], None), ("ilgz", pe_files["il"] + ".gz", None), ("ilhost", pe_files["il"], {"RD_INGEST": "host"})],
            "rrna": [("il", pe_files["il"], None)], "norrna": [("ilgz", pe_files["il"] + ".gz", None)], "both": []}[ensure]
    for tag, inp, env in runs:
        p3, f3, s3 = _run_set(tmp_path, tag, [inp], ensure, ["--windows", "--interleaved"], env=env, paired=True)
        assert f3 == f and same(s3, s), tag


def test_cli_fasta_with_a_contig(tmp_path):
    """a 200 kb contig among short records: 32 windows over it, one over every other record"""
    from ribodetector_amd import synth
    arena, offs, lens = synth.reads_numpy(2500, (60, 100), seed=91, rrna_frac=0.3)
    big, _, _ = synth.reads_numpy(1, 200000, seed=92, rrna_frac=1.0)
    seqs = [arena[offs[i]:offs[i + 1]].tobytes() for i in range(2500)]
    seqs.insert(1300, big.tobytes())
    fa = str(tmp_path / "c.fa")
    with open(fa, "wb") as fh:
        for i, s in enumerate(seqs):
            fh.write(b">rec.%d\n" % i + b"".join(s[k:k + 70] + b"\n" for k in range(0, len(s), 70)))
    o, r, summ = str(tmp_path / "o.fa"), str(tmp_path / "r.fa"), str(tmp_path / "s.json")
    p = I._run(["-l", "100", "-i", fa, "-o", o, "-r", r, "--windows", "--summary", summ] + SMALL)
    want = int(H.plan([len(s) for s in seqs], 100, 100, 32)[-1])
    s = json.load(open(summ))
    assert p.num_read == 2501 and want == 2500 + 32 and s["windows"]["classified"] == [want] and s["truncated_reads"] is not None
    names = [ln[1:] for blob in (I._read(o), I._read(r)) for ln in blob.decode().split("\n") if ln.startswith(">")]
    assert sorted(names) == sorted("rec.%d" % i for i in range(2501))
    p0 = I._run(["-l", "100", "-i", fa, "-o", str(tmp_path / "o0.fa"), "-r", str(tmp_path / "r0.fa")] + SMALL)
    assert p0.num_read == 2501 and abs(p0.num_rrna - p.num_rrna) <= 1       # (only the contig can change sides)


def test_cli_two_ranks_match_one(tmp_path, pe_files):
    """the 250 bp pairs from one interleaved .gz under two ranks (the label gather, sharded by windows x bases): the files of one rank"""
    inp = pe_files["il"] + ".gz"
    args = lambda t: ["-l", "100", "-i", inp, "--interleaved", "--windows", "-e", "both", "-o", str(tmp_path / (t + "_o.fq.gz")), "-r", str(tmp_path / (t + "_r.fq")),      # noqa: E731
                      "--read_report", str(tmp_path / (t + "_rep.tsv")), "--summary", str(tmp_path / (t + "_s.json"))] + SMALL
    p = I._run(args("a"))
    r, port = I._torchrun(2, args("b"))
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-3000:]
    assert "label-gather layout" in text and "4500 + 4500" in text and p.num_read == 1500
    for suffix in ("_o.fq.gz", "_r.fq", "_rep.tsv", "_o.fq.gz.unclassified.gz"):
        a, b = I._read(str(tmp_path / ("a" + suffix))), I._read(str(tmp_path / ("b" + suffix)))
        assert a == b and len(a) > 0, suffix
    sa, sb = (json.load(open(str(tmp_path / (t + "_s.json")))) for t in "ab")
    assert sa == sb and sa["windows"]["classified"] == [4500, 4500]
    assert not [x for x in os.listdir("/dev/shm") if x.startswith("rd_%d_" % port)]
