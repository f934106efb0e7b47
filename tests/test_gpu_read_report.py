"""--read_report on the GPU: the format kernel (rd_report_format through gz.DeviceReport) against the Python formatter of
tests/test_read_report_host.py, and the CLI's report against its own output files, the oracle's logits, the other ingest paths, chunk
sizes and two ranks."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_read_report_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _records(n, seed, fasta=False):
    """n records whose ids are empty, end in a space / tab / CR / newline, and are 1-300 bytes long"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTN", dtype=np.uint8)
    idch = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._:/-|#@>+", dtype=np.uint8)
    recs = []
    for i in range(n):
        k = rng.integers(0, 6)
        ln = 0 if k == 0 else int(rng.integers(1, 301)) if k == 1 else int(rng.integers(1, 40))
        rid = idch[rng.integers(0, len(idch), ln)].tobytes()
        end = [b" desc x", b"\tt", b"\r", b"", b" ", b"\x0bv"][int(rng.integers(0, 6))]
        nl = b"\r\n" if end == b"\r" else b"\n"
        end = b"" if end == b"\r" else end
        seq = alpha[rng.integers(0, 5, int(rng.integers(1, 150)))].tobytes()
        if fasta:
            recs.append(b">" + rid + end + nl + seq + b"\n")
        else:
            recs.append(b"@" + rid + end + nl + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return recs


def _logits(n, rng):
    lg = rng.normal(0, 4, (n, 2)).astype(np.float32)
    k = rng.integers(0, 5, n)
    lg[k == 0, 1] = lg[k == 0, 0]                                             # ties
    lg[k == 1] = np.array([[-40, 40], [40, -40]], dtype=np.float32)[rng.integers(0, 2, int((k == 1).sum()))]
    lg[k == 2, 1] = lg[k == 2, 0] + rng.choice([1e-6, -1e-6, 3e-5, -2e-4], int((k == 2).sum())).astype(np.float32)   # tiny margins
    return lg


def _device_report(recs, la, lb, labels):
    import torch
    from ribodetector_amd.gz import DeviceReport
    text = b"".join(recs)
    rs = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=rs[1:])
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    rep = DeviceReport(dev)
    out, ls, info = rep.format(t, torch.from_numpy(rs).to(dev), torch.from_numpy(la).to(dev), None if lb is None else torch.from_numpy(lb).to(dev),
                               torch.from_numpy(np.asarray(labels, dtype=np.int8)).to(dev))
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    return rep, out, ls, info, t, rs


@pytest.mark.parametrize("fasta", [False, True])
@pytest.mark.parametrize("paired", [False, True])
def test_format_kernel_against_python(fasta, paired):
    import torch
    from ribodetector_amd.gz import DeviceGzip
    for n in (12500, 255, 256, 257):                           # x 4 cases = 50k records; then one tile of the write pass: a line short, full, a line more
        rng = np.random.default_rng(5 + 2 * fasta + paired)
        recs = _records(n, 11 + 2 * fasta + paired, fasta=fasta)
        la = _logits(n, rng)
        lb = _logits(n, rng) if paired else None
        labels = rng.integers(-1 if paired else 0, 2, n)
        rep, out, ls, info, t, rs = _device_report(recs, la, lb, labels)
        assert int(info[3]) == 0 and int(info[0]) == n, n
        nb = int(info[1])
        got = out[:nb].cpu().numpy().tobytes()
        want = H.format_lines(recs, labels, la, lb)
        _, g = H.parse(b"#\n" + got)
        _, w = H.parse(b"#\n" + want)
        assert len(g) == len(w) == n, n
        assert [r[:2] for r in g] == [r[:2] for r in w], n           # ids and labels byte for byte
        dq = np.abs(np.array([r[2] for r in g]) - np.array([r[2] for r in w]))
        assert dq.max() <= 1, n
        starts = ls.cpu().numpy()
        lens = np.array([len(x) + 1 for x in got.split(b"\n")[:-1]])
        assert starts[0] == 0 and (np.diff(starts) == lens).all() and starts[-1] == nb, n
        # the line starts are a record table of the report text: the device gzip deflates all of it
        comp, ginfo = DeviceGzip("cuda:0").compress_selected(out, ls, rep.zeros(n), 0)
        torch.cuda.synchronize()
        assert gzip.decompress(comp[: int(ginfo[0])].cpu().numpy().tobytes()) == got, n


def test_format_kernel_faults():
    import torch
    recs = _records(3000, 3)
    rng = np.random.default_rng(3)
    la = _logits(3000, rng)
    labels = rng.integers(0, 2, 3000)
    _, _, _, info, t, rs = _device_report(recs, la, None, labels)
    assert int(info[3]) == 0
    from ribodetector_amd.gz import DeviceReport
    dev = torch.device("cuda:0")
    rep = DeviceReport(dev)
    lt, labt = torch.from_numpy(la).to(dev), torch.from_numpy(labels.astype(np.int8)).to(dev)
    stray = rs.copy()
    stray[1700] += len(recs[1699].split(b"\n")[0]) + 1           # a start on the sequence line
    long_hdr = rs.copy()
    long_hdr[900] = rs[899] + 1                                  # a record that ends inside its header
    for bad in (stray, long_hdr):
        _, _, info = rep.format(t, torch.from_numpy(bad).to(dev), lt, None, labt)
        torch.cuda.synchronize()
        assert int(info[3]) != 0 and int(info[1]) == 0
    # a report larger than out_cap
    ls = torch.empty(3001, dtype=torch.int64, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    small = torch.empty(4096, dtype=torch.uint8, device=dev)
    from ribodetector_amd import _native as N
    ws = torch.empty(int(N.lib().rd_report_workspace_bytes(3000)), dtype=torch.uint8, device=dev)
    N.check(N.lib().rd_report_format(N.ptr(t), t.numel(), N.ptr(torch.from_numpy(rs).to(dev)), 3000, N.ptr(lt), None, N.ptr(labt), N.ptr(small),
                                     small.numel(), N.ptr(ls), N.ptr(info), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "rd_report_format")
    torch.cuda.synchronize()
    assert int(info[3]) == 1


def _ids(path):
    op = gzip.open if path.endswith("gz") else open
    with op(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    return [ln[1:].split()[0] if len(ln) > 1 else b"" for ln in lines[0::4] if ln]


def _softmax1(g):
    d = g[:, 1].astype(np.float64) - g[:, 0].astype(np.float64)
    return 1.0 / (1.0 + np.exp(-d))


def test_cli_single_end_report(tmp_path, oracle):
    from ribodetector_amd import detect, synth
    arena, off, lens = synth.reads_numpy(10000, 100, seed=0)
    inp = str(tmp_path / "in.fq")
    synth.write_fastq(inp, arena, off, mate=1)
    out, rr, rep = str(tmp_path / "n.fq"), str(tmp_path / "r.fq"), str(tmp_path / "rep.tsv")
    p = detect.main(["-l", "100", "-i", inp, "-o", out, "-r", rr, "--chunk_size", "1", "-m", "3", "-t", "2", "--read_report", rep])
    assert p.num_read == 10000
    hdr, rows = H.parse(H.read_report(rep))
    assert hdr == H.header(False) and len(rows) == 10000
    assert [r[0] for r in rows] == [b"syn.%d/1" % i for i in range(10000)]
    assert [r[0] for r in rows if r[1] == b"rRNA"] == _ids(rr)
    assert [r[0] for r in rows if r[1] == b"nonrRNA"] == _ids(out)
    pr = _softmax1(oracle.forward_packed(arena, off, lens, 100))
    assert np.abs(np.array([r[2][0] for r in rows]) / 1e4 - pr).max() <= 1e-4
    gzrep = str(tmp_path / "rep.tsv.gz")
    detect.main(["-l", "100", "-i", inp, "-o", str(tmp_path / "n2.fq"), "--read_report", gzrep])
    assert subprocess.run(["gzip", "-t", gzrep]).returncode == 0
    assert H.read_report(gzrep) == H.read_report(rep)


@pytest.mark.parametrize("ensure", ["none", "rrna", "norrna", "both"])
def test_cli_paired_report(tmp_path, oracle, ensure):
    from ribodetector_amd import detect, synth
    n = 3000
    a1, o1, l1 = synth.reads_numpy(n, (60, 120), seed=41, rrna_frac=0.3)
    a2, o2, l2 = synth.reads_numpy(n, (60, 120), seed=42, rrna_frac=0.3)
    i1, i2 = str(tmp_path / "r_1.fq.gz"), str(tmp_path / "r_2.fq.gz")
    synth.write_fastq(i1, a1, o1, 1)
    synth.write_fastq(i2, a2, o2, 2)
    outs = [str(tmp_path / "n1.fq"), str(tmp_path / "n2.fq")]
    rrs = [str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")]
    rep = str(tmp_path / "rep.tsv.gz")
    detect.main(["-l", "100", "-i", i1, i2, "-o", *outs, "-r", *rrs, "-e", ensure, "--chunk_size", "1", "-m", "3", "--read_report", rep])
    hdr, rows = H.parse(H.read_report(rep))
    assert hdr == H.header(True) and len(rows) == n
    assert [r[0] for r in rows if r[1] == b"rRNA"] == _ids(rrs[0])
    assert [r[0] for r in rows if r[1] == b"nonrRNA"] == _ids(outs[0])
    unc = [r[0] for r in rows if r[1] == b"unclassified"]
    if ensure == "both":
        assert len(unc) > 0 and unc == _ids(outs[0] + ".unclassified.gz")
    else:
        assert unc == []
    g1, g2 = oracle.forward_packed(a1, o1, l1, 100), oracle.forward_packed(a2, o2, l2, 100)
    q = np.array([r[2] for r in rows])
    assert np.abs(q[:, 0] / 1e4 - _softmax1(g1)).max() <= 1e-4 and np.abs(q[:, 1] / 1e4 - _softmax1(g2)).max() <= 1e-4
    assert np.abs(q[:, 2] / 1e4 - _softmax1(g1 + g2)).max() <= 1e-4
    if ensure == "none":
        lab = np.array([r[1] for r in rows])
        assert (lab[q[:, 2] > 5000] == b"rRNA").all() and (lab[q[:, 2] < 5000] == b"nonrRNA").all()


def _crlf_fastq(path, n, seed):
    from ribodetector_amd import synth
    arena, off, _ = synth.reads_numpy(n, (50, 150), seed=seed, rrna_frac=0.3)
    b = arena.tobytes()
    with open(path, "wb") as fh:
        for i in range(n):
            s = b[off[i]:off[i + 1]]
            fh.write(b"@r%d extra words\r\n%s\r\n+\r\n%s\r\n" % (i, s, b"I" * len(s)))


@pytest.mark.parametrize("kind", ["fq", "crlf", "fa"])
def test_report_same_bytes_across_paths(tmp_path, monkeypatch, kind):
    from ribodetector_amd import detect, synth
    inp = str(tmp_path / ("in.fa" if kind == "fa" else "in.fq"))
    if kind == "crlf":
        _crlf_fastq(inp, 6000, 8)
    else:
        arena, off, _ = synth.reads_numpy(6000, (40, 150), seed=9, rrna_frac=0.3)
        if kind == "fa":
            b = arena.tobytes()
            with open(inp, "wb") as fh:
                for i in range(6000):
                    fh.write(b">s%d\tx\n%s\n" % (i, b[off[i]:off[i + 1]]))
        else:
            synth.write_fastq(inp, arena, off, mate=1)
    reps = []
    for k, (ingest, chunk) in enumerate([("device", None), ("host", None), ("device", "1"), ("host", "1")]):
        monkeypatch.setenv("RD_INGEST", ingest)
        rep = str(tmp_path / ("rep%d.tsv" % k))
        detect.main(["-l", "100", "-i", inp, "-o", str(tmp_path / ("o%d.fq" % k)), "-m", "3", "--read_report", rep]
                    + (["--chunk_size", chunk] if chunk else []))
        reps.append(open(rep, "rb").read())
    assert all(r == reps[0] for r in reps)
    _, rows = H.parse(reps[0])
    assert len(rows) == 6000 and rows[5][0] == (b"s5" if kind == "fa" else b"r5" if kind == "crlf" else b"syn.5/1")


def test_report_of_empty_input(tmp_path):
    from ribodetector_amd import detect
    inp = str(tmp_path / "e.fq")
    open(inp, "wb").close()
    rep = str(tmp_path / "rep.tsv.gz")
    detect.main(["-l", "100", "-i", inp, "-o", str(tmp_path / "o.fq"), "--read_report", rep])
    assert H.read_report(rep) == H.header(False)


def _torchrun(world, args, env_extra=None, timeout=900):
    import socket
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RD_DIST_BACKEND="gloo", RD_LOCAL_DEVICE="0", PYTHONPATH=root, **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ribodetector_amd.detect"] + list(args)
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=timeout)
    return r, port


def test_report_two_ranks(tmp_path):
    from ribodetector_amd import detect, synth
    n = 20000
    a1, o1, _ = synth.reads_numpy(n, (60, 120), seed=61, rrna_frac=0.3)
    a2, o2, _ = synth.reads_numpy(n, (60, 120), seed=62, rrna_frac=0.3)
    i1, i2 = str(tmp_path / "p_1.fq"), str(tmp_path / "p_2.fq")
    synth.write_fastq(i1, a1, o1, 1)
    synth.write_fastq(i2, a2, o2, 2)
    # sharded parse: every rank writes a part of the report, rank 0's with the header
    one = str(tmp_path / "one.tsv")
    detect.main(["-l", "100", "-i", i1, i2, "-o", str(tmp_path / "a1.fq"), str(tmp_path / "a2.fq"), "-e", "both", "--chunk_size", "1", "-m", "3",
                 "--read_report", one])
    two = str(tmp_path / "two.tsv")
    r, _ = _torchrun(2, ["-l", "100", "-i", i1, i2, "-o", str(tmp_path / "b1.fq"), str(tmp_path / "b2.fq"), "-e", "both", "--chunk_size", "1", "-m", "3",
                         "--read_report", two])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Rank 1 parses" in r.stdout + r.stderr
    assert open(two, "rb").read() == open(one, "rb").read() and len(H.parse(open(one, "rb").read())[1]) == n
    # a stored-block gzip that the range decoder refuses: the label gather - every rank formats its shard, rank 0 writes the pieces
    lvl0 = str(tmp_path / "stored.fq.gz")
    open(lvl0, "wb").write(gzip.compress(open(i1, "rb").read(), 0))
    one = str(tmp_path / "one_se.tsv.gz")
    detect.main(["-l", "100", "-i", lvl0, "-o", str(tmp_path / "c.fq"), "--chunk_size", "1", "-m", "3", "--read_report", one])
    two = str(tmp_path / "two_se.tsv")
    r, _ = _torchrun(2, ["-l", "100", "-i", lvl0, "-o", str(tmp_path / "d.fq"), "--chunk_size", "1", "-m", "3", "--read_report", two],
                     {"RD_GZ_SHARD_MIN": "65536"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "one rank decodes" in r.stdout + r.stderr
    assert open(two, "rb").read() == H.read_report(one) and len(H.parse(H.read_report(one))[1]) == n
