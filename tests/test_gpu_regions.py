"""--regions on the GPU: rd_region_format byte for byte against ribodetector_amd/regions.py over synthetic window logits (the kernels
read no sequence text, so lengths and logits are invented), its verdicts, and the CLI's file against the same formatter over the window
logits of SeqModel's own window path on the same reads."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_interleaved as I  # noqa: E402
import test_interleaved_host as IH  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = I.SMALL
TERMS = [b" ", b"\t", b"\r", b"\n", b"\x0b", b"\x0c"]
ID_LENS = [0, 1, 15, 16, 17, 300]
CANARY = 0xAB


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- synthetic chunks ------------------------------------------------------------------------------------------------------------------
def _record(rid, term):
    """a FASTQ record whose header is the id, one of the six terminators and (unless that ended the line) a comment"""
    return b"@" + rid + term + (b"" if term == b"\n" else b"1:N:0 x\n") + b"ACGT\n+\nIIII\n"


def _ids(n, rng):
    """ids of 0, 1, 15, 16, 17 and 300 bytes (the header scan takes 16 bytes a step) among random lengths"""
    ln = np.where(rng.random(n) < 0.4, rng.choice(ID_LENS, n), rng.integers(0, 40, n))
    return [bytes(rng.integers(48, 123, int(k)).astype(np.uint8)) for k in ln]


def tie_distance(d):
    """how far x = p * 1e4 is from the nearest k + 0.5, where rint changes (float64)"""
    d = np.asarray(d, dtype=np.float64)
    x = 1e4 / (1.0 + np.exp(-d))
    return np.abs(x - np.floor(x) - 0.5)


def _logits(total, rng, run=0.7):
    """fp32 window logits in runs (a window keeps its neighbour's side with probability `run`), exact ties l1 == l0 among them; every
    rRNA window's p * 1e4 at least 0.01 away from a rounding tie (redrawn until it is), so that the float64 q is the fp32 q"""
    side = np.empty(total, dtype=bool)
    flip = rng.random(total) >= run
    cur = True
    for j in range(total):
        if flip[j]:
            cur = rng.random() < 0.5
        side[j] = cur
    mag = np.abs(rng.standard_normal(total) * 3) + 1e-3
    l0 = (rng.standard_normal(total) * 2).astype(np.float32)
    l1 = (l0 + np.where(side, mag, -mag)).astype(np.float32)
    for _ in range(50):
        bad = np.flatnonzero((l1 > l0) & (tie_distance(l1 - l0) < 0.01))
        if not len(bad):
            break
        l1[bad] = (l0[bad] + np.abs(rng.standard_normal(len(bad)) * 3) + 1e-3).astype(np.float32)
    ties = rng.random(total) < 0.03
    l1[ties] = l0[ties]
    return np.stack([l0, l1], axis=1)


def _mate(n, rng, L, ids=None, wmax=40):
    """one mate's side of a chunk: ids, invented lengths and window counts (most reads one window, of 0..L bases), window logits"""
    ids = _ids(n, rng) if ids is None else ids
    w = np.where(rng.random(n) < 0.3, rng.integers(2, wmax + 1, n), 1).astype(np.int64)
    lens = np.where(w == 1, rng.integers(0, L + 1, n), rng.integers(L + 1, 50 * L, n)).astype(np.int64)
    lens[(w == 1) & (rng.random(n) < 0.05)] = 7 * L          # (one window on a long read: --max_windows 1)
    first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(w)])
    return {"ids": ids, "lens": lens, "first": first, "wl": _logits(int(first[-1]), rng)}


def _tables(mates, layout, rng):
    """the mates' records as text and record tables: "se" / "two" = one text per mate (rec_stride 1), "il" = one interleaved text
    (rec_stride 2). Returns [(text bytes, rec_start int64, entry of the first record)] per mate."""
    terms = [TERMS[int(k)] for k in rng.integers(0, 6, len(mates[0]["ids"]))]
    recs = [[_record(rid, t) for rid, t in zip(m["ids"], terms)] for m in mates]
    if layout == "il":
        both = IH.interleave(*recs)
        rs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum([len(r) for r in both], dtype=np.int64)])
        text = b"".join(both)
        return [(text, rs, 0), (text, rs, 1)]
    return [(b"".join(r), np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum([len(x) for x in r], dtype=np.int64)]), 0) for r in recs]


def expected(mates, L):
    """the chunk's lines: units in input order, mate 1's lines before mate 2's"""
    from ribodetector_amd import regions
    per = [regions.format_lines(m["ids"], m["lens"], m["first"], m["wl"], L, e + 1) for e, m in enumerate(mates)]
    return b"".join(b"".join(x) for x in zip(*per))


def want_info(mates, L, text):
    from ribodetector_amd import regions
    per = [regions.format_lines(m["ids"], m["lens"], m["first"], m["wl"], L, e + 1) for e, m in enumerate(mates)]
    cnt = [[sum(x.count(b"\n") for x in p) for p in per], [sum(1 for x in p if x) for p in per]]
    pad = [0] * (2 - len(mates))
    return [len(mates) * len(mates[0]["ids"]), len(text), 0, 0] + cnt[0] + pad + cnt[1] + pad


def region_format(mates, tabs, L, out_cap=None, slack=64):
    """rd_region_format through the C ABI -> (the bytes written, info as a list, every byte of out behind them still the canary)"""
    import torch
    from ribodetector_amd import _native as N
    lib = N.lib()
    n = len(mates[0]["ids"])
    stride = 2 if len(tabs) == 2 and tabs[1][2] == 1 else 1
    keep, args = [], []
    texts = {}
    for m, (text, rs, shift) in zip(mates, tabs):
        if id(text) not in texts:
            texts[id(text)] = _dev(np.frombuffer(text + b"\0", np.uint8))
        t = texts[id(text)]
        wl = _dev(m["wl"]) if len(m["wl"]) else torch.empty((1, 2), dtype=torch.float32, device="cuda:0")
        d = [t, _dev(rs)[shift:], _dev(np.asarray(m["lens"], dtype=np.int32)), _dev(np.asarray(m["first"], dtype=np.int64)), wl]
        keep.append(d)
        args += [N.ptr(d[0]), len(text), N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), N.ptr(d[4])]
    if len(mates) == 1:
        args += [None, 0, None, None, None, None]
    total = sum(int(np.max(m["first"])) for m in mates)
    cap = len(expected(mates, L)) if out_cap is None else out_cap
    out = torch.full((((cap + 15) // 16) * 16 + slack,), CANARY, dtype=torch.uint8, device="cuda:0")
    info = torch.full((8,), -7, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(max(int(lib.rd_region_workspace_bytes(n, total)), 256), dtype=torch.uint8, device="cuda:0")
    N.check(lib.rd_region_format(*args, stride, n, L, N.ptr(out), cap, N.ptr(info), N.ptr(ws), ws.numel(), N.stream_ptr(torch.device("cuda:0"))),
            "rd_region_format")
    torch.cuda.synchronize()
    info = [int(x) for x in info.cpu()]
    got = out.cpu().numpy()
    nb = info[1] if not info[3] else 0
    return got[:nb].tobytes(), info, bool((got[nb:] == CANARY).all())


def _check(mates, tabs, L):
    for m in mates:                                  # the condition on the inputs: the float64 q is exact for every rRNA window
        d = (m["wl"][:, 1] - m["wl"][:, 0]).astype(np.float64)
        assert (tie_distance(d[d > 0]) >= 0.01).all()
    want = expected(mates, L)
    got, info, clean = region_format(mates, tabs, L)
    assert info == want_info(mates, L, want)
    assert got == want and clean
    return want


@pytest.mark.parametrize("layout", ["se", "two", "il"])
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049])
def test_format_against_the_reference(n, layout):
    rng = np.random.default_rng(7000 + 3 * n + len(layout))
    L = 100
    a = _mate(n, rng, L)
    mates = [a] if layout == "se" else [a, _mate(n, rng, L, ids=[x + b"/2" for x in a["ids"]])]
    if n == 0:
        import torch
        from ribodetector_amd import _native as N
        info = torch.full((8,), -7, dtype=torch.int64, device="cuda:0")
        N.check(N.lib().rd_region_format(None, 0, None, None, None, None, None, 0, None, None, None, None, 1, 0, L, None, 0, N.ptr(info), None, 0,
                                         N.stream_ptr(torch.device("cuda:0"))), "rd_region_format")
        assert info.cpu().tolist() == [0] * 8
        return
    want = _check(mates, _tables(mates, layout, rng), L)
    if n >= 2047:
        assert want.count(b"\n") > n // 2 and len({len(x) for x in a["ids"]} & set(ID_LENS)) == 6


def test_every_id_length_and_terminator():
    """ids of 0..40 and 300 bytes, each ended by each of the six id terminators; one window per read, all rRNA: 252 lines, and the
    same with 3, 4 and 5 reads more - one tile of the write pass a line short, full, and a line more"""
    for more in (0, 3, 4, 5):
        rng = np.random.default_rng(11)
        lens_of_id = list(range(0, 41)) + [300]
        ids, terms = [], []
        for k in lens_of_id:
            for t in TERMS:
                ids.append(bytes(rng.integers(48, 123, k).astype(np.uint8)))
                terms.append(t)
        for k in range(more):
            ids.append(b"more%d" % k)
            terms.append(TERMS[k])
        n = len(ids)
        m = {"ids": ids, "lens": rng.integers(1, 101, n).astype(np.int64), "first": np.arange(n + 1, dtype=np.int64),
             "wl": np.stack([np.zeros(n), np.full(n, 3.0)], axis=1).astype(np.float32)}
        recs = [_record(rid, t) for rid, t in zip(ids, terms)]
        rs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum([len(r) for r in recs], dtype=np.int64)])
        want = _check([m], [(b"".join(recs), rs, 0)], 100)
        assert want.count(b"\n") == n == 252 + more and want.startswith(b"\t0\t"), n


def test_one_unit_of_4096_alternating_windows_and_starts_of_every_width():
    """2,048 lines of one unit (many workgroups of the write pass) on a read of 2^31 - 1 bases, between units without a region; further
    units whose starts have 1 to 10 digits"""
    L = 100
    shapes = [(50, 1), (2 ** 31 - 1, 4096), (80, 1), (150, 6), (5000, 50), (123456, 300), (2 ** 31 - 1, 7), (2 ** 31 - 1, 2000), (0, 1)]
    w = np.array([s[1] for s in shapes], dtype=np.int64)
    first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(w)])
    wl = np.zeros((int(first[-1]), 2), dtype=np.float32)
    for i, (_, k) in enumerate(shapes):
        if k > 1:
            wl[first[i]:first[i + 1]:2, 1] = np.float32(2.0) + np.arange(len(range(0, k, 2)), dtype=np.float32) / 4096       # windows 0, 2, 4, ...: rRNA
        wl[first[i] + 1:first[i + 1]:2, 0] = 1.0
    keep = (wl[:, 1] > wl[:, 0]) & (tie_distance((wl[:, 1] - wl[:, 0]).astype(np.float64)) < 0.01)
    wl[keep, 1] += np.float32(0.003)
    ids = [b"u%d" % i for i in range(len(shapes))]
    m = {"ids": ids, "lens": np.array([s[0] for s in shapes], dtype=np.int64), "first": first, "wl": wl}
    recs = [_record(rid, b" ") for rid in ids]
    rs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum([len(r) for r in recs], dtype=np.int64)])
    want = _check([m], [(b"".join(recs), rs, 0)], L)
    rows = [ln.split(b"\t") for ln in want.split(b"\n")[:-1]]
    assert sum(1 for r in rows if r[0] == b"u1") == 2048 and {len(r[1]) for r in rows} == set(range(1, 11))
    assert max(int(r[2]) for r in rows) == 2 ** 31 - 1


def test_a_chunk_without_a_region_is_no_bytes():
    rng = np.random.default_rng(5)
    m = _mate(3000, rng, 100)
    m["wl"][:, 1] = m["wl"][:, 0] - np.float32(1.0)
    m["wl"][::7, 1] = m["wl"][::7, 0]                # ties are not rRNA either
    tabs = _tables([m], "se", rng)
    got, info, clean = region_format([m], tabs, 100, out_cap=0)
    assert got == b"" and info == [3000, 0, 0, 0, 0, 0, 0, 0] and clean


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------------
def _fault_case(seed=21, n=2500):
    rng = np.random.default_rng(seed)
    a = _mate(n, rng, 100)
    mates = [a, _mate(n, rng, 100, ids=a["ids"])]
    return mates, _tables(mates, "two", rng)


def test_one_byte_short_is_fault_1_and_nothing_is_written():
    mates, tabs = _fault_case()
    want = expected(mates, 100)
    assert len(want) > 10000
    got, info, clean = region_format(mates, tabs, 100, out_cap=len(want) - 1)
    wi = want_info(mates, 100, want)
    assert info == [0, len(want), 0, 1] + wi[4:] and got == b"" and clean
    got, info, clean = region_format(mates, tabs, 100, out_cap=len(want))
    assert info == wi and got == want and clean


@pytest.mark.parametrize("what", ["header", "header_runs_on", "outside", "seq_len", "win_first"])
def test_tables_that_do_not_describe_the_chunk_are_fault_2(what):
    mates, tabs = _fault_case(22)
    k = 1234
    mates = [dict(m) for m in mates]
    if what == "header":                            # a record that does not start with '@' / '>'
        text, rs, sh = tabs[1]
        tabs[1] = (text[:int(rs[k])] + b"X" + text[int(rs[k]) + 1:], rs, sh)
    elif what == "header_runs_on":                  # no terminator inside the record: the table cuts it inside its id
        text, rs, sh = tabs[0]
        rs = rs.copy()
        big = max(range(len(mates[0]["ids"]) - 1), key=lambda i: len(mates[0]["ids"][i]))
        rs[big + 1] = rs[big] + 5
        tabs[0] = (text, rs, sh)
    elif what == "outside":
        text, rs, sh = tabs[0]
        rs = rs.copy()
        rs[-1] = len(text) + 9
        tabs[0] = (text, rs, sh)
    elif what == "seq_len":
        mates[1]["lens"] = mates[1]["lens"].copy()
        mates[1]["lens"][k] = -1
    else:                                           # a win_first that decreases (its last entry is still the total)
        f = mates[0]["first"].copy()
        f[k] = f[k - 1] - 1
        mates[0]["first"] = f
    got, info, clean = region_format(mates, tabs, 100, out_cap=len(expected(_fault_case(22)[0], 100)) + 4096)
    assert info == [0, 0, 0, 2, 0, 0, 0, 0] and got == b"" and clean


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
def _blocks(golden):
    """the golden 100 bp reads by the reference's label: (rRNA reads, other reads) as bytes"""
    g = golden.npz("se100")
    arena, off, lab = g["arena"].tobytes(), g["offsets"], g["labels"]
    reads = [arena[off[i]:off[i + 1]] for i in range(len(lab))]
    margin = np.abs(g["logits"][:, 1] - g["logits"][:, 0])
    sure = margin > 4.0                              # (reads the reference is sure of: their label survives a neighbour's bases)
    return [r for r, x, s in zip(reads, lab, sure) if x == 1 and s], [r for r, x, s in zip(reads, lab, sure) if x == 0 and s]


def _long_read(rng, rr, nn, pattern, trim=0):
    seq = b"".join((rr if c == "R" else nn)[int(rng.integers(0, len(rr if c == "R" else nn)))] for c in pattern)
    return seq[:len(seq) - trim] if trim else seq


PATTERNS = ["NNNRRRRNNN", "RRRNNNN", "NNNNRRR", "RRRRR", "NNNNNN", "RNRNRNRN", "NNRRNNRRNN", "NR", "RNNNNNNNNNNNNNNNNNNR", "NNNNNNNNRRRRRRRRRRRRRRRRNNNNNNNNNNNNNNNN"]


def _se_reads(golden, seed, n_long=300, n_short=1200):
    rng = np.random.default_rng(seed)
    rr, nn = _blocks(golden)
    assert len(rr) > 100 and len(nn) > 100
    seqs = [_long_read(rng, rr, nn, PATTERNS[i % len(PATTERNS)], trim=int(rng.integers(0, 60)) if i % 3 else 0) for i in range(n_long)]
    seqs += [(rr if rng.random() < 0.3 else nn)[int(rng.integers(0, 100))][:int(rng.integers(40, 101))] for _ in range(n_short)]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def _arrays(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    offs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens, dtype=np.int64)])
    return np.frombuffer(b"".join(seqs), np.uint8), offs, lens


def window_logits(model, seqs, S, K):
    """(win_first, win_logits) of the reads over SeqModel's own window path: plan, table, classify, float64 pass"""
    import torch
    arena, offs, lens = _arrays(seqs)
    d_arena, d_off, d_len = _dev(arena), _dev(offs[:-1]), _dev(lens)
    plan = model.window_plan(d_len, 100, S, K)
    model.window_table(plan, d_off, d_len)
    model.classify_window_table(d_arena, plan)
    model.sync_results()
    torch.cuda.synchronize()
    return plan["win_first"].cpu().numpy(), plan["win_logits"].cpu().numpy()


def cli_expected(model, mates_seqs, mates_ids, S, K):
    """the file the CLI must write, and the condition on the inputs: every rRNA window's q is safe from the rounding tie and no window
    sits inside the float64 pass's band"""
    from ribodetector_amd import regions
    per = []
    for e, (seqs, ids) in enumerate(zip(mates_seqs, mates_ids)):
        first, wl = window_logits(model, seqs, S, K)
        d = (wl[:, 1] - wl[:, 0]).astype(np.float64)
        assert np.abs(d).min() > 2e-4 and (tie_distance(d[d > 0]) >= 0.01).all()
        per.append(regions.format_lines(ids, [len(s) for s in seqs], first, wl, 100, e + 1))
    return regions.HEADER + b"".join(b"".join(x) for x in zip(*per)), per


def settle(model, seqs, rules, filler):
    """the condition on the inputs, made to hold: a read with a window inside the float64 pass's band, or with an rRNA window whose q is
    near a rounding tie, under any of the (S, K) rules is replaced by `filler` (drawn again, as tests/test_summary_host.py does) until
    no read is; cli_expected then asserts the condition on what is left"""
    seqs = list(seqs)
    for _ in range(4):
        bad = set()
        for S, K in rules:
            first, wl = window_logits(model, seqs, S, K)
            d = (wl[:, 1] - wl[:, 0]).astype(np.float64)
            w = np.flatnonzero((np.abs(d) <= 2e-4) | ((d > 0) & (tie_distance(d) < 0.01)))
            bad |= set((np.searchsorted(first, w, side="right") - 1).tolist())
        if not bad:
            break
        for i in bad:
            seqs[i] = filler
    return seqs


def _fastq(seqs, ids):
    return [b"@%s 1:N:0\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in zip(ids, seqs)]


def _win_args(S, K):
    return ["--windows", "--window_stride", str(S), "--max_windows", str(K)]


@pytest.fixture(scope="module")
def se_case(tmp_path_factory, golden, gpu_model):
    d = tmp_path_factory.mktemp("regse")
    seqs = settle(gpu_model, _se_reads(golden, 31), ((100, 32), (30, 4096)), _blocks(golden)[1][0][:80])
    ids = [b"read.%d" % i for i in range(len(seqs))]
    path = str(d / "se.fq")
    open(path, "wb").write(b"".join(_fastq(seqs, ids)))
    want = {sk: cli_expected(gpu_model, [seqs], [ids], *sk) for sk in ((100, 32), (30, 4096))}
    return {"path": path, "seqs": seqs, "ids": ids, "want": want}


def _cli(tmp, tag, inputs, win, extra=(), env=None, regions="reg.bed", ensure="none", chunks=SMALL, outs=None):
    n_out = len(inputs) if outs is None else outs
    o = [str(tmp / ("%s_o%d.fq" % (tag, k))) for k in range(n_out)]
    r = [str(tmp / ("%s_r%d.fq" % (tag, k))) for k in range(n_out)]
    rep, summ, reg = str(tmp / (tag + "_rep.tsv")), str(tmp / (tag + "_s.json")), (str(tmp / (tag + "_" + regions)) if regions else None)
    args = ["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "-e", ensure, "--read_report", rep, "--summary", summ] + list(win) + list(extra) + list(chunks)
    p = I._run(args + (["--regions", reg] if reg else []), env)
    files = {"o": [I._read(x) for x in o], "r": [I._read(x) for x in r], "rep": I._read(rep)}
    return p, files, json.load(open(summ)), (I._read(reg) if reg else None)


@pytest.mark.parametrize("S,K", [(100, 32), (30, 4096)])
def test_cli_single_end_file_is_the_formatters(tmp_path, se_case, S, K):
    want, per = se_case["want"][(S, K)]
    p, f, s, reg = _cli(tmp_path, "dev", [se_case["path"]], _win_args(S, K))
    assert p.ingest["se.fq"]["path"] == "device" and p.num_read == 1500 and p.regions_repeats == 0
    assert reg == want
    rows = [ln.split(b"\t") for ln in reg.split(b"\n")[1:-1]]
    assert len(rows) > 300 and {r[3] for r in rows} == {b"1"}
    lens = dict(zip(se_case["ids"], (len(x) for x in se_case["seqs"])))
    inner = [r for r in rows if int(r[1]) > 0 and int(r[2]) < lens[r[0]]]         # (h) an rRNA stretch inside a read, not touching its ends
    assert len(inner) > 50
    assert s["windows"]["regions"] == [len(rows)] and s["windows"]["reads_with_regions"] == [len({r[0] for r in rows})] == [sum(1 for x in per[0] if x)]
    # (a) one chunk instead of two, (b) the host's parser: the same file
    p2, f2, s2, reg2 = _cli(tmp_path, "big", [se_case["path"]], _win_args(S, K), chunks=[])
    p3, f3, s3, reg3 = _cli(tmp_path, "host", [se_case["path"]], _win_args(S, K), env={"RD_INGEST": "host"})
    assert reg2 == want and reg3 == want and f2 == f and f3 == f and p3.ingest.get("se.fq", {}).get("path") != "device"


def test_cli_gz_path_repeat_path_and_fuse_modes(tmp_path, se_case):
    want, _ = se_case["want"][(100, 32)]
    win = _win_args(100, 32)
    _, _, _, reg = _cli(tmp_path, "gz", [se_case["path"]], win, regions="reg.bed.gz")                 # (d)
    assert reg == want and open(str(tmp_path / "gz_reg.bed.gz"), "rb").read(2) == b"\x1f\x8b"
    p, _, _, reg = _cli(tmp_path, "hint", [se_case["path"]], win, env={"RD_REGIONS_HINT": "64"})      # (f)
    assert reg == want and p.regions_repeats >= 2
    _, _, _, reg = _cli(tmp_path, "max", [se_case["path"]], win + ["--window_fuse", "max"])           # (c)
    assert reg == want


def test_cli_without_the_flag_everything_else_is_the_same(tmp_path, se_case):
    win = _win_args(30, 4096)
    p0, f0, s0, _ = _cli(tmp_path, "off", [se_case["path"]], win, regions=None)
    p1, f1, s1, _ = _cli(tmp_path, "on", [se_case["path"]], win)
    assert f0 == f1 and I._counters(p0) == I._counters(p1) and len(f0["rep"]) > 0
    assert "regions" not in s0["windows"] and "reads_with_regions" not in s0["windows"]
    s1["windows"] = {k: v for k, v in s1["windows"].items() if k not in ("regions", "reads_with_regions")}
    assert s1 == s0


@pytest.mark.parametrize("K", [32, 4096])
def test_cli_fasta_contig(tmp_path, golden, gpu_model, K):
    """a 40 kb contig with a 2 kb rRNA stretch among short records: under K = 32 the windows are 1,287 bases apart"""
    rr, nn = _blocks(golden)
    for seed in range(41, 61):                      # (drawn again until the condition on the inputs holds: cli_expected asserts it)
        rng = np.random.default_rng(seed)
        contig = _long_read(rng, rr, nn, "N" * 150 + "R" * 20 + "N" * 230)
        seqs = [nn[i][:70 + i % 30] for i in range(40)] + [contig] + [rr[i] for i in range(30)]
        settled = settle(gpu_model, seqs, ((100, K),), nn[0][:80])
        if settled[40] == contig:                   # (a short record may be replaced, the contig not)
            seqs = settled
            break
    ids = [b"rec.%d" % i for i in range(len(seqs))]
    fa = str(tmp_path / "c.fa")
    with open(fa, "wb") as fh:
        for i, s in zip(ids, seqs):
            fh.write(b">" + i + b" contig\n" + b"".join(s[k:k + 70] + b"\n" for k in range(0, len(s), 70)))
    want, per = cli_expected(gpu_model, [seqs], [ids], 100, K)
    p, f, s, reg = _cli(tmp_path, "fa", [fa], _win_args(100, K))
    assert reg == want and p.num_read == 71
    rows = [ln.split(b"\t") for ln in per[0][40].split(b"\n")[:-1]]
    # the operon is reported, inside the contig (a window across the junction of two unrelated reads elsewhere may be anything)
    operon = [r for r in rows if 14000 <= int(r[1]) and int(r[2]) <= 18000]
    assert all(r[0] == b"rec.40" for r in rows) and sum(int(r[4]) for r in operon) >= (2 if K == 32 else 15)
    assert max(int(r[4]) for r in rows) == max(int(r[4]) for r in operon)


def _pe_reads(golden, seed, n=1500):
    """pairs of 250 bp mates: two golden reads and a half, of either kind"""
    rng = np.random.default_rng(seed)
    rr, nn = _blocks(golden)
    pats = ["NNN", "RRR", "NRR", "RNN", "NRN", "RRN"]
    return [[_long_read(rng, rr, nn, pats[int(rng.integers(0, 6))], trim=50) for _ in range(n)] for _ in (0, 1)]


@pytest.fixture(scope="module")
def pe_case(tmp_path_factory, golden, gpu_model):
    d = tmp_path_factory.mktemp("regpe")
    m1, m2 = (settle(gpu_model, m, ((30, 32),), _blocks(golden)[1][0] * 2 + _blocks(golden)[1][1][:50]) for m in _pe_reads(golden, 51))
    ids = [[b"pair.%d/%d" % (i, e) for i in range(len(m1))] for e in (1, 2)]
    r1, r2 = _fastq(m1, ids[0]), _fastq(m2, ids[1])
    paths = [str(d / "p_1.fq"), str(d / "p_2.fq"), str(d / "p_il.fq")]
    for p, recs in zip(paths, (r1, r2, IH.interleave(r1, r2))):
        open(p, "wb").write(b"".join(recs))
    open(paths[2] + ".gz", "wb").write(gzip.compress(open(paths[2], "rb").read(), 6))
    want, per = cli_expected(gpu_model, [m1, m2], ids, 30, 32)
    return {"two": paths[:2], "il": paths[2], "want": want, "per": per}


@pytest.mark.parametrize("ensure", I.MODES)
def test_cli_pairs_of_250_bp_in_every_mode(tmp_path, pe_case, ensure):
    """(c) the regions do not depend on -e: two files under every mode; the interleaved file, host ingest and the other fusion one each"""
    win, want = _win_args(30, 32), pe_case["want"]
    p, f, s, reg = _cli(tmp_path, "two", pe_case["two"], win, ensure=ensure)
    assert reg == want and p.num_read == 1500
    rows = [ln.split(b"\t") for ln in reg.split(b"\n")[1:-1]]
    n = [sum(1 for r in rows if r[3] == m) for m in (b"1", b"2")]
    assert min(n) > 300 and s["windows"]["regions"] == n
    assert s["windows"]["reads_with_regions"] == [sum(1 for x in pe_case["per"][e] if x) for e in (0, 1)]
    assert all(r[0].endswith(b"/" + r[3]) for r in rows)                           # every line carries its own mate's id
    extra = {"none": (["--interleaved"], [pe_case["il"]], None), "rrna": (["--interleaved"], [pe_case["il"]], {"RD_INGEST": "host"}),
             "norrna": (["--window_fuse", "max"], pe_case["two"], {"RD_INGEST": "host"}), "both": (["--interleaved"], [pe_case["il"] + ".gz"], None)}[ensure]
    _, _, _, reg2 = _cli(tmp_path, "other", extra[1], win + extra[0], env=extra[2], ensure=ensure, outs=2)
    assert reg2 == want


@pytest.mark.parametrize("layout", ["gather", "ranges"])
def test_cli_two_ranks_write_the_same_file(tmp_path, pe_case, layout):
    """(e) the label gather (an interleaved .gz: every rank formats the regions of its shard of the pairs) and the byte-range layout
    (two plain files: every rank writes its part, the parts are joined)"""
    inputs, extra = ([pe_case["il"] + ".gz"], ["--interleaved"]) if layout == "gather" else (pe_case["two"], [])
    reg, summ = str(tmp_path / "reg.bed.gz"), str(tmp_path / "s.json")
    args = ["-l", "100", "-i", *inputs, "-o", str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq"), "-e", "rrna", "--summary", summ, "--regions", reg] + \
        _win_args(30, 32) + extra + SMALL
    r, port = I._torchrun(2, args)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-3000:]
    assert ("label-gather layout" in text) == (layout == "gather") and ("parses" in text) == (layout == "ranges")
    assert I._read(reg) == pe_case["want"]
    rows = [ln.split(b"\t") for ln in pe_case["want"].split(b"\n")[1:-1]]
    n = [sum(1 for x in rows if x[3] == m) for m in (b"1", b"2")]
    assert json.load(open(summ))["windows"]["regions"] == n and "%d + %d" % tuple(n) in text and "rRNA regions" in text
    assert not [x for x in os.listdir(tmp_path) if ".part" in x or ".joining" in x]
