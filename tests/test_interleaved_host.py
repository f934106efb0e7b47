"""--interleaved without a GPU: the parser flags, the argument rules, a pure-Python reference of the pair rules (read id, mate rule,
split of the tables, label expansion, interleaving two record lists) that tests/test_gpu_interleaved.py compares the device against,
and the numpy views the host writer gets (data_loader/fastx_parser.py)."""
import numpy as np
import pytest

_WS = b" \t\r\n\x0b\x0c"
LABEL_SKIP = 2


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def read_id(record):
    """the bytes of the header line after '@' up to the first of {space, \\t, \\r, \\n, \\v, \\f}"""
    assert record[:1] == b"@"
    end = 1
    while end < len(record) and record[end] not in _WS:
        end += 1
    return record[1:end]


def are_mates(id1, id2):
    """equal ids, or mate 1's ends in /1, mate 2's in /2 and they are equal in front of those two bytes"""
    if id1 == id2:
        return True
    return id1.endswith(b"/1") and id2.endswith(b"/2") and id1[:-2] == id2[:-2]


def first_mismatch(records):
    """index of the first pair (records 2k, 2k + 1) whose ids are not mates, or -1"""
    for k in range(len(records) // 2):
        if not are_mates(read_id(records[2 * k]), read_id(records[2 * k + 1])):
            return k
    return -1


def split_tables(rec_start, seq_off, seq_len):
    """(pair_start[n + 1], seq_off1, seq_len1, seq_off2, seq_len2) of a table of 2n (or 2n + 1) records"""
    n = (len(rec_start) - 1) // 2
    return ([rec_start[2 * k] for k in range(n + 1)], [seq_off[2 * k] for k in range(n)], [seq_len[2 * k] for k in range(n)],
            [seq_off[2 * k + 1] for k in range(n)], [seq_len[2 * k + 1] for k in range(n)])


def expand_labels(pair_labels, mate):
    out = []
    for lab in pair_labels:
        out += [int(lab), LABEL_SKIP] if mate == 0 else [LABEL_SKIP, int(lab)]
    return out


def interleave(recs1, recs2):
    assert len(recs1) == len(recs2)
    return [r for pair in zip(recs1, recs2) for r in pair]


def select(records, labels, want):
    return b"".join(r for r, lab in zip(records, labels) if lab == want)


def synth_pairs(n, seed, style="mixed"):
    """n pairs as two record lists with ids of several styles (all of them mates) and variable lengths"""
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for k in range(n):
        s = k % 6 if style == "mixed" else style
        name = b"read%d" % k + b":" * int(rng.integers(0, 40)) if s != 5 else b""
        if s == 0:
            i1, i2 = name + b"/1", name + b"/2"
        elif s == 1:
            i1, i2 = name + b" 1:N:0:ACGT", name + b" 2:N:0:ACGT"
        elif s == 2:
            i1, i2 = name + b"\tcomment", name
        elif s == 3:
            i1, i2 = name + b"/1", name + b"/1"
        elif s == 4:
            i1 = i2 = name + b"x" * int(rng.integers(0, 70))
        else:
            i1, i2 = b"", b" an empty id"
        for ids, out in ((i1, r1), (i2, r2)):
            L = int(rng.integers(1, 150))
            seq = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].tobytes()
            out.append(b"@" + ids + b"\n" + seq + b"\n+\n" + b"I" * L + b"\n")
    return r1, r2


def tables_of(records):
    """(text, rec_start, seq_off, seq_len) of 4-line FASTQ records"""
    rs, so, sl, pos = [0], [], [], 0
    for r in records:
        h = r.index(b"\n") + 1
        so.append(pos + h)
        sl.append(r.index(b"\n", h) - h)
        pos += len(r)
        rs.append(pos)
    return b"".join(records), np.array(rs, np.int64), np.array(so, np.int64), np.array(sl, np.int32)


# ---- the reference pinned on hand-built cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h1,h2,mates", [
    (b"@r1", b"@r1", True),                              # equal ids
    (b"@r1/1", b"@r1/2", True),                          # /1 with /2
    (b"@r1/2", b"@r1/1", False),                         # /2 with /1 is not a match
    (b"@r1/1", b"@r1/1", True),                          # /1 with /1: the equal rule
    (b"@r1 1:N:0", b"@r1 2:N:0", True),                  # a comment after a space
    (b"@", b"@ comment", True),                          # an empty id
    (b"@r1\r", b"@r1\r", True),                          # CRLF
    (b"@r1", b"@r11", False),                            # ids that differ only in length
    (b"@r1/1", b"@r2/2", False),
    (b"@/1", b"@/2", True),
    (b"@1", b"@2", False),                               # no slash in front
    (b"@r1\tx", b"@r1\x0by", True),
])
def test_reference_mate_rule(h1, h2, mates):
    rec = lambda h: h + b"\nACGT\n+\nIIII\n"      # noqa: E731
    assert are_mates(read_id(rec(h1)), read_id(rec(h2))) is mates
    assert first_mismatch([rec(h1), rec(h2)]) == (-1 if mates else 0)


def test_reference_ids_and_first_mismatch_in_the_last_pair():
    assert read_id(b"@abc def\nA\n+\nI\n") == b"abc" and read_id(b"@\nA\n+\nI\n") == b"" and read_id(b"@a\r\nA\r\n+\r\nI\r\n") == b"a"
    r1, r2 = synth_pairs(12, 1)
    recs = interleave(r1, r2)
    assert first_mismatch(recs) == -1
    recs[-1] = b"@other\nA\n+\nI\n"
    assert first_mismatch(recs) == 11
    del recs[5]                                       # one dropped record shifts every later pair
    assert first_mismatch(recs) == 2


def test_reference_tables_labels_interleave():
    assert split_tables([0, 10, 25, 31, 40], [2, 12, 27, 33], [3, 4, 1, 2]) == ([0, 25, 40], [2, 27], [3, 1], [12, 33], [4, 2])
    assert split_tables([0, 10, 25, 31], [2, 12, 27], [3, 4, 1]) == ([0, 25], [2], [3], [12], [4])      # an odd last record: no pair
    assert expand_labels([1, 0, -1], 0) == [1, 2, 0, 2, -1, 2] and expand_labels([1, 0, -1], 1) == [2, 1, 2, 0, 2, -1]
    assert interleave([b"a", b"b"], [b"c", b"d"]) == [b"a", b"c", b"b", b"d"]


# ---- the CLI's flags and argument rules ---------------------------------------------------------------------------------------------
def test_parser_accepts_the_flags():
    from ribodetector_amd import detect
    a = detect.build_parser().parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq"])
    assert a.interleaved is False and a.no_mate_check is False
    a = detect.build_parser().parse_args(["-l", "100", "-i", "x.fq", "-o", "y.fq", "--interleaved", "--no_mate_check"])
    assert a.interleaved is True and a.no_mate_check is True


def test_argument_rules():
    from ribodetector_amd.detect import check_file_counts
    assert check_file_counts(["i.fq"], ["o.fq"], None, True) is True
    assert check_file_counts(["i.fq.gz"], ["o1.fq", "o2.fq"], None, True) is True
    assert check_file_counts(["i.fq"], ["o.fq"], ["r.fq"], True) is True
    assert check_file_counts(["i.fq"], ["o1.fq", "o2.fq.gz"], ["r1.fq", "r2.fq"], True) is True
    for bad in ((["a.fq", "b.fq"], ["o.fq"], None), (["a.fq", "b.fq"], ["o1.fq", "o2.fq"], None), ([], ["o.fq"], None),
                (["i.fq"], ["o1.fq", "o2.fq", "o3.fq"], None), (["i.fq"], [], None),
                (["i.fq"], ["o.fq"], ["r1.fq", "r2.fq"]), (["i.fq"], ["o1.fq", "o2.fq"], ["r.fq"])):
        with pytest.raises(RuntimeError, match="--interleaved"):
            check_file_counts(*bad, True)
    for fa in ("i.fa", "i.fasta.gz", "i.fna"):
        with pytest.raises(RuntimeError, match="interleaved FASTA is not supported"):
            check_file_counts([fa], ["o.fa"], None, True)


def test_argument_rules_without_the_flag_are_todays():
    from ribodetector_amd.detect import check_file_counts
    counts = "Input or output should have no more than two files and they should have the same number of files."
    rrna = "Ouput rRNA should have no more than two files and they should the same number with input files."
    names = lambda k, p: [p + "%d.fq" % i for i in range(k)]      # noqa: E731
    for n_in in range(0, 4):
        for n_out in range(0, 4):
            for n_r in (None, 0, 1, 2, 3):
                args = (names(n_in, "i"), names(n_out, "o"), None if n_r is None else names(n_r, "r"))
                if n_in != n_out or not 1 <= n_in <= 2:
                    want = counts
                elif n_r is not None and n_r != n_in:
                    want = rrna
                else:
                    assert check_file_counts(*args) is (n_in == 2) and check_file_counts(*args, interleaved=False) is (n_in == 2)
                    continue
                with pytest.raises(RuntimeError) as e:
                    check_file_counts(*args)
                assert str(e.value) == want
    assert check_file_counts(["i.fa"], ["o.fa"], None) is False            # FASTA stays fine without the flag


def test_output_file_lists_know_one_file_per_label():
    from ribodetector_amd.detect import Predictor, check_read_report
    g = Predictor.gz_output_files
    # as before
    assert g(["a.fq.gz", "b.fq"], ["c.fq", "d.fq.gz"], True, "none") == [(1, 1), (0, 0)]
    assert g(["a.fq.gz"], None, False, "none") == [(0, 0)]
    assert g(["a.fq", "b.fq"], None, True, "both") == [(0, -1), (1, -1)]
    # a paired run with ONE file per label (interleaved output)
    assert g(["a.fq.gz"], ["r.fq"], True, "none") == [(0, 0)]
    assert g(["a.fq"], ["r.fq.gz"], True, "both") == [(0, 1), (0, -1)]
    check_read_report("rep.tsv", ["a.fq"], ["r.fq"], True, "both")
    with pytest.raises(RuntimeError, match="unclassified"):
        check_read_report("a.fq.unclassified.gz", ["a.fq"], ["r.fq"], True, "both")
    with pytest.raises(RuntimeError, match="also an output"):
        check_read_report("r.fq", ["a.fq"], ["r.fq"], True, "none")


# ---- the numpy views against the reference ------------------------------------------------------------------------------------------
def _interleaved_file(tmp_path, n, seed, extra=b""):
    r1, r2 = synth_pairs(n, seed)
    path = str(tmp_path / "il.fq")
    with open(path, "wb") as fh:
        fh.write(b"".join(interleave(r1, r2)) + extra)
    return path, r1, r2


def test_views_of_a_host_chunk(tmp_path):
    from ribodetector_amd.data_loader import fastx_parser as fx
    path, r1, r2 = _interleaved_file(tmp_path, 700, 3)
    chunks = list(fx.get_seq_chunks(path, chunk_size=512))
    assert [len(c.seq_len) for c in chunks] == [512, 512, 376]
    k0 = 0
    for c in chunks:
        n = fx.interleaved_pairs(c)
        recs = interleave(r1[k0:k0 + n], r2[k0:k0 + n])
        text, rs, so, sl = tables_of(recs)
        assert c.buf[c.rec_start[0]:c.rec_start[-1]].tobytes() == text
        ps, o1, l1, o2, l2 = split_tables(list(c.rec_start), list(c.seq_off), list(c.seq_len))
        pv = fx.pair_view(c)
        assert list(pv.rec_start) == ps and list(pv.seq_off) == o1 and list(pv.seq_len) == l1 and pv.buf is c.buf and pv.verbatim
        labels = np.random.default_rng(k0).integers(-1, 2, n).astype(np.int8)
        for mate in (0, 1):
            e = fx.expand_pair_labels(labels, mate)
            assert e.dtype == np.int8 and list(e) == expand_labels(labels, mate)
        assert [fx.record_id(c.buf, int(c.rec_start[i]), int(c.rec_start[i + 1])) for i in range(2 * n)] == [read_id(r) for r in recs]
        k0 += n
    from ribodetector_amd import _native as N
    assert N.LABEL_SKIP == LABEL_SKIP


def test_writer_gets_the_interleave_and_the_two_files(tmp_path):
    """NativeWriter.write_selected with the pair view writes exactly the interleave of what it writes for the two mates' files, and the
    split view (the full record table with expanded labels) writes the two-file outputs byte for byte"""
    from ribodetector_amd.data_loader import fastx_parser as fx
    n = 900
    path, r1, r2 = _interleaved_file(tmp_path, n, 5)
    mates = [str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq")]
    for p, recs in zip(mates, (r1, r2)):
        open(p, "wb").write(b"".join(recs))
    labels = np.random.default_rng(9).integers(-1, 2, n).astype(np.int8)
    for want in (0, 1, -1):
        two = []
        for e, p in enumerate(mates):                  # what a two-file run writes
            out = str(tmp_path / ("two%d_%d.fq" % (e, want)))
            fh, k0 = fx.open_for_write(out), 0
            for c in fx.get_seq_chunks(p, chunk_size=256):
                fh.write_selected(c, labels[k0:k0 + len(c.seq_len)], want)
                k0 += len(c.seq_len)
            fh.close()
            two.append(open(out, "rb").read())
            assert two[-1] == select((r1, r2)[e], labels, want)
        il, sp = str(tmp_path / ("il_%d.fq" % want)), [str(tmp_path / ("sp%d_%d.fq" % (e, want))) for e in (0, 1)]
        fi, fs, k0 = fx.open_for_write(il), [fx.open_for_write(p) for p in sp], 0
        for c in fx.get_seq_chunks(path, chunk_size=512):
            m = fx.interleaved_pairs(c)
            fi.write_selected(fx.pair_view(c), labels[k0:k0 + m], want)
            for e in (0, 1):
                fs[e].write_selected(c, fx.expand_pair_labels(labels[k0:k0 + m], e), want)
            k0 += m
        for fh in [fi] + fs:
            fh.close()
        assert k0 == n
        assert open(il, "rb").read() == b"".join(interleave([r for r, lab in zip(r1, labels) if lab == want], [r for r, lab in zip(r2, labels) if lab == want]))
        assert [open(p, "rb").read() for p in sp] == two


def test_odd_record_count(tmp_path):
    from ribodetector_amd.data_loader import fastx_parser as fx
    path, r1, r2 = _interleaved_file(tmp_path, 20, 7, extra=b"@lonely/1\nACGT\n+\nIIII\n")
    chunks = list(fx.get_seq_chunks(path, chunk_size=64))
    assert len(chunks) == 1 and len(chunks[0].seq_len) == 41 and fx.interleaved_pairs(chunks[0]) == 20
    pv = fx.pair_view(chunks[0])
    assert len(pv.rec_start) == 21 and int(pv.rec_start[-1]) == int(chunks[0].rec_start[40])       # the lone record belongs to no pair
    out = str(tmp_path / "o.fq")
    fh = fx.open_for_write(out)
    fh.write_selected(pv, np.zeros(20, np.int8), 0)
    fh.close()
    assert open(out, "rb").read() == b"".join(interleave(r1, r2))
    fx.check_even_records(40)
    with pytest.raises(ValueError) as e:
        fx.check_even_records(41)
    assert str(e.value) == "interleaved input holds an odd number of records (41): the last record has no mate"
