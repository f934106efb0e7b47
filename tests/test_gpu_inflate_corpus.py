"""The device's gunzip decoders on the corpus of tests/deflate_corpus.py - streams from libdeflate and pigz-style compressors, and
hand-built DEFLATE that zlib never writes - with zlib's inflate as the judge of every verdict:
  members  rd_gz_inflate_members (gz.DeviceGunzip, csrc/rd_inflate_dev.hpp): one wave per BGZF / 'RD' member
  stream   rd_gz_stream_inflate (gz.DeviceStreamGunzip, csrc/rd_inflate_stream.hpp): one .gz decoded in speculative sections
  ranges   rd_gz_range_decode / rd_gz_range_resolve (data_loader/gz_shard.py): one .gz shared by W ranks (threads here)
  reader   data_loader/device_reader.py with RD_DEVICE_INFLATE=stream, and the CLI on single-stream .gz inputs
A valid stream gives zlib's bytes (CRC-32 and ISIZE checked); a stream zlib rejects is an error, never text."""
import zlib

import numpy as np
import pytest

import deflate_corpus as D
from test_gpu_gunzip_stream import _inflate, _reader_text
from test_gpu_gz_range import _ranges_text

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the documented refusals of the stream decoder (GZS_* in csrc/rd_inflate_stream.hpp; gz.GZS_ERRORS)
GZS_DECODE, GZS_OVERFLOW, GZS_NOSTOP = 1, 3, 4


def _need_libdeflate(enc):
    if D.ENCODERS[enc][1] and D.libdeflate() is None:
        pytest.skip(D.LIBDEFLATE_MISSING)


# ---- members ----------------------------------------------------------------------------------------------------------------------------

def _member_pieces():
    """(name, raw DEFLATE, text, valid): every hand-built stream, and 64 KiB pieces of every text by every encoder"""
    out = [(n,) + D.valid(n) + (True,) for n in D.VALID]
    out += [(n,) + D.invalid(n) + (False,) for n in D.INVALID]
    # empty members other than BGZF's canonical EOF block (03 00, CRC 0 - not sent to the kernel): decoded and checked like any
    out += [("empty_stored", b"\x01\x00\x00\xff\xff", b"", True), ("empty_dynamic", D.valid_empty_dynamic(), b"", True)]
    for k, name in enumerate(D.TEXTS):
        t = D.text(name)
        piece = t[(k * 77777) % (len(t) - 65280):][:65280]
        for enc, (f, ld) in D.ENCODERS.items():
            if ld and D.libdeflate() is None:
                continue
            out.append(("%s/%s" % (name, enc), f(piece), piece, True))
    return out


def test_members_equal_zlib_and_invalid_members_are_errors():
    """valid and invalid members mixed in ONE launch: each valid member's text is zlib's, each invalid one has a non-zero status
    (its trailer carries the CRC-32 and size of the text a lenient decoder would produce)"""
    from ribodetector_amd import _native as N
    from ribodetector_amd import gz
    pieces = _member_pieces()
    for _, raw, t, ok in pieces:
        D.self_check(raw, t, ok)
    blob = b"".join(D.sized_member(raw, t) for _, raw, t, _ in pieces)
    dg = gz.DeviceGunzip(DEV)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    n, consumed, out_bytes, streaming = dg.index(buf, len(buf))
    assert n == len(pieces) and consumed == len(buf) and not streaming
    dg.submit(buf, consumed, n, out_bytes)
    N.wait_event(dg._slots[0].event)
    status = dg._slots[0].status_host[:n].numpy().copy()
    text = dg._slots[0].text_dev[:out_bytes].cpu().numpy().tobytes()
    pos, wrong = 0, []
    for (name, _, t, ok), s in zip(pieces, status):
        if ok and (s != 0 or text[pos:pos + len(t)] != t):
            wrong.append((name, int(s)))
        if not ok and s == 0:
            wrong.append((name, "accepted"))
        pos += len(t)
    assert not wrong, wrong
    if D.libdeflate() is None:
        pytest.skip(D.LIBDEFLATE_MISSING + " (every other member was checked)")
    assert sum(1 for p in pieces if p[0].endswith("/ld12")) == len(D.TEXTS)


# ---- stream -----------------------------------------------------------------------------------------------------------------------------

HDR = len(D.gzip_member(b"", b"", flags=8)) - 8      # bytes of the member header in front of the DEFLATE data


def _stream(raw, data, batch=None, section=None, states=False):
    """(text or None, last state[, every batch's state]) of the member through DeviceStreamGunzip; a text is zlib's with its trailer
    checked"""
    got, st = _inflate(D.gzip_member(raw, data, flags=8), batch=batch, section=section)
    if got is not None:
        assert got == data and st[-1]["trailer_ok"]
    return (got, st[-1], st) if states else (got, st[-1])


# zlib 1-9, libdeflate 1-12 and pigz-style on FASTQ / FASTA text: decoded on the device, never refused - except the slot overflows
# (GZS_OVERFLOW) below, with the default 16 KiB sections. libdeflate writes blocks of up to ~300,000 symbols (zlib: 16,384) and the search
# does not look for final blocks: a section that takes over its successors can produce more than its SECTION * CAP_RATIO symbols. The
# reader then hands the file to the host (test_reader_takes_libdeflate_and_pigz_files below). These cases may be decoded one day; no
# other case may be refused.
KNOWN_OVERFLOW = {(t, "ld%d" % lv) for t in ("illumina", "illumina_crlf") for lv in range(2, 13)} | {("fasta60", e) for e in ("ld3", "ld10", "ld11", "ld12")}
REALISTIC = ["zlib%d" % lv for lv in range(1, 10)] + ["ld%d" % lv for lv in range(1, 13)] + ["pigz6", "pigz9_64k"]


@pytest.mark.parametrize("name", D.FASTQ_FASTA)
def test_stream_decodes_realistic_text_of_every_encoder(name):
    refused = []
    for enc in REALISTIC:
        _need_libdeflate(enc)
        got, st = _stream(D.compressed(name, enc), D.text(name))
        if got is None:
            refused.append((name, enc, st["status"]))
    assert all(s == GZS_OVERFLOW and (n, e) in KNOWN_OVERFLOW for n, e, s in refused), refused


# the slot overflows of test_stream_sections_and_batches by section size (16 KiB: KNOWN_OVERFLOW). 4 KiB sections hold 98,304 symbols:
# a section that takes over its neighbours outgrows them with zlib's and libdeflate's blocks alike; zlib's Z_FIXED has no block start
# the search finds, below 256 KiB sections
SMALL_SECTION_OVERFLOW = {4096: {("fastq", e) for e in ("ld6", "ld9", "ld12")} | {(t, e) for t in ("illumina_crlf", "fasta60")
                                                                                  for e in ("ld6", "ld9", "ld12", "pigz6")}}
SMALL_BATCH = 1 << 17       # three or more batches per stream: the window, CRC and next start carried on the device, the next start searched in SLACK


@pytest.mark.parametrize("name", ["contig", "lowcomplex"])
def test_stream_on_a_contig_and_low_complexity_reads(name):
    """one line of 3 MiB of ACGT (blocks of literals only), and poly-A / short-period reads mixed with ordinary ones (~3:1, far below
    the 250:1 the decoder refuses by design): zlib's text, in one batch and in 128 KiB batches; libdeflate's streams may overflow a
    slot like those of KNOWN_OVERFLOW"""
    for enc in ("zlib6", "zlib9", "ld1", "ld6", "ld12", "pigz6"):
        _need_libdeflate(enc)
        raw, data = D.compressed(name, enc), D.text(name)
        for batch in (None, SMALL_BATCH):
            got, st, states = _stream(raw, data, batch, None, states=True)
            if got is None:         # (libdeflate's long blocks: the slot overflow of KNOWN_OVERFLOW)
                assert enc.startswith("ld") and st["status"] == GZS_OVERFLOW, (enc, batch, st)
            else:
                assert batch is None or len(states) >= 2


@pytest.mark.parametrize("enc", ["ld1", "ld6", "ld9", "ld12", "pigz6", "zlib6_fixed"])
@pytest.mark.parametrize("name", ["fastq", "illumina_crlf", "fasta60"])
def test_stream_sections_and_batches(name, enc):
    """one batch and 128 KiB batches (three or more per stream), sections from 4 KiB to 256 KiB (to 64 KiB in the small batches): zlib's
    text, or the slot overflows pinned above"""
    _need_libdeflate(enc)
    raw, data = D.compressed(name, enc), D.text(name)
    assert len(raw) > 3 * SMALL_BATCH
    for batch, sections in ((None, (4096, 16384, 65536, 262144)), (SMALL_BATCH, (4096, 16384, 65536))):
        for section in sections:
            got, st, states = _stream(raw, data, batch, section, states=True)
            known = (name, enc) in (KNOWN_OVERFLOW if section == 16384 else SMALL_SECTION_OVERFLOW.get(section, set()))
            if enc == "zlib6_fixed" and section < 262144:
                # (no block start anywhere: section 0 outgrows its slot, or in a small batch decodes on to the end of the bytes it has)
                assert got is not None or st["status"] in (GZS_OVERFLOW, GZS_NOSTOP), (batch, section, st)
            elif known:
                assert got is not None or st["status"] == GZS_OVERFLOW, (batch, section, st)
            else:
                assert got is not None, (batch, section, st)
            if batch and got is not None:
                assert len(states) >= 3, (section, len(states))


@pytest.mark.parametrize("name", list(D.VALID))
def test_stream_on_spliced_hand_built_blocks(name):
    """hand-built blocks in the middle of a zlib stream, met by sections of every size and by a batch edge: the batch ends on the
    first section boundary inside the hand-built blocks (behind them when they are shorter than a section), so that the next batch's
    start is searched among them and the state is carried across them"""
    raw, data, r0, r1 = D.spliced_parts(name)
    for section in (4096, 16384, 65536):
        got, st = _stream(raw, data, None, section)
        assert got is not None, (section, st)
        edge = -(-(HDR + r0 + 1) // section) * section              # (batches are whole sections)
        got, st, states = _stream(raw, data, edge, section, states=True)
        assert got is not None and len(states) >= 2, (section, edge, st)
        if section == 4096 and r1 - r0 >= 2 * section:
            assert HDR + r0 < edge < HDR + r1


@pytest.mark.parametrize("name", list(D.SPLICEABLE_INVALID))
def test_stream_refuses_invalid_blocks(name):
    """an invalid block behind 1 MiB of good text: the batch that holds it fails with GZS_DECODE"""
    raw, data = D.spliced(name)
    for section in (4096, 65536):
        got, st = _stream(raw, data, None, section)
        assert got is None and st["status"] == GZS_DECODE, (section, st)


# ---- ranges -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def range_text():
    return D.text("fastq") + D.text("illumina") + D.text("fasta80")


@pytest.mark.parametrize("enc", ["ld1", "ld6", "ld12", "pigz6", "spliced_v1_cross_repeat"])
def test_ranges_concatenate_to_zlibs_text(tmp_path, range_text, enc):
    from ribodetector_amd.data_loader import gz_shard as gs
    if enc.startswith("spliced_"):
        raw, data, r0, r1 = D.spliced_parts(enc[len("spliced_"):], after=1_056_768)
        size = len(D.gzip_member(raw, data))
        bounds = gs.range_bounds(size, 2)
        assert 10 + r0 < bounds[1] < 10 + r1          # (W = 2: rank 1 searches its first block start among the hand-built blocks)
    else:
        _need_libdeflate(enc)
        raw, data = D.ENCODERS[enc][0](range_text), range_text
    path = str(tmp_path / "x.fq.gz")
    with open(path, "wb") as fh:
        fh.write(D.gzip_member(raw, data))
    for world in (2, 3, 5):
        texts, metas, crc = _ranges_text(path, world)
        assert texts is not None, (world, crc)
        assert b"".join(texts) == data and crc == zlib.crc32(data), world


# ---- reader and CLI ---------------------------------------------------------------------------------------------------------------------

def test_reader_takes_libdeflate_and_pigz_files_on_the_device(tmp_path, monkeypatch):
    """zlib's text; on the device unless the stream decoder overflows a slot (KNOWN_OVERFLOW): then the host's decoder, same text"""
    monkeypatch.setenv("RD_DEVICE_INFLATE", "stream")
    for enc in ("ld1", "ld6", "ld12", "pigz6"):
        _need_libdeflate(enc)
        for name in ("fastq", "illumina"):
            p = str(tmp_path / ("%s_%s.fq.gz" % (name, enc)))
            with open(p, "wb") as fh:
                fh.write(D.gzip_member(D.compressed(name, enc), D.text(name)))
            st = {}
            assert _reader_text(p, stats=st) == D.text(name), (name, enc)
            fallback = st.get("fallback") or st.get("feeder", {}).get("fallback")
            if (name, enc) in KNOWN_OVERFLOW:
                assert fallback in (None, gz_errors()[GZS_OVERFLOW]), (name, enc, st)
            else:
                assert fallback is None and "feeder" in st, (name, enc, st)


def gz_errors():
    from ribodetector_amd import gz
    return gz.GZS_ERRORS


@pytest.mark.parametrize("where", ["alone", "spliced"])
def test_reader_reports_every_invalid_stream(tmp_path, monkeypatch, where):
    monkeypatch.setenv("RD_DEVICE_INFLATE", "stream")
    for name in (D.INVALID if where == "alone" else D.SPLICEABLE_INVALID):
        raw, lenient = D.invalid(name) if where == "alone" else D.spliced(name)
        p = str(tmp_path / (name + ".fastq.gz"))
        with open(p, "wb") as fh:
            fh.write(D.gzip_member(raw, lenient))
        with pytest.raises(ValueError):
            _reader_text(p)


def test_cli_on_libdeflate_single_stream_inputs_writes_the_host_readers_files(tmp_path, monkeypatch):
    from ribodetector_amd import detect, synth
    _need_libdeflate("ld6")
    n = 60000
    ins = []
    for m in range(2):
        a, o, _ = synth.reads_numpy(n, (40, 140), seed=110 + m, rrna_frac=0.3)
        plain = str(tmp_path / ("r_%d.fq" % (m + 1)))
        synth.write_fastq_realistic(plain, a, o, m + 1, seed=m)
        data = open(plain, "rb").read()
        p = plain + ".gz"
        with open(p, "wb") as fh:
            fh.write(D.gzip_member(D.libdeflate_raw(data, 6 + 3 * m), data))
        ins.append(p)

    def run(tag):
        outs = [str(tmp_path / ("%s.non%d.fq" % (tag, e))) for e in range(2)]
        rrs = [str(tmp_path / ("%s.rr%d.fq" % (tag, e))) for e in range(2)]
        pr = detect.main(["-l", "100", "-i", *ins, "-o", *outs, "-r", *rrs, "--chunk_size", "8", "-m", "3", "-e", "rrna"])
        return pr, [open(f, "rb").read() for f in outs + rrs]
    monkeypatch.setenv("RD_INGEST", "host")
    pr_h, want = run("host")
    monkeypatch.delenv("RD_INGEST")
    pr_d, got = run("dev")
    assert got == want and pr_d.num_read == pr_h.num_read == n and pr_d.num_rrna == pr_h.num_rrna > 0
    # (mate 2 - libdeflate level 9 on Illumina-style text - is one of the slot overflows of KNOWN_OVERFLOW: the host decodes it)
    for v in pr_d.ingest.values():
        assert v["path"] == "device" or v.get("fallback") == gz_errors()[GZS_OVERFLOW], pr_d.ingest
    assert pr_d.ingest["r_1.fq.gz"]["path"] == "device", pr_d.ingest
