"""The host's two gunzip decoders - sequential (csrc/rd_inflate.h, rd_host_gunzip) and parallel (csrc/rd_pgzip.h,
rd_host_gunzip_parallel) - on the corpus of tests/deflate_corpus.py: texts compressed by zlib, libdeflate and pigz-style, and hand-built
DEFLATE that zlib never writes. zlib's inflate is the judge: a valid stream gives its bytes exactly, a stream zlib rejects is an error
with zlib's message and no text."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_corpus as D
from test_inflate import gunzip, pgunzip


def _skip_without_libdeflate(enc):
    if D.ENCODERS[enc][1] and D.libdeflate() is None:
        pytest.skip(D.LIBDEFLATE_MISSING)


def _zlib_message(raw):
    try:
        D.zlib_inflate(raw)
    except zlib.error as e:
        return str(e)
    raise AssertionError("zlib accepts it")


def test_corpus_checks_itself():
    """every hand-built valid stream (alone and spliced) is zlib's text, every invalid one a zlib error; the runs that cross from the
    literal/length lengths into the distance lengths are really there"""
    for name in D.VALID:
        D.self_check(*D.valid(name))
        D.self_check(*D.spliced(name))
    for name in D.INVALID:
        D.self_check(*D.invalid(name), ok=False)
    for name in D.SPLICEABLE_INVALID:
        D.self_check(*D.spliced(name), ok=False)
    raw, _ = D.valid("v1_cross_repeat")
    assert raw[0] & 7 == 4                    # (dynamic, not final: the corpus writer's own header bits)


# realistic FASTQ: the parallel decoder must decode it in sections, not hand it to the sequential decoder. (FASTA of random bases from
# libdeflate comes in blocks longer than these 64 KiB sections: no block start in a batch, the sequential decoder takes over - same bytes)
PARALLEL_ENCODERS = ["zlib%d" % lv for lv in range(1, 10)] + ["ld%d" % lv for lv in range(1, 13)] + ["pigz6", "pigz9_64k"]
# sections dropped (no block start in them: the section in front decodes their bytes) - libdeflate's blocks outgrow a 64 KiB section on
# FASTQ with random qualities; zlib's and pigz-style blocks never do
KNOWN_DROPPED = {("fastq", "ld%d" % lv) for lv in range(2, 13)}


@pytest.mark.parametrize("enc", [n for n, _, _ in D.encoders()])
@pytest.mark.parametrize("name", D.TEXTS)
def test_host_decoders_on_every_encoder(tmp_path, name, enc):
    _skip_without_libdeflate(enc)
    data = D.text(name)
    raw = D.compressed(name, enc)
    assert D.zlib_inflate(raw) == data
    p = tmp_path / "x.gz"
    p.write_bytes(D.gzip_member(raw, data, flags=8))
    rc, got, err = gunzip(p, len(data) + 16)
    assert rc == 0 and got == data, (err, len(got))
    rc, got, err, st = pgunzip(p, len(data) + 16, 4, 65536)
    assert rc == 0 and got == data, (err, st)
    if name in D.FASTQ and enc in PARALLEL_ENCODERS:
        assert st["fell_back"] == 0 and st["used"] >= 4, st
        assert st["dropped"] <= st["used"] if (name, enc) in KNOWN_DROPPED else st["dropped"] == 0, st


@pytest.mark.parametrize("enc", ["zlib6", "ld1", "ld6", "ld12", "ld0"])
def test_host_decoders_on_bgzf(tmp_path, enc):
    """BGZF members compressed by libdeflate (what htslib's bgzip writes when built with it)"""
    _skip_without_libdeflate(enc)
    data = D.text("illumina")
    blob = D.bgzf(data, D.ENCODERS[enc][0])
    p = tmp_path / "x.gz"
    p.write_bytes(blob)
    rc, got, err = gunzip(p, len(data) + 16)
    assert rc == 0 and got == data, err
    rc, got, err, st = pgunzip(p, len(data) + 16, 4, 65536)
    assert rc == 0 and got == data and st["fell_back"] == 0, (err, st)


@pytest.mark.parametrize("name", list(D.VALID))
def test_host_decoders_on_hand_built_streams(tmp_path, name):
    """alone, and spliced into the middle of a realistic stream (the parallel decoder's sections meet them anywhere)"""
    p = tmp_path / "x.gz"
    for raw, data in (D.valid(name), D.spliced(name)):
        p.write_bytes(D.gzip_member(raw, data))
        rc, got, err = gunzip(p, len(data) + 16)
        assert rc == 0 and got == data, err
        for threads, section in ((4, 32768), (3, 200000)):
            rc, got, err, st = pgunzip(p, len(data) + 16, threads, section)
            assert rc == 0 and got == data, (err, st)


@pytest.mark.parametrize("name", list(D.INVALID))
def test_host_decoders_reject_what_zlib_rejects(tmp_path, name):
    """the violation is in the first block: an error with zlib's message and not one byte of text, whatever the trailer says"""
    raw, lenient = D.invalid(name)
    want = _zlib_message(raw)
    p = tmp_path / "x.gz"
    p.write_bytes(D.gzip_member(raw, lenient))
    rc, got, err = gunzip(p, len(lenient) + 1024)
    assert rc < 0 and got == b"" and err == want, (err, want, len(got))
    rc, got, err, st = pgunzip(p, len(lenient) + 1024, 4, 32768)
    assert rc < 0 and got == b"" and err == want, (err, want, st)


@pytest.mark.parametrize("name", list(D.SPLICEABLE_INVALID))
def test_host_decoders_reject_invalid_blocks_inside_a_stream(tmp_path, name):
    """behind 1 MiB of good text: an error, and what was handed out before it is the text in front of the violation"""
    raw, lenient = D.spliced(name)
    want = _zlib_message(raw)
    p = tmp_path / "x.gz"
    p.write_bytes(D.gzip_member(raw, lenient))
    for rc, got, err in (gunzip(p, len(lenient) + 1024), pgunzip(p, len(lenient) + 1024, 4, 65536)[:3]):
        assert rc < 0 and err == want, (err, want)
        assert len(got) <= 1 << 20 and got == lenient[:len(got)]


def test_member_index_skips_only_the_canonical_empty_member():
    """rd_host_gz_index lists every sized member for the device's member decoder but BGZF's end-of-file block (03 00, CRC 0): another
    empty member - valid or not - is decoded and checked like any"""
    from ribodetector_amd import _native as N
    good = D.text("illumina")[:50000]
    parts = [(D.zlib_raw(b""), b""), (b"\x01\x00\x00\xff\xff", b""), (D.valid_empty_dynamic(), b""), (D.invalid("btype_3")[0], b""),
             (D.zlib_raw(good), good), (D.zlib_raw(b""), b"")]
    blob = b"".join(D.sized_member(raw, t) for raw, t in parts)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    ent = np.zeros((16, 3), dtype=np.int64)
    n, consumed, ob = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = N.host_lib().rd_host_gz_index(buf.ctypes.data, len(buf), 0, 0, ent.ctypes.data, 16, C.byref(n), C.byref(consumed), C.byref(ob))
    assert rc == 0 and consumed.value == len(blob) and ob.value == len(good)
    assert n.value == 4 and list(ent[:4, 2] >> 32) == [0, 0, 0, len(good)]
    assert list(ent[:4, 2] & 0xffffffff) == [5, len(D.valid_empty_dynamic()), len(D.invalid("btype_3")[0]), len(D.zlib_raw(good))]
