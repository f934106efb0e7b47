"""The model of the device DEFLATE encoder (tests/gz_model.py), its token reader (tests/deflate_tokens.py) and its crafted members
(tests/gz_cases.py), held to zlib, to tools/gzdev_model.c and to themselves on the CPU. tests/test_gpu_gz_model.py compares the
kernel with the model; what is shown here is that the model is a valid encoder, that it is the algorithm the C tool measures, and
that the crafted members would tell a kernel with one rule broken from a right one.
"""
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_tokens as T
import gz_cases as C
import gz_model as M
from test_gpu_gz import _records

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _fastq(rng, n):
    return b"".join(_records(rng, n, "fastq"))


def _texts():
    rng = np.random.default_rng(7)
    return {
        "random": rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
        "fastq": _fastq(rng, 300),
        "runs": b"".join(_records(rng, 40, "runs")),
    }


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (5, zlib.Z_DEFAULT_STRATEGY),
                                            (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)])
def test_token_reader_on_zlibs_own_streams(level, strategy):
    kinds = {T.STORED: 0, T.FIXED: 0, T.DYNAMIC: 0}
    for name, data in _texts().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        raw = c.compress(data) + c.flush()
        blocks = T.read_blocks(raw)
        assert T.expand(T.tokens_of(blocks)) == data, name
        assert blocks[-1].final and not any(b.final for b in blocks[:-1])
        assert (blocks[-1].end_bit + 7) // 8 == len(raw), name          # the reader ends on the last block's last bit
        end = blocks[-1].end_bit
        assert end & 7 == 0 or raw[end >> 3] >> (end & 7) == 0, name          # (and zlib pads with zeros)
        for b in blocks:
            kinds[b.btype] += 1
            if b.btype == T.DYNAMIC:
                assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and 4 <= b.hclen <= 19
    if level == 0:
        assert kinds[T.STORED] and not kinds[T.FIXED] and not kinds[T.DYNAMIC]
    elif strategy == zlib.Z_FIXED:
        assert kinds[T.FIXED] and not kinds[T.DYNAMIC]
    else:
        assert kinds[T.DYNAMIC]


def test_token_reader_refuses_what_is_not_deflate():
    for raw in (b"\x07", b"\x01\x05\x00\x00\x00abcde", b"\x01\x05\x00\xfa\xffabc", b"\x05\xe0"):
        with pytest.raises(T.DeflateError):
            T.read_blocks(raw)


def _members(data):
    return [data[o:o + M.MEMBER] for o in range(0, len(data), M.MEMBER)] or [b""]


def _check_model_member(data):
    tokens = M.parse_member(data)
    assert T.expand(tokens) == data
    assert M.audit_member(tokens, data) == []
    member = M.encode_member(tokens, data)
    assert member[:4] == b"\x1f\x8b\x08\x04" and member[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack("<H", member[16:18])[0] + 1 == len(member) <= 65536
    assert zlib.decompress(member[18:-8], -15) == data                       # zlib is the judge of the stream
    assert struct.unpack("<II", member[-8:]) == (zlib.crc32(data) & 0xffffffff, len(data))
    blocks = T.read_blocks(member[18:-8])
    assert len(blocks) == 1 and (blocks[0].end_bit + 7) // 8 == len(member) - 26
    if blocks[0].btype == T.DYNAMIC:
        assert blocks[0].tokens == tokens and not any(s >= 16 for s in blocks[0].cl_syms)
    else:
        assert blocks[0].btype == T.STORED
    return blocks[0]


@pytest.mark.parametrize("kind", ["fastq", "random", "runs", "tiny", "huge", "fib"])
def test_the_model_is_a_valid_encoder(kind):
    rng = np.random.default_rng(11)
    n = {"fastq": 500, "random": 60, "runs": 60, "tiny": 3000, "huge": 1, "fib": 3}[kind]
    types = set()
    for data in _members(b"".join(_records(rng, n, kind)))[:3]:
        types.add(_check_model_member(data).btype)
    assert types == ({T.STORED} if kind == "random" else {T.DYNAMIC}), types
    if kind == "fib":                                                         # the 15-bit repair is reached
        blk = T.read_blocks(M.encode_member(M.parse_member(data), data)[18:-8])[0]
        assert max(blk.lit_lens) == 15


@pytest.mark.parametrize("n", list(range(0, 21)) + [4079, 4080, 4081, 65280])
def test_the_model_is_a_valid_encoder_at_every_short_length(n):
    rng = np.random.default_rng(n)
    _check_model_member(bytes(rng.choice(list(b"ACGTN\n"), n).astype(np.uint8)))


def test_a_member_with_no_match_sends_two_dummy_distance_codes():
    data = bytes(np.random.default_rng(1).choice(list(b"ACGT"), 3000).astype(np.uint8))
    tokens = list(data)                                 # (any tokens that expand to the data can be encoded)
    blk = T.read_blocks(M.encode_member(tokens, data)[18:-8])[0]
    assert blk.btype == T.DYNAMIC and blk.hdist == 2 and blk.dist_lens == [1, 1]


def test_stored_when_the_dynamic_block_is_no_smaller_or_does_not_fit():
    assert M.is_stored(105, 100) and not M.is_stored(104, 100)
    assert M.is_stored(65263, 65280) and not M.is_stored(65262, 65280)       # 18 + 65263 + 8 + 8 > 65296


def test_the_model_counts_what_the_c_tool_counts(tmp_path):
    """token and match totals of tools/gzdev_model.c (highest lane wins, as in the model) on a FASTQ of six members"""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this machine: tools/gzdev_model.c cannot be built")
    exe = str(tmp_path / "gzdev_model")
    built = subprocess.run([gcc, "-O2", "-o", exe, os.path.join(ROOT, "tools", "gzdev_model.c"), "-lz"], capture_output=True, text=True)
    if built.returncode != 0 and "zlib.h" in built.stderr:
        pytest.skip("no zlib.h on this machine: tools/gzdev_model.c cannot be built")
    assert built.returncode == 0, built.stderr
    data = _fastq(np.random.default_rng(5), 1400)
    assert len(data) > 4 * M.MEMBER
    path = tmp_path / "reads.fastq"
    path.write_bytes(data)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout
    got = re.search(r"(\d+) members, tokens (\d+) \(matches (\d+)\)", out)
    assert got, out
    ntok = nmatch = 0
    for member in _members(data):
        tokens = M.parse_member(member)
        ntok += len(tokens)
        nmatch += sum(isinstance(t, tuple) for t in tokens)
    assert (len(_members(data)), ntok, nmatch) == tuple(int(x) for x in got.groups())


def test_the_crossover_pair_straddles_the_stored_bound():
    (k0, data0, tokens0, dyn0), (k1, data1, tokens1, dyn1) = C.crossover()
    n = len(data0)
    assert k1 == k0 + 1 and len(data1) == n and dyn0 < n + 5 <= dyn1
    assert T.read_blocks(M.encode_member(tokens0, data0)[18:-8])[0].btype == T.DYNAMIC
    assert T.read_blocks(M.encode_member(tokens1, data1)[18:-8])[0].btype == T.STORED


def test_every_crafted_case_finds_a_draw_that_no_insert_can_change():
    cases = C.drawn()                                   # (asserts per case: an unambiguous draw within 20 seeds that shows its rule)
    assert len(cases) == len(C.CASES) and len({name for name, _, _ in cases}) == len(cases)
    for name, data, tokens in cases:
        stats = {}
        assert M.parse_member(data, stats=stats) == tokens and stats["ambiguous"] == 0, name
        assert len(data) <= 2 * M.PART + 7 or "part 15" in name, name
        assert M.audit_member(tokens, data) == [], name
        _check_model_member(data)
    # what section 4 of the plan lists is all there
    names = {name for name, _, _ in cases}
    for L in (7, 8, 15, 16, 17, 79, 80, 81, 143, 144, 145, 207, 208, 209, 257, 258, 259, 600) + T.LBASE[5:]:
        assert "repeat of %d" % L in names
    for R in (5, 6, 7, 15, 16, 17, 258, 1000):
        assert "run of %d" % R in names
    for n in list(range(1, 21)) + [63, 64, 65, 4079, 4080, 4081, 8167]:
        assert "member of %d bytes" % n in names
    for D in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 4584):
        assert "distance %d" % D in names
    dsyms = {M.dist_sym(t[1]) for _, _, tokens in cases for t in tokens if isinstance(t, tuple)}
    lsyms = {M.len_sym(t[0]) for _, _, tokens in cases for t in tokens if isinstance(t, tuple)}
    assert dsyms == set(range(25))                      # every distance symbol a part can reach
    assert lsyms == set(range(3, 29))                   # every length symbol the parse can make (runs of 6 and 7, matches of 8+)


# the case made for each broken rule (others may catch it too)
MADE_FOR = {
    "minimum match 7": "repeat of 8 that starts 7 bytes before the part's end",
    "minimum run 5": "run of 5",
    "run allowed at p == q0": "run over the first byte of a part",
    "no lazy rule": "lazy: 15 then 40 is deferred",
    "lazy look-ahead past the strip's last lane": "lazy: 15 then 40 at lane 63 is not deferred",
    "3 ways": "ways: the longest of four copies, the oldest",
    "exact measure stopped at 16 + 64 bytes": "repeat of 81",
    "no seed": "seed: source 1 before part 1",
    "seed of 448": "seed: source 512 before part 1",
    "ties to the farthest": "ways: two of equal length, the nearest",
    "the insert's way shift dropped": "ways: the longest of four copies",
}


@pytest.mark.parametrize("variant", list(M.VARIANTS))
def test_the_cases_have_teeth(variant):
    """a model with this one rule broken parses at least one crafted member differently: a kernel with that fault would fail there"""
    rules = M.VARIANTS[variant]
    caught = [name for name, data, tokens in C.drawn() if M.parse_member(data, rules) != tokens]
    assert MADE_FOR[variant] in caught, (variant, caught)


def test_seven_agreeing_bytes_never_share_a_bucket():
    """why `minimum match 7` is broken above as `a position with 7 bytes left is hashed`: the other reading - a way that agrees over
    7 bytes is taken - can show on no input. Two 8-byte windows that differ in the last byte alone differ in bits 7-14 of what is
    multiplied, so their hashes lie d * (0x9E3779B1 << 7) apart (mod 2^32) for a d of 1 ... 255: always more than one bucket (2^23)"""
    step = (0x9E3779B1 << 7) & 0xffffffff
    assert min(min((d * step) & 0xffffffff, (-d * step) & 0xffffffff) for d in range(1, 256)) > 1 << (32 - M.HBITS)


def test_audit_sees_what_no_winner_explains():
    name, data, tokens = next(c for c in C.drawn() if c[0] == "repeat of 81")
    at = next(i for i, t in enumerate(tokens) if isinstance(t, tuple))
    p, D = sum(t[0] if isinstance(t, tuple) else 1 for t in tokens[:at]), tokens[at][1]
    assert tokens[at] == (81, D) and M.audit_member(tokens, data) == []
    short = tokens[:at] + [(80, D), data[p + 80]] + tokens[at + 1:]
    assert T.expand(short) == data and any("not maximal" in v for v in M.audit_member(short, data))
    wrong = tokens[:at] + [(81, D + 1)] + tokens[at + 1:]
    assert any("does not repeat" in v for v in M.audit_member(wrong, data))
    name, data, tokens = next(c for c in C.drawn() if c[0] == "run of 17")
    at = tokens.index((17, 1))
    p = sum(t[0] if isinstance(t, tuple) else 1 for t in tokens[:at])
    lits = tokens[:at] + list(data[p:p + 17]) + tokens[at + 1:]
    assert any("where a run" in v for v in M.audit_member(lits, data))
    name, data, tokens = next(c for c in C.drawn() if c[0] == "repeat that ends on the part's end")
    at = tokens.index((40, 340))
    over = tokens[:at] + [(41, 340)] + tokens[at + 2:]
    assert any("crosses the part's end" in v for v in M.audit_member(over, data))
