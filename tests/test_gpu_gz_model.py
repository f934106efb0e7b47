"""The device DEFLATE encoder (rd_gz_deflate_kernel, csrc/rd_deflate.hpp) against a plain model of its parse and its code construction
(tests/gz_model.py), not only against a decoder: tests/test_gpu_gz.py shows that the output inflates to the records - which an
encoder of literals alone would pass.

  * crafted members (tests/gz_cases.py), where no lookup can depend on which lane won an insert: the device's tokens are the
    model's, token for token;
  * every member, crafted or not: the tokens keep what every parse must keep (audit_member), and the member's bytes are what
    encode_member makes of the DEVICE's tokens - code lengths, HLIT / HDIST / HCLEN, the 15-bit repair, the dummy distance codes, the
    stored-block choice, every bit, BSIZE, CRC-32 and ISIZE;
  * the stored / dynamic choice at the two neighbouring inputs where the model's dynamic block crosses len + 5.
A STORED member hides its tokens; there the bytes are compared with what the model writes for its own parse.
"""
import struct
import zlib

import numpy as np
import pytest
import torch

import deflate_tokens as T
import gz_cases as C
import gz_model as M
from test_gpu_gz import _records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dg():
    from ribodetector_amd.gz import DeviceGzip
    return DeviceGzip(DEV)


def _device_members(dg, text):
    """the text as ONE selected record -> its members, walked by BSIZE"""
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV)
    rs = torch.tensor([0, len(text)], dtype=torch.int64, device=DEV)
    out, info = dg.compress_selected(t, rs, torch.ones(1, dtype=torch.int8, device=DEV), 1)
    torch.cuda.synchronize()
    nb, plain, members, flag = (int(x) for x in info.cpu().tolist())
    comp = out[:nb].cpu().numpy().tobytes()
    assert plain == len(text) and flag == 0
    got, p = [], 0
    while p < len(comp):
        assert comp[p:p + 4] == b"\x1f\x8b\x08\x04" and comp[p + 10:p + 16] == b"\x06\x00BC\x02\x00", (p, comp[p:p + 18])
        bsize = struct.unpack("<H", comp[p + 16:p + 18])[0] + 1
        got.append(comp[p:p + bsize])
        p += bsize
    assert p == len(comp) and len(got) == members == (len(text) + M.MEMBER - 1) // M.MEMBER
    return got


def _device_tokens(member):
    """the tokens of a device member, None for a stored one"""
    blocks = T.read_blocks(member[18:-8])
    assert len(blocks) == 1 and blocks[0].final and (blocks[0].end_bit + 7) // 8 == len(member) - 26
    if blocks[0].btype == T.STORED:
        return None
    assert blocks[0].btype == T.DYNAMIC
    return blocks[0].tokens


def _first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "byte %d of %d / %d: %s / %s" % (k, len(a), len(b), a[k:k + 8].hex(), b[k:k + 8].hex())


def _check_member(member, data, model_tokens=None):
    """what holds for every member; with model_tokens also that the device parsed as the model does. Returns the device's tokens."""
    tokens = _device_tokens(member)
    if tokens is None:                      # stored: the bytes the model writes for its own parse (stored as well, or this fails)
        want = M.encode_member(M.parse_member(data) if model_tokens is None else model_tokens, data)
        assert member == want, _first_difference(member, want)
        return None
    assert T.expand(tokens) == data
    assert M.audit_member(tokens, data) == []
    want = M.encode_member(tokens, data)
    assert member == want, _first_difference(member, want)
    if model_tokens is not None:
        at = next((i for i, (x, y) in enumerate(zip(tokens, model_tokens)) if x != y), None)
        assert tokens == model_tokens, "token %s: device %r, model %r" % (at, tokens[at:at + 3] if at is not None else len(tokens),
                                                                         model_tokens[at:at + 3] if at is not None else len(model_tokens))
    return tokens


@pytest.mark.parametrize("name", [name for name, _ in C.CASES])
def test_crafted_member_token_for_token(dg, name):
    _, data, model_tokens = next(c for c in C.drawn() if c[0] == name)
    members = _device_members(dg, data)
    assert len(members) == 1
    tokens = _check_member(members[0], data, model_tokens)
    if len(data) >= 600:                    # (shorter members are stored: 1 ... 65 bytes of the tail cases)
        assert tokens is not None, "a stored member: the tokens cannot be seen"


@pytest.mark.parametrize("kind", ["fastq", "random", "runs", "tiny", "huge", "fib"])
def test_every_member_is_what_the_model_writes_for_the_devices_tokens(dg, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    n = {"fastq": 5000, "random": 400, "runs": 300, "tiny": 20000, "huge": 3, "fib": 6}[kind]
    text = b"".join(_records(rng, n, kind))
    members = _device_members(dg, text)
    seen = {"stored": 0, "dynamic": 0, "no match": 0, "15 bits": 0}
    for k, member in enumerate(members):
        data = text[k * M.MEMBER:(k + 1) * M.MEMBER]
        tokens = _check_member(member, data)
        seen["stored" if tokens is None else "dynamic"] += 1
        if tokens is not None:
            blk = T.read_blocks(member[18:-8])[0]
            seen["15 bits"] += max(blk.lit_lens) == 15
            if not any(isinstance(t, tuple) for t in tokens):
                seen["no match"] += 1
                assert blk.hdist == 2 and blk.dist_lens == [1, 1]       # the two dummy distance codes
    if kind == "random":
        assert seen["dynamic"] == 0, seen
    else:
        assert seen["stored"] == 0, seen
    if kind == "fib":
        assert seen["15 bits"], seen                                    # the repair of the code lengths is reached


def test_a_member_without_a_match_sends_two_dummy_distance_codes(dg):
    name, data, model_tokens = next(c for c in C.drawn() if c[0] == "repeat of 7")
    assert not any(isinstance(t, tuple) for t in model_tokens)
    member = _device_members(dg, data)[0]
    blk = T.read_blocks(member[18:-8])[0]
    assert blk.btype == T.DYNAMIC and blk.tokens == model_tokens and blk.hdist == 2 and blk.dist_lens == [1, 1]


def test_stored_or_dynamic_at_the_crossover(dg):
    (k0, data0, tokens0, dyn0), (k1, data1, tokens1, dyn1) = C.crossover()
    n = len(data0)
    assert k1 == k0 + 1 and dyn0 < n + 5 <= dyn1 and dyn1 - dyn0 <= 4
    m0, m1 = _device_members(dg, data0)[0], _device_members(dg, data1)[0]
    assert _device_tokens(m0) == tokens0, "dynamic block of %d bytes for %d: the device stored it" % (dyn0, n)
    assert _device_tokens(m1) is None, "dynamic block of %d bytes for %d: the device did not store it" % (dyn1, n)
    _check_member(m0, data0, tokens0)
    _check_member(m1, data1, tokens1)
    assert len(m0) == 26 + dyn0 and len(m1) == 26 + 5 + n


def test_fastq_member_against_the_highest_lane_model_recorded(dg, report):
    """One FASTQ-like member of 65,280 bytes, where the answer of many lookups depends on which lane of a strip won the bucket it
    shares with others - which the kernel leaves open ("whichever of them wins") and the model settles for the highest lane.
    RECORDED, not asserted: whether the device's tokens are the model's, else how many differ, and the two member sizes
    (report["device_gzip_model"]). What every winner must keep - the audit, and the bytes for the device's own tokens - is asserted.

    Seen on an MI355X (gfx950, ROCm 7): 1,720 ambiguous lookups in the member, and the device's 28,144 tokens ARE the highest-lane
    model's, every one; both members are 14,195 bytes. So on this part, with this compiler, the highest lane's LDS store is the one
    that stays. The ISA does not promise it, which is why this stays a record."""
    rng = np.random.default_rng(2024)
    data = b"".join(_records(rng, 400, "fastq"))[:M.MEMBER]
    assert len(data) == M.MEMBER
    stats = {}
    model_tokens = M.parse_member(data, stats=stats)
    member = _device_members(dg, data)[0]
    tokens = _check_member(member, data)
    assert tokens is not None

    def placed(toks):
        out, p = set(), 0
        for t in toks:
            out.add((p, t))
            p += t[0] if isinstance(t, tuple) else 1
        return out
    mine, theirs = placed(tokens), placed(model_tokens)
    report["device_gzip_model"] = {
        "bytes": len(data), "ambiguous_lookups": stats["ambiguous"], "tokens_equal": tokens == model_tokens,
        "device_tokens": len(tokens), "model_tokens": len(model_tokens),
        "tokens_only_device": len(mine - theirs), "tokens_only_model": len(theirs - mine),
        "device_member_bytes": len(member), "model_member_bytes": len(M.encode_member(model_tokens, data)),
    }
    print("device_gzip_model", report["device_gzip_model"])
