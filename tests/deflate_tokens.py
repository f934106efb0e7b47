"""A raw-DEFLATE reader that keeps what zlib hides: the blocks, their headers as sent, and the tokens (RFC 1951).

read_blocks(raw) walks a raw DEFLATE stream to its final block and returns one Block per block. expand(blocks) turns the tokens back
into bytes. Plain Python, made to be read next to the RFC; used by the tests of the device encoder (tests/gz_model.py,
tests/test_gpu_gz_model.py), which compare the encoder's PARSE and not only what it inflates to.
"""
from dataclasses import dataclass, field

import numpy as np

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CLORD = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

STORED, FIXED, DYNAMIC = 0, 1, 2


class DeflateError(ValueError):
    pass


@dataclass
class Block:
    btype: int                      # STORED, FIXED or DYNAMIC
    final: bool
    tokens: list                    # a literal is an int 0..255, a match a tuple (length, distance)
    end_bit: int                    # position of the first bit behind the block
    hlit: int = 0                   # dynamic blocks: the counts as they stand for (257.., 1.., 4..), not the header's fields
    hdist: int = 0
    hclen: int = 0
    cl_lens: list = field(default_factory=list)      # the 19 code-length code lengths, by symbol
    lit_lens: list = field(default_factory=list)     # hlit literal/length code lengths as sent
    dist_lens: list = field(default_factory=list)    # hdist distance code lengths as sent
    cl_syms: list = field(default_factory=list)      # the code-length symbols in the order sent (16, 17, 18 included)


class _Bits:
    """LSB-first bit reader: peek[p] holds the 15 bits from bit p on (zeros behind the end), so a field or a code is one lookup"""

    def __init__(self, raw, bit=0):
        b = np.unpackbits(np.frombuffer(bytes(raw), dtype=np.uint8), bitorder="little").astype(np.int32)
        self.nbits = len(b)
        b = np.concatenate([b, np.zeros(16, dtype=np.int32)])
        peek = np.zeros(self.nbits + 1, dtype=np.int32)
        for k in range(15):
            peek |= b[k:k + self.nbits + 1] << k
        self.peek, self.pos = peek.tolist(), bit

    def take(self, n):                       # n <= 15
        if self.pos + n > self.nbits:
            raise DeflateError("stream ends inside a block")
        v = self.peek[self.pos] & ((1 << n) - 1)
        self.pos += n
        return v


def _decoder(lens):
    """canonical Huffman code of the lengths -> table over the next 15 bits as read (LSB first): (symbol, length), None = no code"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << 15)
    for s, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            if c >> l:
                raise DeflateError("oversubscribed code")
            r = int(format(c, "0%db" % l)[::-1], 2)          # DEFLATE packs Huffman codes MSB first
            for hi in range(r, 1 << 15, 1 << l):
                table[hi] = (s, l)
    return table


def _symbol(bits, table):
    e = table[bits.peek[bits.pos]] if bits.pos <= bits.nbits else None
    if e is None or bits.pos + e[1] > bits.nbits:
        raise DeflateError("no code matches at bit %d" % bits.pos)
    bits.pos += e[1]
    return e[0]


_FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST = [5] * 30


def read_blocks(raw, bit=0):
    """the blocks of the raw DEFLATE stream that starts at bit `bit` of raw, up to and with its final block"""
    bits = _Bits(raw, bit)
    blocks, produced = [], 0
    while True:
        final = bool(bits.take(1))
        btype = bits.take(2)
        if btype == STORED:
            bits.pos = (bits.pos + 7) & ~7
            n = bits.take(8) | bits.take(8) << 8
            nn = bits.take(8) | bits.take(8) << 8
            if n ^ nn != 0xffff:
                raise DeflateError("stored block: LEN and NLEN disagree")
            at = bits.pos >> 3
            if at + n > len(raw):
                raise DeflateError("stored block runs past the stream")
            bits.pos += 8 * n
            blk = Block(STORED, final, list(raw[at:at + n]), bits.pos)
        elif btype in (FIXED, DYNAMIC):
            blk = Block(btype, final, [], 0)
            if btype == FIXED:
                lit, dist = _decoder(_FIXED_LIT), _decoder(_FIXED_DIST)
            else:
                blk.hlit, blk.hdist, blk.hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                blk.cl_lens = [0] * 19
                for k in range(blk.hclen):
                    blk.cl_lens[CLORD[k]] = bits.take(3)
                cl = _decoder(blk.cl_lens)
                seq = []
                while len(seq) < blk.hlit + blk.hdist:
                    s = _symbol(bits, cl)
                    blk.cl_syms.append(s)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        if not seq:
                            raise DeflateError("repeat with nothing before it")
                        seq += [seq[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        seq += [0] * (3 + bits.take(3))
                    else:
                        seq += [0] * (11 + bits.take(7))
                if len(seq) != blk.hlit + blk.hdist:
                    raise DeflateError("code lengths overrun their count")
                blk.lit_lens, blk.dist_lens = seq[:blk.hlit], seq[blk.hlit:]
                lit, dist = _decoder(blk.lit_lens), _decoder(blk.dist_lens)
            while True:
                s = _symbol(bits, lit)
                if s < 256:
                    blk.tokens.append(s)
                    produced += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("length symbol %d" % s)
                    length = LBASE[s - 257] + bits.take(LEXTRA[s - 257])
                    d = _symbol(bits, dist)
                    if d > 29:
                        raise DeflateError("distance symbol %d" % d)
                    distance = DBASE[d] + bits.take(DEXTRA[d])
                    if distance > produced:
                        raise DeflateError("distance %d reaches before the stream" % distance)
                    blk.tokens.append((length, distance))
                    produced += length
            blk.end_bit = bits.pos
        else:
            raise DeflateError("block type 3")
        if btype == STORED:
            produced += len(blk.tokens)
        blocks.append(blk)
        if final:
            return blocks


def tokens_of(blocks):
    return [t for b in blocks for t in b.tokens]


def expand(tokens):
    """what the tokens stand for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            length, distance = t
            if distance > len(out):
                raise DeflateError("distance %d at byte %d" % (distance, len(out)))
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
        else:
            out.append(t)
    return bytes(out)
