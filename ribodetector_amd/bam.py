"""Unaligned (or aligned) BAM as an input format: the rule in plain Python - what a record is, which records count, and the FASTQ text
a record becomes. The device side is csrc/rd_bam_index.hpp behind the C ABI rd_bam_index / rd_bam_gather / rd_bam_sample
(data_loader/device_reader.BamIndexer); every table it writes equals the serial walk below. Nothing here touches a GPU.

A BAM file is a BGZF file (gzip members that carry their size). All integers little-endian. Inflated and concatenated:
    magic "BAM\\1", l_text:int32, text[l_text], n_ref:int32, n_ref x (l_name:int32, name[l_name], l_ref:int32)        the header
    then records up to the end of the data. A record at offset p:
    p+0 block_size:int32 (bytes of the record BEHIND this field)   p+4 refID:int32   p+8 pos:int32   p+12 l_read_name:uint8 (with the NUL)
    p+13 mapq:uint8   p+14 bin:uint16   p+16 n_cigar_op:uint16   p+18 flag:uint16   p+20 l_seq:uint32   p+24 next_refID:int32
    p+28 next_pos:int32   p+32 tlen:int32   p+36 read_name, cigar[4 n_cigar_op], seq[(l_seq + 1) / 2], qual[l_seq], tags to p + 4 + block_size
    base i = high nibble of seq[i / 2] for even i, else the low one; code c = "=ACMGRSVTWYHKDBN"[c]
    well-formed: 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size, l_read_name >= 1, read_name ends in NUL.

The walk (records): at p == end the data is over. Fewer than 4 bytes left, or p + 4 + block_size > end: the data ends inside a record
("truncated BAM record at end of file"). block_size < 32, or a record that is not well-formed: "malformed BAM record N", N counting
every record of the file from 0. Else the next record starts at p + 4 + block_size.

Record -> FASTQ text (fastq_text):  '@' name-without-NUL '\\n' SEQ '\\n' '+' '\\n' QUAL '\\n'  = 2 l_seq + l_read_name + 5 bytes.
QUAL[i] = min(qual[i], 93) + 33; qualities absent (l_seq > 0 and qual[0] == 0xFF): every QUAL[i] = '"'. flag & 0x10: SEQ reverse-
complemented (the complement of code c is the 4-bit bit reversal of c: "=TGKCYSBAWRDMHVN"[c]) and QUAL reversed, as samtools fastq
does. flag & 0x900 (secondary / supplementary): the record is skipped - each read appears once. Tags, CIGAR, mapq, references: ignored.

BAM output (detect.py --bam_output; device side csrc/rd_bam_raw.hpp): an output file is header(path of its input) followed by
select(data, keep) - the kept records as they stand in the input, every tag included, in input order - in BGZF members.

Optional fields (find_tag; device side csrc/rd_bam_tags.hpp, C ABI rd_bam_tag_find): the tags of a record lie between the qualities and
the record's end E = p + 4 + block_size, each one as tag[2] type[1] value. Type A c C: 1 byte; s S: 2; i I f: 4; Z H: bytes up to and
with a NUL; B: subtype[1] (one of cCsSiIf) count:uint32 and count elements. Every length is data: a tag whose value does not end at or in
front of E, an unknown type, fewer than 3 bytes left in front of E: the tags are malformed. Read groups (detect.py --read_groups): the
header text declares them ('@RG' lines, read_groups), a record names its group with RG:Z:<id>, and group_row says which row of the
per-group counters a record is counted in.

Tags in FASTQ header lines (detect.py --bam_tags; device side csrc/rd_bam_tagtext.hpp, C ABI rd_bam_tag_splice): tag_comment says what
a record's listed tags become behind its read name - '\\tTG:T:text' per tag, SAM's text form, as `samtools fastq -T` writes it - and
fastq_text_tagged is fastq_text with that comment in front of the first newline of every record. Float-typed values (f, B:f) are left
out and counted, or, with floats=True (--bam_tag_floats), written as float_g says: printf's %g, stated in whole numbers (device side
csrc/rd_float_text.hpp, C ABI rd_float_text / rd_bam_tag_splice_ex). A record whose listed tags cannot be walked, or hold a byte that
would break a FASTQ header line, gets no comment.

FASTQ / FASTA text as BAM records (detect.py --ubam_output; device side csrc/rd_bam_encode.hpp, C ABI rd_bam_encode): from_fastq says
what a record of the text becomes - encode_record of its name (ubam_name: the report's read id, without the mate's /1 or /2 in a paired
run, '*' when empty), its bases as the letters of CODES (either case, U as T, anything else N), its qualities clamped to 0..93 (FASTA:
absent) and the flag 4 / 77 / 141; an output file is encode_header((), UBAM_HEADER_TEXT) and the selected records in BGZF members.
"""
import os
import re
import struct
import zlib

from . import _native as N

SEGMENT = N.BAM_SEGMENT          # bytes per segment of the device framing (RD_BAM_SEGMENT), counted from the first record of a batch
MAGIC = b"BAM\1"
CODES = b"=ACMGRSVTWYHKDBN"
COMPLEMENT = b"=TGKCYSBAWRDMHVN"
SKIP_FLAGS = 0x900
MALFORMED = "malformed BAM record %d"
TRUNCATED = "truncated BAM record at end of file"
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# --bam_shard (data_loader/bam_shard.py): a share of a rank begins where find_record_start says a record starts
NO_START = "no BAM record start within %d bytes behind offset %d of %s"
NOT_A_BOUNDARY = ("the share boundary at offset %d of %s is not a BAM record boundary (a byte pattern that looks like %d records in a row): "
                  "run this file on one rank")


def header_len(data):
    """the length of the header at the start of `data` (inflated bytes); None while the header is not complete; ValueError: bad magic"""
    if bytes(data[:4]) != MAGIC[:len(data[:4])]:
        raise ValueError("not a BAM file (the inflated data does not start with 'BAM\\1')")
    if len(data) < 8:
        return None
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0:
        raise ValueError("not a BAM file (negative header text length)")
    p = 8 + l_text
    if len(data) < p + 4:
        return None
    n_ref = struct.unpack_from("<i", data, p)[0]
    if n_ref < 0:
        raise ValueError("not a BAM file (negative reference count)")
    p += 4
    for _ in range(n_ref):
        if len(data) < p + 4:
            return None
        l_name = struct.unpack_from("<i", data, p)[0]
        if l_name < 0:
            raise ValueError("not a BAM file (negative reference name length)")
        p += 4 + l_name + 4
    return p if len(data) >= p else None


def header_bytes(path):
    """the header's length in inflated bytes: host zlib over the leading gzip members until the header is complete. ValueError on bad
    magic or a header the file ends in"""
    data = bytearray()
    with open(path, "rb") as fh:
        d = zlib.decompressobj(31)
        raw = b""
        while True:
            if not raw:
                raw = fh.read(1 << 16)
                if not raw:
                    break
            try:
                data += d.decompress(raw)
            except zlib.error as e:
                raise ValueError("%s: %s" % (path, e))
            raw = b""
            if d.eof:
                raw, d = d.unused_data, zlib.decompressobj(31)
            n = header_len(data)
            if n is not None:
                return n
    header_len(data)
    raise ValueError("truncated BAM header")


def header(path):
    """the header's inflated bytes (magic, text, references) - what every BAM output of a run starts with, byte for byte: host zlib over
    the leading gzip members, like header_bytes. ValueError on bad magic or a header the file ends in"""
    n = header_bytes(path)
    data = bytearray()
    with open(path, "rb") as fh:
        d = zlib.decompressobj(31)
        while len(data) < n:
            raw = fh.read(1 << 16)
            if not raw:
                raise ValueError("truncated BAM header")
            while raw and len(data) < n:
                data += d.decompress(raw)
                raw = b""
                if d.eof:
                    raw, d = d.unused_data, zlib.decompressobj(31)
    return bytes(data[:n])


def select(data, keep, start=None):
    """BAM output (--bam_output): the records of `data` (records(data, start)) that are not skipped and whose index among the delivered
    records is in `keep`, as they stand in the input - block_size, fixed fields, name, CIGAR, packed bases, qualities, every tag -
    joined in input order. Nothing is decoded; a record on the reverse strand stays as it is stored."""
    data, keep = bytes(data), set(int(k) for k in keep)
    delivered = (r for r in records(data, start) if not r.skipped)
    return b"".join(data[r.offset:r.offset + r.size] for k, r in enumerate(delivered) if k in keep)


class Record:
    """one record of the walk: where it lies in the data (offset, size with the block_size field) and what the text depends on"""
    __slots__ = ("offset", "size", "name", "flag", "codes", "qual")

    def __init__(self, offset, size, name, flag, codes, qual):
        self.offset, self.size, self.name, self.flag, self.codes, self.qual = offset, size, name, flag, codes, qual

    @property
    def skipped(self):
        return bool(self.flag & SKIP_FLAGS)

    def fastq(self):
        codes, qual = self.codes, self.qual
        if len(qual) and qual[0] == 0xFF:
            q = b'"' * len(qual)
        else:
            q = bytes(min(x, 93) + 33 for x in qual)
        if self.flag & 0x10:
            s = bytes(COMPLEMENT[c] for c in reversed(codes))
            q = q[::-1]
        else:
            s = bytes(CODES[c] for c in codes)
        return b"@" + self.name + b"\n" + s + b"\n+\n" + q + b"\n"


def records(data, start=None):
    """the plain serial walk over the inflated bytes of a BAM file (start: where the records begin; None: behind the header, which
    `data` then starts with). Yields Record objects - the skipped ones too - and raises ValueError at the damage, behind the records in
    front of it."""
    data = bytes(data)
    p = header_len(data) if start is None else int(start)
    if p is None:
        raise ValueError("truncated BAM header")
    end, k = len(data), 0
    while p < end:
        if end - p < 4:
            raise ValueError(TRUNCATED)
        block = struct.unpack_from("<i", data, p)[0]
        if block < 32:
            raise ValueError(MALFORMED % k)
        if p + 4 + block > end:
            raise ValueError(TRUNCATED)
        l_name, n_cigar, flag, l_seq = data[p + 12], struct.unpack_from("<H", data, p + 16)[0], struct.unpack_from("<H", data, p + 18)[0], \
            struct.unpack_from("<I", data, p + 20)[0]
        if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block or l_name < 1 or data[p + 36 + l_name - 1] != 0:
            raise ValueError(MALFORMED % k)
        s = p + 36 + l_name + 4 * n_cigar
        packed = data[s:s + (l_seq + 1) // 2]
        codes = [(packed[i >> 1] & 15) if i & 1 else (packed[i >> 1] >> 4) for i in range(l_seq)]
        yield Record(p, 4 + block, data[p + 36:p + 36 + l_name - 1], flag, codes, data[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq])
        p += 4 + block
        k += 1


def fastq_text(data, start=None):
    """the FASTQ text of the records of `data` that count (module docstring); raises what records() raises"""
    return b"".join(r.fastq() for r in records(data, start) if not r.skipped)


# ---- a record start at or behind an offset (detect.py --bam_shard; device side csrc/rd_bam_shard.hpp, C ABI rd_bam_find_start) ------

CONFIRM = N.BAM_CONFIRM          # RD_BAM_CONFIRM: records in a row that make a candidate offset a record start


def plausible(data, q, end):
    """does offset q of `data` carry the SIGNATURE of a record (bam_plausible of csrc/rd_bam_index.hpp, restated)? block_size in
    33..2^26; refID, pos, next_refID, next_pos >= -1; l_read_name >= 1; the lengths fit in block_size; the name's NUL where it belongs
    when it lies in front of `end`; the first min(l_read_name - 1, 16) name bytes (those in front of `end`) in 33..126. No byte at or
    behind `end` is looked at; q + 36 > end: False."""
    if q + 36 > end:
        return False
    block, ref_id, pos = struct.unpack_from("<iii", data, q)
    if block < 33 or block > (1 << 26):
        return False
    next_ref, next_pos = struct.unpack_from("<ii", data, q + 24)
    if ref_id < -1 or pos < -1 or next_ref < -1 or next_pos < -1:
        return False
    l_name, n_cigar, l_seq = data[q + 12], struct.unpack_from("<H", data, q + 16)[0], struct.unpack_from("<I", data, q + 20)[0]
    if l_name < 1 or 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block:
        return False
    nul = q + 36 + l_name - 1
    if nul < end and data[nul] != 0:
        return False
    for i in range(min(l_name - 1, 16)):
        if q + 36 + i >= end:
            break
        if not 33 <= data[q + 36 + i] <= 126:
            return False
    return True


CONFIRMED, REJECTED, UNDECIDED = 1, 0, -1


def chain_verdict(data, q, end, at_eof, confirm=CONFIRM):
    """the verdict on candidate q of find_record_start: the chain of records from q is followed for `confirm` records.
    At p == end (behind at least one record): CONFIRMED with at_eof, else UNDECIDED. Fewer than 36 bytes in front of `end`: the
    signature cannot be tested - REJECTED with at_eof (the walk of `records` ends in a truncated record there), else UNDECIDED. A
    record that is not plausible: REJECTED. One that is, and does not lie in front of `end` as a whole: REJECTED with at_eof, else
    UNDECIDED. (A plausible record that lies in front of `end` as a whole is well-formed by the rule of `records`: the signature holds
    every one of its tests.) `confirm` such records: CONFIRMED."""
    p = q
    for _ in range(confirm):
        if p == end:
            return CONFIRMED if at_eof else UNDECIDED
        if p + 36 > end:
            return REJECTED if at_eof else UNDECIDED
        if not plausible(data, p, end):
            return REJECTED
        block = struct.unpack_from("<i", data, p)[0]
        if p + 4 + block > end:
            return REJECTED if at_eof else UNDECIDED
        p += 4 + block
    return CONFIRMED


def find_record_start(data, lo, hi, at_eof, confirm=CONFIRM):
    """(found, undecided) among the candidate offsets [lo, hi) of the window `data` (inflated BAM bytes, hi <= len(data)): found = the
    smallest candidate whose chain_verdict is CONFIRMED, undecided = the smallest one whose verdict is UNDECIDED (the window ends before
    its chain is confirmed or rejected); -1: none. at_eof: the window ends where the file's data ends. A caller accepts `found` only
    when no smaller candidate is undecided, and looks again with more bytes otherwise. `found` is a record start unless `confirm`
    records in a row are imitated by the bytes of a record (a tag's payload, say); it need not be the FIRST one at or behind lo - a record
    of more than 64 MiB is not plausible, and is stepped over."""
    data = bytes(data)
    end = len(data)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi > end:
        raise ValueError("find_record_start: [lo, hi) does not lie in the window")
    import numpy as np
    # (nearly every offset is rejected by its block_size alone: those are sorted out at once, the rule is applied to the others)
    a = np.frombuffer(data, dtype=np.uint8)
    full = max(lo, min(hi, end - 35))               # candidates [lo, full) have their 36 fixed bytes in the window
    cand = []
    if full > lo:
        # block_size in 33 .. 2^26: its top byte is 0..4 (a negative one: >= 0x80) - a test of one byte sorts out most offsets
        few = lo + np.flatnonzero(a[lo + 3:full + 3] <= 4)
        b = [a[few + k].astype(np.uint32) for k in range(4)]
        block = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)
        cand = few[(block >= 33) & (block <= (1 << 26))].tolist()
    found = undecided = -1
    for q in cand + list(range(full, hi)):
        if found >= 0 and undecided >= 0:
            break
        v = chain_verdict(data, q, end, at_eof, confirm)
        if v == CONFIRMED and found < 0:
            found = q
        elif v == UNDECIDED and undecided < 0:
            undecided = q
    return found, undecided


# ---- a writer that follows the specification (tests and tools make their inputs with it) --------------------------------------------

def _reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


_CIGAR_OPS = "MIDNSHP=X"


def encode_record(read):
    """one record as bytes, block_size included. read: bytes (taken as they are - a record made by hand) or a dict with
    name (bytes, no NUL), seq (the letters of CODES, str or bytes), qual (raw Phred bytes, or None: absent), and optionally flag (4),
    ref_id / pos / next_ref_id / next_pos (-1), mapq (0), tlen (0), cigar ([(length, op letter)]), tags (bytes, already encoded)"""
    if isinstance(read, (bytes, bytearray)):
        return bytes(read)
    name = bytes(read["name"]) + b"\0"
    seq = read["seq"].encode() if isinstance(read["seq"], str) else bytes(read["seq"])
    codes = [CODES.index(c) for c in seq]
    if len(codes) & 1:
        codes.append(0)
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    qual = read.get("qual")
    qual = b"\xff" * len(seq) if qual is None else bytes(qual)
    if len(qual) != len(seq) or len(name) > 255:
        raise ValueError("encode_record: qual and seq differ in length, or the name is longer than 254 bytes")
    cigar = list(read.get("cigar", ()))
    pos = int(read.get("pos", -1))
    ref_len = sum(n for n, op in cigar if op in "MDN=X")
    body = struct.pack("<iiBBHHHIiii", int(read.get("ref_id", -1)), pos, len(name), int(read.get("mapq", 0)),
                       _reg2bin(pos, pos + max(ref_len, 1)) if pos >= 0 else 4680, len(cigar), int(read.get("flag", 4)), len(seq),
                       int(read.get("next_ref_id", -1)), int(read.get("next_pos", -1)), int(read.get("tlen", 0)))
    body += name + b"".join(struct.pack("<I", (n << 4) | _CIGAR_OPS.index(op)) for n, op in cigar) + packed + qual + bytes(read.get("tags", b""))
    return struct.pack("<i", len(body)) + body


def encode_header(refs=(), text=b""):
    """the header: refs = [(name bytes, length)]"""
    out = MAGIC + struct.pack("<i", len(text)) + bytes(text) + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + bytes(name) + b"\0" + struct.pack("<i", int(length))
    return out


def payload(reads, refs=(), text=b""):
    """the inflated bytes of the file write_bam writes"""
    return encode_header(refs, text) + b"".join(encode_record(r) for r in reads)


def bgzf_member(data, level=6):
    """one BGZF member (a gzip member with the 'BC' subfield that holds its size - 1) of `data`, at most 0xff00 bytes"""
    if len(data) > 0xff00:
        raise ValueError("bgzf_member: at most 0xff00 bytes per member")
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(bytes(data)) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
            struct.pack("<II", zlib.crc32(bytes(data)) & 0xffffffff, len(data)))


def write_bam(path, reads, *, refs=(), text=b"", level=6, member_bytes=0xff00, eof=True):
    """a BAM file of `reads` (encode_record) behind a header (refs, text): BGZF members of member_bytes inflated bytes each - an integer, or
    a sequence of sizes used in order, the last one for the rest (0: an empty member) - and BGZF's 28-byte end-of-file member.
    Returns the inflated bytes."""
    data = payload(reads, refs, text)
    sizes = [member_bytes] if isinstance(member_bytes, int) else list(member_bytes)
    if not sizes or sizes[-1] < 1 or any(s < 0 or s > 0xff00 for s in sizes):
        raise ValueError("write_bam: member sizes are in [0, 0xff00], the last one >= 1")
    with open(path, "wb") as fh:
        p, k = 0, 0
        while p < len(data):
            n = sizes[min(k, len(sizes) - 1)]
            fh.write(bgzf_member(data[p:p + n], level))
            p += n
            k += 1
        if eof:
            fh.write(EOF_MEMBER)
    return data


# ---- FASTQ / FASTA text as unaligned BAM records (detect.py --ubam_output; device side csrc/rd_bam_encode.hpp, C ABI rd_bam_encode) ------
# A record of the text becomes encode_record({"name": ubam_name(...), "seq": SEQ', "qual": QUAL', "flag": UBAM_FLAGS[...]}): no
# reference, no CIGAR, no tags. This is this project's own rule; it is not claimed to be what `samtools import` writes.
UBAM_HEADER_TEXT = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"      # no @PG line, no references: the header's bytes are deterministic
UBAM_FLAGS = {(1, 0): 4, (2, 0): 77, (2, 1): 141}              # (mates of the run, mate) -> flag: unmapped; paired, both unmapped, first / last
UBAM_NAME_MAX = 254                                            # l_read_name is one byte and counts the NUL
UBAM_NAME_ERROR = "--ubam_output: the name of record %d is longer than 254 bytes"
UBAM_LENGTH_ERROR = "--ubam_output: the quality line of record %d is not as long as its sequence"
INTERLEAVED = -1                                               # from_fastq(mate=INTERLEAVED): the records alternate mate 1, mate 2
_ID_END = b" \t\r\n\v\f"
_UP = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))
UBAM_LETTER = bytes(CODES[CODES.index(_UP[c])] if _UP[c] in CODES else (ord("T") if _UP[c] == ord("U") else ord("N")) for c in range(256))
UBAM_CODE = bytes(CODES.index(UBAM_LETTER[c]) for c in range(256))        # input byte -> 4-bit code
UBAM_QUAL = bytes(min(max(c, 33), 126) - 33 for c in range(256))          # input byte -> stored quality
_SHL4 = bytes((c << 4) & 0xff for c in range(256))
_SAME_LETTER = bytes(c for c in range(256) if UBAM_LETTER[c] == c)
_IN_RANGE = bytes(range(33, 127))


def ubam_name(header_line, n_mates=1, mate=0):
    """the QNAME of a record from its header line ('@...' / '>...', with or without the line's end): the read_id of the per-read
    report - the bytes behind the first one up to the first space, \\t, \\r, \\n, \\v or \\f -, in a paired run (n_mates 2) without a
    trailing /1 on a mate-1 record (mate 0) or /2 on a mate-2 record (mate 1), decided from this record alone; an id that is empty
    after this becomes '*'. Longer than 254 bytes: returned as it is - from_fastq and the run refuse it."""
    return _ubam_id(header_line, n_mates, mate) or b"*"


def _ubam_id(header_line, n_mates, mate):
    """ubam_name in front of its last step: empty where the name is '*'"""
    line = bytes(header_line)[1:]
    end = min((p for p in (line.find(bytes([c])) for c in _ID_END) if p >= 0), default=len(line))
    name = line[:end]
    if n_mates == 2 and name.endswith(b"/1" if mate == 0 else b"/2"):
        name = name[:-2]
    return name


def _text_records(text, fasta):
    """(header line, sequence, quality or None) of every record of FASTQ text (four lines per record) or FASTA text ('>' lines, the
    lines between them joined)"""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if fasta:
        head, seq = None, []
        for ln in lines:
            if ln[:1] == b">":
                if head is not None:
                    yield head, b"".join(seq), None
                head, seq = ln, []
            elif head is None:
                raise ValueError("from_fastq: FASTA text does not start with '>'")
            else:
                seq.append(ln)
        if head is not None:
            yield head, b"".join(seq), None
        return
    if len(lines) % 4:
        raise ValueError("from_fastq: FASTQ text is not four lines per record")
    for k in range(0, len(lines), 4):
        if lines[k][:1] != b"@":
            raise ValueError("from_fastq: record %d does not start with '@'" % (k // 4))
        yield lines[k], lines[k + 1], lines[k + 3]


def _ubam_record(name, seq, qual, flag, tags=b""):
    """encode_record({"name", "seq": seq through UBAM_LETTER, "qual": qual through UBAM_QUAL or None, "flag"}), without the Python
    loop per base (tests/test_ubam_host.py holds the two against each other); tags: the bytes of its optional fields"""
    codes = seq.translate(UBAM_CODE)
    n = (len(codes) + 1) // 2
    hi, lo = codes[0::2].translate(_SHL4), codes[1::2]
    packed = (int.from_bytes(hi, "little") | int.from_bytes(lo, "little")).to_bytes(n, "little")
    q = b"\xff" * len(seq) if qual is None else qual.translate(UBAM_QUAL)
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, 0, flag, len(seq), -1, -1, 0) + name + b"\0" + packed + q + tags
    return struct.pack("<i", len(body)) + body


# --ubam_tags LIST (device side csrc/rd_bam_encode.hpp, C ABI rd_bam_encode_ex): the inverse of --bam_tags. A SAM-style comment of the
# header line - '@id' one terminator byte 'XY:T:value' '\t' 'XY:T:value' ... - becomes the record's tags.
_UBAM_TAG_TYPES = b"AiZHBf"
_B_RANGE = {ord("c"): (-128, 127), ord("C"): (0, 255), ord("s"): (-32768, 32767), ord("S"): (0, 65535),
            ord("i"): (-2 ** 31, 2 ** 31 - 1), ord("I"): (0, 2 ** 32 - 1)}
_ALPHA = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
_ALNUM = _ALPHA | frozenset(b"0123456789")


def _tag_int(text):
    """the value of [+-]?[0-9]{1,10}, None for any other text"""
    digits = text[1:] if text[:1] in (b"+", b"-") else text
    if not 1 <= len(digits) <= 10 or any(c < 48 or c > 57 for c in digits):
        return None
    return -int(digits) if text[:1] == b"-" else int(digits)


def _small_int(v):
    """type and bytes of v in [-2^31, 2^32 - 1] in the smallest type, as htslib's SAM parser stores an i value"""
    if v >= 0:
        return (b"C", "<B") if v <= 255 else (b"S", "<H") if v <= 65535 else (b"I", "<I")
    return (b"c", "<b") if v >= -128 else (b"s", "<h") if v >= -32768 else (b"i", "<i")


def ubam_comment(header_line):
    """the comment of a header line ('@...' / '>...', with or without the line's end), or None when it has none: the line ends in
    front of its '\\n', and one '\\r' at its end is not part of it; the id ends at the first of space, \\t, \\r, \\v, \\f (ubam_name's
    rule); the comment is every byte behind that ONE byte"""
    line = bytes(header_line)
    nl = line.find(b"\n")
    if nl >= 0:
        line = line[:nl]
    if line.endswith(b"\r"):
        line = line[:-1]
    body = line[1:]
    end = min((p for p in (body.find(bytes([c])) for c in _ID_END) if p >= 0), default=-1)
    return None if end < 0 else body[end + 1:]


FLOAT_SKIPPED = -1               # float_from_text: the syntax is right, but the value has more than FLOAT_DIGITS significant digits
FLOAT_DIGITS = 17                # %.9g of a float, %.17g of a double, repr(): M < 10^17 < 2^57 bounds the device arithmetic
_FLOAT_TEXT = re.compile(rb"([+-]?)(?:(?:([0-9]+)|([0-9]*)\.([0-9]+))(?:[eE]([+-]?[0-9]{1,4}))?|([iI][nN][fF]|[nN][aA][nN]))")


def float_from_text(text):
    """the bit pattern of the float32 that the text of an f value stands for (detect.py --ubam_tag_floats; device side
    csrc/rd_float_parse.hpp, C ABI rd_float_parse): the inverse of float_g, stated in whole numbers. None: not of the syntax
        [+-]? ( D+ | D* '.' D+ ) ( [eE] [+-]? D{1,4} )?   or   [+-]? 'inf' / 'nan' in any letter case        (D = [0-9])
    - SAM's own grammar: a fraction exists only behind a point, '5.' and '1e' are no values, nor are hex floats, 'infinity', 'nan(1)'.
    inf is 0x7f800000, nan 0x7fc00000, the sign bit set for '-'. Else the integer and fraction digits, joined, without their leading
    and trailing zeros, are the integer M of s digits, and the value is EXACTLY v = M 10^q, q = the written exponent - the fraction's
    length + the trailing zeros dropped. M = 0 is +-0. s > FLOAT_DIGITS: FLOAT_SKIPPED. Else the float32 nearest to v, ties to the
    even mantissa, denormals included, in ONE rounding: v >= 2^128 - 2^103 is infinity, v <= 2^-150 zero."""
    m = _FLOAT_TEXT.fullmatch(bytes(text))
    if m is None:
        return None
    sign = 0x80000000 if m.group(1) == b"-" else 0
    if m.group(6):
        return sign | (0x7f800000 if m.group(6)[:1] in b"iI" else 0x7fc00000)
    whole, frac = (m.group(2), b"") if m.group(2) is not None else (m.group(3), m.group(4))
    digits = (whole + frac).lstrip(b"0")
    stripped = digits.rstrip(b"0")
    if not stripped:
        return sign
    if len(stripped) > FLOAT_DIGITS:
        return FLOAT_SKIPPED
    M, s = int(stripped), len(stripped)
    q = int(m.group(5) or 0) - len(frac) + len(digits) - s
    if s + q > 39:                                        # v >= 10^39 > 2^128
        return sign | 0x7f800000
    if s + q < -45:                                       # v < 10^-46 < 2^-150
        return sign
    num, den = (M * 10 ** q, 1) if q >= 0 else (M, 10 ** -q)
    e = num.bit_length() - den.bit_length()               # floor(log2 v) or one more
    if (num << -e if e < 0 else num) < (den << e if e > 0 else den):
        e -= 1
    E = max(e, -126)                                      # the exponent of the result's ulp is E - 23
    sh = E - 23
    a, b = (num << -sh, den) if sh < 0 else (num, den << sh)
    n, r = divmod(a, b)
    if 2 * r > b or (2 * r == b and n & 1):
        n += 1
    bits = ((E + 126) << 23) + n                          # n < 2^23: a denormal; n = 2^24: the rounding carried into the next exponent
    return sign | min(bits, 0x7f800000)


def _float_tag(t, v):
    """the bytes behind the name of an f value / a B:f value v (behind 'XY:T:') under floats=True: None malformed, FLOAT_SKIPPED"""
    if t == b"f":
        x = float_from_text(v)
        return x if x is None or x == FLOAT_SKIPPED else b"f" + struct.pack("<I", x)
    if len(v) > 1 and v[1] != 44:
        return None
    vals = [float_from_text(e) for e in v[2:].split(b",")] if len(v) > 1 else []
    if any(x is None for x in vals):
        return None
    if any(x == FLOAT_SKIPPED for x in vals):
        return FLOAT_SKIPPED
    return b"Bf" + struct.pack("<I%dI" % len(vals), len(vals), *vals)


def tags_from_comment(header_line, tags, floats=False):
    """(tag_bytes, copied, malformed, floats) of a header line and the listed names (2 bytes each): tag_bytes = the optional fields
    that go behind the record's qualities, in COMMENT order; copied = one bool per listed name; malformed = the record gets no tags
    (tag_bytes empty, copied all False, floats 0); floats = the f and B:f values, which are left out.
    The comment (ubam_comment) is split at \\t only. A field is a tag field when it is at least 5 bytes 'XY:T:...' with X a letter, Y a
    letter or digit, T one of A i Z H B f and ':' at bytes 2 and 4; every other field is ignored, and so is a tag field whose name is
    not listed (it is not validated). Of the tag fields with a listed name only the FIRST per name counts. Its value:
      A  one byte 0x21..0x7E -> XY A b
      i  [+-]?[0-9]{1,10} with value v in [-2^31, 2^32 - 1] -> the smallest type: C S I for v >= 0, c s i for v < 0
      Z  zero or more bytes 0x20..0x7E -> XY Z bytes NUL
      H  an even number of hex digits -> XY H bytes NUL
      B  a subtype of cCsSiI, then ',int' per element (the syntax of i, inside the subtype's range) -> XY B s count:uint32 elements
      f, B with subtype f: left out, counted - the value is not looked at
    floats=True (--ubam_tag_floats): an f value is float_from_text's float32 -> XY f bits; a B:f value is 'f', then ',value' per element
    ('XY:B:f' alone: none) -> XY B f count:uint32 bits...; such a tag counts as copied. A value - or an element - that is not of
    float_from_text's syntax, an empty element, a trailing comma, a byte behind 'f' that is no comma: malformed. A value or an element
    of more than FLOAT_DIGITS significant digits (FLOAT_SKIPPED): the tag is left out and adds 1 to floats.
    Anything else - an empty A / i / B value, a bad digit, a value out of range, an unknown subtype, an empty element or a trailing
    comma, odd or non-hex H, a byte outside 0x20..0x7E - is malformed."""
    tags, floats_on = [bytes(t) for t in tags], bool(floats)
    bad = (b"", [False] * len(tags), True, 0)
    comment = ubam_comment(header_line)
    out, copied, floats, seen = [], [False] * len(tags), 0, set()
    for f in (comment.split(b"\t") if comment is not None else ()):
        if not (len(f) >= 5 and f[0] in _ALPHA and f[1] in _ALNUM and f[2] == 58 and f[4] == 58 and f[3] in _UBAM_TAG_TYPES):
            continue
        name, t, v = f[:2], f[3:4], f[5:]
        if name not in tags or name in seen:
            continue
        seen.add(name)
        if t == b"A":
            if len(v) != 1 or not 0x21 <= v[0] <= 0x7E:
                return bad
            enc = b"A" + v
        elif t == b"i":
            x = _tag_int(v)
            if x is None or not -2 ** 31 <= x <= 2 ** 32 - 1:
                return bad
            ty, fmt = _small_int(x)
            enc = ty + struct.pack(fmt, x)
        elif t in (b"Z", b"H"):
            if any(c < 0x20 or c > 0x7E for c in v):
                return bad
            if t == b"H" and (len(v) & 1 or any(c not in _HEX for c in v)):
                return bad
            enc = t + v + b"\0"
        elif t == b"f" or v[:1] == b"f":
            enc = _float_tag(t, v) if floats_on else FLOAT_SKIPPED
            if enc is None:
                return bad
            if enc == FLOAT_SKIPPED:
                floats += 1
                continue
        else:
            if not v or v[0] not in _B_RANGE or (len(v) > 1 and v[1] != 44):
                return bad
            lo, hi = _B_RANGE[v[0]]
            vals = [_tag_int(e) for e in v[2:].split(b",")] if len(v) > 1 else []
            if any(x is None or not lo <= x <= hi for x in vals):
                return bad
            enc = b"B" + v[:1] + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), _TAG_INT[v[0]][1]), *vals)
        out.append(name + enc)
        copied[tags.index(name)] = True
    return b"".join(out), copied, False, floats


def ubam_tag_counts(text, tags, fasta=False, floats=False):
    """the counters of a run with --ubam_tags over the records of `text`: {"copied": [records in which name j was copied],
    "malformed_records": ..., "float_values_skipped": ...}"""
    copied, mal, fl = [0] * len(tags), 0, 0
    for head, _, _ in _text_records(text, fasta):
        _, c, m, f = tags_from_comment(head, tags, floats)
        mal += bool(m)
        fl += f
        for j, x in enumerate(c):
            copied[j] += bool(x)
    return {"copied": copied, "malformed_records": mal, "float_values_skipped": fl}


def from_fastq(text, n_mates=1, mate=0, fasta=False, tags=None, floats=False):
    """the BAM records (their bytes, joined; no header) of FASTQ - or, fasta=True, FASTA - text: what --ubam_output makes of a file's
    records. n_mates: 1 single-end, 2 a paired run; mate: 0 / 1 - which mate's file the text is -, or INTERLEAVED: the records
    alternate mate 1, mate 2. Per record: name = ubam_name; flag = UBAM_FLAGS; a base = the letter of CODES it is in either case, U as
    T, every other byte N (UBAM_LETTER); a quality = min(max(b, 33), 126) - 33 (UBAM_QUAL), FASTA: absent (0xFF throughout).
    tags (--ubam_tags: names of 2 bytes): the record ends in tags_from_comment(header line, tags, floats)'s bytes (floats:
    --ubam_tag_floats).
    ValueError: a name of more than 254 bytes (UBAM_NAME_ERROR), a quality line that is not as long as its sequence
    (UBAM_LENGTH_ERROR) - N counts the text's records from 0."""
    out = []
    for k, (head, seq, qual) in enumerate(_text_records(text, fasta)):
        m = (k & 1) if mate == INTERLEAVED else int(mate)
        name = ubam_name(head, n_mates, m)
        if len(name) > UBAM_NAME_MAX:
            raise ValueError(UBAM_NAME_ERROR % k)
        if qual is not None and len(qual) != len(seq):
            raise ValueError(UBAM_LENGTH_ERROR % k)
        extra = tags_from_comment(head, tags, floats)[0] if tags else b""
        out.append(_ubam_record(name, seq, qual, UBAM_FLAGS[(int(n_mates), m)], extra))
    return b"".join(out)


def ubam_counts(text, n_mates=1, mate=0, fasta=False):
    """the counters of a run with --ubam_output over the records of `text` (from_fastq's arguments): bases_changed = the bytes whose BAM
    letter differs from the input byte, quals_clamped = the quality bytes outside '!'..'~', names_starred = the ids replaced by '*'"""
    changed = clamped = starred = 0
    for k, (head, seq, qual) in enumerate(_text_records(text, fasta)):
        m = (k & 1) if mate == INTERLEAVED else int(mate)
        changed += len(seq.translate(None, _SAME_LETTER))
        clamped += len((qual or b"").translate(None, _IN_RANGE))
        starred += not _ubam_id(head, n_mates, m)
    return {"bases_changed": changed, "quals_clamped": clamped, "names_starred": starred}


def ubam_bound(text_bytes, n, fasta=False):
    """bytes that always hold from_fastq's records of n records in text_bytes bytes of text (csrc/rd_bam_encode.hpp derives them):
    FASTQ text + 32 n; FASTA text + (text + 1) / 2 + 40 n"""
    text_bytes, n = int(text_bytes), int(n)
    return text_bytes + (text_bytes + 1) // 2 + 40 * n if fasta else text_bytes + 32 * n


# ---- optional fields (tags) and read groups: the rule the device side (csrc/rd_bam_tags.hpp) is compared against ----------------------

TAG_NONE, TAG_MALFORMED = -1, -2
_TAG_FIXED = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
_TAG_B_SIZE = {ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


def find_tag(data, rec_off, tag):
    """(val_off, val_len, val_type) of the first optional field `tag` (2 bytes) of the record at data[rec_off:] (its block_size field):
    val_off = where the value starts in `data`, val_len = its bytes (Z / H: without the NUL; B: with subtype and count), val_type = the
    type byte. (-1, 0, 0): the record has no such tag; (-2, 0, 0): its tags are malformed in front of or at the tag (module docstring) -
    a malformed tag BEHIND the first occurrence is not seen. No byte at or behind the record's end p + 4 + block_size is looked at."""
    data, tag, r = bytes(data), bytes(tag), int(rec_off)
    bad = (TAG_MALFORMED, 0, 0)
    if len(tag) != 2:
        raise ValueError("find_tag: a tag has 2 bytes")
    if r < 0 or r + 36 > len(data):
        return bad
    block = struct.unpack_from("<i", data, r)[0]
    E = r + 4 + block
    if block < 32 or E > len(data):
        return bad
    l_name, n_cigar, l_seq = data[r + 12], struct.unpack_from("<H", data, r + 16)[0], struct.unpack_from("<i", data, r + 20)[0]
    if l_seq < 0:
        return bad
    p = r + 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    if p > E:
        return bad
    while p < E:
        if E - p < 3:
            return bad
        name, t, v = data[p:p + 2], data[p + 2], p + 3
        if t in _TAG_FIXED:
            n = _TAG_FIXED[t]
            if v + n > E:
                return bad
            nxt = v + n
        elif t in (ord("Z"), ord("H")):
            q = data.find(b"\0", v, E)
            if q < 0:
                return bad
            n, nxt = q - v, q + 1
        elif t == ord("B"):
            if v + 5 > E or data[v] not in _TAG_B_SIZE:
                return bad
            n = 5 + struct.unpack_from("<I", data, v + 1)[0] * _TAG_B_SIZE[data[v]]
            if v + n > E:
                return bad
            nxt = v + n
        else:
            return bad
        if name == tag:
            return (v, n, t)
        p = nxt
    return (TAG_NONE, 0, 0)


# ---- tags as the comment of a FASTQ header line (detect.py --bam_tags; device side csrc/rd_bam_tagtext.hpp) ---------------------------------

TAGS_MAX = N.BAM_TAGS_MAX        # RD_BAM_TAGS_MAX: the most names a tag list holds
_TAG_INT = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}
_HEX = frozenset(b"0123456789ABCDEFabcdef")


def parse_tag_list(text):
    """the names of a tag list 'MM,ML,RG' as 2-byte strings, in list order. ValueError: an empty list, a name that is not
    [A-Za-z][A-Za-z0-9], a name that appears twice, more than TAGS_MAX names."""
    names = [t for t in str(text).split(",")] if str(text) else []
    if not names:
        raise ValueError("the tag list is empty")
    out = []
    for t in names:
        ok = len(t) == 2 and t.isascii() and t[0].isalpha() and t[1].isalnum()
        if not ok:
            raise ValueError("'%s' is not a tag name ([A-Za-z][A-Za-z0-9])" % t)
        if t.encode() in out:
            raise ValueError("the tag %s appears twice" % t)
        out.append(t.encode())
    if len(out) > TAGS_MAX:
        raise ValueError("the list holds %d tags, more than %d" % (len(out), TAGS_MAX))
    return out


_P10 = [10 ** i for i in range(52)]      # (5 - X <= 50 for the smallest denormal, X - 5 <= 33 for the largest float)


def float_g(bits):
    """the text of the float32 with bit pattern `bits` (detect.py --bam_tag_floats; device side csrc/rd_float_text.hpp, C ABI
    rd_float_text): what a C library's printf("%g", (double)v) prints, stated in whole numbers.
    '-' in front when the sign bit is set (-0, -inf and -nan included). Infinity is 'inf', a NaN 'nan', zero '0'. Every other value,
    denormals included, is the EXACT number m 2^e, rounded to 6 significant decimal digits, ties to the even digit (a tie needs an
    exact half at the 7th digit: 100000.5, 1234565). X is the decimal exponent AFTER the rounding (999999.5 -> 1.00000 10^6: X = 6).
    X < -4 or X >= 6: d.ddddde+XX / e-XX, the trailing zeros of the fraction removed and the point with them when none is left, the
    exponent with at least two digits. Else fixed notation with 5 - X decimals, trailing zeros and then the point removed.
    At most 12 bytes ('-1.17549e-38')."""
    bits = int(bits) & 0xffffffff
    sign = b"-" if bits >> 31 else b""
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    if ef == 0xff:
        return sign + (b"nan" if mf else b"inf")
    if ef == 0 and mf == 0:
        return sign + b"0"
    m, e = (mf | 0x800000, ef - 150) if ef else (mf, -149)
    num, den = (m << e, 1) if e >= 0 else (m, 1 << -e)            # the value = num / den
    if num >= den:                                        # X = floor(log10 v)
        X = len(str(num // den)) - 1
    else:
        X = -1
        while num * _P10[-X] < den:
            X -= 1
    a, b = (num * _P10[5 - X], den) if X <= 5 else (num, den * _P10[X - 5])          # v 10^(5 - X) = a / b, in [10^5, 10^6)
    n, r = divmod(a, b)
    if 2 * r > b or (2 * r == b and n & 1):               # above the half, or the half itself and an odd last digit
        n += 1
    if n == 1000000:                                      # 999999.5 and above: the rounding carried into the next decade
        n, X = 100000, X + 1
    digits = str(n)
    if X < -4 or X >= 6:
        frac = digits[1:].rstrip("0")
        text = digits[0] + ("." + frac if frac else "") + "e%s%02d" % ("-" if X < 0 else "+", abs(X))
    elif X >= 0:
        frac = digits[X + 1:].rstrip("0")
        text = digits[:X + 1] + ("." + frac if frac else "")
    else:
        text = "0." + "0" * (-X - 1) + digits.rstrip("0")
    return sign + text.encode()


def tag_comment(data, rec_off, tags, floats=False):
    """(comment, copied, malformed, floats) of the record at data[rec_off:] and the listed tags (2-byte names, list order): comment =
    the bytes that go behind the read name ('\\tTG:T:text' per tag that is present and not float-typed; b"" when there is none),
    copied = one bool per listed tag (found and formatted), malformed = the record gets no comment because a listed tag gives
    TAG_MALFORMED, an A / Z / H value of a listed tag holds a byte outside 0x20..0x7E, or an H value has odd length or a non-hex
    character (copied is all False and floats 0 then), floats = the listed tags of type f or B:f, which are left out.
    A c C s S i I: TG:A:c / TG:i:decimal; Z H: the bytes verbatim; B: TG:B:s and ',v' per element.
    floats=True (--bam_tag_floats): an f value is TG:f:float_g, a B:f array TG:B:f and ',float_g' per element ('TG:B:f' alone when it
    has none); such a tag counts as copied, and the floats returned are 0."""
    data, floats_on = bytes(data), bool(floats)
    parts, copied, floats = [], [], 0
    bad = (b"", [False] * len(tags), True, 0)
    for tag in tags:
        tag = bytes(tag)
        off, n, t = find_tag(data, rec_off, tag)
        if off == TAG_MALFORMED:
            return bad
        if off == TAG_NONE:
            copied.append(False)
            continue
        v = data[off:off + n]
        if t == ord("f") or (t == ord("B") and v[0] == ord("f")):
            if not floats_on:
                floats += 1
                copied.append(False)
                continue
            if t == ord("f"):
                if n != 4:
                    return bad
                text = b"f:" + float_g(struct.unpack("<I", v)[0])
            else:
                count = struct.unpack_from("<I", v, 1)[0]
                text = b"B:f" + b"".join(b"," + float_g(x) for x in struct.unpack_from("<%dI" % count, v, 5))
        elif t in (ord("A"), ord("Z"), ord("H")):
            if any(c < 0x20 or c > 0x7E for c in v):
                return bad
            if t == ord("H") and (n & 1 or any(c not in _HEX for c in v)):
                return bad
            text = bytes([t]) + b":" + v
        elif t in _TAG_INT:
            text = b"i:" + str(struct.unpack(_TAG_INT[t], v)[0]).encode()
        else:                                             # B: subtype, count, elements
            fmt, count = _TAG_INT[v[0]], struct.unpack_from("<I", v, 1)[0]
            vals = struct.unpack_from("<%d%s" % (count, fmt[1]), v, 5)
            text = b"B:" + v[:1] + b"".join(b",%d" % x for x in vals)
        parts.append(b"\t" + tag + b":" + text)
        copied.append(True)
    return b"".join(parts), copied, False, floats


def fastq_text_tagged(data, tags, start=None, floats=False):
    """fastq_text with every record's tag_comment inserted in front of its first newline (behind the read name). Skipped records stay
    skipped; a record on the reverse strand gets the same comment as it would on the forward strand (tags are not reversed)."""
    data = bytes(data)
    out = []
    for r in records(data, start):
        if r.skipped:
            continue
        text = r.fastq()
        at = text.index(b"\n")
        out.append(text[:at] + tag_comment(data, r.offset, tags, floats)[0] + text[at:])
    return b"".join(out)


def tag_counts(data, tags, start=None, floats=False):
    """the counters of a run with --bam_tags over the delivered records of `data`: {"copied": [records in which tag j was copied],
    "malformed_records": ..., "float_values_skipped": ...}"""
    data = bytes(data)
    copied, mal, fl = [0] * len(tags), 0, 0
    for r in records(data, start):
        if r.skipped:
            continue
        _, c, m, f = tag_comment(data, r.offset, tags, floats)
        mal += bool(m)
        fl += f
        for j, x in enumerate(c):
            copied[j] += bool(x)
    return {"copied": copied, "malformed_records": mal, "float_values_skipped": fl}


def read_groups(header_bytes):
    """[(id bytes, {field: value})] of the '@RG' lines of a header (the bytes header() returns), in header order; field = the two
    letters in front of the colon (str), value = the rest (str, latin-1). ValueError: an @RG line without ID, with an empty ID, or an
    ID that an earlier line declared - the message names the line or the ID."""
    data = bytes(header_bytes)
    if data[:4] != MAGIC or len(data) < 8:
        raise ValueError("read_groups: not a BAM header")
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0 or 8 + l_text > len(data):
        raise ValueError("read_groups: the header text does not lie inside the header")
    out, seen = [], set()
    for k, line in enumerate(data[8:8 + l_text].split(b"\0")[0].split(b"\n")):
        line = line.rstrip(b"\r")
        if line[:3] != b"@RG" or (len(line) > 3 and line[3:4] != b"\t"):
            continue
        fields, rid = {}, None
        for f in line.split(b"\t")[1:]:
            if len(f) >= 3 and f[2:3] == b":":
                if f[:2] == b"ID" and rid is None:
                    rid = f[3:]
                fields.setdefault(f[:2].decode("latin-1"), f[3:].decode("latin-1"))
        if rid is None:
            raise ValueError("@RG line without ID (header line %d): %s" % (k + 1, line.decode("latin-1")))
        if not rid:
            raise ValueError("@RG line with an empty ID (header line %d)" % (k + 1))
        if rid in seen:
            raise ValueError("duplicate @RG ID '%s' (header line %d)" % (rid.decode("latin-1"), k + 1))
        seen.add(rid)
        out.append((rid, fields))
    return out


def sorted_ids(ids):
    """(the ids sorted bytewise as unsigned bytes - a prefix in front of what it is a prefix of -, order): sorted[j] = ids[order[j]].
    The device's dictionary (rd_bam_group_rows) is the sorted list; order maps its rows back to header order."""
    order = sorted(range(len(ids)), key=lambda j: bytes(ids[j]))
    return [bytes(ids[j]) for j in order], order


def group_row(data, val_off, val_len, val_type, ids):
    """the row a record is counted in, from find_tag(data, rec_off, b"RG") and the G = len(ids) declared ids: j for a Z value equal to
    ids[j]; G: no RG tag; G + 1: a Z value that no @RG line declares; G + 2: malformed tags, or an RG that is not of type Z."""
    G = len(ids)
    if val_off == TAG_NONE:
        return G
    if val_off < 0 or val_type != ord("Z"):
        return G + 2
    value = bytes(data[val_off:val_off + val_len])
    for j, rid in enumerate(ids):
        if bytes(rid) == value:
            return j
    return G + 1


# ---- outputs per read group (detect.py --split_groups): the names of a family's files --------------------------------------------------
SPLIT_GROUPS_MAX = N.SPLIT_GROUPS_MAX      # RD_SPLIT_GROUPS_MAX: the most declared groups a run splits its outputs by
UNASSIGNED = None                          # the row id of a family's last member: no RG tag, an undeclared value, malformed tags
_ESC_KEEP = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789._+=@,-")


def esc(rid):
    """a read-group id as part of a file name: the bytes A-Z a-z 0-9 . _ + = @ , - stay, every other byte - '%' included - becomes
    %XX in upper-case hex. Injective; the result holds no '/'."""
    return "".join(chr(b) if b in _ESC_KEEP else "%%%02X" % b for b in bytes(rid))


def split_name(path, row_id):
    """the name of the member of `path`'s family for the declared id `row_id` (bytes), or for the unassigned records (UNASSIGNED): the
    marker '.rg-<esc(id)>' / '.unassigned' goes in front of the first '.' of the basename that is not its first byte, or behind the
    name when there is no such dot: non.fq.gz -> non.rg-lib7.fq.gz, non.unassigned.fq.gz. The 'rg-' keeps declared ids apart from
    'unassigned'."""
    head, base = os.path.split(path)
    marker = ".unassigned" if row_id is UNASSIGNED else ".rg-" + esc(row_id)
    dot = base.find(".", 1)
    base = base + marker if dot < 0 else base[:dot] + marker + base[dot:]
    return os.path.join(head, base)


def split_paths(path, ids):
    """the G + 1 names of `path`'s family: a member per declared id, in the order of `ids`, and the unassigned member last"""
    return [split_name(path, rid) for rid in ids] + [split_name(path, UNASSIGNED)]
