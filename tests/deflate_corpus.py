"""DEFLATE streams for the gunzip decoders' tests (tests/test_inflate_corpus.py, tests/test_gpu_inflate_corpus.py): texts shaped like
what this product reads, compressed by zlib (every level and strategy), by libdeflate and pigz-style, and raw DEFLATE written by hand -
legal streams that zlib never writes (runs of code lengths across the two codes, one or no distance code, 15-bit codewords, EOB-only
blocks, ...) and streams zlib's inflate rejects. zlib's inflate is the judge of every stream here: self_check() proves that each valid
stream decodes to its text and each invalid one raises zlib.error, so a corpus mistake can never pass for a decoder bug.

Everything is a deterministic function of fixed seeds; results are cached per process."""
import bisect
import ctypes as C
import functools
import heapq
import struct
import zlib

import numpy as np

# ---- texts --------------------------------------------------------------------------------------------------------------------------


def fastq_bytes(n, seed=3):
    """FASTQ with random qualities (tests/test_inflate.py's payload)"""
    from ribodetector_amd import synth
    arena, off, _ = synth.reads_numpy(n, (60, 150), seed=seed)
    b = arena.tobytes()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = b[off[i]:off[i + 1]]
        q = bytes(rng.integers(35, 74, len(s), dtype=np.uint8))
        out.append(b"@read.%d/1 lane=3\n%s\n+\n%s\n" % (i, s, q))
    return b"".join(out)


def fastq_illumina(n, seed=5, eol=b"\n"):
    """Illumina headers, NovaSeq-like binned qualities (F : , #)"""
    from ribodetector_amd import synth
    arena, off, _ = synth.reads_numpy(n, (100, 151), seed=seed)
    b = arena.tobytes()
    rng = np.random.default_rng(seed)
    qual = np.frombuffer(b"F:,#", dtype=np.uint8)[rng.choice(4, size=len(b), p=[0.90, 0.06, 0.03, 0.01])].tobytes()
    out = []
    for i in range(n):
        a, z = int(off[i]), int(off[i + 1])
        out.append(b"@A00123:45:HKJ3TDSXY:2:%d:%d:%d 1:N:0:ACGTACGT+TTGACCAA%s%s%s+%s%s%s" % (
            1101 + i // 5000, 1000 + (i * 7919) % 30000, 1000 + i // 3, eol, b[a:z], eol, eol, qual[a:z], eol))
    return b"".join(out)


def fasta_bytes(n_rec, width, seed=7):
    """multi-record FASTA wrapped at `width` columns, with lowercase soft-masked runs"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n_rec):
        L = int(rng.integers(2000, 12000))
        s = acgt[rng.integers(0, 4, L)].copy()
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(0, L))
            s[a:a + int(rng.integers(20, 600))] += 32          # soft mask: a..z
        s = s.tobytes()
        out.append(b">chr%d_%d len=%d\n" % (seed, i, L) + b"".join(s[k:k + width] + b"\n" for k in range(0, L, width)))
    return b"".join(out)


def contig_bytes(mib=3, seed=9):
    """one FASTA contig of ACGT only, on one line"""
    rng = np.random.default_rng(seed)
    return b">contig_1\n" + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, mib << 20)].tobytes() + b"\n"


def lowcomplex_fastq(n, seed=11):
    """FASTQ with poly-A, short-period and ordinary reads mixed (compresses ~3:1: the runs are far below the 250:1 the stream decoder refuses)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(80, 151))
        k = i % 5
        if k == 0:
            s = b"A" * L
        elif k == 1:
            per = acgt[rng.integers(0, 4, int(rng.integers(2, 7)))].tobytes()
            s = (per * (L // len(per) + 1))[:L]
        else:
            s = acgt[rng.integers(0, 4, L)].tobytes()
        q = b"F" * L if k < 2 else bytes(rng.integers(35, 74, L, dtype=np.uint8))
        out.append(b"@lc.%d\n%s\n+\n%s\n" % (i, s, q))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def text(name):
    """the corpus texts, 2-3 MB each"""
    return {"fastq": lambda: fastq_bytes(8000),
            "illumina": lambda: fastq_illumina(7000),
            "illumina_crlf": lambda: fastq_illumina(7000, eol=b"\r\n"),
            "fasta60": lambda: fasta_bytes(300, 60),
            "fasta80": lambda: fasta_bytes(300, 80, seed=8),
            "contig": lambda: contig_bytes(3),
            "lowcomplex": lambda: lowcomplex_fastq(12000)}[name]()


TEXTS = ("fastq", "illumina", "illumina_crlf", "fasta60", "fasta80", "contig", "lowcomplex")
FASTQ = ("fastq", "illumina", "illumina_crlf")
FASTQ_FASTA = FASTQ + ("fasta60", "fasta80")      # what the reader is for

# ---- encoders: raw DEFLATE ------------------------------------------------------------------------------------------------------------

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


def zlib_raw(data, level=6, strategy="default"):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, STRATEGIES[strategy])
    return co.compress(data) + co.flush()


_LD = []


def libdeflate():
    """the ctypes handle of libdeflate.so.0, or None when the machine has no libdeflate"""
    if not _LD:
        try:
            ld = C.CDLL("libdeflate.so.0")
            ld.libdeflate_alloc_compressor.restype = C.c_void_p
            ld.libdeflate_alloc_compressor.argtypes = [C.c_int]
            ld.libdeflate_deflate_compress_bound.restype = C.c_size_t
            ld.libdeflate_deflate_compress_bound.argtypes = [C.c_void_p, C.c_size_t]
            ld.libdeflate_deflate_compress.restype = C.c_size_t
            ld.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
            ld.libdeflate_free_compressor.argtypes = [C.c_void_p]
        except OSError:
            ld = None
        _LD.append(ld)
    return _LD[0]


LIBDEFLATE_MISSING = "libdeflate.so.0 cannot be loaded on this machine"


def libdeflate_raw(data, level=6):
    ld = libdeflate()
    if ld is None:
        raise RuntimeError(LIBDEFLATE_MISSING)
    c = ld.libdeflate_alloc_compressor(level)
    assert c, level
    try:
        cap = ld.libdeflate_deflate_compress_bound(c, len(data))
        buf = C.create_string_buffer(cap)
        n = ld.libdeflate_deflate_compress(c, data, len(data), buf, cap)
        assert n > 0
        return buf.raw[:n]
    finally:
        ld.libdeflate_free_compressor(c)


def pigz_raw(data, level=6, piece=128 << 10):
    """pigz's layout: pieces compressed independently, each primed with the 32 KiB before it and closed with a sync flush (an empty
    stored block), the last one with the final block - one DEFLATE stream"""
    out = []
    for a in range(0, max(len(data), 1), piece):
        prime = data[max(0, a - 32768):a]
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, prime) if prime else zlib.compressobj(level, zlib.DEFLATED, -15)
        last = a + piece >= len(data)
        out.append(co.compress(data[a:a + piece]) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH))
    return b"".join(out)


def encoders():
    """(name, function(data) -> raw DEFLATE, needs libdeflate) of every encoder of the corpus"""
    out = [("zlib%d" % lv, functools.partial(zlib_raw, level=lv), False) for lv in range(1, 10)]
    out += [("zlib6_%s" % s, functools.partial(zlib_raw, level=6, strategy=s), False) for s in ("filtered", "huffman", "rle", "fixed")]
    out += [("zlib1_fixed", functools.partial(zlib_raw, level=1, strategy="fixed"), False), ("zlib9_fixed", functools.partial(zlib_raw, level=9, strategy="fixed"), False)]
    out += [("ld%d" % lv, functools.partial(libdeflate_raw, level=lv), True) for lv in range(0, 13)]
    out += [("pigz6", pigz_raw, False), ("pigz9_64k", functools.partial(pigz_raw, level=9, piece=64 << 10), False)]
    return out


ENCODERS = {n: (f, ld) for n, f, ld in encoders()}


@functools.lru_cache(maxsize=None)
def compressed(text_name, enc):
    """raw DEFLATE of text(text_name) by encoder `enc` (cached)"""
    return ENCODERS[enc][0](text(text_name))


# ---- framing -------------------------------------------------------------------------------------------------------------------------


def gzip_member(raw, data, flags=0):
    """raw DEFLATE -> one gzip member; `data` gives the trailer's CRC-32 and ISIZE"""
    hdr = b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\xff"
    if flags & 8:
        hdr += b"reads.fq\0"
    return hdr + raw + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)


def sized_member(raw, data):
    """a member that carries its size: BGZF's 'BC' subfield when it fits 64 KiB, this build's 'RD' subfield (32-bit size) otherwise"""
    tail = struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)
    if 18 + len(raw) + 8 <= 65536:
        return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HccHH", 6, b"B", b"C", 2, 18 + len(raw) + 8 - 1) + raw + tail
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HccHI", 8, b"R", b"D", 4, 20 + len(raw) + 8 - 1) + raw + tail


def bgzf(data, compress, block=65280):
    """BGZF members of `block` text bytes each, compressed by `compress` (raw DEFLATE), closed by the empty EOF member"""
    pieces = [data[i:i + block] for i in range(0, len(data), block)] + [b""]
    return b"".join(sized_member(zlib_raw(p) if not p else compress(p), p) for p in pieces)


# ---- a raw DEFLATE writer (RFC 1951) ---------------------------------------------------------------------------------------------------

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_sym(n):
    return 257 + bisect.bisect_right(LBASE, n) - 1


def dist_sym(d):
    return bisect.bisect_right(DBASE, d) - 1


class BitWriter:
    """bits LSB first (RFC 1951 3.1.1); Huffman codewords MSB first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.put(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """RFC 1951 3.2.2: codes from code lengths"""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else None)
        if l:
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^-len over the non-zero lengths, in units of 2^-15 (32768 = a complete code)"""
    return sum(1 << (15 - l) for l in lens if l)


def huffman_lengths(freq, limit=15):
    """Huffman code lengths of the symbols with freq > 0 (one symbol alone gets length 1), at most `limit` bits"""
    f = list(freq)
    while True:
        used = [s for s, x in enumerate(f) if x]
        lens = [0] * len(f)
        if len(used) == 1:
            lens[used[0]] = 1
            return lens
        h = [(f[s], s, (s,)) for s in used]
        heapq.heapify(h)
        k = len(f)
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2]))
            k += 1
        if max(lens) <= limit:
            return lens
        f = [(x + 1) // 2 if x else 0 for x in f]


def deepen(lens, sym, fillers):
    """give `sym` a 15-bit codeword: its slot of length l becomes codewords of lengths l+1 .. 15, 15 - one for sym, the others for
    unused symbols taken from `fillers` (the code stays complete)"""
    lens = list(lens)
    l = lens[sym]
    fill = [s for s in fillers if not lens[s]][: 15 - l]
    assert len(fill) == 15 - l, "not enough free symbols"
    for k, s in enumerate(fill):
        lens[s] = l + 1 + k
    lens[sym] = 15
    return lens


def rle(lens):
    """code-length symbols of `lens` (the two codes' lengths in ONE sequence, as RFC 1951 allows: runs may cross from the
    literal/length lengths into the distance lengths): [(symbol, extra bits value)]"""
    ops, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r - 11))
                run -= r
            while run >= 3:
                r = min(run, 10)
                ops.append((17, r - 3))
                run -= r
            ops += [(0, 0)] * run
        else:
            ops.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r - 3))
                run -= r
            ops += [(v, 0)] * run
        i = j
    return ops


def op_runs(ops):
    """(start index, count, symbol, value) of every code-length symbol of `ops`"""
    out, i, prev = [], 0, None
    for s, x in ops:
        cnt, val = (1, s) if s < 16 else ((3 + x, prev) if s == 16 else ((3 + x, 0) if s == 17 else (11 + x, 0)))
        out.append((i, cnt, s, val))
        i += cnt
        prev = val
    return out


def crossing(ops, hlit):
    """the runs (16/17/18) that cross from the literal/length lengths into the distance lengths: [(symbol, value)]"""
    return [(s, v) for i, c, s, v in op_runs(ops) if s >= 16 and i < hlit < i + c]


def lz77(data, start=0, min_dist=1, max_dist=32768, max_len=258, allow=None, chain=24):
    """greedy LZ77 of data[start:] (data[:start] is history): tokens = byte values and (length, distance) pairs"""
    head, prev, toks = {}, {}, []
    for k in range(max(0, start - max_dist), start):
        key = data[k:k + 3]
        if len(key) == 3:
            prev[k] = head.get(key)
            head[key] = k
    i, n = start, len(data)
    while i < n:
        best, bd = 0, 0
        key = data[i:i + 3]
        if len(key) == 3:
            c, steps = head.get(key), 0
            while c is not None and steps < chain and i - c <= max_dist:
                d = i - c
                if d >= min_dist and (allow is None or allow(d)):
                    m = 3
                    lim = min(max_len, n - i)
                    while m < lim and data[c + m] == data[i + m]:
                        m += 1
                    if m > best:
                        best, bd = m, d
                        if m == lim:
                            break
                c, steps = prev.get(c), steps + 1
        step = best if best >= 3 else 1
        toks.append((best, bd) if best >= 3 else data[i])
        for k in range(i, i + step):
            key = data[k:k + 3]
            if len(key) == 3:
                prev[k] = head.get(key)
                head[key] = k
        i += step
    return toks


def token_syms(tok):
    """(literal/length symbol, length extra (value, bits), distance symbol, distance extra (value, bits)) of a token; a match may
    name its symbols itself: (length, distance, lsym, dsym)"""
    if isinstance(tok, int):
        return tok, None, None, None
    ln, d = tok[0], tok[1]
    ls = tok[2] if len(tok) > 2 and tok[2] is not None else len_sym(ln)
    ds = tok[3] if len(tok) > 3 and tok[3] is not None else dist_sym(d)
    lx = (ln - LBASE[ls - 257], LEXT[ls - 257]) if ls < 286 else (0, 0)
    dx = (d - DBASE[ds], DEXT[ds]) if ds < 30 else (0, 0)
    return ls, lx, ds, dx


def freqs(tokens):
    fl, fd = [0] * 286, [0] * 30
    for t in tokens:
        ls, _, ds, _ = token_syms(t)
        fl[ls] += 1
        if ds is not None:
            fd[ds] += 1
    fl[256] += 1
    return fl, fd


def write_symbols(bw, tokens, lcodes, llens, dcodes, dlens, eob=True):
    for t in tokens:
        ls, lx, ds, dx = token_syms(t)
        assert llens[ls] and (lx is None or dlens[ds]), "a symbol without a codeword"
        bw.code(lcodes[ls], llens[ls])
        if lx is None:
            continue
        bw.put(lx[0], lx[1])
        bw.code(dcodes[ds], dlens[ds])
        bw.put(dx[0], dx[1])
    if eob:
        bw.code(lcodes[256], llens[256])


def dynamic_block(bw, tokens, final=False, lit=None, dist=None, hlit=None, hdist=None, ops=None, pre=None, hclen=None, eob=True):
    """a dynamic-Huffman block. Left out, the codes follow from the tokens (Huffman); hlit / hdist / hclen are the header's counts (not
    checked: an invalid header is written as given); ops = the code-length symbols (default: rle of the lengths)"""
    fl, fd = freqs(tokens)
    lit = list(lit) if lit is not None else huffman_lengths(fl)
    dist = list(dist) if dist is not None else (huffman_lengths(fd) if any(fd) else [0])
    if hlit is None:
        hlit = max(257, max(s for s, l in enumerate(lit) if l) + 1)
    if hdist is None:
        hdist = max([1] + [s + 1 for s, l in enumerate(dist) if l])
    lit, dist = (lit + [0] * 320)[:hlit], (dist + [0] * 40)[:hdist]
    if ops is None:
        ops = rle(lit + dist)
    if pre is None:
        pf = [0] * 19
        for s, _ in ops:
            pf[s] += 1
        pre = huffman_lengths(pf, 7)
    if hclen is None:
        hclen = max(4, max(k + 1 for k, s in enumerate(CLORD) if pre[s]))
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(pre[CLORD[k]], 3)
    pc = canonical(pre)
    for s, x in ops:
        bw.code(pc[s], pre[s])
        if s >= 16:
            bw.put(x, {16: 2, 17: 3, 18: 7}[s])
    write_symbols(bw, tokens, canonical(lit + [0] * (288 - len(lit))), lit + [0] * (288 - len(lit)), canonical(dist + [0] * (32 - len(dist))),
                  dist + [0] * (32 - len(dist)), eob)
    return ops


def fixed_block(bw, tokens, final=False):
    bw.put(1 if final else 0, 1)
    bw.put(1, 2)
    write_symbols(bw, tokens, canonical(FIXED_LIT), FIXED_LIT, canonical(FIXED_DIST), FIXED_DIST)


def stored_block(bw, data, final=False, nlen=None):
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    bw.out += data


def detok(tokens, hist=b""):
    """the text `tokens` stand for behind `hist`"""
    out = bytearray(hist)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t[0], t[1]
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out[len(hist):])


# ---- the hand-built streams ----------------------------------------------------------------------------------------------------------
# Each builder writes blocks into a BitWriter behind `hist` (the text already in the window: matches may reach into it) and returns
# the text of its blocks. None of them ends the stream: finish() appends an empty final block (or the caller splices them).

def _fq(k, n=40000):
    """a piece of FASTQ text for the hand-built blocks (distinct pieces for distinct k)"""
    t = text("illumina")
    a = (k * 104729) % (len(t) - n)
    return t[a:a + n]


def v1_cross_zero_runs(bw, hist):
    """V1a: 18 and 17 runs of zero lengths from the literal/length lengths into the distance lengths (HLIT padded with unused
    length symbols, the short distance codes unused)"""
    out = b""
    for k, (max_len, min_dist, pad) in enumerate(((34, 9, 11), (66, 5, 2))):   # (11+ zeros: 18 crossing; 2 + 4 zeros: 17 crossing)
        data = _fq(10 + k, 20000)
        toks = lz77(hist + out + data, start=len(hist + out), min_dist=min_dist, max_len=max_len)
        fl, fd = freqs(toks)
        lit, dist = huffman_lengths(fl), huffman_lengths(fd)
        top = max(s for s, l in enumerate(lit) if l)
        hlit = min(286, top + 1 + pad)
        ops = dynamic_block(bw, toks, lit=lit, dist=dist, hlit=hlit, hdist=30)
        cr = crossing(ops, hlit)
        assert cr and cr[0][0] == (18 if k == 0 else 17) and cr[0][1] == 0, (k, cr, top, [l for l in dist[:8]])
        out += data
    return out


V1_DIST = [9, 9, 9, 9] + [0] * 19 + [7, 6, 5, 4, 3, 2, 1]      # complete: 4/512 + 1/128 + ... + 1/2; distances 1-4 and 3073-32768


def v1_cross_repeat(bw, hist):
    """V1b: a 16 run of a NON-zero length (9) that crosses from the literal/length lengths into the distance lengths: every
    literal/length symbol 226-285 and distance symbols 0-3 have 9-bit codewords (both codes complete)"""
    lit = [8] * 226 + [9] * 60
    assert kraft(lit) == 32768 and kraft(V1_DIST) == 32768
    data = _fq(20, 30000)
    toks = lz77(hist + data, start=len(hist), allow=lambda d: d <= 4 or d > 3072)
    ops = dynamic_block(bw, toks, lit=lit, dist=V1_DIST, hlit=286, hdist=30)
    assert any(s == 16 and v == 9 for s, v in crossing(ops, 286)), crossing(ops, 286)
    return data


def v2_one_distance_code(bw, hist):
    """V2: exactly one distance code, of length 1 (incomplete, legal), used by every match"""
    data = _fq(30, 30000)
    _, fd = freqs(lz77(hist + data, start=len(hist)))
    ds = int(np.argmax(fd))
    toks = lz77(hist + data, start=len(hist), allow=lambda d: dist_sym(d) == ds)
    assert any(not isinstance(t, int) for t in toks)
    dist = [0] * 30
    dist[ds] = 1
    dynamic_block(bw, toks, dist=dist)
    return data


def v3_no_distance_code(bw, hist):
    """V3: literals only, HDIST = 1 with a zero length (no distance code at all)"""
    data = _fq(40, 12000)
    dynamic_block(bw, list(data), dist=[0], hdist=1)
    return data


def v4_minimal_header(bw, hist):
    """V4: HLIT 257, HDIST 1 (literals and the end-of-block code; one distance code of length 1 that nothing uses)"""
    data = _fq(50, 12000)
    ops = dynamic_block(bw, list(data), dist=[1], hlit=257, hdist=1)
    assert ops
    return data


def v5_15bit_codes(bw, hist):
    """V5: 15-bit literal/length and distance codewords in use (a frequent literal and a frequent distance symbol deepened to 15 bits)"""
    data = _fq(60, 30000)
    toks = lz77(hist + data, start=len(hist), allow=lambda d: d > 2048)
    fl, fd = freqs(toks)
    lit, dist = huffman_lengths(fl), huffman_lengths(fd)
    ls = max(range(256), key=lambda s: fl[s])
    lit = deepen(lit, ls, [s for s in range(256) if not fl[s]])
    ds = max(range(30), key=lambda s: fd[s])
    dist = deepen(dist, ds, range(30))
    assert kraft(lit) == 32768 and kraft(dist) == 32768 and fl[ls] and fd[ds]
    dynamic_block(bw, toks, lit=lit, dist=dist)
    return data


def v6_extreme_matches(bw, hist):
    """V6: a distance of 32,768 back to the first byte of the window, length 258 by symbol 285 and by symbol 284 + extra 31,
    length-3 / distance-1 runs"""
    toks = [] if len(hist) >= 32768 else list(_fq(70, 32768))
    toks.append((258, 32768))
    toks += [ord("A")] + [(258, 1)] + [(258, 1, 284)] + [(3, 1)] * 40 + [ord("C"), ord("G")] + [(3, 2)] * 10
    tail = _fq(71, 8000)
    toks += lz77(bytes(detok(toks, hist)) + tail, start=len(detok(toks, hist)))
    full = detok(toks, hist)
    fl, fd = freqs(toks)
    dynamic_block(bw, toks, lit=huffman_lengths(fl), dist=huffman_lengths(fd))
    return full


def v7_stored(bw, hist):
    """V7: stored blocks of 0, 1 and 65,535 bytes"""
    big = (_fq(80, 70000))[:65535]
    out = b""
    for piece in (b"", b"@", big, b"\n", b""):
        stored_block(bw, piece)
        out += piece
    tail = _fq(81, 6000)
    dynamic_block(bw, lz77(hist + out + tail, start=len(hist + out)))
    return out + tail


def v8_fixed_between(bw, hist):
    """V8: fixed blocks between dynamic ones (finish(..., fixed_last=True) ends the stream with a fixed block)"""
    out = b""
    for k, fixed in enumerate((False, True, False, True, True, False)):
        data = _fq(90 + k, 6000)
        toks = lz77(hist + out + data, start=len(hist + out))
        (fixed_block if fixed else dynamic_block)(bw, toks)
        out += data
    return out


def v9_eob_only(bw, hist):
    """V9: EOB-only blocks (a literal/length code of the single symbol 256, length 1) between text blocks"""
    lit = [0] * 257
    lit[256] = 1
    a, b = _fq(100, 8000), _fq(101, 8000)
    dynamic_block(bw, lz77(hist + a, start=len(hist)))
    dynamic_block(bw, [], lit=lit, dist=[0], hlit=257, hdist=1)
    dynamic_block(bw, [], lit=lit, dist=[1], hlit=257, hdist=1)
    dynamic_block(bw, lz77(hist + a + b, start=len(hist + a)))
    return a + b


VALID = {"v1_cross_zero_runs": v1_cross_zero_runs, "v1_cross_repeat": v1_cross_repeat, "v2_one_distance_code": v2_one_distance_code,
         "v3_no_distance_code": v3_no_distance_code, "v4_minimal_header": v4_minimal_header, "v5_15bit_codes": v5_15bit_codes,
         "v6_extreme_matches": v6_extreme_matches, "v7_stored": v7_stored, "v8_fixed_between": v8_fixed_between, "v9_eob_only": v9_eob_only}
def finish(bw, fixed_last=False):
    """end the stream: an empty final block (fixed, or stored)"""
    if fixed_last:
        fixed_block(bw, [], final=True)
    else:
        stored_block(bw, b"", final=True)
    return bw.getvalue()


def valid_empty_dynamic():
    """an empty stream that is not zlib's (03 00): one final dynamic block of the end-of-block code alone"""
    lit = [0] * 257
    lit[256] = 1
    bw = BitWriter()
    dynamic_block(bw, [], final=True, lit=lit, dist=[0], hlit=257, hdist=1)
    raw = bw.getvalue()
    assert zlib_inflate(raw) == b""
    return raw


@functools.lru_cache(maxsize=None)
def valid(name):
    """hand-built valid stream `name` on its own: (raw DEFLATE, text)"""
    bw = BitWriter()
    t = VALID[name](bw, b"")
    return finish(bw, fixed_last=name == "v8_fixed_between"), t


# ---- invalid streams: zlib's inflate rejects each. The violation comes before the first symbol is decoded, so no decoder may hand out
# any text; each builder takes `final` (False: the block is spliced into a longer stream) and returns the LENIENT text - what a decoder
# that overlooks the violation would deliver (the member trailers carry its CRC-32 and size: only the violation can give it away).

def _lens(toks):
    fl, fd = freqs(toks)
    return huffman_lengths(fl), (huffman_lengths(fd) if any(fd) else [0])


def _text_block(k, n=5000, allow=lambda d: d > 4):
    data = _fq(200 + k, n)
    toks = lz77(data, allow=allow)
    return data, toks, _lens(toks)


def i_over_lit(bw, final):
    data, toks, (lit, dist) = _text_block(0)
    lit[[s for s in range(256) if not lit[s]][0]] = 2           # a complete code plus one codeword of 2 bits: over-subscribed
    dynamic_block(bw, toks, final, lit=lit, dist=dist)
    return data


def i_over_dist(bw, final):
    data, toks, (lit, dist) = _text_block(1)
    dist[[s for s in range(30) if not dist[s]][0]] = 2
    dynamic_block(bw, toks, final, lit=lit, dist=dist)
    return data


def _longer(lens):
    """one used code made a bit longer: the code is incomplete, every used symbol still has its codeword"""
    m = max((s for s in range(len(lens)) if 0 < lens[s] < 15), key=lambda s: lens[s])
    lens[m] += 1
    assert kraft(lens) < 32768
    return lens


def i_incomplete_lit(bw, final):
    data, toks, (lit, dist) = _text_block(2)
    dynamic_block(bw, toks, final, lit=_longer(lit), dist=dist)
    return data


def i_incomplete_dist(bw, final):
    data, toks, (lit, dist) = _text_block(3)
    dynamic_block(bw, toks, final, lit=lit, dist=_longer(dist))
    return data


def i_one_dist_code_of_length_2(bw, final):
    """one distance code of length 2 (zlib takes an incomplete code only as one codeword of ONE bit)"""
    data = _fq(204, 5000)
    _, fd = freqs(lz77(data))
    ds = int(np.argmax(fd))
    toks = lz77(data, allow=lambda d: dist_sym(d) == ds)
    dist = [0] * 30
    dist[ds] = 2
    dynamic_block(bw, toks, final, lit=_lens(toks)[0], dist=dist)
    return data


def i_incomplete_code_length_code(bw, final):
    data, toks, (lit, dist) = _text_block(5)
    ops = rle(lit + dist)
    pf = [0] * 19
    for s, _ in ops:
        pf[s] += 1
    pre = huffman_lengths(pf, 6)
    m = max((s for s in range(19) if pre[s]), key=lambda s: pre[s])
    pre[m] += 1
    assert kraft(pre) < 32768
    dynamic_block(bw, toks, final, lit=lit, dist=dist, ops=ops, pre=pre)
    return data


def _too_many(hlit, hdist):
    def b(bw, final):
        data = _fq(206, 3000)
        toks = list(data)
        lit, _ = _lens(toks)
        dynamic_block(bw, toks, final, lit=lit + [0] * 40, dist=[1] + [0] * 40, hlit=hlit, hdist=hdist)
        return data
    return b


def _fixed_sym(lsym=None, dsym=None):
    def b(bw, final):
        data = _fq(207, 3000)
        fixed_block(bw, [(3, 1, lsym, dsym)] + list(data), final)
        return data[:1] * 3 + data
    return b


def i_too_far_back(bw, final):
    """the first symbol is a match: it reaches behind the member's first byte"""
    data = _fq(208, 3000)
    fixed_block(bw, [(20, 1)] + list(data), final)
    return bytes(20) + data


def i_first_length_is_16(bw, final):
    data, toks, (lit, dist) = _text_block(9)
    assert lit[:3] == [0, 0, 0]
    dynamic_block(bw, toks, final, lit=lit, dist=dist, ops=[(16, 0)] + rle((lit + dist)[3:]))   # (a lenient decoder repeats a 0)
    return data


def i_run_past_hlit_hdist(bw, final):
    data, toks, (lit, dist) = _text_block(10)
    lit = lit[:max(s for s in range(286) if lit[s]) + 1]
    dist = dist[:max(s for s in range(30) if dist[s]) + 1] + [0, 0]
    assert len(dist) <= 30
    ops = rle(lit + dist)
    assert ops[-2:] == [(0, 0), (0, 0)]
    ops[-2:] = [(18, 127)]                           # the last two (zero) lengths as a run of 138 zeros
    dynamic_block(bw, toks, final, lit=lit, dist=dist, hlit=len(lit), hdist=len(dist), ops=ops)
    return data


def i_stored_nlen(bw, final):
    data = _fq(211, 3000)
    stored_block(bw, data, final, nlen=0x1234)
    return data


def i_btype_3(bw, final):
    bw.put(1 if final else 0, 1)
    bw.put(3, 2)
    bw.put(0, 29)
    return b""


def i_no_eob_code(bw, final):
    data = _fq(212, 3000)
    toks = list(data)
    lit, _ = _lens(toks)
    lit[256] = 0
    dynamic_block(bw, toks, final, lit=lit, dist=[1], eob=False)
    return data


INVALID = {"over_subscribed_lit": i_over_lit, "over_subscribed_dist": i_over_dist, "incomplete_lit": i_incomplete_lit,
           "incomplete_dist": i_incomplete_dist, "one_dist_code_of_length_2": i_one_dist_code_of_length_2,
           "incomplete_code_length_code": i_incomplete_code_length_code, "hlit_287": _too_many(287, 1), "hlit_288": _too_many(288, 1),
           "hdist_31": _too_many(257, 31), "hdist_32": _too_many(257, 32), "dist_sym_30": _fixed_sym(dsym=30), "dist_sym_31": _fixed_sym(dsym=31),
           "len_sym_286": _fixed_sym(lsym=286), "len_sym_287": _fixed_sym(lsym=287), "too_far_back": i_too_far_back,
           "first_length_is_16": i_first_length_is_16, "run_past_hlit_hdist": i_run_past_hlit_hdist, "stored_nlen": i_stored_nlen,
           "btype_3": i_btype_3, "no_eob_code": i_no_eob_code}
# a violation wherever it stands (too_far_back is one only at the start of a member)
SPLICEABLE_INVALID = tuple(n for n in INVALID if n != "too_far_back")


@functools.lru_cache(maxsize=None)
def invalid(name):
    """invalid stream `name` on its own: (raw DEFLATE, lenient text)"""
    bw = BitWriter()
    t = INVALID[name](bw, True)
    return bw.getvalue(), t


# ---- splices: hand-built blocks in the middle of a realistic stream -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spliced_parts(name, before=1 << 20, after=1 << 20):
    """a zlib piece of `before` text bytes closed by a full flush, the hand-built blocks of `name` (VALID, or INVALID: its block goes in
    non-final), an empty stored block (to a byte boundary), a zlib piece of `after` bytes primed with the 32 KiB in front of it:
    (raw DEFLATE, text - for an invalid block the lenient text -, first byte of the hand-built blocks, first byte behind them)"""
    t = text("fastq") * 2                        # (a second copy lies far behind the 32 KiB window: no match reaches it)
    a = t[:before]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH)
    bw = BitWriter()
    mid = VALID[name](bw, a[-32768:]) if name in VALID else INVALID[name](bw, False)
    stored_block(bw, b"")
    hand = bw.getvalue()
    b = t[before:before + after]
    assert len(b) == after
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, (a + mid)[-32768:])
    return raw + hand + co.compress(b) + co.flush(), a + mid + b, len(raw), len(raw) + len(hand)


def spliced(name, before=1 << 20, after=1 << 20):
    """spliced_parts without the offsets: (raw DEFLATE, text)"""
    return spliced_parts(name, before, after)[:2]


# ---- the corpus checks itself with zlib ----------------------------------------------------------------------------------------------

def zlib_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw) + d.flush()
    if not d.eof:
        raise zlib.error("incomplete stream")
    return out


def self_check(raw, data, ok=True):
    if ok:
        assert zlib_inflate(raw) == data
    else:
        try:
            zlib_inflate(raw)
        except zlib.error:
            return
        raise AssertionError("zlib accepts a stream the corpus calls invalid")
