"""A plain model of the device DEFLATE encoder (ribodetector_amd/csrc/rd_deflate.hpp, rd_gz_deflate_kernel): its parse, its code
construction and its framing, written out rule by rule in Python so that the kernel can be compared with something other than a decoder.

  parse_member(data)            the tokens of one member (at most 65,280 bytes), as the kernel's rules give them
  encode_member(tokens, data)   the member's bytes for those tokens: code lengths, block header, bits, BGZF framing, stored fallback
  audit_member(tokens, data)    what must hold for ANY tokens the kernel may produce, whichever lane wins an insert

The one thing the rules leave open is the winner of an insert: the lanes of a strip that share a bucket store to it at once, one
store stays, and the loser's position is never inserted. The model takes the highest lane (as tools/gzdev_model.c does) and keeps,
per way, the SET of positions that could stand there; a lookup that matters to the parse and reads a way whose set holds more than one
position, any of which agrees with the looker over 8 bytes, is counted as ambiguous (stats["ambiguous"]). Where that count is 0 the
tokens do not depend on the winner and a device must produce exactly them. The lookups that matter are those at a position where a
token starts and at its successor during the lazy look-ahead. One exception keeps long runs decidable: a lane that takes the run,
none of whose open ways could hold a longer candidate, takes it whoever won (inside a run every earlier position of the run shares
the bucket, agrees over 8 bytes and ties with the run, and the run wins ties).

One rule is finer than its one-line form. A lane first compares each way over the 16 bytes at the two positions - NOT cut at the
part's end - and picks the longest of those capped lengths (the nearest on ties; the run when it is as long); only then is the length
cut to min(258, q1 - p), and only ways that agreed over all 16 bytes go on to the exact measure. Within the last 15 positions of a
part this can pick a farther way than a choice among lengths already cut would; the length is the same either way.
"""
import struct
import zlib
from dataclasses import dataclass, replace

import numpy as np

from deflate_tokens import CLORD, DBASE, DEXTRA, LBASE, LEXTRA

MEMBER, NQ = 65280, 16
PART = MEMBER // NQ
CAP, MAXM, HBITS = 16, 258, 9
TEXT_BYTES = MEMBER + 16            # the LDS buffer the kernel assembles a dynamic block in


@dataclass(frozen=True)
class Rules:
    """the kernel's rules; the tests break them one at a time to show that the cases would notice"""
    min_match: int = 8              # bytes a way must agree over, and bytes that must be left in the part to hash a position
    min_run: int = 6
    run_at_q0: bool = False
    lazy: bool = True
    lazy_past_strip: bool = False
    ways: int = 4                   # ways probed (the table always has 4)
    measure_stop: int = MAXM        # where the exact measure gives up
    seed: int = 512
    farthest: bool = False
    shift: bool = True


KERNEL = Rules()
VARIANTS = {
    "minimum match 7": replace(KERNEL, min_match=7),
    "minimum run 5": replace(KERNEL, min_run=5),
    "run allowed at p == q0": replace(KERNEL, run_at_q0=True),
    "no lazy rule": replace(KERNEL, lazy=False),
    "lazy look-ahead past the strip's last lane": replace(KERNEL, lazy_past_strip=True),
    "3 ways": replace(KERNEL, ways=3),
    "exact measure stopped at 16 + 64 bytes": replace(KERNEL, measure_stop=CAP + 64),
    "no seed": replace(KERNEL, seed=0),
    "seed of 448": replace(KERNEL, seed=448),
    "ties to the farthest": replace(KERNEL, farthest=True),
    "the insert's way shift dropped": replace(KERNEL, shift=False),
}


def gz_hash(data_padded):
    """gz_hash of every position: ((a ^ rotl(b, 15)) * 0x9E3779B1) >> 23 over the two little-endian dwords there; also the 8 bytes
    as one number (two positions agree over 8 bytes when these are equal)"""
    w = data_padded.astype(np.uint32)
    m = len(w) - 8
    d32 = w[0:m + 4] | (w[1:m + 5] << 8) | (w[2:m + 6] << 16) | (w[3:m + 7] << 24)
    a, b = d32[:m], d32[4:m + 4]
    hh = (a ^ ((b << 15) | (b >> 17))) * np.uint32(0x9E3779B1)
    return (hh >> (32 - HBITS)).tolist(), (a.astype(np.uint64) | (b.astype(np.uint64) << 32)).tolist()


def parse_member(data, rules=KERNEL, stats=None):
    """the tokens of one member: a literal is an int, a match (length, distance). stats (a dict) receives "ambiguous": the number of
    positions whose lookup mattered to the parse and could depend on which lane won an insert."""
    n = len(data)
    assert n <= MEMBER
    pad = np.zeros(n + 40, dtype=np.uint8)
    pad[:n] = np.frombuffer(bytes(data), dtype=np.uint8)
    B = pad.tobytes()                                   # the member with zeros behind it, as it lies in LDS
    bucket, key8 = gz_hash(pad)
    tokens, ambiguous = [], set()

    def agree(p, c, lim):
        if B[p:p + lim] == B[c:c + lim]:
            return lim
        k = 0
        while k < lim and B[p + k] == B[c + k]:
            k += 1
        return k

    for q0 in range(0, n, PART):
        q1 = min(n, q0 + PART)
        qb = max(0, q0 - rules.seed)
        win = [[-1] * 4 for _ in range(1 << HBITS)]     # per bucket: the 4 nearest earlier positions, nearest first
        could = [[()] * 4 for _ in range(1 << HBITS)]   # per way: every position that could stand there

        def insert(ps):
            groups = {}
            for p in ps:
                groups.setdefault(bucket[p], []).append(p)
            for h, g in groups.items():                 # once per bucket and strip: the occupants move down, the winner takes way 0
                win[h] = [g[-1]] + (win[h][:3] if rules.shift else win[h][1:])
                could[h] = [tuple(g)] + (could[h][:3] if rules.shift else could[h][1:])

        def look(p, win, could):
            """one lane, on the table as given: (capped length, distance, the bucket's ways, those that agree over 16 bytes,
            whether the run does, ambiguous)"""
            lim = min(MAXM, q1 - p)
            Lc, Dc, tab, full, runfull, open_ = 0, 0, None, [], False, set()
            if p + rules.min_match <= q1:
                h, k8 = bucket[p], key8[p]
                tab, best = win[h], -1
                for u in range(rules.ways):
                    c = tab[u]
                    cs = could[h][u]
                    if len(cs) > 1:
                        open_.update(x for x in cs if key8[x] == k8)
                    if c < 0 or (key8[c] != k8 and rules.min_match >= 8):
                        continue
                    k = agree(p, c, CAP)
                    if k < rules.min_match:
                        continue
                    if k == CAP:
                        full.append(u)
                    key = (k << 2) | (u if rules.farthest else 3 - u)
                    if key > best:
                        best, Lc, Dc = key, k, p - c
            if (p > q0 or (rules.run_at_q0 and p > 0)) and lim >= rules.min_run:
                k = agree(p, p - 1, CAP)
                if k >= rules.min_run:
                    runfull = k == CAP
                    if k >= Lc:
                        Lc, Dc = k, 1
                        # the lane takes the run whatever stands in the open ways, when none of their possible occupants is longer
                        # (inside a long run every earlier position of the run is such an occupant, and ties with it)
                        r = agree(p, p - 1, lim)
                        if all(agree(p, x, CAP) <= k and agree(p, x, lim) <= r for x in open_):
                            open_ = ()
            return min(Lc, lim), Dc, tab, full, runfull, bool(open_)

        def measure(p, Lc, Dc, full, runfull, tab):
            """the exact length of a chosen match: only the ways (and the run) that agreed over all 16 bytes are measured"""
            if not full and not runfull:
                return Lc, Dc
            lim = min(MAXM, q1 - p)
            bestL, bestD, best = 0, Dc, -1
            for u in full:
                c = tab[u]
                g = min(agree(p, c, lim), rules.measure_stop)
                key = (g << 2) | (u if rules.farthest else 3 - u)
                if key > best:
                    best, bestL, bestD = key, g, p - c
            if runfull:
                r = agree(p, p - 1, lim)
                if r >= bestL:
                    bestL, bestD = r, 1
            return bestL, bestD

        if rules.seed:
            for s0 in range(qb, q0, 64):                # the end of the part before: inserted, not parsed
                insert(range(s0, min(s0 + 64, q0)))
        carry = 0
        for s0 in range(q0, q1, 64):
            ns = min(64, q1 - s0)
            before = (win[:], could[:])                 # every lane looks before any lane inserts (insert() replaces a bucket's lists)
            lanes = {}

            def lane(l):
                if l not in lanes:
                    lanes[l] = look(s0 + l, *before)
                return lanes[l]
            insert(p for p in range(s0, s0 + ns) if p + rules.min_match <= q1)
            if carry >= ns:
                carry -= ns
                continue
            pos = carry
            while pos < ns:
                Lc, Dc, tab, full, runfull, amb = lane(pos)
                if amb:
                    ambiguous.add(s0 + pos)
                Ln = 0
                if 0 < Lc < CAP and rules.lazy:
                    nxt = None
                    if pos + 1 < ns:
                        nxt = lane(pos + 1)
                    elif rules.lazy_past_strip and s0 + pos + 1 < q1:
                        nxt = look(s0 + pos + 1, win, could)
                    if nxt is not None:
                        Ln = nxt[0]
                        if nxt[5]:
                            ambiguous.add(s0 + pos + 1)
                if Lc > 0 and not (Lc < CAP and Ln > Lc):
                    L, D = measure(s0 + pos, Lc, Dc, full, runfull, tab)
                    tokens.append((L, D))
                    pos += L
                else:
                    tokens.append(B[s0 + pos])
                    pos += 1
            carry = pos - ns
    if stats is not None:
        stats["ambiguous"] = len(ambiguous)
    return tokens


# ---- codes, block header, framing --------------------------------------------------------------------------------------------------

def len_sym(L):
    s = 28
    while LBASE[s] > L:
        s -= 1
    return s


def dist_sym(D):
    s = 29
    while DBASE[s] > D:
        s -= 1
    return s


def code_lengths(freq, maxbits):
    """rank sort of the used symbols by (frequency, symbol); two-queue merge, a tie goes to the leaf; depths clamped; zlib's gen_bitlen
    repair; the rarest leaves get the longest codes"""
    freq = list(freq)
    used = sum(1 for f in freq if f)
    for i in range(len(freq)):                          # at least two codes: the lowest unused symbols get frequency 1
        if used >= 2:
            break
        if not freq[i]:
            freq[i] = 1
            used += 1
    order = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    ns = len(order)
    w = [freq[s] for s in order]
    parent = {}
    a, b, nn = 0, ns, ns
    while nn < 2 * ns - 1:
        total = 0
        for _ in range(2):
            if a < ns and (b >= nn or w[a] <= w[b]):
                pick, a = a, a + 1
            else:
                pick, b = b, b + 1
            parent[pick] = nn
            total += w[pick]
        w.append(total)
        nn += 1
    depth = {nn - 1: 0}
    for i in range(nn - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    bl = [0] * (maxbits + 1)
    for i in range(ns):
        bl[min(depth[i], maxbits)] += 1
    K = sum(bl[k] << (maxbits - k) for k in range(1, maxbits + 1))
    while K > (1 << maxbits):                           # a leaf moves one level down and takes an overflowed leaf as its brother
        bits = maxbits - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[maxbits] -= 1
        K -= 1
    lens = [0] * len(freq)
    i = 0
    for k in range(maxbits, 0, -1):
        for _ in range(bl[k]):
            lens[order[i]] = k
            i += 1
    return lens


def canonical_codes(lens):
    """canonical codes, bit-reversed (DEFLATE sends Huffman codes MSB first)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return codes


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.nb, self.total = bytearray(), 0, 0, 0

    def put(self, v, n):
        self.acc |= v << self.nb
        self.nb += n
        self.total += n
        while self.nb >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.nb -= 8

    def finish(self):
        if self.nb:
            self.out.append(self.acc & 0xff)            # padding bits are zero
        return bytes(self.out)


def dynamic_block(tokens):
    """the member's one dynamic block as the kernel builds it: (bytes, header fields)"""
    fl, fd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            fl[257 + len_sym(t[0])] += 1
            fd[dist_sym(t[1])] += 1
        else:
            fl[t] += 1
    fl[256] += 1
    ll, dl = code_lengths(fl, 15), code_lengths(fd, 15)
    lc, dc = canonical_codes(ll), canonical_codes(dl)
    hlit, hdist = 286, 30
    while hlit > 257 and ll[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and dl[hdist - 1] == 0:
        hdist -= 1
    seq = ll[:hlit] + dl[:hdist]                        # sent one by one: no symbols 16-18
    fc = [0] * 19
    for s in seq:
        fc[s] += 1
    cl = code_lengths(fc, 7)
    cc = canonical_codes(cl)
    hclen = 19
    while hclen > 4 and cl[CLORD[hclen - 1]] == 0:
        hclen -= 1
    w = _BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl[CLORD[k]], 3)
    for s in seq:
        w.put(cc[s], cl[s])
    for t in tokens:
        if isinstance(t, tuple):
            ls, ds = len_sym(t[0]), dist_sym(t[1])
            w.put(lc[257 + ls], ll[257 + ls])
            w.put(t[0] - LBASE[ls], LEXTRA[ls])
            w.put(dc[ds], dl[ds])
            w.put(t[1] - DBASE[ds], DEXTRA[ds])
        else:
            w.put(lc[t], ll[t])
    w.put(lc[256], ll[256])
    return w.finish(), {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl_lens": cl, "lit_lens": ll[:hlit], "dist_lens": dl[:hdist]}


def is_stored(dynamic_bytes, n):
    """the kernel's choice: stored when the dynamic block is no smaller, or would not fit the buffer it is assembled in
    (18 + bytes + 8 + 8 > 65,296)"""
    return dynamic_bytes >= n + 5 or 18 + dynamic_bytes + 8 + 8 > TEXT_BYTES


def encode_member(tokens, data):
    """the BGZF member the kernel writes for these tokens of data"""
    data = bytes(data)
    n = len(data)
    body, _ = dynamic_block(tokens)
    if is_stored(len(body), n):
        body = b"\x01" + struct.pack("<HH", n, ~n & 0xffff) + data
    total = 18 + len(body) + 8
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff\x06\x00" + b"BC\x02\x00" + struct.pack("<H", total - 1)
    return head + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, n)


# ---- what holds whichever lane wins ------------------------------------------------------------------------------------------------

def audit_member(tokens, data):
    """the violations of what every parse of the kernel must keep, as a list of strings (empty: none):
      * a token starts on every multiple of 4,080 (no match crosses a part's end);
      * a match at p in part [q0, q1), qb = max(0, q0 - 512): 8 <= L <= 258, or D == 1 with 6 <= L <= 7 and p > q0; p + L <= q1;
        p - D >= qb; it repeats the text; it is maximal (L == 258, or it ends on q1, or the next byte differs);
      * a literal at p where a run of 6+ was there (p > q0, six bytes equal to the byte before, q1 - p >= 6) can only be the lazy rule's
        doing: the run's length r (counted up to 16 and q1 - p) is below 16 and a longer match follows - at once, or after j more
        literals of a chain of deferrals within the strip, and then it is longer than r + j (with j = 0 this is `the next token is
        a match longer than the run`; FASTQ quality strings do produce chains, which that shorter form would call violations)."""
    data = bytes(data)
    n = len(data)
    bad, p, starts = [], 0, set()
    for i, t in enumerate(tokens):
        starts.add(p)
        if p >= n:
            bad.append("token %d starts at %d, behind the member's %d bytes" % (i, p, n))
            break
        q0 = p - p % PART
        q1 = min(n, q0 + PART)
        qb = max(0, q0 - 512)
        if isinstance(t, tuple):
            L, D = t
            if not (8 <= L <= MAXM or (D == 1 and 6 <= L <= 7 and p > q0)):
                bad.append("match (%d, %d) at %d: length not allowed" % (L, D, p))
            if p + L > q1:
                bad.append("match (%d, %d) at %d crosses the part's end %d" % (L, D, p, q1))
            if p - D < qb:
                bad.append("match (%d, %d) at %d reaches before %d" % (L, D, p, qb))
            elif any(data[p + k] != data[p + k - D] for k in range(min(L, n - p))):
                bad.append("match (%d, %d) at %d does not repeat the text" % (L, D, p))
            elif not (L == MAXM or p + L >= q1 or data[p + L] != data[p + L - D]):
                bad.append("match (%d, %d) at %d is not maximal" % (L, D, p))
            p += L
        else:
            if t != data[p]:
                bad.append("literal %d at %d, the text has %d" % (t, p, data[p]))
            if p > q0 and q1 - p >= 6 and data[p:p + 6] == data[p - 1:p] * 6:
                run = 6
                while run < min(CAP, q1 - p) and data[p + run] == data[p - 1]:
                    run += 1
                # only the lazy rule turns such a position into a literal: its length (the run's at least) is below 16 and the next
                # lane holds a longer one - which may yield in turn, so j more literals may follow, each lane's length above the one
                # before, all in one strip; the match that ends the chain is then longer than the run by more than j
                j = 0
                while i + 1 + j < len(tokens) and not isinstance(tokens[i + 1 + j], tuple):
                    j += 1
                nxt = tokens[i + 1 + j] if i + 1 + j < len(tokens) else None
                if not (nxt is not None and run < CAP and nxt[0] > run + j and (p - q0) % 64 + j + 1 <= 63):
                    bad.append("literal at %d where a run of %d was there: %d more literals, then %r" % (p, run, j, nxt))
            p += 1
    if p != n and not bad:
        bad.append("the tokens cover %d of %d bytes" % (p, n))
    for q in range(0, n, PART):
        if q not in starts:
            bad.append("no token starts at the part boundary %d" % q)
    return bad
