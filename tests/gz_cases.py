"""Crafted members for the device DEFLATE encoder: random bytes over 256 values with planted repeats and runs, one rule of the parse
per case (tests/gz_model.py has the rules). A case redraws its filler until the model reports no ambiguous lookup - no lookup whose
answer could depend on which lane won an insert - so a device must produce the model's tokens exactly.

drawn() builds every case once: (name, member bytes, the model's tokens). Each case also states what its tokens must show (the
planted match, the literals where a rule forbids one), so a case cannot silently stop exercising its rule.
"""
import functools
import zlib

import numpy as np

import gz_model as M
from deflate_tokens import LBASE, DBASE

DRAWS = 20
PART = M.PART


# The filler: random bytes over all 256 values, the k-th most frequent of them with a share of 0.95^k (which value that is, is drawn
# too). About 5.7 bits a byte: uniform bytes would make every member a STORED block, and a stored block hides the tokens. Eight bytes
# agree by chance with a probability of 2e-13, six equal bytes in a row with 6e-8.
_SHARE = 0.95 ** np.arange(256)
_SHARE /= _SHARE.sum()


def fill(rng, n):
    values = rng.permutation(256).astype(np.uint8)
    return bytearray(values[rng.choice(256, n, p=_SHARE)].tobytes())


def differ(rng, *avoid):
    while True:
        v = int(rng.integers(0, 256))
        if v not in avoid:
            return v


def plant(rng, b, src, dst, L):
    """b[dst : dst + L] repeats b[src : src + L] and no more: the bytes before and behind differ (dst - src < L: a periodic stretch)"""
    for k in range(L):
        b[dst + k] = b[src + k]
    if dst + L < len(b):
        b[dst + L] = differ(rng, b[src + L])
    if src > 0:
        b[src - 1] = differ(rng, b[dst - 1])


def keep_in_table(rng, b, src, dst, spans):
    """a bucket keeps its 4 nearest positions, and over thousands of bytes of filler a source is pushed out of its own: change the
    filler (outside the spans (first, last) that the case has written) until nothing between the source and its repeat shares the
    source's bucket but its copies"""
    safe = lambda j: not any(lo <= j <= hi for lo, hi in spans)
    for _ in range(100):
        h, k8 = M.gz_hash(np.frombuffer(bytes(b) + bytes(16), dtype=np.uint8))
        bad = [x for x in range(src + 1, dst) if h[x] == h[src] and k8[x] != k8[src]]
        if not bad:
            return
        for x in bad:
            for j in range(x, min(x + 8, len(b))):
                if safe(j):
                    b[j] = int(rng.integers(0, 256))
                    break


def starts(tokens):
    at, p = {}, 0
    for t in tokens:
        at[p] = t
        p += t[0] if isinstance(t, tuple) else 1
    return at


def matches(tokens):
    return [t for t in tokens if isinstance(t, tuple)]


def pieces(at, p, L, D, least=8):
    """a repeat of L at p comes out as matches of at most 258, then literals for a rest too short to match"""
    while L >= least:
        k = min(L, M.MAXM)
        assert at.get(p) == (k, D), (p, at.get(p), (k, D))
        p, L = p + k, L - k
    for k in range(L):
        assert isinstance(at.get(p + k), int), (p + k, at.get(p + k))


def lit(at, p):
    assert isinstance(at.get(p), int), (p, at.get(p))


CASES = []


def case(name):
    def deco(fn):
        CASES.append((name, fn))
        return fn
    return deco


def _add(name, build):
    CASES.append((name, build))


# ---- one planted repeat: the minimum, the cap of 16, every round of the exact measure, every length symbol ---------------------------
def _repeat(L):
    def build(rng):
        src = 133
        dst = 64 * ((src + L + 200) // 64 + 1) + 17
        b = fill(rng, dst + L + 150)
        plant(rng, b, src, dst, L)

        def expect(tokens):
            at = starts(tokens)
            if L < 8:
                assert not matches(tokens)
            else:
                pieces(at, dst, L, dst - src)
                assert sum(t[0] for t in matches(tokens)) == L - (L % M.MAXM if L % M.MAXM < 8 else 0)
        return bytes(b), expect
    return build


REPEATS = sorted({7, 8, 15, 16, 17, 79, 80, 81, 143, 144, 145, 207, 208, 209, 257, 258, 259, 600} | set(LBASE[5:]))
for _L in REPEATS:
    _add("repeat of %d" % _L, _repeat(_L))


# ---- the part's end -----------------------------------------------------------------------------------------------------------------
@case("repeat cut by the part's end")
def _(rng):
    b = fill(rng, PART + 600)
    plant(rng, b, 3700, 4050, 50)

    def expect(tokens):
        at = starts(tokens)
        assert at.get(4050) == (30, 350) and at.get(4080) == (20, 350), (at.get(4050), at.get(4080))
    return bytes(b), expect


@case("repeat that ends on the part's end")
def _(rng):
    b = fill(rng, PART + 600)
    plant(rng, b, 3700, 4040, 40)

    def expect(tokens):
        at = starts(tokens)
        assert at.get(4040) == (40, 340)
        lit(at, 4080)
    return bytes(b), expect


@case("repeat of 8 that starts 7 bytes before the part's end")
def _(rng):
    b = fill(rng, PART + 600)
    plant(rng, b, 3700, PART - 7, 8)                # 7 bytes are left at its position: not hashed, so not found

    def expect(tokens):
        assert not matches(tokens), matches(tokens)
    return bytes(b), expect


# ---- runs ---------------------------------------------------------------------------------------------------------------------------
def _run(R):
    def build(rng):
        p0 = 700
        b = fill(rng, p0 + R + 300)
        x = differ(rng, b[p0 - 1])
        for k in range(R + 1):                      # R + 1 equal bytes: a run of R at distance 1 behind the first
            b[p0 + k] = x
        b[p0 + R + 1] = differ(rng, x)

        def expect(tokens):
            at = starts(tokens)
            lit(at, p0)
            if R < 6:
                assert not matches(tokens)
            else:
                pieces(at, p0 + 1, R, 1, least=6)
        return bytes(b), expect
    return build


for _R in (5, 6, 7, 15, 16, 17, 258, 1000):
    _add("run of %d" % _R, _run(_R))


@case("run over the first byte of a part")
def _(rng):
    b = fill(rng, PART + 600)
    x = differ(rng, b[PART - 2])
    for k in range(8):                              # 4079 .. 4086: seven of them from the part's first byte on
        b[PART - 1 + k] = x
    b[PART + 7] = differ(rng, x)

    def expect(tokens):
        at = starts(tokens)
        lit(at, PART)                               # no distance-1 match at p == q0 (and the seed's 4079 agrees over 7 bytes only)
        assert at.get(PART + 1) == (6, 1), at.get(PART + 1)
    return bytes(b), expect


@case("run against a hash candidate of equal length")
def _(rng):
    b = fill(rng, 2000)
    a = 65
    s2, src, p = 300, 500, 64 * 15 + 20
    for k in range(s2 - 12, s2 + 3):
        if b[k] == a:
            b[k] = differ(rng, a)
    b[s2] = a                                       # ... a, then not a: what the match in front of p repeats
    b[src - 1] = differ(rng, a)
    for k in range(8):
        b[src + k] = a
    b[src + 8] = differ(rng, a)
    b[p - 11:p] = b[s2 - 10:s2 + 1]                 # a match of 11 that ends with an a at p - 1: a token starts at p
    b[p - 12] = differ(rng, b[s2 - 11])
    for k in range(8):
        b[p + k] = a
    b[p + 8] = differ(rng, a, b[src + 8])

    def expect(tokens):
        at = starts(tokens)
        assert at.get(p - 11) == (11, p - 1 - s2) and at.get(p) == (8, 1), (at.get(p - 11), at.get(p))
    return bytes(b), expect


# ---- the lazy rule ------------------------------------------------------------------------------------------------------------------
def _stack(lens, lane, expect_fn):
    """lens[i] bytes repeat at p + i (each from a source of its own, in a strip of its own), p at the given lane"""
    def build(rng):
        b = fill(rng, 2200)
        p = 64 * 20 + lane
        srcs = []
        for i, L in enumerate(lens):
            s = 133 + 192 * i
            srcs.append(s)
            b[s:s + L] = b[p + i:p + i + L]
            b[s + L] = differ(rng, b[p + i + L])
            b[s - 1] = differ(rng, b[p + i - 1])
        for _ in range(2):
            for s in srcs:
                keep_in_table(rng, b, s, p, [(s - 1, s + L) for s, L in zip(srcs, lens)] + [(p - 1, p + 64)])
        return bytes(b), lambda tokens: expect_fn(starts(tokens), p, srcs)
    return build


def _deferred(at, p, s):
    lit(at, p)
    assert at.get(p + 1) == (40, p + 1 - s[1]), at.get(p + 1)


def _kept16(at, p, s):
    assert at.get(p) == (16, p - s[0]) and at.get(p + 16) == (25, p + 1 - s[1]), (at.get(p), at.get(p + 16))


def _kept15(at, p, s):
    assert at.get(p) == (15, p - s[0]) and at.get(p + 15) == (26, p + 1 - s[1]), (at.get(p), at.get(p + 15))


def _chain(at, p, s):
    for k in range(3):
        lit(at, p + k)
    assert at.get(p + 3) == (40, p + 3 - s[3]), at.get(p + 3)


_add("lazy: 15 then 40 is deferred", _stack((15, 40), 10, _deferred))
_add("lazy: 16 then 40 is not deferred", _stack((16, 40), 10, _kept16))
_add("lazy: 15 then 40 at lane 63 is not deferred", _stack((15, 40), 63, _kept15))
_add("lazy: 16 then 40 at lane 63 is not deferred", _stack((16, 40), 63, _kept16))
_add("lazy: a chain of three deferrals", _stack((9, 10, 11, 40), 10, _chain))


# ---- the four ways ------------------------------------------------------------------------------------------------------------------
def _copies(follow, want):
    """earlier copies of one 8-byte prefix (oldest first), copy i agreeing with the looker over follow[i] bytes"""
    def build(rng):
        p = 64 * ((133 + 192 * len(follow)) // 64 + 2) + 20
        b = fill(rng, p + 300)
        srcs = []
        for i, L in enumerate(follow):
            s = 133 + 192 * i
            srcs.append(s)
            b[s:s + L] = b[p:p + L]
            b[s + L] = differ(rng, b[p + L])
            b[s - 1] = differ(rng, b[p - 1])
        keep_in_table(rng, b, srcs[0], p, [(s - 1, s + L) for s, L in zip(srcs, follow)] + [(p - 1, p + 64)])

        def expect(tokens):
            at = starts(tokens)
            assert at.get(p) == (follow[want], p - srcs[want]), (at.get(p), follow[want], p - srcs[want])
        return bytes(b), expect
    return build


_add("ways: the longest of four copies, the oldest", _copies((30, 12, 20, 9), 0))
_add("ways: the longest of four copies", _copies((12, 30, 20, 9), 1))
_add("ways: two of equal length, the nearest", _copies((12, 20, 20, 9), 2))
_add("ways: five copies, the oldest is gone", _copies((40, 12, 20, 14, 9), 2))


# ---- matches over several strips ----------------------------------------------------------------------------------------------------
def _long(L, lane):
    def build(rng):
        src, dst, p2 = 133, 64 * 12 + lane, 64 * 22 + 9
        inner = dst + 80                            # inside the match (L = 200: in a strip that is inserted and not searched)
        b = fill(rng, p2 + 200)
        plant(rng, b, src, dst, L)
        b[p2:p2 + 12] = b[inner:inner + 12]
        b[p2 + 12] = differ(rng, b[inner + 12], b[src + 80 + 12])
        b[p2 - 1] = differ(rng, b[inner - 1], b[src + 80 - 1])

        def expect(tokens):
            at = starts(tokens)
            assert at.get(dst) == (L, dst - src), at.get(dst)
            assert at.get(p2) == (12, p2 - inner), at.get(p2)      # the nearer of two equal copies: the one inside the match
        return bytes(b), expect
    return build


for _L in (100, 200):
    for _lane in (0, 1, 63):
        _add("match of %d from lane %d, a position inside it found later" % (_L, _lane), _long(_L, _lane))


# ---- the seed -----------------------------------------------------------------------------------------------------------------------
def _seed(k, part):
    def build(rng):
        x = PART if part else 1000                  # part 1: the source k bytes before the part's start; part 0: the same, no seed
        src, dst = x - k, x + 337
        b = fill(rng, x + 700)
        plant(rng, b, src, dst, 8)

        def expect(tokens):
            if part and k > 512:
                assert not matches(tokens)
            else:
                assert starts(tokens).get(dst) == (8, dst - src)
        return bytes(b), expect
    return build


for _k in (1, 511, 512, 513):
    _add("seed: source %d before part 1" % _k, _seed(_k, 1))
for _k in (1, 511, 512, 513):
    _add("no seed in part 0: source %d before byte 1000" % _k, _seed(_k, 0))


# ---- every distance symbol a part can reach, the farthest distance -------------------------------------------------------------------
def _distance(D):
    def build(rng):
        L = 12
        if D <= 3073:
            dst = 64 * ((D + 70) // 64 + 1)         # lane 0: the source lies in an earlier strip at any distance
        elif D == 4097:
            dst = PART + 64 * 57                    # the source in the seed of part 1
        else:
            dst, L = 2 * PART - 8, 8                # the last hashable position of part 1, the first byte of its seed
        b = fill(rng, min(dst + 150, 2 * PART) if D > 3073 else dst + 150)
        plant(rng, b, dst - D, dst, L)
        if D > L:
            keep_in_table(rng, b, dst - D, dst, [(dst - D - 1, dst - D + L), (dst - 1, dst + L)])

        def expect(tokens):
            assert starts(tokens).get(dst) == (L, D), (starts(tokens).get(dst), (L, D))
        return bytes(b), expect
    return build


# (p - D >= q0 - 512 and p + 8 <= q1: 4,584 is the farthest a match can reach)
DISTANCES = [d for d in DBASE if d <= 4097] + [PART - 8 + 512]
for _D in DISTANCES:
    _add("distance %d" % _D, _distance(_D))


# ---- short members and the tails of parts --------------------------------------------------------------------------------------------
def _length(n):
    def build(rng):
        b, want = fill(rng, n), {}
        rep_end = {PART - 1: PART - 1, PART: PART, PART + 1: PART, 2 * PART + 7: 2 * PART}.get(n)
        if rep_end:                                 # a repeat of 8 at the last hashable position of a part: p + 8 == q1
            p = rep_end - 8
            plant(rng, b, p - 350, p, 8)
            want[p] = (8, 350)
        if n >= 8 and n not in (PART - 1, PART, PART + 1):
            x = differ(rng, b[n - 8])               # seven equal bytes at the very end: a run of 6 where nothing is hashed any more
            for k in range(7):
                b[n - 7 + k] = x
            want[n - 6] = (6, 1)

        def expect(tokens):
            at = starts(tokens)
            for p, t in want.items():
                assert at.get(p) == t, (n, p, at.get(p), t)
        return bytes(b), expect
    return build


LENGTHS = list(range(1, 21)) + [63, 64, 65, PART - 1, PART, PART + 1, 2 * PART + 7]
for _n in LENGTHS:
    _add("member of %d bytes" % _n, _length(_n))


# ---- the last wave -------------------------------------------------------------------------------------------------------------------
@case("seed and repeat in part 15 of a full member")
def _(rng):
    b = fill(rng, M.MEMBER)
    src, dst = 15 * PART - 300, 15 * PART + 517
    plant(rng, b, src, dst, 20)
    return bytes(b), lambda tokens: pieces(starts(tokens), dst, 20, dst - src)


@functools.lru_cache(maxsize=None)
def drawn():
    """every case, drawn until the model sees no ambiguous lookup: [(name, data, tokens)]; a case that finds no such draw in DRAWS
    seeds, or whose tokens do not show what it was made for, is an error"""
    out = []
    for name, build in CASES:
        why = []
        for seed in range(DRAWS):
            data, expect = build(np.random.default_rng([zlib.crc32(name.encode()), seed]))
            stats = {}
            tokens = M.parse_member(data, stats=stats)
            if stats["ambiguous"]:
                why.append("%d ambiguous" % stats["ambiguous"])
                continue
            try:                                    # (the filler can get in the way: four later positions in the source's bucket)
                expect(tokens)
            except AssertionError as e:
                why.append("not what the case is for: %s" % (e,))
                continue
            break
        else:
            raise AssertionError("%s: no draw in %d seeds: %s" % (name, DRAWS, why))
        REDRAWN[name] = why
        out.append((name, data, tokens))
    return out


@functools.lru_cache(maxsize=None)
def crossover(n=4000):
    """stored or dynamic, at the edge: the first k bytes of the member are uniform over 256 values (8 bits each, nothing to gain),
    the rest is the filler above (about 5.7). k is the dial: the model's dynamic block grows with it, and the two neighbouring
    settings are returned where it is last below n + 5 bytes and first not - [(k, data, tokens, dynamic bytes)] * 2, both without an
    ambiguous lookup"""
    for seed in range(DRAWS):
        rng = np.random.default_rng([77, seed])
        flat, skew = bytes(rng.integers(0, 256, n, dtype=np.uint8)), bytes(fill(rng, n))

        def at(k):
            data, stats = flat[:k] + skew[k:], {}
            tokens = M.parse_member(data, stats=stats)
            return k, data, tokens, len(M.dynamic_block(tokens)[0]), stats["ambiguous"]
        lo, hi = at(0), at(n)
        assert lo[3] < n + 5 <= hi[3]
        while hi[0] - lo[0] > 1:
            mid = at((lo[0] + hi[0]) // 2)
            lo, hi = (mid, hi) if mid[3] < n + 5 else (lo, mid)
        if lo[4] == 0 and hi[4] == 0:
            return [lo[:4], hi[:4]]
    raise AssertionError("crossover: no unambiguous draw in %d seeds" % DRAWS)


REDRAWN = {}        # per case: why the draws before the one kept were given up
