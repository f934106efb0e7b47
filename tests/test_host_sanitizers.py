"""The host reader, gzip decoders and writer (csrc/rd_host.cpp, rd_inflate.h, rd_pgzip.h) under AddressSanitizer + UBSan and under
ThreadSanitizer. CPU-only: nothing here touches a GPU or librd_hip.

tests/san/rd_host_san.cpp - a stand-alone program that calls every entry point of include/ribodetector_amd_host.h with heap buffers of
exactly the capacity it passes - is compiled together with rd_host.cpp twice (-fsanitize=address,undefined and -fsanitize=thread) into
pytest's temporary directory and run as child processes over manifests of commands. The sanitized code is never loaded into python.

Two properties per input: (1) no sanitizer report and exit status 0; (2) the child's result line - rc, byte count, CRC-32 of the output,
record count, CRC-32 of the record tables, error text - equals the line computed here from the product librd_host.so through ctypes
(same calls, same capacities), and for valid inputs the bytes are zlib's. The self-tests prove that each binary really is sanitized.

Wall time, measured on 8 CPUs with this module alone (194 s in all): building the two drivers 18 s (side by side, in the fixture);
AddressSanitizer + UBSan 125 s - reader 38, valid texts 29, libdeflate's texts 16, mutations 9, byte ranges and early close 9, feed reader 8,
writer 8, hand-built streams 4, framing and pigz-style streams 3, member index 1; ThreadSanitizer 50 s - parallel decoder 19, writer 15,
reader and early close 10, feed reader 5, two readers and a writer 2. About 9,000 commands run under ASan + UBSan, about 450 under TSan.
"""
import ctypes as C
import gzip
import os
import struct
import subprocess
import threading
import zlib

import numpy as np
import pytest

import deflate_corpus as D
from ribodetector_amd import _native as N
from ribodetector_amd import synth
from test_inflate import PAYLOADS, gunzip, member, pgunzip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SOURCES = [os.path.join(ROOT, "tests", "san", "rd_host_san.cpp"), os.path.join(ROOT, "ribodetector_amd", "csrc", "rd_host.cpp")]
BASE_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include")]
SAN_FLAGS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
CHILD_ENV = {"ASAN_OPTIONS": "abort_on_error=0:detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1",
             "TSAN_OPTIONS": "halt_on_error=1"}
JOBS = max(1, min(16, len(os.sched_getaffinity(0))))
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FEED_ERROR = "injected: the fed stream is damaged"
GZ_THREADS = "@gzthreads"             # in a case's environment: not a variable but a call of rd_host_set_gz_threads


# ---- building and running the driver ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def san(tmp_path_factory):
    """{'asan': path, 'tsan': path}: the driver built under each sanitizer. Skips only when a two-line program cannot be linked with
    the sanitizer's runtime (with the compiler's message); a driver that does not compile is a failure"""
    cxx = os.environ.get("CXX", "g++")
    d = tmp_path_factory.mktemp("san")
    probe = d / "probe.cpp"
    probe.write_text("#include <stdio.h>\nint main() { puts(\"ok\"); return 0; }\n")
    for kind, flags in SAN_FLAGS.items():
        r = subprocess.run([cxx] + BASE_FLAGS + flags + [str(probe), "-o", str(d / ("probe_" + kind))], capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("%s cannot link a program with %s: %s" % (cxx, " ".join(flags), r.stderr.strip()[-600:]))
    procs = {kind: subprocess.Popen([cxx] + BASE_FLAGS + flags + SOURCES + ["-o", str(d / ("rd_host_san_" + kind)), "-lz", "-ldl"],
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for kind, flags in SAN_FLAGS.items()}
    out = {}
    for kind, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, "the %s build of the driver failed:\n%s" % (kind, log[-4000:])
        out[kind] = str(d / ("rd_host_san_" + kind))
    return out


def child_env(extra=None):
    env = dict(os.environ)
    env.update(CHILD_ENV)
    for k in ("OMP_NUM_THREADS", "MAX_JOBS"):
        env[k] = str(min(16, int(env.get(k, "16") or 16)))
    for k in ("RD_HOST_ZLIB", "RD_GZ_THREADS", "RD_GZ_PARALLEL_MIN", "RD_GZ_SECTION", "RD_READER_MMAP"):
        env.pop(k, None)
    env.update(extra or {})
    return env


def run_child(binary, args, timeout, extra_env=None):
    return subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=child_env(extra_env))


class Case:
    """one command of the driver: tokens (without the label), the environment it runs in, and what is known about its answer"""

    def __init__(self, label, tokens, env=None, data=None, check=None):
        self.label, self.tokens, self.env, self.data, self.check = label, [str(t) for t in tokens], env or {}, data, check

    def line(self):
        return " ".join([self.tokens[0], self.label] + self.tokens[1:])


def run_cases(binary, cases, tmp, timeout=600, extra_env=None, jobs=JOBS):
    """the driver's result lines, one list per case (manifests of cases, run as `jobs` children at a time)"""
    jobs = max(1, min(jobs, len(cases)))
    shards = [[] for _ in range(jobs)]
    for k, c in enumerate(cases):
        shards[k % jobs].append(c)
    procs = []
    for s, shard in enumerate(shards):
        path = os.path.join(str(tmp), "manifest_%s_%d.txt" % (os.path.basename(binary), s))
        with open(path, "w") as fh:
            for c in shard:
                for k, v in c.env.items():
                    fh.write("gzthreads %s\n" % v if k == GZ_THREADS else "env %s %s\n" % (k, v))
                fh.write(c.line() + "\n")
                for k in c.env:
                    fh.write("gzthreads -1\n" if k == GZ_THREADS else "env %s\n" % k)
        procs.append(subprocess.Popen([binary, "manifest", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=child_env(extra_env)))
    got = {}
    for s, (p, shard) in enumerate(zip(procs, shards)):
        try:
            out, err = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0 and "Sanitizer" not in err, "manifest %d (%s ...): exit status %d\n%s\n%s" % (
            s, shard[0].label, p.returncode, out[-1500:], err[-6000:])
        lines = out.splitlines()
        want = sum(3 if c.tokens[0] == "pair" else 1 for c in shard)
        assert len(lines) == want, (len(lines), want, lines[-3:])
        at = 0
        for c in shard:
            k = 3 if c.tokens[0] == "pair" else 1
            got[c.label] = lines[at:at + k]
            at += k
    return [got[c.label] for c in cases]


# ---- the same commands on the product library, through ctypes ------------------------------------------------------------------------

def fmt_line(label, rc, nbytes, crc, nrec, err, extra=""):
    return '%s %d %d %08x %d "%s"%s' % (label, rc, nbytes, crc & 0xffffffff, nrec, err if rc < 0 else "", extra)


def last_error():
    return N.host_lib().rd_host_last_error().decode()


class Agg:
    def __init__(self):
        self.rc, self.nbytes, self.nrec, self.calls, self.c, self.tc, self.err = 0, 0, 0, 0, 0, 0, ""

    def line(self, label, extra=""):
        return fmt_line(label, self.rc, self.nbytes, self.c, self.nrec, self.err, " %08x%s" % (self.tc & 0xffffffff, extra))


def read_all(r, max_records, buf_cap, stop, a):
    L = N.host_lib()
    cap = buf_cap
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    rs, so, sl = np.empty(max_records + 1, dtype=np.int64), np.empty(max_records, dtype=np.int64), np.empty(max_records, dtype=np.int32)
    n, nb = C.c_int64(0), C.c_int64(0)
    while stop < 0 or a.calls < stop:
        rc = L.rd_reader_next(r, max_records, buf.ctypes.data, cap, rs.ctypes.data, so.ctypes.data, sl.ctypes.data, C.byref(n), C.byref(nb))
        a.calls += 1
        a.rc = rc
        if rc < 0:
            a.err = last_error()
            break
        if rc == 0 and n.value == 0:
            if nb.value <= cap:
                a.rc, a.err = -2, "driver: the reader delivers nothing and asks for no larger buffer"
                break
            cap = nb.value
            buf = np.empty(cap, dtype=np.uint8)
            continue
        k = n.value
        piece = buf[:nb.value].tobytes()
        a.c = zlib.crc32(piece, a.c)
        a.tc = zlib.crc32(sl[:k].tobytes(), zlib.crc32(so[:k].tobytes(), zlib.crc32(rs[:k + 1].tobytes(), a.tc)))
        a.nbytes += nb.value
        a.nrec += k
        if rc == 1:
            break


def p_gunzip(label, cap, path):
    rc, got, err = gunzip(path, int(cap))
    return [fmt_line(label, rc, len(got), zlib.crc32(got), 0, err)]


def p_pgunzip(label, threads, section, cap, path):
    rc, got, err, st = pgunzip(path, int(cap), int(threads), int(section))
    return [fmt_line(label, rc, len(got), zlib.crc32(got), 0, err, " used=%d dropped=%d fell_back=%d" % (st["used"], st["dropped"], st["fell_back"]))]


def p_read(label, fmt, max_records, buf_cap, stop, path, agg=None):
    L = N.host_lib()
    r, a = C.c_void_p(), agg or Agg()
    if L.rd_reader_open(path.encode(), int(fmt), C.byref(r)) != 0:
        a.rc, a.err = -1, last_error()
        return [a.line(label)]
    read_all(r, int(max_records), int(buf_cap), int(stop), a)
    L.rd_reader_close(r)
    return [a.line(label)]


def p_read_range(label, fmt, step, path, agg=None):
    L = N.host_lib()
    fmt, step, a, pb = int(fmt), int(step), agg or Agg(), path.encode()
    size, isgz, v = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    if L.rd_host_file_info(pb, C.byref(size), C.byref(isgz)) != 0:
        a.rc, a.err = -1, last_error()
        return [a.line(label)]
    cut = [0]
    for pos in range(step, size.value, step):
        if L.rd_host_find_record_start(pb, fmt, pos, C.byref(v)) != 0:
            a.rc, a.err = -1, last_error()
            return [a.line(label)]
        if v.value > cut[-1]:
            cut.append(v.value)
    if size.value > cut[-1]:
        cut.append(size.value)
    counted = shares = 0
    skip_ok = 1
    for lo, hi in zip(cut[:-1], cut[1:]):
        c, e, r = C.c_int64(0), C.c_int64(0), C.c_void_p()
        if L.rd_host_count_records(pb, fmt, lo, hi, C.byref(c)) != 0 or L.rd_host_skip_records(pb, fmt, lo, c.value, C.byref(e)) != 0 or \
                L.rd_reader_open_range(pb, fmt, lo, hi, C.byref(r)) != 0:
            a.rc, a.err = -1, last_error()
            break
        counted += c.value
        skip_ok &= int(e.value == hi)
        shares += 1
        read_all(r, 1000, 1 << 20, -1, a)
        L.rd_reader_close(r)
        if a.rc < 0:
            break
    return [a.line(label, " gzip=%d shares=%d counted=%d skip_ok=%d" % (isgz.value, shares, counted, skip_ok))]


def p_feed(label, variant, fmt, piece, path, agg=None):
    L = N.host_lib()
    piece, a, r = int(piece), agg or Agg(), C.c_void_p()
    data = open(path, "rb").read()
    assert L.rd_reader_open_feed(int(fmt), C.byref(r)) == 0
    abort_it = variant == "abort"
    if variant == "tail":
        L.rd_reader_set_flush_empty_tail(r, 1)
    res = [0]

    def feeder():
        rounds = 0
        while True:
            for off in range(0, len(data), piece):
                p = data[off:off + piece]
                rc = L.rd_reader_feed(r, p, len(p))
                if rc < 0:
                    res[0] = rc
                    return
            rounds += 1
            if not (abort_it and data and rounds < 64):
                break
        res[0] = L.rd_reader_feed_end(r, FEED_ERROR.encode() if variant == "error" else None)

    th = threading.Thread(target=feeder)
    th.start()
    read_all(r, 7 if abort_it else 1000, 1 << 20, 1 if abort_it else -1, a)
    if abort_it or a.rc != 1:                                                 # stopped before the end of the stream: wake the feeder, join it, then close
        L.rd_reader_feed_abort(r)
    th.join()
    L.rd_reader_close(r)
    return [a.line(label, " feeder=%d" % res[0] if abort_it else "")]


def p_index(label, grow, cap, path):
    L = N.host_lib()
    grow, cap = int(grow), int(cap)
    data = open(path, "rb").read()
    pos = avail = total = ob = c = 0
    ent = np.zeros((cap, 3), dtype=np.int64)
    n, consumed, outb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    while True:
        buf = np.frombuffer(data[pos:avail] + b"\0", dtype=np.uint8)          # (one byte more: an empty array has no address)
        rc = L.rd_host_gz_index(buf.ctypes.data, avail - pos, pos, ob, ent.ctypes.data, cap, C.byref(n), C.byref(consumed), C.byref(outb))
        if rc < 0:
            break
        c = zlib.crc32(ent[:n.value].tobytes(), c)
        total += n.value
        pos += consumed.value
        ob += outb.value
        if rc == 1:
            break
        if consumed.value > 0:
            continue
        if avail == len(data):
            break
        avail = min(len(data), avail + grow)
    return [fmt_line(label, rc, pos, c, total, last_error(), " out_bytes=%d" % ob)]


def write_inputs(prefix):
    txt = np.fromfile(prefix + ".txt", dtype=np.uint8)
    rs = np.fromfile(prefix + ".rs", dtype=np.int64)
    lab = np.fromfile(prefix + ".lab", dtype=np.int8)
    mem = np.fromfile(prefix + ".mem", dtype=np.uint8)
    return txt, rs, lab, mem


def selected(txt, rs, lab, want, lo, hi):
    b = txt.tobytes()
    return b"".join(b[rs[i]:rs[i + 1]] for i in range(lo, hi) if lab[i] == want)


def p_write(label, threads, want, eof_marker, prefix, out):
    L = N.host_lib()
    threads, want, eof_marker = int(threads), int(want), int(eof_marker)
    txt, rs, lab, mem = write_inputs(prefix)
    n = len(lab)
    n1, n2 = n // 3, 2 * n // 3
    L.rd_host_set_threads(threads)
    w = C.c_void_p()
    if L.rd_writer_open(out.encode(), C.byref(w)) != 0:
        return [fmt_line(label, -1, 0, 0, 0, last_error())]
    wt = L.rd_writer_threads(w)
    text = np.frombuffer(selected(txt, rs, lab, want, n1, n2) + b"\0", dtype=np.uint8)
    tb = txt if len(txt) else np.zeros(1, dtype=np.uint8)
    lb = lab if n else np.zeros(1, dtype=np.int8)
    state = [0, ""]

    def step(rc):
        if rc != 0 and state[0] == 0:
            state[0], state[1] = rc, last_error()
    step(L.rd_writer_write_selected(w, tb.ctypes.data, rs.ctypes.data, n1, lb.ctypes.data, want))
    step(L.rd_writer_write_text(w, text.ctypes.data, len(text) - 1))
    if out.endswith("gz") and len(mem):
        step(L.rd_writer_write_members(w, mem.ctypes.data, len(mem)))
    step(L.rd_writer_write_selected(w, tb.ctypes.data, rs[n2:].ctypes.data, n - n2, lb[n2:].ctypes.data if n else lb.ctypes.data, want))
    step(L.rd_writer_set_eof_marker(w, eof_marker))
    step(L.rd_writer_close(w))
    L.rd_host_set_threads(0)
    res = open(out, "rb").read()
    return [fmt_line(label, state[0], len(res), zlib.crc32(res), int((lab == want).sum()), state[1], " threads=%d" % wt)]


def p_pair(label, a, b, prefix, out):
    return p_read(label + ".a", -1, 1000, 1 << 20, -1, a) + p_read(label + ".b", -1, 7, 4096, -1, b) + p_write(label + ".w", 2, 0, 1, prefix, out)


PRODUCT = {"gunzip": p_gunzip, "pgunzip": p_pgunzip, "read": p_read, "read-range": p_read_range, "feed": p_feed, "index": p_index,
           "write": p_write, "pair": p_pair}


def product_lines(cases):
    """the lines the product library answers the same commands with (its own output files: '<out>' -> '<out>.product')"""
    out = []
    for c in cases:
        env = {k: v for k, v in c.env.items() if k != GZ_THREADS}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        N.host_lib().rd_host_set_gz_threads(int(c.env.get(GZ_THREADS, -1)))
        try:
            t = list(c.tokens)
            if t[0] in ("write", "pair"):
                t[-1] = product_path(t[-1])
            out.append(PRODUCT[t[0]](c.label, *t[1:]))
        finally:
            N.host_lib().rd_host_set_gz_threads(-1)
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
    return out


def product_path(out):
    d, b = os.path.split(out)
    return os.path.join(d, "product." + b)


def fields(line):
    """(label, rc, nbytes, crc, nrec, error text, the rest) of a result line"""
    head, err, rest = line.split('"', 2)
    label, rc, nbytes, crc, nrec = head.split()
    return label, int(rc), int(nbytes), int(crc, 16), int(nrec), err, rest.strip()


def differential(binary, cases, tmp, timeout=600, extra_env=None, jobs=JOBS, same=lambda got, want: got == want):
    """run the cases under the sanitizer and on the product library: the same lines; for a case that knows its text (c.data) the bytes
    are that text's - by length and zlib's CRC-32. Returns (driver lines, product lines)"""
    want = product_lines(cases)
    got = run_cases(binary, cases, tmp, timeout, extra_env, jobs)
    bad = [(c.line(), g, w) for c, g, w in zip(cases, got, want) if not same(g, w)]
    assert not bad, "%d of %d result lines differ from the product library's; the first:\n%r" % (len(bad), len(cases), bad[:3])
    for c, g in zip(cases, got):
        if c.data is not None:
            _, rc, nbytes, crc, _, err, _ = fields(g[0])
            assert rc >= 0 and nbytes == len(c.data) and crc == zlib.crc32(c.data), (c.line(), g)
        if c.check is not None:
            c.check(fields(g[0]))
    return got, want


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

class Files:
    """inputs written once into one directory; names carry no blanks"""

    def __init__(self, d):
        self.d, self.k = str(d), 0

    def put(self, name, blob):
        self.k += 1
        p = os.path.join(self.d, "%05d_%s" % (self.k, name))
        with open(p, "wb") as fh:
            fh.write(blob)
        return p


def decoder_cases(files, label, blob, data=None, cap=None, threads=4, section=32768, check=None):
    """one gzip file through both decoders"""
    p = files.put(label + ".gz", blob)
    cap = cap if cap is not None else len(data) + 16
    return [Case(label + ".seq", ["gunzip", cap, p], data=data),
            Case(label + ".par", ["pgunzip", threads, section, cap, p], data=data, check=check)]


def trimmed(name):
    return D.text(name)[:1 << 20]


def _used4(f):
    st = dict(kv.split("=") for kv in f[6].split())
    assert int(st["used"]) >= 4 and int(st["fell_back"]) == 0, f


def valid_text_cases(files, libdeflate):
    """deflate_corpus.TEXTS x ENCODERS at <= 1 MB of text each (libdeflate's encoders are a leg of their own)"""
    import test_inflate_corpus as TC
    out = []
    for name in D.TEXTS:
        data = trimmed(name)
        for enc, (f, needs_ld) in D.ENCODERS.items():
            if needs_ld != libdeflate:
                continue
            # several sections really decoded with an unknown window - asserted for zlib's and the pigz-style streams, whose blocks are
            # shorter than a section; libdeflate's blocks outgrow it (KNOWN_DROPPED, and at 1 MB of text too few sections remain:
            # test_host_decoders_on_every_encoder asserts those at full size)
            sections = name in D.FASTQ and enc in TC.PARALLEL_ENCODERS and not needs_ld
            out += decoder_cases(files, "text.%s.%s" % (name, enc), D.gzip_member(f(data), data, flags=8), data, check=_used4 if sections else None)
    return out


def hand_built_cases(files):
    out = []
    for name in D.VALID:
        for how, (raw, data) in (("alone", D.valid(name)), ("spliced", D.spliced(name, 65536, 65536))):
            out += decoder_cases(files, "valid.%s.%s" % (name, how), D.gzip_member(raw, data), data)
    out += decoder_cases(files, "valid.empty_dynamic", D.gzip_member(D.valid_empty_dynamic(), b""), b"")
    for name in D.INVALID:
        raw, lenient = D.invalid(name)
        out += decoder_cases(files, "invalid.%s.alone" % name, D.gzip_member(raw, lenient), cap=len(lenient) + 1024, check=_rejected)
    for name in D.SPLICEABLE_INVALID:
        raw, lenient = D.spliced(name, 65536, 65536)
        out += decoder_cases(files, "invalid.%s.spliced" % name, D.gzip_member(raw, lenient), cap=len(lenient) + 1024, check=_rejected)
    return out


def _rejected(f):
    assert f[1] < 0 and f[5], f


def framing_cases(files):
    out = []
    fq = PAYLOADS["fastq"]
    for flags in range(32):                                                    # FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT in every combination
        data = fq[flags * 1000:flags * 1000 + 100000]
        out += decoder_cases(files, "flags.%02d" % flags, member(data, 5, flags=flags), data)
    # found by this module: the parallel decoder handed an EMPTY section to memcpy with a null source (UBSan: rd_pgzip.h, read())
    out += decoder_cases(files, "finding.empty_member", member(b"", 6), b"", threads=4, section=65536)
    ill = trimmed("illumina")
    out += decoder_cases(files, "bgzf.zlib", D.bgzf(ill, D.zlib_raw), ill)
    out += decoder_cases(files, "sized.rd", D.sized_member(D.zlib_raw(ill), ill) + D.sized_member(D.zlib_raw(b""), b""), ill)
    assert len(D.zlib_raw(ill)) > 65536                                       # (the 'RD' subfield: a member too long for BGZF's 16 bits)
    a, b, c = fq[:300000], b"second member\n" * 1000, PAYLOADS["random"][:70000]
    blob = member(a, 5, flags=4 | 8 | 16 | 2) + member(b"", 6) + member(b, 9, flags=8) + bytes(37) + member(c, 1) + bytes(512)
    out += decoder_cases(files, "multi.padded", blob, a + b + c, cap=len(a + b + c) + 1)
    out += decoder_cases(files, "bgzf.padded", D.bgzf(ill, D.zlib_raw) + bytes(100) + member(b, 6), ill + b)
    return out


def pigz_cases(files):
    """the flushed streams of test_sequential_decoder_on_pigz_streams_larger_than_its_input_buffer, shortened to the least that still
    spans two refills of the decoder's 1 MiB input buffer"""
    arena, off, _ = synth.reads_numpy(50000, 100, seed=9)
    src = os.path.join(files.d, "pigz_src.fq")
    synth.write_fastq_realistic(src, arena, off, 1, seed=9)
    data = open(src, "rb").read()
    out = []
    for chunk in (300000, 131072, 70001):
        p = os.path.join(files.d, "pigz_%d.fq.gz" % chunk)
        synth.pgzip_file(src, p, level=6, chunk=chunk)
        assert os.path.getsize(p) > 2 * (1 << 20) + 65536                    # more than two input buffers
        out += [Case("pigz.%d.seq" % chunk, ["gunzip", len(data) + 16, p], data=data),
                Case("pigz.%d.par" % chunk, ["pgunzip", 4, 65536, len(data) + 16, p], data=data, check=_used4)]
    return out


def mutation_cases(files):
    """the loops of test_random_deflate_streams_never_crash and test_parallel_decoder_fuzz_never_crashes (same seeds, same counts), and
    one member cut at 64 evenly spaced places"""
    out = []
    rng = np.random.default_rng(9)
    for i in range(300):
        body = rng.integers(0, 256, int(rng.integers(1, 4000)), dtype=np.uint8).tobytes()
        out += decoder_cases(files, "fuzz.body.%d" % i, b"\x1f\x8b\x08\0\0\0\0\0\x02\xff" + body, cap=1 << 20, threads=3, section=20000)
    good = member(PAYLOADS["fastq"][:100000], 6)
    for i in range(300):
        x = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            x[int(rng.integers(10, len(x)))] = int(rng.integers(0, 256))
        out += decoder_cases(files, "fuzz.mutated.%d" % i, bytes(x), cap=1 << 20, threads=3, section=20000)
    out += parallel_fuzz_cases(files, 150)
    for k in range(64):
        cut = (k * len(good)) // 64
        out += decoder_cases(files, "cut.%d" % cut, good[:cut], cap=1 << 20, threads=3, section=20000)
    return out


def parallel_fuzz_cases(files, count):
    out = []
    rng = np.random.default_rng(10)
    good = member(PAYLOADS["fastq"][:400000], 6)
    for i in range(count):
        x = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            x[int(rng.integers(10, len(x)))] = int(rng.integers(0, 256))
        out += decoder_cases(files, "pfuzz.%d" % i, bytes(x), cap=1 << 21, threads=3, section=20000)
    return out


MALFORMED_GOOD = b"".join(b"@r%d\nACGT\n+\nFFFF\n" % i for i in range(50))
MALFORMED = {"header": MALFORMED_GOOD + b"r50\nAC\n+\nFF\n" + MALFORMED_GOOD, "truncated": MALFORMED_GOOD + b"@x\nAC\n+\n",
             "truncated_one_line": MALFORMED_GOOD + b"@x", "four_blank_lines": MALFORMED_GOOD + b"\n\n\n\n", "blank_header_crlf": b"\r\n" + MALFORMED_GOOD}


_TEXTS = []


def reader_texts(golden):
    if not _TEXTS:
        _TEXTS.extend(_reader_texts(golden))
    return _TEXTS


def _reader_texts(golden):
    """(name, format, text): 100 fuzzed FASTQ and 60 fuzzed FASTA files of tests/test_gpu_device_reader.py's generators (its record
    counts), its five malformed FASTQ files and the texts the reference's parser was run on"""
    from test_gpu_device_reader import _fuzz_fasta, _fuzz_text
    out = []
    rng = np.random.default_rng(11)
    for i in range(100):
        out.append(("fq%d" % i, 0, _fuzz_text(rng, int(rng.choice([0, 1, 2, 3, 5, 17, 100, 400, 1500])))))
    rng = np.random.default_rng(12)
    for i in range(60):
        out.append(("fa%d" % i, 1, _fuzz_fasta(rng, int(rng.choice([0, 1, 2, 3, 5, 17, 100, 400])))))
    out += [("bad_" + k, 0, v) for k, v in MALFORMED.items()]
    g = golden.json("parser")
    out += [("ref_fastq", 0, g["fastq_text"].encode()), ("ref_fasta", 1, g["fasta_text"].encode())]
    return out


PARALLEL_READER = {"RD_GZ_THREADS": "3", "RD_GZ_PARALLEL_MIN": "0", "RD_GZ_SECTION": "50000"}
SET_GZ_THREADS = {GZ_THREADS: "3", "RD_GZ_PARALLEL_MIN": "0", "RD_GZ_SECTION": "50000"}   # (parallel where the machine has >= 4 cores)
READER_MODES = (("mmap", False, {}), ("nommap", False, {"RD_READER_MMAP": "0"}), ("gzseq", True, {"RD_GZ_THREADS": "0"}), ("gzpar", True, PARALLEL_READER))


def reader_cases(files, golden):
    out = []
    for name, fmt, text in reader_texts(golden):
        ext = ".fasta" if fmt else ".fastq"
        plain, packed = files.put(name + ext, text), files.put(name + ext + ".gz", gzip.compress(text, 6))
        for mode, gz, env in READER_MODES:
            for max_records in (1, 7, 1000):
                for buf_cap in (64, 4096, 1 << 20):
                    out.append(Case("read.%s.%s.%d.%d" % (name, mode, max_records, buf_cap), ["read", fmt, max_records, buf_cap, -1, packed if gz else plain], env=env))
    return out


def big_fastq(n=1500, seed=21):
    arena, off, _ = synth.reads_numpy(n, (60, 150), seed=seed)
    b = arena.tobytes()
    return b"".join(b"@big.%d\n%s\n+\n%s\n" % (i, b[off[i]:off[i + 1]], b"F" * int(off[i + 1] - off[i])) for i in range(n))


def write_tables(files, name, n, seed=5):
    """PREFIX.txt / .rs / .lab / .mem for the driver's write command: n ragged records (0 .. 900 bytes), labels in {0, 1, -1}, and members
    'made elsewhere'. Returns (prefix, text of the members)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 901, n)
    rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    txt = rng.integers(33, 127, int(rs[-1]), dtype=np.uint8)
    if n:
        txt[rs[1:][lens > 0] - 1] = 10
    lab = rng.choice(np.array([0, 1, -1], dtype=np.int8), n, p=[0.6, 0.3, 0.1])
    extra = D.text("illumina")[:150000]
    mem = b"".join(D.sized_member(D.zlib_raw(extra[i:i + 60000]), extra[i:i + 60000]) for i in range(0, len(extra), 60000))
    prefix = os.path.join(files.d, name)
    for ext, arr in ((".txt", txt), (".rs", rs), (".lab", lab), (".mem", np.frombuffer(mem, dtype=np.uint8))):
        arr.tofile(prefix + ext)
    return prefix, extra


def check_written(prefix, extra, want, eof_marker, path):
    """the file the writer made holds the Python join of the selected records (and the members' text where they were appended)"""
    txt, rs, lab, mem = write_inputs(prefix)
    n = len(lab)
    n1, n2 = n // 3, 2 * n // 3
    a, b, c = selected(txt, rs, lab, want, 0, n1), selected(txt, rs, lab, want, n1, n2), selected(txt, rs, lab, want, n2, n)
    blob = open(path, "rb").read()
    if path.endswith("gz"):
        assert gzip.decompress(blob) == a + b + extra + c, path
        assert blob.endswith(EOF_MARKER) == bool(eof_marker), path
    else:
        assert blob == a + b + c, path


def write_cases(files, tag, threads_list, n=30000):
    """[(case, check)]: 30,000 ragged records, every `want`, the end-of-file marker on and off, a plain output, an empty selection
    (want = 5) and an empty chunk"""
    prefix, extra = write_tables(files, "tables_%s" % tag, n)
    empty, _ = write_tables(files, "tables_%s_empty" % tag, 0)
    out = []
    for threads in threads_list:
        for want in (0, 1, -1, 5):
            for eof in ((1, 0) if want in (0, 5) else (1,)):
                path = os.path.join(files.d, "out_%s_%d_%d_%d.fq.gz" % (tag, threads, want + 1, eof))
                out.append((Case("write.%s.%d.%d.%d" % (tag, threads, want, eof), ["write", threads, want, eof, prefix, path]), (prefix, extra, want, eof, path)))
        path = os.path.join(files.d, "out_%s_%d_plain.fq" % (tag, threads))
        out.append((Case("write.%s.%d.plain" % (tag, threads), ["write", threads, 0, 1, prefix, path]), (prefix, b"", 0, 1, path)))
        path = os.path.join(files.d, "out_%s_%d_empty.fq.gz" % (tag, threads))
        out.append((Case("write.%s.%d.empty" % (tag, threads), ["write", threads, 0, 0, empty, path]), (empty, extra, 0, 0, path)))
    return out


def run_write_legs(binary, files, tmp, threads_list, n, tag):
    """the write command once with zlib (RD_HOST_ZLIB=1) and once with libdeflate (skipped by name where it cannot be loaded). The
    compressed bytes are compared with the product's only where both use the same compressor"""
    ran = []
    for leg, env in (("zlib", {"RD_HOST_ZLIB": "1"}), ("libdeflate", {})):
        if leg == "libdeflate" and D.libdeflate() is None:
            continue
        pairs = write_cases(files, "%s_%s" % (tag, leg), threads_list, n)
        cases = [c for c, _ in pairs]
        same_backend = (leg == "zlib") == (os.environ.get("RD_HOST_ZLIB", "")[:1] == "1")

        def same(got, want, exact=same_backend):
            g, w = fields(got[-1]), fields(want[-1])
            return got[:-1] == want[:-1] and (g == w if exact or not g[0].split(".")[-1].isdigit() else (g[:2] + g[4:]) == (w[:2] + w[4:]))
        differential(binary, cases, tmp, extra_env=env, same=same, jobs=4)
        for c, args in pairs:
            check_written(*args)
            check_written(*args[:-1], product_path(args[-1]))
        ran.append(leg)
    return ran


# ---- the tests -----------------------------------------------------------------------------------------------------------------------

def test_driver_calls_every_entry_point_of_the_header():
    """every RD_API function of include/ribodetector_amd_host.h is called in tests/san/rd_host_san.cpp"""
    import re
    header = open(os.path.join(ROOT, "include", "ribodetector_amd_host.h")).read()
    names = re.findall(r"RD_API[^;(]*?\b(rd_\w+)\(", header)
    assert len(names) == len(set(names)) == len(N.HOST_SYMBOLS) and set(names) == set(N.HOST_SYMBOLS), sorted(set(names) ^ set(N.HOST_SYMBOLS))
    driver = open(SOURCES[0]).read()
    assert [n for n in names if not re.search(r"\b%s\(" % n, driver)] == []


def test_selftest_heap_overrun_is_reported(san):
    """a one-byte overrun of the driver's own buffer: the ASan build must exit non-zero and name AddressSanitizer"""
    r = run_child(san["asan"], ["selftest-heap"], 60)
    assert r.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_selftest_race_is_reported(san):
    """two driver threads incrementing one plain int: the TSan build must exit non-zero and name ThreadSanitizer"""
    r = run_child(san["tsan"], ["selftest-race"], 60)
    assert r.returncode != 0 and "ThreadSanitizer: data race" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("san_inputs"))


def test_asan_decoders_on_valid_texts(san, files, tmp_path):
    differential(san["asan"], valid_text_cases(files, libdeflate=False), tmp_path)


def test_asan_decoders_on_libdeflate_texts(san, files, tmp_path):
    if D.libdeflate() is None:
        pytest.skip(D.LIBDEFLATE_MISSING)
    differential(san["asan"], valid_text_cases(files, libdeflate=True), tmp_path)


def test_asan_decoders_on_hand_built_streams(san, files, tmp_path):
    """every VALID and INVALID stream of the corpus, alone and spliced between 64 KiB of zlib's blocks: the invalid ones are where a
    decoder reads past a table or copies from before its window"""
    differential(san["asan"], hand_built_cases(files), tmp_path)


def test_asan_decoders_on_framing(san, files, tmp_path):
    differential(san["asan"], framing_cases(files) + pigz_cases(files), tmp_path)


def test_asan_decoders_on_mutations(san, files, tmp_path):
    differential(san["asan"], mutation_cases(files), tmp_path)


def test_asan_reader(san, files, tmp_path, golden):
    """fuzzed, malformed and reference-made FASTQ / FASTA: mapped, buffered, and gzip-compressed through both decoders, with batches of
    1, 7 and 1000 records and buffers of 64 bytes (every record: grow and retry), 4 KiB and 1 MiB"""
    cases = reader_cases(files, golden)
    got, _ = differential(san["asan"], cases, tmp_path)
    by = {c.label: fields(g[0]) for c, g in zip(cases, got)}
    for name, fmt, text in reader_texts(golden):
        ref = by["read.%s.mmap.1000.%d" % (name, 1 << 20)]
        for mode, _, _ in READER_MODES:                                       # the same records whatever the path, batch and buffer
            for max_records in (1, 7, 1000):
                for buf_cap in (64, 4096, 1 << 20):
                    f = by["read.%s.%s.%d.%d" % (name, mode, max_records, buf_cap)]
                    assert (f[1] < 0) == (ref[1] < 0) and f[5] == ref[5] and (f[1] < 0 or f[2:5] == ref[2:5]), (name, mode, max_records, buf_cap, f, ref)


def range_files(files):
    fq = big_fastq(1500)
    assert len(fq) > 200000
    arena, off, lens = synth.reads_numpy(3000, (40, 150), seed=5)             # 60-column FASTA (test_fasta_large_file_and_what_stays_with_the_host)
    fa = b"".join(b">read%d\n" % i + b"\n".join(arena[off[i]:off[i] + lens[i]].tobytes()[o:o + 60] for o in range(0, int(lens[i]), 60)) + b"\n"
                  for i in range(len(lens)))
    return files.put("range.fastq", fq), fq, files.put("range.fasta", fa), fa


def test_asan_read_range_and_early_close(san, files, tmp_path):
    """cuts at every 997th byte: the shares' records are the whole file's; readers closed after 0, 1 and 3 calls"""
    pq, fq, pa, fa = range_files(files)
    cases = [Case("range.fastq", ["read-range", 0, 997, pq]), Case("range.fasta", ["read-range", 1, 997, pa]),
             Case("whole.fastq", ["read", 0, 1000, 1 << 20, -1, pq]), Case("whole.fasta", ["read", 1, 1000, 1 << 20, -1, pa])]
    gz = files.put("early.fastq.gz", gzip.compress(big_fastq(20000, seed=22), 1))
    for k in (0, 1, 3):
        cases += [Case("early.plain.%d" % k, ["read", 0, 100, 1 << 20, k, pq], env={"RD_READER_MMAP": "0"}),
                  Case("early.gzseq.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env={"RD_GZ_THREADS": "0"}),
                  Case("early.gzpar.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env=PARALLEL_READER),
                  Case("early.gzset.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env=SET_GZ_THREADS)]
    got, _ = differential(san["asan"], cases, tmp_path)
    f = [fields(g[0]) for g in got]
    for rng_, whole, text in ((f[0], f[2], fq), (f[1], f[3], None)):
        assert rng_[1] == 1 and rng_[2:5] == whole[2:5], (rng_, whole)          # the concatenated shares == the whole file
        st = dict(kv.split("=") for kv in rng_[6].split()[1:])
        assert int(st["shares"]) > 100 and int(st["counted"]) == rng_[4] and st["skip_ok"] == "1", rng_
        if text is not None:
            assert rng_[2] == len(text) and rng_[3] == zlib.crc32(text)


def feed_cases(files, golden, pieces, count):
    out = []
    texts = [t for t in reader_texts(golden) if len(t[2]) < 30000][:count] + [t for t in reader_texts(golden) if t[0].startswith(("bad_", "ref_"))]
    for name, fmt, text in texts:
        p = files.put("feed_" + name, text)
        for piece in pieces:
            if piece == 1 and len(text) > 6000:
                continue
            for variant in ("end", "error", "tail", "abort"):
                out.append(Case("feed.%s.%s.%d" % (name, variant, piece), ["feed", variant, fmt, piece, p]))
            out.append(Case("feedref.%s.%d" % (name, piece), ["read", fmt, 1000, 1 << 20, -1, p], env={"RD_READER_MMAP": "0"}))
    return out


def check_feed(cases, got):
    by = {c.label: fields(g[0]) for c, g in zip(cases, got)}
    for label, f in by.items():
        if label.startswith("feed.") and ".end." in label:                    # a fed stream parses like a file of those bytes
            ref = by["feedref." + label.split(".")[1] + "." + label.split(".")[-1]]
            assert f[1:6] == ref[1:6] and f[6].split()[0] == ref[6].split()[0], (label, f, ref)
        if label.startswith("feed.") and ".error." in label:                  # the feeder's error comes after the records before it
            ref = by["feedref." + label.split(".")[1] + "." + label.split(".")[-1]]
            assert f[1] < 0 and (f[5] == FEED_ERROR or f[5] == ref[5]), (label, f, ref)


def test_asan_feed_reader(san, files, tmp_path, golden):
    cases = feed_cases(files, golden, (1, 7, 4096), 40)
    got, _ = differential(san["asan"], cases, tmp_path)
    check_feed(cases, got)


def index_files(files):
    text = D.text("illumina")[:40000]
    blob = D.bgzf(text, D.zlib_raw, block=3000)
    lying = bytearray(blob)
    at = struct.unpack_from("<H", blob, 16)[0] + 1                               # the second member's 'BC' size
    lying[at + 16:at + 18] = b"\xff\xff"
    small = bytearray(blob)
    small[at + 16:at + 18] = b"\x05\x00"
    third = at + struct.unpack_from("<H", blob, at + 16)[0] + 1
    return {"bgzf": blob, "lying_size": bytes(lying), "size_too_small": bytes(small), "cut_in_header": blob[:third + 9],
            "unsized_tail": blob + member(b"tail\n" * 100, 6)}, text


def test_asan_gz_index(san, files, tmp_path):
    """rd_host_gz_index on prefixes growing by 1, 17 and 4096 bytes with room for 1, 3 and 4096 entries"""
    blobs, text = index_files(files)
    cases = []
    for name, blob in blobs.items():
        p = files.put("index_" + name + ".gz", blob)
        for grow in (1, 17, 4096):
            for cap in (1, 3, 4096):
                cases.append(Case("index.%s.%d.%d" % (name, grow, cap), ["index", grow, cap, p]))
    got, _ = differential(san["asan"], cases, tmp_path)
    by = {c.label: fields(g[0]) for c, g in zip(cases, got)}
    for name in blobs:                                                        # however the bytes arrive: the same members
        ref = by["index.%s.4096.4096" % name]
        for grow in (1, 17, 4096):
            for cap in (1, 3, 4096):
                f = by["index.%s.%d.%d" % (name, grow, cap)]                  # (an error keeps the members in front of it to itself)
                assert (f[1], f[5]) == (ref[1], ref[5]) and (ref[1] < 0 or f[1:] == ref[1:]), (name, grow, cap, f, ref)
    whole = by["index.bgzf.4096.4096"]
    assert whole[1] == 0 and whole[2] == len(blobs["bgzf"]) and whole[4] == -(-len(text) // 3000) and whole[6] == "out_bytes=%d" % len(text)
    assert by["index.unsized_tail.1.1"][1] == 1 and by["index.unsized_tail.1.1"][2] == len(blobs["bgzf"])
    assert by["index.size_too_small.17.3"][1] < 0 and "too small" in by["index.size_too_small.17.3"][5]
    assert by["index.cut_in_header.1.3"][1] == 0 and by["index.cut_in_header.1.3"][4] == 2


def test_asan_writer(san, files, tmp_path):
    ran = run_write_legs(san["asan"], files, tmp_path, (1, 3), 30000, "asan")
    assert "zlib" in ran


# ---- ThreadSanitizer: the same commands on a smaller set ------------------------------------------------------------------------------

def test_tsan_parallel_decoder(san, files, tmp_path):
    data = PAYLOADS["fastq"]
    good = files.put("tsan_good.gz", member(data, 5))
    rep = b"@read\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" * 400000
    repz = files.put("tsan_rep.gz", member(rep, 6))

    def fell_back(f):
        assert "fell_back=1" in f[6], f
    cases = []
    for threads, section in ((2, 16384), (3, 20000), (8, 65536)):
        cases.append(Case("tsan.good.%d" % threads, ["pgunzip", threads, section, len(data) + 16, good], data=data, check=_used4 if threads == 8 else None))
        cases.append(Case("tsan.rep.%d" % threads, ["pgunzip", threads, section, len(rep) + 16, repz], data=rep))
    # sections of <= 64 KiB never reach the decoder's bound on this text (16 M symbols per section; tried up to 170 MB of it): the
    # sequential decoder takes over at the section size of test_parallel_decoder_bounds_its_buffers_on_extremely_compressible_text
    cases.append(Case("tsan.rep.fallback", ["pgunzip", 4, 131072, len(rep) + 16, repz], data=rep, check=fell_back))
    fuzz = parallel_fuzz_cases(files, 30)[1::2]
    for threads, section in ((2, 16384), (3, 20000), (8, 65536)):
        for c in fuzz:
            cases.append(Case("tsan.%s.%d" % (c.label, threads), ["pgunzip", threads, section] + c.tokens[3:]))
    differential(san["tsan"], cases, tmp_path)


def test_tsan_reader_and_early_close(san, files, tmp_path):
    gz = files.put("tsan_reader.fastq.gz", gzip.compress(big_fastq(20000, seed=23), 1))
    cases = [Case("tsan.read.gzpar", ["read", 0, 1000, 1 << 20, -1, gz], env=PARALLEL_READER),
             Case("tsan.read.gzseq", ["read", 0, 1000, 1 << 20, -1, gz], env={"RD_GZ_THREADS": "0"})]
    for k in (0, 1, 3):
        cases += [Case("tsan.early.gzpar.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env=PARALLEL_READER),
                  Case("tsan.early.gzseq.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env={"RD_GZ_THREADS": "0"}),
                  Case("tsan.early.gzset.%d" % k, ["read", 0, 100, 1 << 20, k, gz], env=SET_GZ_THREADS),
                  Case("tsan.early.plain.%d" % k, ["read", 0, 100, 1 << 20, k, range_files(files)[0]], env={"RD_READER_MMAP": "0"})]
    # the entry points without threads of their own, so that the ThreadSanitizer build has run the whole header too
    pq, fq, pa, fa = range_files(files)
    bg = files.put("tsan_index.gz", index_files(files)[0]["bgzf"])
    cases += [Case("tsan.gunzip", ["gunzip", len(fq) + 16, files.put("tsan_gunzip.gz", member(fq, 6))], data=fq),
              Case("tsan.range.fastq", ["read-range", 0, 9973, pq]), Case("tsan.range.fasta", ["read-range", 1, 9973, pa]),
              Case("tsan.index", ["index", 4096, 3, bg])]
    got, _ = differential(san["tsan"], cases, tmp_path)
    a, b = fields(got[0][0]), fields(got[1][0])
    assert a[1] == 1 and a[4] == 20000 and a[1:] == b[1:]


def test_tsan_feed_reader(san, files, tmp_path, golden):
    cases = feed_cases(files, golden, (1, 7, 4096), 12)
    got, _ = differential(san["tsan"], cases, tmp_path)
    check_feed(cases, got)


def test_tsan_writer(san, files, tmp_path):
    ran = run_write_legs(san["tsan"], files, tmp_path, (1, 2, 8), 30000, "tsan")
    assert "zlib" in ran


def test_tsan_two_readers_and_a_writer_in_one_process(san, files, tmp_path):
    """the CLI's paired-end run: two readers and a writer at once, each in its own thread - one of the readers on a damaged file, so
    that two threads set their error texts at the same time. Found by this test: rd_host_set_threads (the writer's thread) wrote the
    plain int that rd_reader_open (a reader's thread) read through usable_threads() - a data race; the two settings are atomics now"""
    blob = gzip.compress(big_fastq(8000, seed=24), 1)
    a = files.put("pair_a.fastq.gz", blob)
    b = files.put("pair_b.fastq.gz", blob[:len(blob) * 2 // 3])
    c = files.put("pair_c.fastq", MALFORMED["header"])
    prefix, extra = write_tables(files, "tables_pair", 6000)
    cases = [Case("pair.gz", ["pair", a, b, prefix, os.path.join(files.d, "pair_out1.fq.gz")], env=PARALLEL_READER),
             Case("pair.bad", ["pair", b, c, prefix, os.path.join(files.d, "pair_out2.fq.gz")], env={"RD_GZ_THREADS": "0"})]
    got, _ = differential(san["tsan"], cases, tmp_path, jobs=1)
    assert fields(got[0][0])[1] == 1 and "ended before the end-of-stream marker" in fields(got[0][1])[5]
    assert "ended before" in fields(got[1][0])[5] and "does not start with '@'" in fields(got[1][1])[5]
    for k in (1, 2):
        check_written(prefix, extra, 0, 1, os.path.join(files.d, "pair_out%d.fq.gz" % k))
