// rd_host_san - a stand-alone driver for the whole C ABI of include/ribodetector_amd_host.h, made to be compiled TOGETHER with
// ribodetector_amd/csrc/rd_host.cpp under a sanitizer (tests/test_host_sanitizers.py builds it with -fsanitize=address,undefined and
// with -fsanitize=thread):
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -pthread -Iinclude tests/san/rd_host_san.cpp ribodetector_amd/csrc/rd_host.cpp -lz -ldl
//
// Every buffer handed to the library is a heap allocation of exactly the size passed as its capacity, so that an overrun of one byte
// lands in a redzone. Every call prints ONE result line
//
//     label rc nbytes crc32(output) n_records "last_error" [crc32(rec_start / seq_off / seq_len)] [key=value ...]
//
// which the test compares with the line it computes from the product library (librd_host.so through ctypes).
//
// By hand, on a file a user reports (see tools/README.md):
//     rd_host_san gunzip FILE.gz ...              rd_host_san pgunzip THREADS SECTION FILE.gz ...
//     rd_host_san read FORMAT MAX_RECORDS BUF_CAP FILE ...        (FORMAT: 0 FASTQ, 1 FASTA, -1 by extension)
//     rd_host_san read-close-early K FILE ...     rd_host_san read-range STEP FILE ...
//     rd_host_san feed PIECE_BYTES FILE ...       rd_host_san index FILE.gz ...
//     rd_host_san write THREADS PREFIX OUT        rd_host_san manifest FILE     (one command per line, see run_line)
//     rd_host_san selftest-heap | selftest-race   (a deliberate one-byte overrun / data race IN THE DRIVER: proves the build is sanitized)
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "ribodetector_amd_host.h"

namespace {

std::string fmt(const char *f, ...) {
    char b[2048];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}

uint32_t crc(uint32_t c, const void *p, size_t n) {
    const uint8_t *q = (const uint8_t *)p;
    while (n) {   // (zlib takes 32-bit lengths)
        const size_t k = std::min<size_t>(n, 1u << 30);
        c = (uint32_t)crc32(c, q, (uInt)k);
        q += k;
        n -= k;
    }
    return c;
}

// a whole file in a heap block of exactly its size (nullptr: cannot be read)
struct Blob {
    uint8_t *p = nullptr;
    int64_t n = 0;
    bool ok = false;
    explicit Blob(const std::string &path) {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return;
        fseek(f, 0, SEEK_END);
        n = (int64_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        p = new uint8_t[(size_t)n];
        ok = (int64_t)fread(p, 1, (size_t)n, f) == n;
        fclose(f);
    }
    ~Blob() { delete[] p; }
    Blob(const Blob &) = delete;
    Blob &operator=(const Blob &) = delete;
};

std::string line(const std::string &label, int rc, int64_t nbytes, uint32_t c, int64_t nrec, const std::string &err, const std::string &extra = "") {
    return fmt("%s %d %lld %08x %lld \"%s\"%s", label.c_str(), rc, (long long)nbytes, c, (long long)nrec, rc < 0 ? err.c_str() : "", extra.c_str());
}

std::string last_error() { return rd_host_last_error(); }

// ---- gunzip / pgunzip ------------------------------------------------------------------------------------------------------------
std::string cmd_gunzip(const std::string &label, int64_t cap, const std::string &path) {
    uint8_t *out = new uint8_t[(size_t)cap];
    int64_t n = 0;
    const int rc = rd_host_gunzip(path.c_str(), out, cap, &n);
    const std::string s = line(label, rc, n, crc(0, out, (size_t)n), 0, last_error());
    delete[] out;
    return s;
}

std::string cmd_pgunzip(const std::string &label, int threads, int64_t section, int64_t cap, const std::string &path) {
    uint8_t *out = new uint8_t[(size_t)cap];
    int64_t n = 0;
    int64_t *st = new int64_t[4]();
    const int rc = rd_host_gunzip_parallel(path.c_str(), out, cap, &n, threads, section, st);
    const std::string s = line(label, rc, n, crc(0, out, (size_t)n), 0, last_error(),
                               fmt(" used=%lld dropped=%lld fell_back=%lld", (long long)st[0], (long long)st[1], (long long)st[3]));
    delete[] out;
    delete[] st;
    return s;
}

// ---- readers -----------------------------------------------------------------------------------------------------------------------
struct ReadAgg {
    int rc = 0;
    int64_t nbytes = 0, nrec = 0, calls = 0;
    uint32_t c = 0, tc = 0;
    std::string err;
};

// rd_reader_next until the end of the stream (stop < 0) or for `stop` calls; a record that does not fit (*n == 0, rc 0) is answered with a
// new buffer of exactly the size the reader asks for
void read_all(rd_reader *r, int64_t max_records, int64_t buf_cap, int64_t stop, ReadAgg &a) {
    int64_t cap = buf_cap;
    uint8_t *buf = new uint8_t[(size_t)cap];
    int64_t *rs = new int64_t[(size_t)max_records + 1], *so = new int64_t[(size_t)max_records];
    int32_t *sl = new int32_t[(size_t)max_records];
    while (stop < 0 || a.calls < stop) {
        int64_t n = 0, nb = 0;
        const int rc = rd_reader_next(r, max_records, buf, cap, rs, so, sl, &n, &nb);
        ++a.calls;
        a.rc = rc;
        if (rc < 0) {
            a.err = last_error();
            break;
        }
        if (rc == 0 && n == 0) {
            if (nb <= cap) {
                a.rc = -2;
                a.err = "driver: the reader delivers nothing and asks for no larger buffer";
                break;
            }
            delete[] buf;
            cap = nb;
            buf = new uint8_t[(size_t)cap];
            continue;
        }
        a.c = crc(a.c, buf, (size_t)nb);
        a.tc = crc(a.tc, rs, (size_t)(n + 1) * 8);
        a.tc = crc(a.tc, so, (size_t)n * 8);
        a.tc = crc(a.tc, sl, (size_t)n * 4);
        a.nbytes += nb;
        a.nrec += n;
        if (rc == 1) break;
    }
    delete[] buf;
    delete[] rs;
    delete[] so;
    delete[] sl;
}

std::string agg_line(const std::string &label, const ReadAgg &a, const std::string &extra = "") {
    return line(label, a.rc, a.nbytes, a.c, a.nrec, a.err, fmt(" %08x", a.tc) + extra);
}

std::string cmd_read(const std::string &label, int format, int64_t max_records, int64_t buf_cap, int64_t stop, const std::string &path) {
    rd_reader *r = nullptr;
    ReadAgg a;
    if (rd_reader_open(path.c_str(), format, &r) != 0) {
        a.rc = -1;
        a.err = last_error();
        return agg_line(label, a);
    }
    read_all(r, max_records, buf_cap, stop, a);
    rd_reader_close(r);   // (stop >= 0: while the prefetch thread / the parallel decoder still work)
    return agg_line(label, a);
}

// the multi-rank CLI's byte ranges: boundaries at every `step`-th byte, every share counted, skipped over and read by a range reader
std::string cmd_read_range(const std::string &label, int format, int64_t step, const std::string &path) {
    ReadAgg a;
    int64_t size = 0;
    int32_t is_gz = 0;
    if (rd_host_file_info(path.c_str(), &size, &is_gz) != 0) {
        a.rc = -1;
        a.err = last_error();
        return agg_line(label, a);
    }
    std::vector<int64_t> cut{0};
    for (int64_t pos = step; pos < size; pos += step) {
        int64_t b = 0;
        if (rd_host_find_record_start(path.c_str(), format, pos, &b) != 0) {
            a.rc = -1;
            a.err = last_error();
            return agg_line(label, a);
        }
        if (b > cut.back()) cut.push_back(b);
    }
    if (size > cut.back()) cut.push_back(size);
    int64_t counted = 0, shares = 0;
    int skip_ok = 1;
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        int64_t c = 0, e = 0;
        rd_reader *r = nullptr;
        if (rd_host_count_records(path.c_str(), format, cut[k], cut[k + 1], &c) != 0 || rd_host_skip_records(path.c_str(), format, cut[k], c, &e) != 0 ||
            rd_reader_open_range(path.c_str(), format, cut[k], cut[k + 1], &r) != 0) {
            a.rc = -1;
            a.err = last_error();
            break;
        }
        counted += c;
        skip_ok &= e == cut[k + 1];
        ++shares;
        read_all(r, 1000, 1 << 20, -1, a);
        rd_reader_close(r);
        if (a.rc < 0) break;
    }
    return agg_line(label, a, fmt(" gzip=%d shares=%lld counted=%lld skip_ok=%d", (int)is_gz, (long long)shares, (long long)counted, skip_ok));
}

// a feeder thread hands the file over in pieces (each piece a heap block of its own size) while this thread parses.
// variant: "end" = rd_reader_feed_end(no error); "error" = feed_end with a text; "tail" = end, with set_flush_empty_tail(1);
// "abort" = the feeder feeds the file over and over, this thread takes ONE batch of 7 records, calls rd_reader_feed_abort while the
// feeder waits inside rd_reader_feed, joins it and only then closes the reader
std::string cmd_feed(const std::string &label, const std::string &variant, int format, int64_t piece, const std::string &path) {
    Blob data(path);
    ReadAgg a;
    rd_reader *r = nullptr;
    if (!data.ok || piece < 1 || rd_reader_open_feed(format, &r) != 0) {
        a.rc = -1;
        a.err = data.ok && piece >= 1 ? last_error() : "driver: cannot read the file";
        return agg_line(label, a);
    }
    const bool abort_it = variant == "abort";
    if (variant == "tail") rd_reader_set_flush_empty_tail(r, 1);
    int feeder_rc = 0;   // written by the feeder, read after join()
    std::thread th([&]() {
        int rounds = 0;
        do {
            for (int64_t off = 0; off < data.n; off += piece) {
                const int64_t k = std::min(piece, data.n - off);
                uint8_t *p = new uint8_t[(size_t)k];
                memcpy(p, data.p + off, (size_t)k);
                const int rc = rd_reader_feed(r, p, k);
                delete[] p;
                if (rc < 0) {
                    feeder_rc = rc;
                    return;
                }
            }
        } while (abort_it && data.n > 0 && ++rounds < 64);   // (bounded: a text without 7 records must not be fed for ever)
        feeder_rc = rd_reader_feed_end(r, variant == "error" ? "injected: the fed stream is damaged" : nullptr);
    });
    read_all(r, abort_it ? 7 : 1000, 1 << 20, abort_it ? 1 : -1, a);
    if (abort_it || a.rc != 1) {   // this thread stops before the end of the stream (on purpose, or a damaged text): wake the feeder first
        if (abort_it) std::this_thread::sleep_for(std::chrono::milliseconds(20));   // the feeder is inside its next rd_reader_feed by now
        rd_reader_feed_abort(r);
    }
    th.join();
    rd_reader_close(r);
    // (after a damaged text the feeder was woken or had finished, as the threads fell: its answer is part of the line for "abort" only)
    return agg_line(label, a, abort_it ? fmt(" feeder=%d", feeder_rc) : "");
}

// ---- rd_host_gz_index: called again and again as the bytes arrive `grow` at a time, `cap` entries per call ----------------------------
std::string cmd_index(const std::string &label, int64_t grow, int64_t cap, const std::string &path) {
    Blob data(path);
    if (!data.ok || grow < 1) return line(label, -1, 0, 0, 0, "driver: cannot read the file");
    int64_t pos = 0, avail = 0, total_n = 0, ob = 0;
    uint32_t c = 0;
    int rc = 0;
    rd_host_gz_member *ent = new rd_host_gz_member[(size_t)cap];
    for (;;) {
        const int64_t len = avail - pos;
        uint8_t *buf = new uint8_t[(size_t)len];
        memcpy(buf, data.p + pos, (size_t)len);
        int64_t n = 0, consumed = 0, out_bytes = 0;
        rc = rd_host_gz_index(buf, len, pos, ob, ent, cap, &n, &consumed, &out_bytes);
        delete[] buf;
        if (rc < 0) break;
        c = crc(c, ent, (size_t)n * sizeof(rd_host_gz_member));
        total_n += n;
        pos += consumed;
        ob += out_bytes;
        if (rc == 1) break;
        if (consumed > 0) continue;          // more members may be complete already
        if (avail == data.n) break;          // an incomplete member at the end of the file
        avail = std::min(data.n, avail + grow);
    }
    delete[] ent;
    return line(label, rc, pos, c, total_n, last_error(), fmt(" out_bytes=%lld", (long long)ob));
}

// ---- the writer: write_selected, write_text and write_members interleaved on one file -------------------------------------------------
// PREFIX.txt = the records' text, PREFIX.rs = rec_start (int64, n + 1), PREFIX.lab = labels (int8, n), PREFIX.mem = gzip members made
// elsewhere (may be empty). Records [0, n/3) go through write_selected, [n/3, 2n/3) are gathered here and go through write_text, then
// the members (gzip output only), then [2n/3, n) through write_selected.
std::string cmd_write(const std::string &label, int threads, int want, int eof_marker, const std::string &prefix, const std::string &out) {
    Blob txt(prefix + ".txt"), rsb(prefix + ".rs"), lab(prefix + ".lab"), mem(prefix + ".mem");
    if (!txt.ok || !rsb.ok || !lab.ok || rsb.n != (lab.n + 1) * 8) return line(label, -1, 0, 0, 0, "driver: cannot read the input tables");
    const int64_t n = lab.n, n1 = n / 3, n2 = 2 * n / 3;
    const int64_t *rs = (const int64_t *)rsb.p;
    const int8_t *lb = (const int8_t *)lab.p;
    const bool gz = out.size() >= 2 && out.compare(out.size() - 2, 2, "gz") == 0;
    rd_host_set_threads(threads);
    rd_writer *w = nullptr;
    if (rd_writer_open(out.c_str(), &w) != 0) return line(label, -1, 0, 0, 0, last_error());
    const int wt = rd_writer_threads(w);
    int rc = 0;
    std::string err;
    int64_t nsel = 0, tlen = 0;
    for (int64_t i = 0; i < n; ++i) nsel += lb[i] == want;
    for (int64_t i = n1; i < n2; ++i)
        if (lb[i] == want) tlen += rs[i + 1] - rs[i];
    uint8_t *text = new uint8_t[(size_t)tlen];
    for (int64_t i = n1, o = 0; i < n2; ++i)
        if (lb[i] == want) {
            memcpy(text + o, txt.p + rs[i], (size_t)(rs[i + 1] - rs[i]));
            o += rs[i + 1] - rs[i];
        }
    auto step = [&](int r) {
        if (r != 0 && rc == 0) {
            rc = r;
            err = last_error();
        }
    };
    step(rd_writer_write_selected(w, txt.p, rs, n1, lb, want));
    step(rd_writer_write_text(w, text, tlen));
    if (gz && mem.ok && mem.n > 0) step(rd_writer_write_members(w, mem.p, mem.n));
    step(rd_writer_write_selected(w, txt.p, rs + n2, n - n2, lb + n2, want));
    step(rd_writer_set_eof_marker(w, eof_marker));
    step(rd_writer_close(w));
    delete[] text;
    rd_host_set_threads(0);
    Blob res(out);
    return line(label, rc, res.n, crc(0, res.p, (size_t)res.n), nsel, err, fmt(" threads=%d", wt));
}

// two readers and a writer live in one process at once, each in its own thread (the CLI's paired-end run): every thread fails or
// succeeds with its own rd_host_last_error
std::string cmd_pair(const std::string &label, const std::string &a, const std::string &b, const std::string &prefix, const std::string &out) {
    std::string la, lb2, lw;
    std::thread ta([&]() { la = cmd_read(label + ".a", -1, 1000, 1 << 20, -1, a); });
    std::thread tb([&]() { lb2 = cmd_read(label + ".b", -1, 7, 4096, -1, b); });
    std::thread tw([&]() { lw = cmd_write(label + ".w", 2, 0, 1, prefix, out); });
    ta.join();
    tb.join();
    tw.join();
    return la + "\n" + lb2 + "\n" + lw;
}

// ---- self-tests: faults of the DRIVER's own, so that a build without its sanitizer cannot pass for a clean run ------------------------
int selftest_heap() {
    volatile size_t n = 16;
    uint8_t *p = new uint8_t[n];
    memset(p, 0, n);
    p[n] = 1;   // one byte past the block
    printf("selftest-heap wrote p[%zu]\n", (size_t)n);
    delete[] p;
    return 0;
}

void bump(int *counter) {
    for (int i = 0; i < 100000; ++i) ++*counter;
}

int selftest_race() {
    int counter = 0;   // a plain int, two threads, no lock
    std::thread a(bump, &counter), b(bump, &counter);
    a.join();
    b.join();
    printf("selftest-race counted %d\n", counter);
    return 0;
}

// ---- manifest ------------------------------------------------------------------------------------------------------------------------
std::vector<std::string> split(const std::string &s) {
    std::vector<std::string> t;
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\r' || s[i] == '\n')) ++i;
        size_t j = i;
        while (j < s.size() && !(s[j] == ' ' || s[j] == '\t' || s[j] == '\r' || s[j] == '\n')) ++j;
        if (j > i) t.push_back(s.substr(i, j - i));
        i = j;
    }
    return t;
}

long long num(const std::string &s) { return atoll(s.c_str()); }

// one command (tokens; paths hold no blanks):
//   env NAME [VALUE]                                   set / unset an environment variable for the commands that follow
//   gzthreads N                                        rd_host_set_gz_threads
//   gunzip LABEL CAP PATH                              pgunzip LABEL THREADS SECTION CAP PATH
//   read LABEL FORMAT MAX_RECORDS BUF_CAP STOP PATH    (STOP < 0: to the end, else close after STOP calls)
//   read-range LABEL FORMAT STEP PATH                  feed LABEL end|error|tail|abort FORMAT PIECE PATH
//   index LABEL GROW CAP PATH                          write LABEL THREADS WANT EOF_MARKER PREFIX OUT
//   pair LABEL PATH_A PATH_B PREFIX OUT
bool run_line(const std::vector<std::string> &t) {
    if (t.empty() || t[0][0] == '#') return true;
    const std::string &c = t[0];
    std::string out;
    if (c == "env" && t.size() == 3) { setenv(t[1].c_str(), t[2].c_str(), 1); return true; }
    if (c == "env" && t.size() == 2) { unsetenv(t[1].c_str()); return true; }
    if (c == "gzthreads" && t.size() == 2) { rd_host_set_gz_threads((int)num(t[1])); return true; }
    if (c == "gunzip" && t.size() == 4) out = cmd_gunzip(t[1], num(t[2]), t[3]);
    else if (c == "pgunzip" && t.size() == 6) out = cmd_pgunzip(t[1], (int)num(t[2]), num(t[3]), num(t[4]), t[5]);
    else if (c == "read" && t.size() == 7) out = cmd_read(t[1], (int)num(t[2]), num(t[3]), num(t[4]), num(t[5]), t[6]);
    else if (c == "read-range" && t.size() == 5) out = cmd_read_range(t[1], (int)num(t[2]), num(t[3]), t[4]);
    else if (c == "feed" && t.size() == 6) out = cmd_feed(t[1], t[2], (int)num(t[3]), num(t[4]), t[5]);
    else if (c == "index" && t.size() == 5) out = cmd_index(t[1], num(t[2]), num(t[3]), t[4]);
    else if (c == "write" && t.size() == 7) out = cmd_write(t[1], (int)num(t[2]), (int)num(t[3]), (int)num(t[4]), t[5], t[6]);
    else if (c == "pair" && t.size() == 6) out = cmd_pair(t[1], t[2], t[3], t[4], t[5]);
    else {
        fprintf(stderr, "rd_host_san: bad command line: %s (%zu tokens)\n", c.c_str(), t.size());
        return false;
    }
    printf("%s\n", out.c_str());
    fflush(stdout);
    return true;
}

std::string base(const std::string &p) {
    const size_t k = p.rfind('/');
    return k == std::string::npos ? p : p.substr(k + 1);
}

int64_t file_size(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 ? (int64_t)st.st_size : 0;
}

int format_of(const std::string &p) {   // for the feed command, which has no path to look at: FASTA by extension, else FASTQ
    std::string s = p;
    if (s.size() > 3 && s.compare(s.size() - 3, 3, ".gz") == 0) s.resize(s.size() - 3);
    for (const char *e : {".fasta", ".fa", ".fna", ".fas"})
        if (s.size() >= strlen(e) && s.compare(s.size() - strlen(e), strlen(e), e) == 0) return 1;
    return 0;
}

int usage() {
    fprintf(stderr,
            "usage: rd_host_san gunzip FILE... | pgunzip THREADS SECTION FILE... | read FORMAT MAX_RECORDS BUF_CAP FILE... |\n"
            "       read-close-early K FILE... | read-range STEP FILE... | feed PIECE_BYTES FILE... | index FILE... |\n"
            "       write THREADS PREFIX OUT | manifest FILE | selftest-heap | selftest-race\n");
    return 2;
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> a(argv + 1, argv + argc);
    if (a.empty()) return usage();
    const std::string &c = a[0];
    if (c == "selftest-heap") return selftest_heap();
    if (c == "selftest-race") return selftest_race();
    if (c == "manifest" && a.size() == 2) {
        FILE *f = fopen(a[1].c_str(), "r");
        if (!f) return usage();
        std::string text;
        char b[65536];
        size_t k;
        while ((k = fread(b, 1, sizeof(b), f)) > 0) text.append(b, k);
        fclose(f);
        size_t i = 0;
        while (i < text.size()) {
            size_t j = text.find('\n', i);
            if (j == std::string::npos) j = text.size();
            if (!run_line(split(text.substr(i, j - i)))) return 2;
            i = j + 1;
        }
        return 0;
    }
    // by hand: the same commands with the capacities worked out here (a whole-file gunzip grows its buffer until the text fits)
    const size_t fixed = c == "gunzip" || c == "index" ? 1 : c == "pgunzip" ? 3 : c == "read" ? 4 : c == "read-close-early" || c == "read-range" || c == "feed" ? 2 : 0;
    if (c == "write" && a.size() == 4) return run_line({"write", base(a[3]), a[1], "0", "1", a[2], a[3]}) ? 0 : 2;
    if (!fixed || a.size() <= fixed) return usage();
    for (size_t i = fixed; i < a.size(); ++i) {
        const std::string &p = a[i], l = base(p);
        bool ok = true;
        if (c == "gunzip" || c == "pgunzip") {
            for (int64_t cap = std::max<int64_t>(1 << 20, 8 * file_size(p));; cap *= 4) {
                const std::string s = c == "gunzip" ? cmd_gunzip(l, cap, p) : cmd_pgunzip(l, (int)num(a[1]), num(a[2]), cap, p);
                if (s.find("output exceeds the buffer") != std::string::npos && cap < (int64_t(1) << 36)) continue;
                printf("%s\n", s.c_str());
                break;
            }
        } else if (c == "read") ok = run_line({"read", l, a[1], a[2], a[3], "-1", p});
        else if (c == "read-close-early") ok = run_line({"read", l, "-1", "1000", "1048576", a[1], p});
        else if (c == "read-range") ok = run_line({"read-range", l, "-1", a[1], p});
        else if (c == "index") ok = run_line({"index", l, "4096", "4096", p});
        else
            for (const char *v : {"end", "error", "tail", "abort"}) ok = ok && run_line({"feed", l + "." + v, v, std::to_string(format_of(p)), a[1], p});
        if (!ok) return 2;
    }
    return 0;
}
