// rd_bam_tagtext.hpp - the listed tags of raw BAM records as text, spliced into the header lines of the records' FASTQ text: the TAGGED
// view of a chunk (rd_bam_tt_* kernels; C ABI rd_bam_tag_splice, the CLI's --bam_tags). Part of the single translation unit
// rd_kernels.hip (included from there, behind rd_bam_tags.hpp, whose walk finds the values); DESIGN.md §3.25.
// The rule is ribodetector_amd/bam.py (tag_comment, fastq_text_tagged): record k of the FASTQ view, '@name\n...', becomes
// '@name' + comment + '\n...', comment = '\tTG:T:text' per listed tag of raw record k that is present and not float-typed. With floats on
// (template parameter F of the count and the write pass; rd_bam_tag_splice_ex with RD_BAM_TAGS_FLOATS) an f value is TG:f:text and a B:f
// array TG:B:f and ',text' per element, text = the value's %g form (rd_float_text.hpp: ft_format); without, they are counted and left out.
//
// The values come from rd_bam_tag_find_kernel, once per listed tag: (val_off, val_len, val_type)[tag][record] - every length is
// checked there against the record's end, so a value lies inside its record. L lanes (4 or 16, the mapping of the walk) share a record:
//
//   rd_bam_tt_count_kernel<L>  the header line's end (the first '\n' of the FASTQ record: 16 bytes per lane and step, a ballot finds
//                              the first), then per listed tag the bytes of its text - the lanes of the group stride over the bytes
//                              of a Z / H value (and validate them: 0x20..0x7E, H: hex digits, even length) and over the elements of a
//                              B array (1 + sign + digits each; F: an f value is an array of one element without the comma, so the
//                              formatter stands once in each pass); the partial sums meet in shuffles BEHIND the strided loops, where
//                              every lane of the wave stands again. Writes the record's tagged length (into out_start), the header
//                              length, a flag (1: malformed tags - no comment; 2: a record that is none) and tag_bytes[tag][record];
//                              counts the copied tags, the malformed records and the skipped float values per workgroup in LDS
//   rd_scan_* (rd_scan.hpp)    the lengths -> out_start (exclusive scan in place, all three passes: the count pass has L lanes per
//                              record and no sum of its own), then TtVerdict: the totals and the verdict into info
//   rd_bam_tt_write_kernel<L>  nothing on a fault. '@name', the comment, the rest of the record: a copy writes the 16-byte aligned
//                              pieces of its OUTPUT range with one unaligned load and one aligned store each, lane j of the group the
//                              j-th piece of a step, and the ragged ends byte by byte - pieces of neighbouring ranges never overlap.
//                              The elements of a B array: L per step, placed by a prefix sum of their text lengths over the group
//                              (shuffles) and a running base; that loop is stepped by the whole wave (a ballot ends it), so the
//                              shuffles are executed by all 64 lanes. Decimal digits are written per lane.
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"
#include "rd_bam_tags.hpp"
#include "rd_float_text.hpp"

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_CNT = 2 + RD_BAM_TAGS_MAX;     // counters: malformed records, float values skipped, records per copied tag

struct TtNames {                                // the listed names, by value
    uint8_t b[2 * RD_BAM_TAGS_MAX];
};

// index (0..15) of the first byte equal to '\n' of the 16 bytes v holds, 16 when there is none
__device__ __forceinline__ int tt_first_newline(u32x4 v) {
    const u32x4 x = {v[0] ^ 0x0a0a0a0au, v[1] ^ 0x0a0a0a0au, v[2] ^ 0x0a0a0a0au, v[3] ^ 0x0a0a0a0au};
    return tg_first_zero(x);
}

__device__ __forceinline__ bool tt_text_byte(uint32_t c, bool hex) {      // may the byte stand in a header line (and in an H value)?
    if (c < 0x20u || c > 0x7eu) return false;
    return !hex || (c >= '0' && c <= '9') || (c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f');
}

__device__ __forceinline__ bool tt_is_int(uint8_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }

// the integer of type t (one of cCsSiI) at p
__device__ __forceinline__ int64_t tt_load_int(const uint8_t *__restrict__ p, uint8_t t) {
    if (t == 'c') return (int8_t)p[0];
    if (t == 'C') return p[0];
    if (t == 's' || t == 'S') {
        uint16_t v;
        __builtin_memcpy(&v, p, 2);
        return t == 's' ? (int64_t)(int16_t)v : (int64_t)v;
    }
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return t == 'i' ? (int64_t)(int32_t)v : (int64_t)v;
}

__device__ __forceinline__ uint32_t tt_load_u32(const uint8_t *__restrict__ p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ int tt_dec_len(int64_t v) {      // '-' and digits of |v| < 2^32
    const uint32_t u = (uint32_t)(v < 0 ? -v : v);
    int d = 1;
    for (uint32_t p = 10; d < 10 && u >= p; p *= 10) ++d;
    return d + (v < 0 ? 1 : 0);
}

__device__ __forceinline__ void tt_put_dec(uint8_t *__restrict__ p, int64_t v, int len) {      // len = tt_dec_len(v)
    uint32_t u = (uint32_t)(v < 0 ? -v : v);
    for (int i = len - 1; i >= (v < 0 ? 1 : 0); --i) {
        p[i] = (uint8_t)('0' + u % 10u);
        u /= 10u;
    }
    if (v < 0) p[0] = '-';
}

// out[o0, o0 + len) = src[0, len) by the L lanes of a group: the aligned 16-byte pieces of the output range whole, its ends bytewise
template <int L>
__device__ __forceinline__ void tt_copy(uint8_t *__restrict__ out, int64_t o0, const uint8_t *__restrict__ src, int64_t len, int sub) {
    const int64_t o1 = o0 + len;
    for (int64_t o = (o0 & ~(int64_t)15) + 16 * (int64_t)sub; o < o1; o += 16 * L) {
        const int64_t a = o < o0 ? o0 : o, e = o + 16 < o1 ? o + 16 : o1;
        if (a == o && e == o + 16) {
            u32x4 v;
            __builtin_memcpy(&v, src + (o - o0), 16);
            *reinterpret_cast<u32x4 *>(out + o) = v;
        } else {
            for (int64_t p = a; p < e; ++p) out[p] = src[p - o0];
        }
    }
}

template <int L, bool F>
__global__ __launch_bounds__(TT_THREADS) void rd_bam_tt_count_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ rec_start,
                                                                    const uint8_t *__restrict__ raw, int64_t raw_bytes, const int64_t *__restrict__ raw_start,
                                                                    int64_t n_rec, int n_tags, const int64_t *__restrict__ val_off,
                                                                    const int32_t *__restrict__ val_len, const uint8_t *__restrict__ val_type,
                                                                    int64_t *__restrict__ tag_bytes, int64_t *__restrict__ hdr, uint8_t *__restrict__ flags,
                                                                    int64_t *__restrict__ out_len, unsigned long long *__restrict__ cnt,
                                                                    int32_t *__restrict__ fault) {
    __shared__ unsigned int scnt[TT_CNT];
    if (threadIdx.x < TT_CNT) scnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1), gbase = lane & ~(L - 1);
    const unsigned long long gmask = L == 64 ? ~0ull : ((1ull << L) - 1ull) << gbase;
    const int64_t k = ((int64_t)blockIdx.x * TT_THREADS + threadIdx.x) / L;
    const bool live = k < n_rec;
    int64_t a = 0, b = 0, s = 0, e = 0;
    bool bad = false;                                     // the record is none: fault 2
    if (live) {
        a = rec_start[k], b = rec_start[k + 1];
        s = raw_start[k], e = raw_start[k + 1];
        bad = !(a >= 0 && a < b && b <= text_bytes) || !(s >= 0 && s <= e && e <= raw_bytes);
        if (!bad) bad = text[a] != '@';
    }
    // the end of the header line: the first '\n' in [a + 1, b)
    int64_t p = a + 1, nl = a;
    bool searching = live && !bad;
    if (searching && p >= b) { searching = false; bad = true; }
    for (;;) {
        if (!__ballot(searching)) break;                  // (wave-uniform: the ballot and the shuffle below are executed by every lane)
        int z = 16;
        if (searching) {
            const int64_t q0 = p + 16 * sub;
            if (q0 + 16 <= b) {
                u32x4 w;
                __builtin_memcpy(&w, text + q0, 16);
                z = tt_first_newline(w);
            } else {
                for (int64_t q = q0; q < b; ++q)
                    if (text[q] == '\n') { z = (int)(q - q0); break; }
            }
        }
        const unsigned long long found = __ballot(z < 16) & gmask;
        const int first = found ? __ffsll((long long)found) - 1 : gbase;
        const int zf = __shfl(z, first);
        if (searching) {
            if (found) {
                nl = p + 16 * (int64_t)(first - gbase) + zf;
                searching = false;
            } else {
                p += 16 * L;
                if (p >= b) { searching = false; bad = true; }      // a header line that runs past its record
            }
        }
    }
    const bool walk = live && !bad;
    bool mal = false;
    uint32_t copied = 0;
    int floats = 0;
    int64_t comment = 0;
    for (int j = 0; j < n_tags; ++j) {                    // (uniform: every lane takes part in the shuffles behind the strided loops)
        int64_t tb = 0;                                   // this lane's share of the text bytes of tag j
        int lbad = 0, is_float = 0;
        if (walk) {
            const int64_t at = (int64_t)j * n_rec + k;
            const int64_t vo = val_off[at];
            const int64_t vl = val_len[at];
            const uint8_t vt = val_type[at];
            if (vo == -2 || (vo >= 0 && (vo < s || vo + vl > e))) lbad = 1;      // (a value lies inside its record: the walk's contract)
            else if (vo >= 0) {
                const uint8_t *__restrict__ v = raw + vo;
                if (vt == 'A') {
                    if (vl != 1 || !tt_text_byte(v[0], false)) lbad = 1;
                    if (sub == 0) tb = 7;
                } else if (tt_is_int(vt)) {
                    if (vl != tg_elem_size(vt)) lbad = 1;
                    else if (sub == 0) tb = 6 + tt_dec_len(tt_load_int(v, vt));
                } else if (vt == 'f' && !F) {
                    is_float = 1;
                } else if (F && (vt == 'f' || (vt == 'B' && vl >= 5 && v[0] == 'f'))) {      // 'TG:f:' text / 'TG:B:f' and ',' text per element
                    const int comma = vt == 'B';
                    const uint8_t *__restrict__ fe = v + 5 * comma;
                    const int64_t count = comma ? (vl - 5) / 4 : 1;
                    if (!comma && vl != 4) lbad = 1;
                    else {
                        if (sub == 0) tb = 6 + comma;
                        for (int64_t i = sub; i < count; i += L) tb += comma + ft_length(tt_load_u32(fe + 4 * i));
                    }
                } else if (vt == 'Z' || vt == 'H') {
                    const bool hex = vt == 'H';
                    if (hex && (vl & 1)) lbad = 1;
                    if (sub == 0) tb = 6 + vl;
                    for (int64_t i = 16 * (int64_t)sub; i < vl; i += 16 * L) {
                        if (i + 16 <= vl) {
                            u32x4 w;
                            __builtin_memcpy(&w, v + i, 16);
#pragma unroll
                            for (int c = 0; c < 16; ++c)
                                if (!tt_text_byte((w[c >> 2] >> (8 * (c & 3))) & 0xffu, hex)) lbad = 1;
                        } else {
                            for (int64_t q = i; q < vl; ++q)
                                if (!tt_text_byte(v[q], hex)) lbad = 1;
                        }
                    }
                } else if (vt == 'B' && vl >= 5) {
                    const uint8_t st = v[0];
                    if (st == 'f') is_float = 1;
                    else if (tt_is_int(st)) {
                        const int es = tg_elem_size(st);
                        const int64_t count = (vl - 5) / es;
                        if (sub == 0) tb = 7;
                        for (int64_t i = sub; i < count; i += L) tb += 1 + tt_dec_len(tt_load_int(v + 5 + i * es, st));
                    } else lbad = 1;
                } else lbad = 1;
            }
        }
#pragma unroll
        for (int o = L / 2; o >= 1; o >>= 1) {
            tb += __shfl_xor(tb, o);
            lbad |= __shfl_xor(lbad, o);
        }
        if (lbad) mal = true;
        else if (tb > 0) copied |= 1u << j;
        floats += is_float;
        comment += tb;
        if (walk && sub == 0) tag_bytes[(int64_t)j * n_rec + k] = tb;
    }
    if (mal) { comment = 0; copied = 0; floats = 0; }
    if (live && sub == 0) {
        out_len[k] = bad ? 0 : (b - a) + comment;
        hdr[k] = bad ? 0 : nl - a;
        flags[k] = bad ? 2 : mal ? 1 : 0;
        if (bad) atomicOr(fault, 1);
        if (!bad && mal) atomicAdd(&scnt[0], 1u);
        if (!bad && floats) atomicAdd(&scnt[1], (unsigned int)floats);
    }
    for (int j = 0; j < n_tags; ++j) {                    // (uniform) one LDS add per wave and tag
        const unsigned long long m = __ballot(walk && sub == 0 && ((copied >> j) & 1u));
        if (lane == 0 && m) atomicAdd(&scnt[2 + j], (unsigned int)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < TT_CNT && scnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// the verdict behind the scan of out_start: info = {records, bytes, 0, fault, malformed records, float values skipped, 0, 0, records
// per copied tag}. fault 2: a record that is none; fault 1: more bytes than out_cap. tot: the int64[4] of rd_scan_base_kernel
struct TtVerdict {
    int64_t n;
    const int64_t *tot;
    const unsigned long long *cnt;
    const int32_t *fault;
    int64_t out_cap;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        const int64_t bytes = tot[1];
        const int f = *fault != 0 ? 2 : bytes > out_cap ? 1 : 0;
        info[0] = f == 2 ? 0 : n;
        info[1] = f == 2 ? 0 : bytes;
        info[2] = 0;
        info[3] = f;
        info[4] = f == 2 ? 0 : (int64_t)cnt[0];
        info[5] = f == 2 ? 0 : (int64_t)cnt[1];
        info[6] = info[7] = 0;
        for (int j = 0; j < RD_BAM_TAGS_MAX; ++j) info[8 + j] = f == 2 ? 0 : (int64_t)cnt[2 + j];
    }
};

template <int L, bool F>
__global__ __launch_bounds__(TT_THREADS) void rd_bam_tt_write_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ rec_start,
                                                                    const uint8_t *__restrict__ raw, int64_t n_rec, int n_tags, TtNames names,
                                                                    const int64_t *__restrict__ val_off, const int32_t *__restrict__ val_len,
                                                                    const uint8_t *__restrict__ val_type, const int64_t *__restrict__ tag_bytes,
                                                                    const int64_t *__restrict__ hdr, const uint8_t *__restrict__ flags,
                                                                    const int64_t *__restrict__ out_start, uint8_t *__restrict__ out,
                                                                    const int64_t *__restrict__ info) {
    if (info[3]) return;                                  // (every lane of the grid: nothing is written on a fault)
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1), gbase = lane & ~(L - 1);
    const int64_t k = ((int64_t)blockIdx.x * TT_THREADS + threadIdx.x) / L;
    const bool live = k < n_rec;
    int64_t a = 0, len = 0, hd = 0, o = 0;
    bool tagged = false;
    if (live) {
        a = rec_start[k];
        len = rec_start[k + 1] - a;
        hd = hdr[k];
        o = out_start[k];
        tagged = flags[k] == 0;
    }
    tt_copy<L>(out, o, text + a, hd, sub);                // '@name'
    o += hd;
    for (int j = 0; j < n_tags; ++j) {                    // (uniform)
        const int64_t at = (int64_t)j * n_rec + k;
        const int64_t tb = tagged ? tag_bytes[at] : 0;
        int64_t count = 0, run = 0;                       // a B array: its elements and where the next one's text goes
        const uint8_t *__restrict__ el = raw;
        uint8_t st = 'C';
        int es = 1, comma = 1;                            // (F: 0 for the one element that an f value is)
        if (tb > 0) {
            const uint8_t *__restrict__ v = raw + val_off[at];
            const int64_t vl = val_len[at];
            const uint8_t vt = val_type[at];
            if (sub == 0) {
                uint8_t *__restrict__ q = out + o;
                q[0] = '\t';
                q[1] = names.b[2 * j];
                q[2] = names.b[2 * j + 1];
                q[3] = ':';
                q[4] = tt_is_int(vt) ? (uint8_t)'i' : vt;
                q[5] = ':';
                if (vt == 'A') q[6] = v[0];
                else if (tt_is_int(vt)) {
                    const int64_t x = tt_load_int(v, vt);
                    tt_put_dec(q + 6, x, tt_dec_len(x));
                } else if (vt == 'B') q[6] = v[0];
            }
            if (vt == 'Z' || vt == 'H') tt_copy<L>(out, o + 6, v, vl, sub);
            else if (vt == 'B') {
                st = v[0];
                es = tg_elem_size(st);
                count = (vl - 5) / es;
                el = v + 5;
                run = o + 7;
            } else if (F && vt == 'f') {
                st = 'f';
                es = 4;
                count = 1;
                el = v;
                run = o + 6;
                comma = 0;
            }
        }
        for (int64_t i0 = 0;; i0 += L) {
            if (!__ballot(i0 < count)) break;             // (wave-uniform: the shuffles below are executed by every lane)
            const int64_t i = i0 + sub;
            int64_t x = 0;
            int dl = 0, mine = 0;
            uint64_t ft[2] = {0, 0};
            const bool fl = F && st == 'f';
            if (i < count) {
                if (fl) dl = ft_format(tt_load_u32(el + i * es), ft);
                else {
                    x = tt_load_int(el + i * es, st);
                    dl = tt_dec_len(x);
                }
                mine = (F ? comma : 1) + dl;
            }
            int inc = mine;
#pragma unroll
            for (int d = 1; d < L; d <<= 1) {
                const int t = __shfl_up(inc, d, L);
                if (sub >= d) inc += t;
            }
            const int total = __shfl(inc, gbase + L - 1);
            if (mine) {
                uint8_t *__restrict__ q = out + run + (inc - mine);
                const int c = F ? comma : 1;
                if (c) q[0] = ',';
                if (fl) ft_put(q + c, ft, dl);
                else tt_put_dec(q + c, x, dl);
            }
            run += total;
        }
        o += tb;
    }
    tt_copy<L>(out, o, text + a + hd, len - hd, sub);     // '\n' SEQ '\n+\n' QUAL '\n'
}

// the tables of a call in its workspace (carved by tagtext_ws of rd_kernels.hip), and the launches of one lane mapping
struct TagTextWs {
    int nb;
    int64_t *val_off, *tag_bytes, *hdr, *bsum, *tot;
    int32_t *val_len, *fault;
    uint8_t *val_type, *flags;
    unsigned long long *cnt;
    size_t total;
};

template <int L, bool F>
void tagtext_launch(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start, int64_t n_rec,
                    int32_t n_tags, const TtNames &names, uint8_t *out, int64_t cap, int64_t *out_start, int64_t *info, const TagTextWs &p, hipStream_t st) {
    const int64_t per = TT_THREADS / L;
    const dim3 grid((unsigned)((n_rec + per - 1) / per));
    for (int j = 0; j < n_tags; ++j)
        tag_find_launch<L>(raw, raw_bytes, raw_start, n_rec, (uint32_t)names.b[2 * j] | ((uint32_t)names.b[2 * j + 1] << 8), p.val_off + (size_t)j * n_rec,
                           p.val_len + (size_t)j * n_rec, p.val_type + (size_t)j * n_rec, st);
    hipLaunchKernelGGL((rd_bam_tt_count_kernel<L, F>), grid, dim3(TT_THREADS), 0, st, text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, (int)n_tags,
                       (const int64_t *)p.val_off, (const int32_t *)p.val_len, (const uint8_t *)p.val_type, p.tag_bytes, p.hdr, p.flags, out_start, p.cnt, p.fault);
    hipLaunchKernelGGL((rd_scan_sum_kernel<8, ScanTab<1>>), dim3(p.nb), dim3(256), 0, st, ScanTab<1>{{out_start}}, n_rec, p.bsum);
    scan_base(p.bsum, p.nb, p.tot, INT64_MAX, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, ScanTab<1>, TtVerdict>), dim3(p.nb), dim3(256), 0, st, ScanTab<1>{{out_start}}, n_rec, ScanOut<1>{{out_start}, {p.bsum}},
                       TtVerdict{n_rec, p.tot, p.cnt, p.fault, cap, info});
    hipLaunchKernelGGL((rd_bam_tt_write_kernel<L, F>), grid, dim3(TT_THREADS), 0, st, text, rec_start, raw, n_rec, (int)n_tags, names, (const int64_t *)p.val_off,
                       (const int32_t *)p.val_len, (const uint8_t *)p.val_type, (const int64_t *)p.tag_bytes, (const int64_t *)p.hdr, (const uint8_t *)p.flags,
                       (const int64_t *)out_start, out, (const int64_t *)info);
}

}  // namespace
