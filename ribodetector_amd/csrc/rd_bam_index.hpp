// rd_bam_index.hpp - the records of inflated BAM bytes in HBM, framed and re-written as FASTQ text (rd_bam_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, in order); DESIGN.md §3.21. The rule is
// ribodetector_amd/bam.py (records / fastq_text): every table written here equals that serial walk's, on every input.
//
// A BAM record is  block_size:int32  then block_size bytes; the next record starts behind them: a length-prefixed CHAIN, which
// cannot be framed by a scan the way newline-delimited text is. The window [begin, end) of a batch (begin = pad - carry, the raw
// bytes behind the last complete record of the batch before, copied in front like the FASTQ carry) is cut into segments of
// RD_BAM_SEGMENT bytes, counted from `begin`:
//
//   rd_bam_walk_kernel    one wave per segment, the segment (+ the bytes a record that starts in it can need for its checks) staged
//                         in LDS: the lanes test consecutive offsets for the SIGNATURE of a record (plausible block_size, the
//                         lengths fit in it, a printable name that ends in NUL, refID / pos / next_refID / next_pos >= -1) - the first hit is the
//                         segment's GUESSED entry - and the chain is walked from there to the segment's end: per delivered record
//                         (source offset, bytes of FASTQ text in front of it within the segment) into the segment's local list;
//                         records walked and delivered, bytes of text, the EXIT (first record start at or behind the segment's end)
//                         and how the walk ended. Segment 0's entry is `begin`: no guess.
//   rd_bam_stitch_kernel  one wave, the segments in order from the true entry of the batch: a segment whose true entry lies behind
//                         its end has no records; one whose guess IS the true entry is accepted as walked; any other is walked
//                         again from the true entry there and then (from global memory: rare - a tag payload or a quality block that
//                         looks like a record). 64 segments at a time are first tried WITHOUT a serial step: the set of segments on
//                         the chain is found as a fixed point of prefix maxima of their exits, and taken only when it is provably
//                         the serial result (the kernel has the argument). The guess decides the speed, never the result. Also: the exclusive bases of the
//                         segments' record counts and text bytes, the batch's verdict, carry (`consumed`) and totals.
//   rd_bam_table_kernel   local lists -> rec_tab / hdr_tab / the source offset of every record, at the scanned positions
//   rd_bam_emit_kernel    `norm`, dealt by OUTPUT bytes: 16 per thread, the record of a byte by binary search in rec_tab (bounded by the
//                         workgroup's first and last record) - a 1 Mb read next to 100 b reads does not serialise a wave. Per byte: '@' /
//                         name / '\n' / base (4-bit code -> letter; reverse strand: complemented, from the far end) / '+' / quality
//                         (min(q, 93) + 33; absent: '"'; reverse strand: from the far end)
//
// Every length of a record is DATA: block_size, l_read_name, n_cigar_op, l_seq are compared in 64-bit arithmetic against the window
// before any byte they point to is read; a record is walked past only when it lies inside [begin, end) as a whole and is
// well-formed, and only such records reach the tables the emit pass reads from. A damaged file ends in a status word.
// Flag 0x900 (secondary / supplementary): walked, not delivered.
#pragma once
#include "rd_fasta_index.hpp"

namespace {

constexpr int BAM_S = RD_BAM_SEGMENT;
constexpr int BAM_LIST = BAM_S / 37 + 1;                 // a well-formed record is >= 37 bytes: the most record starts in a segment
constexpr int BAM_REACH = 320;                           // bytes behind a record's start that its checks read: 36 fixed + a name of <= 255
constexpr int BAM_STAGE = BAM_S + 16 + BAM_REACH;        // (+ 16: the stage starts at the 16-byte boundary in front of the segment)
constexpr int BAM_EMIT_BYTES = 16 * FQ_THREADS;          // bytes of `norm` per workgroup and trip
enum { BAM_RAN = 0, BAM_INCOMPLETE = 1, BAM_ILL = 2 };   // how a walk ended: past the segment's end / inside a record / at an ill-formed one

__device__ const uint8_t BAM_FWD[16] = {'=', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'};
__device__ const uint8_t BAM_REV[16] = {'=', 'T', 'G', 'K', 'C', 'Y', 'S', 'B', 'A', 'W', 'R', 'D', 'M', 'H', 'V', 'N'};

struct BamSeg {               // what the walk of one segment found (32 bytes)
    int32_t guess;            // the entry the walk started from (-1: no offset of the segment looks like a record)
    int32_t exit;             // first record start at or behind the segment's end, or where the walk stopped
    int32_t kind;             // BAM_RAN / BAM_INCOMPLETE / BAM_ILL
    int32_t walked, cnt;      // records walked, records delivered (= entries of the local list)
    int32_t pad;
    int64_t norm;             // bytes of FASTQ text of the delivered records
};

struct BamScratch {           // device scratch of one rd_bam_index call
    int64_t nseg_used;        // segments the stitch reached (the tables of the others are not read)
    int64_t reserved[7];
};

// bytes of the window at absolute offsets of the batch buffer: base[a - off] (LDS stage: off = where the stage starts; global: 0)
struct BamBytes {
    const uint8_t *base;
    int64_t off;
    __device__ __forceinline__ uint32_t u8(int64_t a) const { return base[a - off]; }
    __device__ __forceinline__ uint32_t u16(int64_t a) const { return u8(a) | (u8(a + 1) << 8); }
    __device__ __forceinline__ uint32_t u32(int64_t a) const { return u16(a) | (u16(a + 2) << 16); }
};

__device__ __forceinline__ bool bam_status_framed(int status) { return status == RD_FQ_OK || status == RD_BAM_RECORD || status == RD_BAM_TRUNCATED; }

// the fixed fields of the record at p that the text depends on; p + 36 <= end has been checked
struct BamRec {
    int64_t block, lrn, ncig, lseq, need;
    uint32_t flag;
};
__device__ __forceinline__ BamRec bam_fields(const BamBytes &b, int64_t p) {
    BamRec r;
    r.block = (int64_t)(int32_t)b.u32(p);
    r.lrn = b.u8(p + 12);
    r.ncig = b.u16(p + 16);
    r.flag = b.u16(p + 18);
    r.lseq = b.u32(p + 20);
    r.need = 32 + r.lrn + 4 * r.ncig + (r.lseq + 1) / 2 + r.lseq;
    return r;
}

// the chain from p (lo <= p) to the first record start at or behind hi: THE serial walk of bam.records, one segment of it. Executed by a
// whole wave on the same values; lane 0 writes the list (BAM_LIST entries: enough by construction, checked all the same).
__device__ __forceinline__ BamSeg bam_walk(const BamBytes &b, int64_t p, int64_t hi, int64_t end, int2 *__restrict__ list, bool lane0) {
    BamSeg w;
    w.guess = (int32_t)p;
    w.kind = BAM_RAN;
    w.walked = w.cnt = w.pad = 0;
    w.norm = 0;
    while (p < hi && p < end) {
        if (end - p < 4) { w.kind = BAM_INCOMPLETE; break; }
        const int64_t block = (int64_t)(int32_t)b.u32(p);
        if (block < 32) { w.kind = BAM_ILL; break; }
        if (p + 4 + block > end) { w.kind = BAM_INCOMPLETE; break; }
        const BamRec r = bam_fields(b, p);                        // (p + 36 <= p + 4 + block <= end)
        if (r.need > block || r.lrn < 1 || b.u8(p + 36 + r.lrn - 1) != 0) { w.kind = BAM_ILL; break; }
        ++w.walked;
        if (!(r.flag & 0x900u)) {
            if (lane0 && w.cnt < BAM_LIST) list[w.cnt] = make_int2((int)p, (int)w.norm);
            ++w.cnt;
            w.norm += 2 * r.lseq + r.lrn + 5;
        }
        p += 4 + block;
    }
    w.exit = (int32_t)p;
    return w;
}

// does offset q look like the start of a record? A heuristic: it chooses where a segment's speculative walk starts, nothing else.
__device__ __forceinline__ bool bam_plausible(const BamBytes &b, int64_t q, int64_t end) {
    if (q + 36 > end) return false;
    const int64_t block = (int64_t)(int32_t)b.u32(q);
    if (block < 33 || block > (1 << 26)) return false;                 // (a record of more than 64 MiB is found by the in-order pass)
    if ((int32_t)b.u32(q + 4) < -1 || (int32_t)b.u32(q + 8) < -1 || (int32_t)b.u32(q + 24) < -1 || (int32_t)b.u32(q + 28) < -1) return false;
    const BamRec r = bam_fields(b, q);
    if (r.lrn < 1 || r.need > block) return false;
    const int64_t nul = q + 36 + r.lrn - 1;
    if (nul < end && b.u8(nul) != 0) return false;
    const int64_t shown = r.lrn - 1 < 16 ? r.lrn - 1 : 16;            // the first bytes of the name: printable
    for (int64_t i = 0; i < shown && q + 36 + i < end; ++i) {
        const uint32_t c = b.u8(q + 36 + i);
        if (c < 33 || c > 126) return false;
    }
    return true;
}

// TABLES: the local lists of the delivered records are written (rd_bam_index); false: the records are counted only (rd_bam_count,
// rd_bam_shard.hpp - `lists` is not touched)
template <bool TABLES>
__global__ __launch_bounds__(64) void rd_bam_walk_kernel(const uint8_t *__restrict__ text, const FqSummary *__restrict__ sum, BamSeg *__restrict__ seg,
                                                         int2 *__restrict__ lists) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[BAM_STAGE];
    const int lane = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t begin = sum->begin, end = sum->end;
    const int64_t lo = begin + s * BAM_S, hi = lo + BAM_S;
    if (sum->status != RD_FQ_OK || lo >= end) {
        if (lane == 0) {
            BamSeg w = {};
            w.guess = -1;
            w.exit = (int32_t)(lo < end ? lo : end);
            seg[s] = w;
        }
        return;
    }
    // [a0, stop) -> LDS in aligned 16-byte pieces; the buffer is readable up to the 64-byte boundary behind `end` (rd_fastq_index's rule)
    const int64_t a0 = lo & ~(int64_t)15;
    int64_t stop = hi + BAM_REACH;
    if (stop > end) stop = end;
    for (int64_t a = a0 + 16 * lane; a < stop; a += 16 * 64)
        *reinterpret_cast<u32x4 *>(stage + (a - a0)) = *reinterpret_cast<const u32x4 *>(text + a);
    __syncthreads();
    const BamBytes b = {stage, a0};
    // every read below is of an offset < min(hi + BAM_REACH, end): bam_plausible and bam_walk compare with `end` first, and a record
    // that starts in front of hi has its fixed fields and the end of its name within BAM_REACH bytes
    int64_t entry = -1;
    if (s == 0) {
        entry = begin;
    } else {
        for (int64_t q0 = lo; q0 < hi && q0 < end; q0 += 64) {
            const int64_t q = q0 + lane;
            const bool hit = q < hi && bam_plausible(b, q, end);
            const unsigned long long m = __ballot(hit);
            if (m) {
                entry = q0 + (__ffsll((long long)m) - 1);
                break;
            }
        }
    }
    BamSeg w = {};
    w.guess = -1;
    w.exit = (int32_t)lo;
    if (entry >= 0) w = bam_walk(b, entry, hi, end, TABLES ? lists + s * BAM_LIST : nullptr, TABLES && lane == 0);
    if (lane == 0) seg[s] = w;
}

// TABLES: as in the walk; false: seg_rbase / seg_nbase / seg_cnt / sc / rec_tab are not touched, and no table can be too small
template <bool TABLES>
__global__ __launch_bounds__(64) void rd_bam_stitch_kernel(const uint8_t *__restrict__ text, FqSummary *__restrict__ sum, BamSeg *__restrict__ seg,
                                                           int2 *__restrict__ lists, int nseg, int32_t *__restrict__ seg_rbase, int64_t *__restrict__ seg_nbase,
                                                           int32_t *__restrict__ seg_cnt, BamScratch *__restrict__ sc, int final, int64_t norm_cap,
                                                           int64_t cap_records, int64_t *__restrict__ rec_tab) {
    const int lane = threadIdx.x;
    if (sum->status != RD_FQ_OK) {
        if (TABLES && lane == 0) sc->nseg_used = 0;
        return;
    }
    const int64_t begin = sum->begin, end = sum->end;
    const BamBytes g = {text, 0};
    int64_t p = begin, walked = 0, n = 0, norm = 0, used = 0;
    int kind = BAM_RAN, rewalks = 0;
    bool over = false;
    for (int s0 = 0; s0 < nseg && !over; s0 += 64) {
        // the 64 segments of this round, one per lane; the serial part below takes them from the lanes (no memory in the chain)
        BamSeg mine = {};
        if (s0 + lane < nseg) mine = seg[s0 + lane];
        int32_t my_rbase = 0, my_cnt = 0;
        int64_t my_nbase = 0;
        // The common case, without a serial step: suppose a set of segments ON the chain. The true entry of a segment is then the largest
        // exit in front of it (exits grow along the chain), P; it is on the chain when P lies in it and IS its guess, and has no records
        // when P lies behind its end. A set that reproduces itself, with no segment left over (one whose guess is not P) and no walk that
        // stopped, is the serial walk's: by induction over the segments, P is the serial entry of each. Anything else: the loop below.
        {
            const int64_t lo_l = begin + (int64_t)(s0 + lane) * BAM_S, hi_l = lo_l + BAM_S;
            const bool live = s0 + lane < nseg && lo_l < end;
            bool on = live && mine.guess >= 0, stable = false;
            int32_t P = 0, top = 0;
            for (int it = 0; it < 4 && !stable; ++it) {
                int32_t inc = on ? mine.exit : 0;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int32_t t = __shfl_up(inc, o);
                    if (lane >= o && t > inc) inc = t;
                }
                const int32_t ex = __shfl_up(inc, 1);
                P = lane ? ex : 0;
                if ((int64_t)P < p) P = (int32_t)p;
                top = __builtin_amdgcn_readlane(inc, 63);
                const bool on2 = live && (int64_t)P < hi_l && mine.guess == P;
                stable = !__any(on2 != on);
                on = on2;
            }
            const bool left_over = live && !on && (int64_t)P < hi_l;
            if (stable && !__any(left_over || (on && mine.kind != BAM_RAN))) {
                int32_t c = on ? mine.cnt : 0, wk = on ? mine.walked : 0;
                int64_t nb = on ? mine.norm : 0;
                const int32_t c0 = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int32_t tc = __shfl_up(c, o), tw = __shfl_up(wk, o);
                    const int64_t tn = __shfl_up(nb, o);
                    if (lane >= o) { c += tc; wk += tw; nb += tn; }
                }
                if (TABLES && live) {
                    seg_rbase[s0 + lane] = (int32_t)n + c - c0;
                    seg_nbase[s0 + lane] = norm + nb - (on ? mine.norm : 0);
                    seg_cnt[s0 + lane] = c0;
                }
                n += __builtin_amdgcn_readlane(c, 63);
                walked += __builtin_amdgcn_readlane(wk, 63);
                norm += __shfl(nb, 63);
                if ((int64_t)top > p) p = top;
                const int n_live = __popcll(__ballot(live));
                used = s0 + n_live;
                if (n_live < 64) over = true;
                continue;
            }
        }
        for (int k = 0; k < 64 && s0 + k < nseg; ++k) {
            const int64_t lo = begin + (int64_t)(s0 + k) * BAM_S, hi = lo + BAM_S;
            if (lo >= end) { over = true; break; }
            used = s0 + k + 1;
            BamSeg w;                                // (read from lane k into scalar registers: the chain below is scalar work)
            w.guess = __builtin_amdgcn_readlane(mine.guess, k);
            w.exit = __builtin_amdgcn_readlane(mine.exit, k);
            w.kind = __builtin_amdgcn_readlane(mine.kind, k);
            w.walked = __builtin_amdgcn_readlane(mine.walked, k);
            w.cnt = __builtin_amdgcn_readlane(mine.cnt, k);
            w.norm = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(mine.norm >> 32), k) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(mine.norm & 0xffffffffLL), k));
            if (p >= hi) {                           // inside a record that spans the segment
                w.cnt = 0;
            } else {
                if ((int64_t)w.guess != p) {         // the guess was wrong (or there was none): the walk from the true entry
                    w = bam_walk(g, p, hi, end, TABLES ? lists + (int64_t)(s0 + k) * BAM_LIST : nullptr, TABLES && lane == 0);
                    w.exit = __builtin_amdgcn_readfirstlane(w.exit);       // (every lane walked the same chain)
                    w.kind = __builtin_amdgcn_readfirstlane(w.kind);
                    w.walked = __builtin_amdgcn_readfirstlane(w.walked);
                    w.cnt = __builtin_amdgcn_readfirstlane(w.cnt);
                    w.norm = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(w.norm >> 32)) << 32) |
                                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(w.norm & 0xffffffffLL)));
                    ++rewalks;
                }
                if (lane == k) { my_rbase = (int32_t)n; my_nbase = norm; }
                walked += w.walked;
                n += w.cnt;
                norm += w.norm;
                p = w.exit;
                kind = w.kind;
            }
            if (lane == k) my_cnt = w.cnt;
            if (kind != BAM_RAN) { over = true; break; }
        }
        if (TABLES && s0 + lane < used) {
            seg_rbase[s0 + lane] = my_rbase;
            seg_nbase[s0 + lane] = my_nbase;
            seg_cnt[s0 + lane] = my_cnt;
        }
    }
    if (lane == 0) {
        if (TABLES) sc->nseg_used = used;
        sum->n_lines = walked;                       // (BAM: the records walked, the skipped ones included)
        sum->dirty = rewalks;                        // (BAM: the segments walked again by the stitch)
        if (TABLES && (n + 1 > cap_records || norm > norm_cap)) {
            sum->status = RD_FQ_LINES;               // the caller's tables are too small for this batch: framed again with full-size ones
            sum->n_records = 0;
            sum->consumed = begin;
            sum->reserved = 0;
        } else {
            sum->n_records = n;
            sum->consumed = p;
            sum->reserved = norm;
            if (TABLES) rec_tab[n] = norm;
            if (kind == BAM_ILL) {
                sum->status = RD_BAM_RECORD;
                sum->bad_record = (unsigned long long)walked;
            } else if (p < end && final) {
                sum->status = RD_BAM_TRUNCATED;
            }
        }
    }
}

__global__ __launch_bounds__(64) void rd_bam_table_kernel(const uint8_t *__restrict__ text, const FqSummary *__restrict__ sum, const BamScratch *__restrict__ sc,
                                                          const int2 *__restrict__ lists, const int32_t *__restrict__ seg_rbase,
                                                          const int64_t *__restrict__ seg_nbase, const int32_t *__restrict__ seg_cnt,
                                                          int64_t *__restrict__ rec_tab, int32_t *__restrict__ hdr_tab, int32_t *__restrict__ src_tab) {
    const int64_t s = blockIdx.x;
    if (!bam_status_framed(sum->status) || s >= sc->nseg_used) return;
    const int cnt = seg_cnt[s] < BAM_LIST ? seg_cnt[s] : BAM_LIST;
    const int64_t rbase = seg_rbase[s], nbase = seg_nbase[s], n = sum->n_records;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        const int2 e = lists[s * BAM_LIST + i];
        const int64_t r = rbase + i;
        if (r >= n) break;
        rec_tab[r] = nbase + e.y;
        src_tab[r] = e.x;
        hdr_tab[r] = (int32_t)text[(int64_t)e.x + 12];           // '@' + the name without its NUL = l_read_name bytes
    }
}

__global__ __launch_bounds__(FQ_THREADS) void rd_bam_emit_kernel(const uint8_t *__restrict__ text, const FqSummary *__restrict__ sum,
                                                                const int64_t *__restrict__ rec_tab, const int32_t *__restrict__ src_tab,
                                                                uint8_t *__restrict__ norm, int64_t norm_cap) {
    __shared__ int64_t r_bounds[2];
    if (!bam_status_framed(sum->status)) return;
    const int64_t n = sum->n_records, T = sum->reserved;
    const BamBytes b = {text, 0};
    for (int64_t o0 = (int64_t)blockIdx.x * BAM_EMIT_BYTES; o0 < T; o0 += (int64_t)gridDim.x * BAM_EMIT_BYTES) {
        __syncthreads();
        if (threadIdx.x < 2) {                       // the records of the workgroup's first and last byte: rec_tab[r] <= o < rec_tab[r + 1]
            int64_t o = threadIdx.x ? o0 + BAM_EMIT_BYTES - 1 : o0;
            if (o > T - 1) o = T - 1;
            int64_t lo = 0, hi = n - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (rec_tab[mid] <= o) lo = mid; else hi = mid - 1;
            }
            r_bounds[threadIdx.x] = lo;
        }
        __syncthreads();
        const int64_t o = o0 + 16 * (int64_t)threadIdx.x;
        if (o >= T) continue;
        int64_t lo = r_bounds[0], hi = r_bounds[1];
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (rec_tab[mid] <= o) lo = mid; else hi = mid - 1;
        }
        int64_t r = lo, rs = 0, re = -1, p = 0, lrn = 0, lseq = 0, seqp = 0, qualp = 0;
        bool rev = false, noqual = false;
        unsigned long long out_lo = 0, out_hi = 0;     // the 16 bytes, little-endian (bytes behind T stay 0)
#pragma unroll 1
        for (int j = 0; j < 16; ++j) {
            const int64_t pos = o + j;
            if (pos >= T) break;
            if (pos >= re) {                         // (the first byte, and every byte that begins another record)
                if (re >= 0) ++r;
                while (rec_tab[r + 1] <= pos) ++r;   // (cannot run past n: rec_tab[n] = T > pos)
                rs = rec_tab[r];
                re = rec_tab[r + 1];
                p = src_tab[r];
                const BamRec f = bam_fields(b, p);
                lrn = f.lrn;
                lseq = f.lseq;
                seqp = p + 36 + f.lrn + 4 * f.ncig;
                qualp = seqp + (f.lseq + 1) / 2;
                rev = (f.flag & 0x10u) != 0;
                noqual = lseq > 0 && text[qualp] == 0xff;
            }
            const int64_t k = pos - rs;
            uint32_t c;
            if (k == 0) c = '@';
            else if (k < lrn) c = text[p + 36 + k - 1];
            else if (k == lrn) c = '\n';
            else {
                const int64_t k2 = k - lrn - 1;
                if (k2 < lseq) {
                    const int64_t i = rev ? lseq - 1 - k2 : k2;
                    const uint32_t v = text[seqp + (i >> 1)];
                    const uint32_t code = (i & 1) ? (v & 15u) : (v >> 4);
                    c = rev ? BAM_REV[code] : BAM_FWD[code];
                } else {
                    const int64_t k3 = k2 - lseq;
                    if (k3 == 0 || k3 == 2) c = '\n';
                    else if (k3 == 1) c = '+';
                    else if (k3 - 3 < lseq) {
                        const int64_t i = rev ? lseq - 1 - (k3 - 3) : k3 - 3;
                        const uint32_t q = text[qualp + i];
                        c = noqual ? '"' : (q < 93u ? q : 93u) + 33u;
                    } else c = '\n';
                }
            }
            if (j < 8) out_lo |= (unsigned long long)c << (8 * j); else out_hi |= (unsigned long long)c << (8 * (j - 8));
        }
        if (o + 16 <= norm_cap) {
            u32x4 v = {(uint32_t)out_lo, (uint32_t)(out_lo >> 32), (uint32_t)out_hi, (uint32_t)(out_hi >> 32)};
            *reinterpret_cast<u32x4 *>(norm + o) = v;
        } else {
            for (int j = 0; j < 16 && o + j < T; ++j) norm[o + j] = (uint8_t)((j < 8 ? out_lo >> (8 * j) : out_hi >> (8 * (j - 8))) & 0xffu);
        }
    }
}

struct BamWs {
    int nseg;
    BamSeg *seg;
    int2 *lists;
    int32_t *seg_rbase, *seg_cnt, *src_tab;
    int64_t *seg_nbase;
    BamScratch *sc;
    size_t total;
};
BamWs bam_ws(void *workspace, int64_t text_end) {
    BamWs p;
    Carver c(workspace);
    p.nseg = (int)(text_end / BAM_S) + 1;                 // (begin >= 0: the window is at most text_end bytes)
    p.seg = c.take<BamSeg>((size_t)p.nseg);
    p.lists = c.take<int2>((size_t)p.nseg * BAM_LIST);
    p.seg_rbase = c.take<int32_t>((size_t)p.nseg);
    p.seg_cnt = c.take<int32_t>((size_t)p.nseg);
    p.seg_nbase = c.take<int64_t>((size_t)p.nseg);
    p.src_tab = c.take<int32_t>((size_t)(text_end / 37 + 2));
    p.sc = c.take<BamScratch>(1);
    p.total = c.off;
    return p;
}

}  // namespace
