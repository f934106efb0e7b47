// rd_report.hpp - the per-read classification report of a chunk (`--read_report`), formatted on the device (rd_report_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, after rd_deflate.hpp, whose scan it reuses).
//
// One text line per record: `<id>\t<label>\t<p>` (single-end) or `<id>\t<label>\t<p_1>\t<p_2>\t<p_pair>` (pairs), in input order;
// id = the header line's bytes after '@' / '>' up to the first of {space, \t, \r, \n, \v, \f}; label = rRNA / nonrRNA / unclassified
// (the int8 label 1 / 0 / -1 that chose the output file); p = softmax(logits)[1] in fp32 printed as q = rint(p * 1e4): "0.dddd" or
// "1.0000". The records' text, their starts and the final logits are already in HBM; only the report's bytes travel to the host.
//
//   rd_report_len_kernel     one thread per 8 records: id length (16-byte loads), q values, line length (into line_start) and the
//                            workgroup's sum - the block sums of rd_gz_sel_*, so that rd_gz_sel_base_kernel turns them into bases
//   rd_report_off_kernel     line lengths -> line_start (exclusive offsets in place, entry n = the total); record faults -> info[3]
//   rd_report_write_kernel   a workgroup takes 256 consecutive lines (a contiguous output range) with their table staged in LDS; every
//                            lane assembles one 16-byte piece of the range in registers and writes it with one aligned 16-byte store
//                            (only the two pieces a workgroup shares with its neighbours are written byte by byte)
#pragma once
#include "rd_common.hpp"

namespace {

constexpr int RP_LINES = 256;                   // lines per workgroup of the write pass
constexpr int RP_MAX_SUFFIX = 35;               // "\tunclassified" + 3 x "\t0.dddd" + "\n": bytes of a line besides its id

__constant__ char RP_LABEL[3][13] = {"unclassified", "nonrRNA", "rRNA"};   // label -1, 0, 1
__constant__ int RP_LABEL_LEN[3] = {12, 7, 4};

__device__ __forceinline__ bool rp_ws(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }   // space, \t \n \v \f \r

// (q = rp_q(l1 - l0): rd_common.hpp - the run summary bins the same value, rd_summary.hpp)

__global__ __launch_bounds__(256) void rd_report_len_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ rec_start,
                                                           int64_t n, const float *__restrict__ la, const float *__restrict__ lb,
                                                           const int8_t *__restrict__ labels, int64_t *__restrict__ line_len, int32_t *__restrict__ idlen,
                                                           uint64_t *__restrict__ qs, int64_t *__restrict__ bsum, int32_t *__restrict__ fault) {
    __shared__ int64_t sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * GZ_SCAN_ITEMS + threadIdx.x * 8;
    int64_t s = 0;
    bool bad_any = false;
    for (int k = 0; k < 8; ++k) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const int64_t a = rec_start[i], b = rec_start[i + 1];
        bool bad = !(a >= 0 && a < b && b <= text_bytes);
        int64_t p = a + 1;
        if (!bad) bad = text[a] != '@' && text[a] != '>';
        if (!bad) {
            bool found = false;
            for (; p + 16 <= b && !found; ) {          // 16 bytes per step while they lie inside the record
                u32x4 v;
                __builtin_memcpy(&v, text + p, 16);
                int j = 16;
#pragma unroll
                for (int w = 3; w >= 0; --w)
#pragma unroll
                    for (int c = 3; c >= 0; --c)
                        if (rp_ws((v[w] >> (8 * c)) & 0xffu)) j = 4 * w + c;
                if (j < 16) { p += j; found = true; } else p += 16;
            }
            for (; p < b && !found; ++p)
                if (rp_ws(text[p])) { found = true; break; }
            bad = !found;                               // the header line runs past the record
        }
        const int l = labels[i];
        bad = bad || l < -1 || l > 1 || p - a - 1 > 0x7fffffffLL;
        int64_t len = 0, L = 0;
        uint64_t q = 0;
        if (!bad) {
            L = p - a - 1;
            q = rp_q(la[2 * i + 1] - la[2 * i]);
            if (lb) {
                q |= (uint64_t)rp_q(lb[2 * i + 1] - lb[2 * i]) << 16;
                q |= (uint64_t)rp_q((la[2 * i + 1] + lb[2 * i + 1]) - (la[2 * i] + lb[2 * i])) << 32;   // the summed logits of rd_pair_fuse ('none')
            }
            len = L + 1 + RP_LABEL_LEN[l + 1] + (lb ? 21 : 7) + 1;
        }
        bad_any |= bad;
        line_len[i] = len;
        idlen[i] = (int32_t)L;
        qs[i] = q;
        s += len;
    }
    if (bad_any) atomicOr(fault, 1);
    int64_t total;
    gz_block_scan(s, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// line lengths -> exclusive offsets, in place (every thread reads its 8 entries before it writes them); entry n = the total
__global__ __launch_bounds__(256) void rd_report_off_kernel(int64_t *__restrict__ line_start, int64_t n, const int64_t *__restrict__ bbase,
                                                           const int32_t *__restrict__ fault, int64_t *__restrict__ info) {
    __shared__ int64_t sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * GZ_SCAN_ITEMS + threadIdx.x * 8;
    int64_t v[8], s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n ? line_start[i0 + k] : 0; s += v[k]; }
    int64_t total;
    int64_t run = bbase[blockIdx.x] + gz_block_scan(s, sh, total);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (i0 + k <= n) line_start[i0 + k] = run;
        run += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // info = {lines, bytes, 0, fault}: the base kernel has set info[1] and info[3] (1: more bytes than out_cap); a record that does
        // not start with '@' / '>', whose header runs past its end or whose label is not -1 / 0 / 1 makes it 2 (nothing is written)
        const bool bad = *fault != 0 || info[3] != 0;
        info[0] = bad ? 0 : n;
        info[2] = 0;
        if (*fault) { info[1] = 0; info[3] = 2; }
    }
}

// byte j of the line of staged entry r (its id from the text, the rest from the label and the q values)
__device__ __forceinline__ uint32_t rp_byte(const uint8_t *__restrict__ text, int64_t src, int32_t L, uint64_t q, int lab, int nf, int64_t j) {
    if (j < L) return text[src + j];
    int t = (int)(j - L);
    if (t == 0) return '\t';
    t -= 1;
    const int ll = RP_LABEL_LEN[lab + 1];
    if (t < ll) return (uint8_t)RP_LABEL[lab + 1][t];
    t -= ll;
    const int f = t / 7, c = t - 7 * f;
    if (f >= nf) return '\n';
    if (c == 0) return '\t';
    const uint32_t v = (uint32_t)(q >> (16 * f)) & 0xffffu;
    if (c == 2) return '.';
    if (v >= 10000u) return c == 1 ? '1' : '0';
    if (c == 1) return '0';
    const uint32_t div = c == 3 ? 1000u : c == 4 ? 100u : c == 5 ? 10u : 1u;
    return '0' + (v / div) % 10u;
}

__global__ __launch_bounds__(256) void rd_report_write_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ rec_start,
                                                             const int64_t *__restrict__ line_start, int64_t n, const int32_t *__restrict__ idlen,
                                                             const uint64_t *__restrict__ qs, const int8_t *__restrict__ labels, int nf,
                                                             uint8_t *__restrict__ out, const int64_t *__restrict__ info) {
    __shared__ int64_t offs[RP_LINES + 1];
    __shared__ int64_t srcs[RP_LINES];
    __shared__ uint64_t qv[RP_LINES];
    __shared__ int32_t idl[RP_LINES];
    __shared__ int8_t lab[RP_LINES];
    if (info[3]) return;
    const int64_t r0 = (int64_t)blockIdx.x * RP_LINES;
    const int nr = (int)(n - r0 < RP_LINES ? n - r0 : RP_LINES);
    for (int k = threadIdx.x; k <= nr; k += 256) offs[k] = line_start[r0 + k];
    for (int k = threadIdx.x; k < nr; k += 256) {
        srcs[k] = rec_start[r0 + k] + 1;
        qv[k] = qs[r0 + k];
        idl[k] = idlen[r0 + k];
        lab[k] = labels[r0 + k];
    }
    __syncthreads();
    const int64_t ob = offs[0], oe = offs[nr];
    for (int64_t o = (ob & ~(int64_t)15) + 16 * (int64_t)threadIdx.x; o < oe; o += 16 * 256) {
        const int64_t a = o < ob ? ob : o;             // the piece is [a, e) (its neighbours in other workgroups write the rest)
        const int64_t e = o + 16 < oe ? o + 16 : oe;
        int lo = 0, hi = nr;                            // the line that holds byte a (lines are never empty)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offs[mid] <= a) lo = mid; else hi = mid;
        }
        int r = lo;
        const bool whole = a == o && e == o + 16;
        if (whole && o + 16 <= offs[r] + idl[r]) {     // 16 bytes of one id: one unaligned load, one aligned store
            u32x4 v;
            __builtin_memcpy(&v, text + srcs[r] + (o - offs[r]), 16);
            *reinterpret_cast<u32x4 *>(out + o) = v;
            continue;
        }
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int64_t p = o + b;
            if (p >= a && p < e) {
                while (offs[r + 1] <= p) ++r;
                const uint32_t c = rp_byte(text, srcs[r], idl[r], qv[r], lab[r], nf, p - offs[r]);
                v[b >> 2] |= c << (8 * (b & 3));
            }
        }
        if (whole) {
            *reinterpret_cast<u32x4 *>(out + o) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (o + b >= a && o + b < e) out[o + b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));
        }
    }
}

}  // namespace
