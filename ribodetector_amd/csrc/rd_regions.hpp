// rd_regions.hpp - where the rRNA is inside the reads that `--windows` classified over windows (`--regions`): a BED-like text, formatted
// on the device (rd_region_* kernels). Part of the single translation unit rd_kernels.hip (included from there, after rd_windows.hpp,
// whose rule it uses, and rd_report.hpp, whose id rule, q value and write scheme it uses).
//
// A unit is one read: record i of a single-end chunk, or mate m of pair i (unit 2 i + m: mate 1's lines stand before mate 2's). Window j
// of a unit is an rRNA window when its final fp32 logits have l1 > l0 (a tie is not); a region is a maximal run a..b of rRNA windows
// and covers [start of window a, end of window b) in 0-based bases of the read (wn_start of rd_windows.hpp; W == 1: [0, min(len, L))).
// One line per region: `<id>\t<start>\t<end>\t<mate>\t<windows>\t<p>\n`, id as in rd_report.hpp, p = the largest q = rp_q(l1 - l0) of
// the run as "0.dddd" / "1.0000". A region of no bases (a read of 0 bases) has no line. Only header bytes, seq_len, win_first and
// win_logits are read - no sequence text.
//
// The mapping. The window walks (count and line pass) take ONE LANE PER UNIT and one float2 load per window, which is exactly the
// loop of rd_window_fuse_kernel (W <= 4096): a unit of thousands of windows holds its wave as long as it does there, not longer, and
// the usual chunk (W of 1..3 everywhere) is one coalesced pass over win_logits. What must not sit behind one lane is the text: a unit
// of 4,096 alternating windows has 2,048 lines. So the line pass writes no text, only one 24-byte entry per region into a LINE TABLE
// (there are at most (windows + units) / 2 regions, which sizes it), and the write pass is the report's tile writer (rp_write_tile)
// over that table: a workgroup takes 256 consecutive LINES, whichever units they belong to - a contiguous output range - and every
// lane assembles 16-byte pieces of it.
//
//   rd_region_count_kernel   one lane per unit: id length (rp_id_len), regions and exact line bytes of the unit; the workgroup's sums
//                            of both (the sums pass of rd_scan.hpp); the counters of info[4..8)
//   rd_scan_off_kernel<1, 2> per unit byte offset and line index (both tables scanned in place by one launch), then RgVerdict: the
//                            totals and the verdict info[8]
//   rd_region_lines_kernel   one lane per unit walks its windows again: one line-table entry per region
//   rd_region_write_kernel   256 consecutive lines per workgroup -> text, in aligned 16-byte stores
#pragma once
#include "rd_common.hpp"
#include "rd_report.hpp"
#include "rd_windows.hpp"

namespace {

constexpr int RG_UNITS = 256;                   // units per workgroup of the unit passes (one lane each)
constexpr int RG_LINES = 256;                   // lines per workgroup of the write pass
constexpr int RG_FIXED = 13;                    // bytes of a line besides its id and the digits of start, end and windows: 5 tabs, mate, p, \n

struct RgMate {                                 // one mate's tables (text_b == nullptr: single-end)
    const uint8_t *text;
    int64_t bytes;
    const int64_t *rec_start;
    const int32_t *seq_len;
    const int64_t *win_first;
    const float2 *win_logits;
};

__device__ __forceinline__ int rg_digits(uint32_t v) {
    int d = 1;
    for (uint32_t p = 10; d < 10 && v >= p; p *= 10) ++d;
    return d;
}
__device__ __forceinline__ uint32_t rg_pow10(int k) {
    uint32_t p = 1;
    for (int i = 0; i < k; ++i) p *= 10u;
    return p;
}

// The walk over a unit's windows that the count pass and the line pass share: emit(start, end, windows, q) per region, in ascending
// start. len >= 0, 1 <= W <= RD_WINDOW_MAX (the callers have checked both).
template <class Emit>
__device__ __forceinline__ void rg_walk(const float2 *__restrict__ wl, int64_t f, int64_t W, int64_t len, int64_t L, Emit emit) {
    if (W == 1) {
        const float2 w = wl[f];
        const int64_t end = len < L ? len : L;
        if (w.y > w.x && end > 0) emit((int64_t)0, end, 1, rp_q(w.y - w.x));
        return;
    }
    int64_t a = -1;
    uint32_t q = 0;
#pragma unroll 1
    for (int64_t j = 0; j < W; ++j) {
        const float2 w = wl[f + j];
        if (w.y > w.x) {
            const uint32_t qj = rp_q(w.y - w.x);
            if (a < 0) { a = j; q = qj; } else if (qj > q) q = qj;
        } else if (a >= 0) {
            emit(wn_start(a, len, L, W), wn_start(j - 1, len, L, W) + L, (int)(j - a), q);
            a = -1;
        }
    }
    if (a >= 0) emit(wn_start(a, len, L, W), len, (int)(W - a), q);     // (the last window ends at the read's end)
}

__device__ __forceinline__ const RgMate &rg_mate(const RgMate &ma, const RgMate &mb, int mates, int64_t u, int64_t &i, int &m) {
    m = mates == 2 ? (int)(u & 1) : 0;
    i = mates == 2 ? u >> 1 : u;
    return m ? mb : ma;
}

// unit_bytes / unit_lines: what the unit's lines need; the offsets pass turns both into exclusive offsets in place. cnt[4]: regions of mate
// 1 / 2, reads of mate 1 / 2 with a region.
__global__ __launch_bounds__(256) void rd_region_count_kernel(RgMate ma, RgMate mb, int mates, int64_t rec_stride, int64_t n, int64_t L,
                                                             int64_t *__restrict__ unit_bytes, int64_t *__restrict__ unit_lines,
                                                             int32_t *__restrict__ idlen, int64_t *__restrict__ bsum_bytes,
                                                             int64_t *__restrict__ bsum_lines, unsigned long long *__restrict__ cnt,
                                                             int32_t *__restrict__ fault) {
    __shared__ int64_t sh[4];
    __shared__ unsigned int scnt[4];
    if (threadIdx.x < 4) scnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t units = n * mates;
    const int64_t u = (int64_t)blockIdx.x * RG_UNITS + threadIdx.x;
    int64_t bytes = 0, lines = 0;
    if (u < units) {
        int64_t i;
        int m;
        const RgMate &t = rg_mate(ma, mb, mates, u, i, m);
        const int64_t idl = rp_id_len(t.text, t.bytes, t.rec_start[i * rec_stride], t.rec_start[i * rec_stride + 1]);
        const int64_t len = t.seq_len[i], f = t.win_first[i], W = t.win_first[i + 1] - f;
        // (every entry in [0, total] and every step in 1..RD_WINDOW_MAX, total = entry n: no window outside win_logits is read; several
        // windows are those of a read longer than L, or the starts would be negative)
        const bool bad = idl < 0 || len < 0 || f < 0 || W < 1 || W > RD_WINDOW_MAX || f + W > t.win_first[n] || (W > 1 && len <= L);
        if (bad) {
            atomicOr(fault, 1);
        } else {
            rg_walk(t.win_logits, f, W, len, L, [&](int64_t s, int64_t e, int w, uint32_t) {
                lines += 1;
                bytes += idl + RG_FIXED + rg_digits((uint32_t)s) + rg_digits((uint32_t)e) + rg_digits((uint32_t)w);
            });
            if (lines) {
                atomicAdd(&scnt[m], (unsigned int)lines);
                atomicAdd(&scnt[2 + m], 1u);
            }
        }
        unit_bytes[u] = bytes;
        unit_lines[u] = lines;
        idlen[u] = bad ? 0 : (int32_t)idl;
    }
    scan_store_sum(bytes, sh, bsum_bytes);
    scan_store_sum(lines, sh, bsum_lines);
    if (threadIdx.x < 4 && scnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// The verdict behind the offsets pass (unit_bytes / unit_lines -> exclusive offsets in place, entry `units` = the totals): info = {units,
// bytes, 0, fault, regions of mate 1, of mate 2, reads of mate 1 with a region, of mate 2}. tot_bytes / tot_lines: the int64[4] that
// rd_scan_base_kernel wrote ([1] = the total). fault 2: a unit that is none, or more lines than the line table holds (windows that the
// workspace was not sized for); fault 1: more bytes than out_cap, info[1] = the bytes needed. Either way the passes behind write nothing.
struct RgVerdict {
    int64_t units;
    const int64_t *tot_bytes, *tot_lines;
    const unsigned long long *cnt;
    const int32_t *fault;
    int64_t out_cap, line_cap;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        const int64_t bytes = tot_bytes[1], lines = tot_lines[1];
        const int f = (*fault != 0 || lines > line_cap) ? 2 : bytes > out_cap ? 1 : 0;
        info[0] = f ? 0 : units;
        info[1] = f == 2 ? 0 : bytes;
        info[2] = 0;
        info[3] = f;
        for (int k = 0; k < 4; ++k) info[4 + k] = f == 2 ? 0 : (int64_t)cnt[k];
    }
};

// one line-table entry per region: where its line starts in the output, its unit, start, end, and windows << 16 | q
__global__ __launch_bounds__(256) void rd_region_lines_kernel(RgMate ma, RgMate mb, int mates, int64_t n, int64_t L,
                                                             const int64_t *__restrict__ unit_off, const int64_t *__restrict__ unit_line,
                                                             const int32_t *__restrict__ idlen, const int64_t *__restrict__ info, int64_t line_cap,
                                                             int64_t *__restrict__ line_off, int32_t *__restrict__ line_unit,
                                                             int32_t *__restrict__ line_start, int32_t *__restrict__ line_end,
                                                             uint32_t *__restrict__ line_wq) {
    if (info[3]) return;
    const int64_t units = n * mates;
    const int64_t u = (int64_t)blockIdx.x * RG_UNITS + threadIdx.x;
    if (u > units) return;
    if (u == units) {                              // (entry `lines` of line_off = the total, as in every offset table here)
        line_off[unit_line[units]] = unit_off[units];
        return;
    }
    int64_t k = unit_line[u];
    const int64_t k_end = unit_line[u + 1];
    if (k == k_end) return;
    int64_t i;
    int m;
    const RgMate &t = rg_mate(ma, mb, mates, u, i, m);
    const int64_t f = t.win_first[i], W = t.win_first[i + 1] - f, idl = idlen[u];
    int64_t o = unit_off[u];
    rg_walk(t.win_logits, f, W, (int64_t)t.seq_len[i], L, [&](int64_t s, int64_t e, int w, uint32_t q) {
        if (k < k_end && k < line_cap) {           // (what the count pass counted; never an entry outside the table)
            line_off[k] = o;
            line_unit[k] = (int32_t)u;
            line_start[k] = (int32_t)s;
            line_end[k] = (int32_t)e;
            line_wq[k] = ((uint32_t)w << 16) | q;
        }
        o += idl + RG_FIXED + rg_digits((uint32_t)s) + rg_digits((uint32_t)e) + rg_digits((uint32_t)w);
        ++k;
    });
}

// byte j of a line: id, \t start \t end \t mate \t windows \t p \n
__device__ __forceinline__ uint32_t rg_byte(const uint8_t *__restrict__ src, int32_t idl, uint32_t s, uint32_t e, uint32_t wq, int mate, int64_t j) {
    if (j < idl) return src[j];
    int t = (int)(j - idl);
    if (t == 0) return '\t';
    t -= 1;
    const uint32_t num[3] = {s, e, wq >> 16};
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const int nd = rg_digits(num[f]);
        if (t < nd) return '0' + (num[f] / rg_pow10(nd - 1 - t)) % 10u;
        if (t == nd) return '\t';
        t -= nd + 1;
        if (f == 1) {                              // (the mate stands between end and windows)
            if (t == 0) return '0' + (uint32_t)mate;
            if (t == 1) return '\t';
            t -= 2;
        }
    }
    return t >= 6 ? '\n' : rp_prob_byte(wq & 0xffffu, t);
}

// A workgroup takes tiles of RG_LINES consecutive lines (a contiguous output range each), the tiles dealt round over the grid: the
// number of lines is known on the device only. Within a tile: rp_write_tile.
__global__ __launch_bounds__(256) void rd_region_write_kernel(RgMate ma, RgMate mb, int mates, int64_t rec_stride, const int64_t *__restrict__ unit_line,
                                                             int64_t units, const int32_t *__restrict__ idlen, const int64_t *__restrict__ line_off,
                                                             const int32_t *__restrict__ line_unit, const int32_t *__restrict__ line_start,
                                                             const int32_t *__restrict__ line_end, const uint32_t *__restrict__ line_wq,
                                                             uint8_t *__restrict__ out, const int64_t *__restrict__ info) {
    __shared__ int64_t offs[RG_LINES + 1];
    __shared__ const uint8_t *srcs[RG_LINES];
    __shared__ int32_t idl[RG_LINES];
    __shared__ uint32_t ss[RG_LINES], es[RG_LINES], wqs[RG_LINES];
    __shared__ uint8_t mt[RG_LINES];
    if (info[3]) return;
    const int64_t lines = unit_line[units];
    for (int64_t r0 = (int64_t)blockIdx.x * RG_LINES; r0 < lines; r0 += (int64_t)gridDim.x * RG_LINES) {
        const int nr = (int)(lines - r0 < RG_LINES ? lines - r0 : RG_LINES);
        __syncthreads();                           // (the tile before is written)
        for (int k = threadIdx.x; k <= nr; k += 256) offs[k] = line_off[r0 + k];
        for (int k = threadIdx.x; k < nr; k += 256) {
            const int64_t u = line_unit[r0 + k];
            int64_t i;
            int m;
            const RgMate &t = rg_mate(ma, mb, mates, u, i, m);
            srcs[k] = t.text + t.rec_start[i * rec_stride] + 1;
            idl[k] = idlen[u];
            ss[k] = (uint32_t)line_start[r0 + k];
            es[k] = (uint32_t)line_end[r0 + k];
            wqs[k] = line_wq[r0 + k];
            mt[k] = (uint8_t)(m + 1);
        }
        __syncthreads();
        rp_write_tile(offs, nr, out,
                      [&](int r, int64_t j) { return j + 16 <= idl[r] ? srcs[r] + j : nullptr; },
                      [&](int r, int64_t j) { return rg_byte(srcs[r], idl[r], ss[r], es[r], wqs[r], mt[r], j); });
    }
}

}  // namespace
