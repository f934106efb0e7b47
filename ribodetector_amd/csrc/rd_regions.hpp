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
// (there are at most (windows + units) / 2 regions, which sizes it), and the write pass is rd_report_write_kernel's scheme over that
// table: a workgroup takes 256 consecutive LINES, whichever units they belong to - a contiguous output range - and every lane
// assembles 16-byte pieces of it.
//
//   rd_region_count_kernel   one lane per unit: id length (the 16-byte header scan of the report), regions and exact line bytes of the
//                            unit; the workgroup's sums of both (block sums for rd_gz_sel_base_kernel); the counters of info[4..8)
//   rd_region_off_kernel     per unit byte offset and line index (exclusive scans in place), the totals and the verdict info[8]
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

// the id of a record [a, b): its length, or -1 when the record is not one (outside the text, no '@' / '>', a header past its end)
__device__ __forceinline__ int64_t rg_id_len(const uint8_t *__restrict__ text, int64_t text_bytes, int64_t a, int64_t b) {
    if (!(a >= 0 && a < b && b <= text_bytes)) return -1;
    if (text[a] != '@' && text[a] != '>') return -1;
    int64_t p = a + 1;
    for (; p + 16 <= b; p += 16) {               // 16 bytes per step while they lie inside the record
        u32x4 v;
        __builtin_memcpy(&v, text + p, 16);
        int j = 16;
#pragma unroll
        for (int w = 3; w >= 0; --w)
#pragma unroll
            for (int c = 3; c >= 0; --c)
                if (rp_ws((v[w] >> (8 * c)) & 0xffu)) j = 4 * w + c;
        if (j < 16) return p + j - a - 1 > 0x7fffffffLL ? -1 : p + j - a - 1;
    }
    for (; p < b; ++p)
        if (rp_ws(text[p])) return p - a - 1 > 0x7fffffffLL ? -1 : p - a - 1;
    return -1;
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

// unit_bytes / unit_lines: what the unit's lines need; the off pass turns both into exclusive offsets in place. cnt[4]: regions of mate
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
        const int64_t idl = rg_id_len(t.text, t.bytes, t.rec_start[i * rec_stride], t.rec_start[i * rec_stride + 1]);
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
    int64_t total;
    gz_block_scan(bytes, sh, total);
    if (threadIdx.x == 0) bsum_bytes[blockIdx.x] = total;
    gz_block_scan(lines, sh, total);
    if (threadIdx.x == 0) bsum_lines[blockIdx.x] = total;
    if (threadIdx.x < 4 && scnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// unit_bytes / unit_lines -> exclusive offsets in place (entry `units` = the totals); info = {units, bytes, 0, fault, regions of mate 1,
// of mate 2, reads of mate 1 with a region, of mate 2}. tot_bytes / tot_lines: the int64[4] that rd_gz_sel_base_kernel wrote ([1] = the
// total). fault 2: a unit that is none, or more lines than the line table holds (windows that the workspace was not sized for);
// fault 1: more bytes than out_cap, info[1] = the bytes needed. Either way the passes behind this one write nothing.
__global__ __launch_bounds__(256) void rd_region_off_kernel(int64_t *__restrict__ unit_bytes, int64_t *__restrict__ unit_lines, int64_t units,
                                                           const int64_t *__restrict__ bb_bytes, const int64_t *__restrict__ bb_lines,
                                                           const int64_t *__restrict__ tot_bytes, const int64_t *__restrict__ tot_lines,
                                                           const unsigned long long *__restrict__ cnt, const int32_t *__restrict__ fault,
                                                           int64_t out_cap, int64_t line_cap, int64_t *__restrict__ info) {
    __shared__ int64_t sh[4];
    const int64_t u = (int64_t)blockIdx.x * RG_UNITS + threadIdx.x;
    const int64_t vb = u < units ? unit_bytes[u] : 0, vl = u < units ? unit_lines[u] : 0;
    int64_t total;
    const int64_t ob = bb_bytes[blockIdx.x] + gz_block_scan(vb, sh, total);
    const int64_t ol = bb_lines[blockIdx.x] + gz_block_scan(vl, sh, total);
    if (u <= units) {
        unit_bytes[u] = ob;
        unit_lines[u] = ol;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t bytes = tot_bytes[1], lines = tot_lines[1];
        const int f = (*fault != 0 || lines > line_cap) ? 2 : bytes > out_cap ? 1 : 0;
        info[0] = f ? 0 : units;
        info[1] = f == 2 ? 0 : bytes;
        info[2] = 0;
        info[3] = f;
        for (int k = 0; k < 4; ++k) info[4 + k] = f == 2 ? 0 : (int64_t)cnt[k];
    }
}

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
    const uint32_t v = wq & 0xffffu;               // p, as rp_byte prints it
    if (t >= 6) return '\n';
    if (t == 1) return '.';
    if (v >= 10000u) return t == 0 ? '1' : '0';
    if (t == 0) return '0';
    const uint32_t div = t == 2 ? 1000u : t == 3 ? 100u : t == 4 ? 10u : 1u;
    return '0' + (v / div) % 10u;
}

// A workgroup takes tiles of RG_LINES consecutive lines (a contiguous output range each), the tiles dealt round over the grid: the
// number of lines is known on the device only. Within a tile: rd_report_write_kernel's scheme.
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
        const int64_t ob = offs[0], oe = offs[nr];
        for (int64_t o = (ob & ~(int64_t)15) + 16 * (int64_t)threadIdx.x; o < oe; o += 16 * 256) {
            const int64_t a = o < ob ? ob : o;         // the piece is [a, e) (its neighbours in other tiles write the rest)
            const int64_t e = o + 16 < oe ? o + 16 : oe;
            int lo = 0, hi = nr;                        // the line that holds byte a (lines are never empty)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (offs[mid] <= a) lo = mid; else hi = mid;
            }
            int r = lo;
            const bool whole = a == o && e == o + 16;
            if (whole && o + 16 <= offs[r] + idl[r]) {     // 16 bytes of one id: one unaligned load, one aligned store
                u32x4 v;
                __builtin_memcpy(&v, srcs[r] + (o - offs[r]), 16);
                *reinterpret_cast<u32x4 *>(out + o) = v;
                continue;
            }
            u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int64_t p = o + b;
                if (p >= a && p < e) {
                    while (offs[r + 1] <= p) ++r;
                    const uint32_t c = rg_byte(srcs[r], idl[r], ss[r], es[r], wqs[r], mt[r], p - offs[r]);
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
}

}  // namespace
