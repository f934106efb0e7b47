// rd_report.hpp - the per-read classification report of a chunk (`--read_report`), formatted on the device (rd_report_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, after rd_scan.hpp, whose scan it uses).
//
// One text line per record: `<id>\t<label>\t<p>` (single-end) or `<id>\t<label>\t<p_1>\t<p_2>\t<p_pair>` (pairs), in input order;
// id = the header line's bytes after '@' / '>' up to the first of {space, \t, \r, \n, \v, \f}; label = rRNA / nonrRNA / unclassified
// (the int8 label 1 / 0 / -1 that chose the output file); p = softmax(logits)[1] in fp32 printed as q = rint(p * 1e4): "0.dddd" or
// "1.0000". The records' text, their starts and the final logits are already in HBM; only the report's bytes travel to the host.
//
//   rd_report_len_kernel     one thread per 8 records: id length (16-byte loads), q values, line length (into line_start) and the
//                            workgroup's sum - the sums pass of rd_scan.hpp, whose base and offsets passes turn line_start into exclusive
//                            offsets in place (entry n = the total); RpVerdict: record faults -> info[3]
//   rd_report_write_kernel   a workgroup takes 256 consecutive lines (a contiguous output range) with their table staged in LDS; every
//                            lane assembles one 16-byte piece of the range in registers and writes it with one aligned 16-byte store
//                            (only the two pieces a workgroup shares with its neighbours are written byte by byte): rp_write_tile,
//                            which rd_regions.hpp's write pass calls too
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"

namespace {

constexpr int RP_LINES = 256;                   // lines per workgroup of the write pass
constexpr int RP_MAX_SUFFIX = 35;               // "\tunclassified" + 3 x "\t0.dddd" + "\n": bytes of a line besides its id

__constant__ char RP_LABEL[3][13] = {"unclassified", "nonrRNA", "rRNA"};   // label -1, 0, 1
__constant__ int RP_LABEL_LEN[3] = {12, 7, 4};

__device__ __forceinline__ bool rp_ws(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }   // space, \t \n \v \f \r

// (q = rp_q(l1 - l0): rd_common.hpp - the run summary bins the same value, rd_summary.hpp)

// the id of a record [a, b): its length, or -1 when the record is not one (outside the text, no '@' / '>', a header past its end)
__device__ __forceinline__ int64_t rp_id_len(const uint8_t *__restrict__ text, int64_t text_bytes, int64_t a, int64_t b) {
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
        const int64_t idl = rp_id_len(text, text_bytes, rec_start[i], rec_start[i + 1]);
        const int l = labels[i];
        const bool bad = idl < 0 || l < -1 || l > 1;
        int64_t len = 0, L = 0;
        uint64_t q = 0;
        if (!bad) {
            L = idl;
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
    scan_store_sum(s, sh, bsum);
}

// info = {lines, bytes, 0, fault}: the base kernel has set info[1] and info[3] (1: more bytes than out_cap); a record that does
// not start with '@' / '>', whose header runs past its end or whose label is not -1 / 0 / 1 makes it 2 (nothing is written)
struct RpVerdict {
    int64_t n;
    const int32_t *fault;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        const bool bad = *fault != 0 || info[3] != 0;
        info[0] = bad ? 0 : n;
        info[2] = 0;
        if (*fault) { info[1] = 0; info[3] = 2; }
    }
};

// byte t (0..5) of "0.dddd" / "1.0000" for q = v
__device__ __forceinline__ uint32_t rp_prob_byte(uint32_t v, int t) {
    if (t == 1) return '.';
    if (v >= 10000u) return t == 0 ? '1' : '0';
    if (t == 0) return '0';
    const uint32_t div = t == 2 ? 1000u : t == 3 ? 100u : t == 4 ? 10u : 1u;
    return '0' + (v / div) % 10u;
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
    return rp_prob_byte((uint32_t)(q >> (16 * f)) & 0xffffu, c - 1);
}

// The write pass of a tile: lines [0, nr) at out[offs[r], offs[r + 1]) - a contiguous range, no line empty, offs in LDS. Every lane
// takes 16-byte pieces of the range and bisects for the line of a piece. src16(r, j): where bytes [j, j + 16) of line r stand in
// the text when all of them do, else null; byte(r, j): byte j of line r. The pieces that the range shares with its neighbours
// (other workgroups or tiles write the rest of them) go byte by byte. piece16(r, j, v): a caller whose bytes are COMPUTED from the text
// (rd_bam_encode.hpp) makes the 16 bytes [j, j + 16) of line r in v when they lie in one field, and says whether it did.
struct RpNoPiece16 {
    __device__ __forceinline__ bool operator()(int, int64_t, u32x4 &) const { return false; }
};

template <class Src16, class Byte, class Piece16>
__device__ __forceinline__ void rp_write_tile(const int64_t *offs, int nr, uint8_t *__restrict__ out, Src16 src16, Byte byte, Piece16 piece16) {
    const int64_t ob = offs[0], oe = offs[nr];
    for (int64_t o = (ob & ~(int64_t)15) + 16 * (int64_t)threadIdx.x; o < oe; o += 16 * 256) {
        const int64_t a = o < ob ? ob : o;             // the piece is [a, e)
        const int64_t e = o + 16 < oe ? o + 16 : oe;
        int lo = 0, hi = nr;                            // the line that holds byte a
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offs[mid] <= a) lo = mid; else hi = mid;
        }
        int r = lo;
        const bool whole = a == o && e == o + 16;
        const uint8_t *src = whole ? src16(r, o - offs[r]) : nullptr;
        if (src) {                                      // 16 bytes of one id: one unaligned load, one aligned store
            u32x4 v;
            __builtin_memcpy(&v, src, 16);
            *reinterpret_cast<u32x4 *>(out + o) = v;
            continue;
        }
        u32x4 v = {0u, 0u, 0u, 0u};
        if (whole && piece16(r, o - offs[r], v)) {
            *reinterpret_cast<u32x4 *>(out + o) = v;
            continue;
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int64_t p = o + b;
            if (p >= a && p < e) {
                while (offs[r + 1] <= p) ++r;
                v[b >> 2] |= byte(r, p - offs[r]) << (8 * (b & 3));
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

template <class Src16, class Byte>
__device__ __forceinline__ void rp_write_tile(const int64_t *offs, int nr, uint8_t *__restrict__ out, Src16 src16, Byte byte) {
    rp_write_tile(offs, nr, out, src16, byte, RpNoPiece16{});
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
    rp_write_tile(offs, nr, out,
                  [&](int r, int64_t j) { return j + 16 <= idl[r] ? text + srcs[r] + j : nullptr; },
                  [&](int r, int64_t j) { return rp_byte(text, srcs[r], idl[r], qv[r], lab[r], nf, j); });
}

}  // namespace
