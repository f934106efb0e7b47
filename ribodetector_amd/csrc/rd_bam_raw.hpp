// rd_bam_raw.hpp - the delivered records of a framed BAM batch as they stand in the input: the RAW view next to the FASTQ text (rd_bam_raw_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, behind rd_bam_index.hpp); DESIGN.md §3.22. The rule is
// ribodetector_amd/bam.py (select): the bytes [offset, offset + size) of every record that is not skipped, joined in input order.
//
// rd_bam_index leaves the source offset of every delivered record in its workspace (src_tab, rd_bam_table_kernel) and is not changed.
// The delivered records are NOT contiguous in the source - the skipped ones lie between them - so the raw view is a table and a gather:
//
//   rd_bam_raw_local_kernel   raw_tab[r + 1] = the bytes (4 + block_size, clamped to the window) of the records of r's block of
//                             GZ_SCAN_ITEMS records up to and including r: an inclusive scan per workgroup, written where the
//                             result goes - the block's total lands in the entry the next block starts from
//   rd_bam_raw_base_kernel    one workgroup: those totals (every GZ_SCAN_ITEMS-th entry) -> their running sum, in place
//   rd_bam_raw_add_kernel     every other entry of a block += the entry the block starts from. raw_tab is now the exclusive scan of
//                             the record sizes, raw_tab[n_records] their total; no workspace: the table is its own scratch
//   rd_bam_raw_sample_kernel  samples[k] = raw_tab[min(k * every, n_records)]: closed by the total, so that the host bounds the raw
//                             bytes of any record range from the samples alone
//   rd_bam_raw_gather_kernel  records [lo, hi) -> out behind a device-side cursor, dealt by OUTPUT bytes like rd_bam_emit_kernel: 16 per
//                             thread at the 16-byte granules of `out`, the record of a byte by binary search in raw_tab (bounded by the
//                             workgroup's first and last record) - a 1 Mb record next to 40-byte records does not serialise a wave. A
//                             granule that lies inside ONE record is one unaligned 16-byte load (the source is unaligned at every residue;
//                             global loads take any address) and one aligned 16-byte store; a granule that crosses a record boundary is read
//                             byte by byte; the partial granules at the two ends of the piece are WRITTEN byte by byte: the bytes in
//                             front of *cursor_in and behind *cursor_out belong to the pieces of other launches.
//
// Every length that is followed has been validated by rd_bam_index (only well-formed records inside the window reach src_tab); all the
// same a record is clamped to [begin, end) when its size is taken, and no byte outside the window is read.
#pragma once
#include "rd_bam_index.hpp"
#include "rd_scan.hpp"

namespace {

constexpr int BAM_RAW_BYTES = 16 * FQ_THREADS;           // bytes of `out` per workgroup and trip

// bytes of delivered record r as they stand in the source, the block_size field included (0 behind the batch's records)
__device__ __forceinline__ int64_t bam_raw_size(const uint8_t *__restrict__ text, const int32_t *__restrict__ src_tab, int64_t r, int64_t n, int64_t begin, int64_t end) {
    if (r >= n) return 0;
    const int64_t p = src_tab[r];
    if (p < begin || p + 4 > end) return 0;
    const BamBytes b = {text, 0};
    int64_t size = 4 + (int64_t)(int32_t)b.u32(p);
    if (size < 0) size = 0;
    return p + size > end ? end - p : size;
}

__global__ __launch_bounds__(256) void rd_bam_raw_local_kernel(const uint8_t *__restrict__ text, const int32_t *__restrict__ src_tab, const FqSummary *__restrict__ sum,
                                                              int64_t *__restrict__ raw_tab, int64_t cap_records) {
    __shared__ int64_t sh[4];
    if (!bam_status_framed(sum->status)) return;
    const int64_t n = sum->n_records, begin = sum->begin, end = sum->end;
    const int64_t b0 = (int64_t)blockIdx.x * GZ_SCAN_ITEMS;
    if (b0 >= n && blockIdx.x) return;                   // (the whole workgroup: no record of the batch is in this block)
    const int64_t i0 = b0 + threadIdx.x * 8;
    int64_t v[8], s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = bam_raw_size(text, src_tab, i0 + k, n, begin, end); s += v[k]; }
    int64_t total;
    int64_t run = gz_block_scan(s, sh, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) raw_tab[0] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        run += v[k];
        if (i0 + k < n && i0 + k + 1 < cap_records) raw_tab[i0 + k + 1] = run;
    }
}

__global__ __launch_bounds__(256) void rd_bam_raw_base_kernel(const FqSummary *__restrict__ sum, int64_t *__restrict__ raw_tab) {
    __shared__ int64_t sh[4];
    __shared__ int64_t run_s;
    if (!bam_status_framed(sum->status)) return;
    const int64_t nb = sum->n_records / GZ_SCAN_ITEMS;   // blocks that are full: their totals are at (b + 1) * GZ_SCAN_ITEMS <= n_records
    if (threadIdx.x == 0) run_s = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < nb ? raw_tab[(b + 1) * GZ_SCAN_ITEMS] : 0;
        int64_t total;
        const int64_t ex = gz_block_scan(v, sh, total);
        const int64_t run = run_s;
        if (b < nb) raw_tab[(b + 1) * GZ_SCAN_ITEMS] = run + ex + v;
        __syncthreads();
        if (threadIdx.x == 0) run_s = run + total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rd_bam_raw_add_kernel(const FqSummary *__restrict__ sum, int64_t *__restrict__ raw_tab) {
    if (!bam_status_framed(sum->status)) return;
    const int64_t n = sum->n_records;
    const int64_t b0 = ((int64_t)blockIdx.x + 1) * GZ_SCAN_ITEMS;       // (block 0 starts from 0: nothing to add)
    if (b0 >= n) return;
    const int64_t base = raw_tab[b0];                    // final since rd_bam_raw_base_kernel; no workgroup of this launch writes it
    int64_t last = b0 + GZ_SCAN_ITEMS - 1;               // (the entry behind it is the next block's base: final already)
    if (last > n) last = n;
    for (int64_t i = b0 + 1 + threadIdx.x; i <= last; i += 256) raw_tab[i] += base;
}

__global__ __launch_bounds__(FQ_THREADS) void rd_bam_raw_sample_kernel(const int64_t *__restrict__ raw_tab, const FqSummary *__restrict__ sum, int64_t every,
                                                                      int32_t *__restrict__ samples, int64_t cap) {
    const int64_t n = bam_status_framed(sum->status) ? sum->n_records : -1;
    const int64_t stride = (int64_t)gridDim.x * FQ_THREADS;
    for (int64_t k = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; k < cap; k += stride)
        samples[k] = n < 0 ? -1 : (int32_t)raw_tab[k * every < n ? k * every : n];
}

__global__ __launch_bounds__(FQ_THREADS) void rd_bam_raw_gather_kernel(const uint8_t *__restrict__ text, const int32_t *__restrict__ src_tab,
                                                                      const int64_t *__restrict__ raw_tab, const FqSummary *__restrict__ sum, int64_t lo, int64_t hi,
                                                                      uint8_t *__restrict__ out, int64_t out_cap, const int64_t *__restrict__ cursor_in,
                                                                      int64_t *__restrict__ cursor_out, int64_t *__restrict__ raw_start) {
    __shared__ int64_t r_bounds[2];
    const int64_t d0 = *cursor_in;
    const bool ok = bam_status_framed(sum->status) && lo >= 0 && lo <= hi && hi <= sum->n_records && d0 >= 0;
    const int64_t q0 = ok ? raw_tab[lo] : 0, q1 = ok ? raw_tab[hi] : 0;
    const int64_t nbytes = q1 - q0;
    const int64_t gtid = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * FQ_THREADS;
    if (!ok || nbytes < 0 || d0 + nbytes > out_cap) {     // a cursor of -1 poisons every later piece of the chunk: the host sees it in the chunk's total
        if (gtid == 0) *cursor_out = -1;
        return;
    }
    const int64_t d1 = d0 + nbytes, begin = sum->begin, end = sum->end;
    const int64_t shift = d0 - q0;                       // offset in `out` = position in the raw view + shift
    if (nbytes > 0) {
        for (int64_t o0 = (d0 & ~(int64_t)15) + (int64_t)blockIdx.x * BAM_RAW_BYTES; o0 < d1; o0 += (int64_t)gridDim.x * BAM_RAW_BYTES) {
            __syncthreads();
            if (threadIdx.x < 2) {                       // the records of the workgroup's first and last byte: raw_tab[r] <= q < raw_tab[r + 1]
                int64_t o = threadIdx.x ? o0 + BAM_RAW_BYTES - 1 : o0;
                if (o < d0) o = d0;
                if (o > d1 - 1) o = d1 - 1;
                const int64_t q = o - shift;
                int64_t a = lo, b = hi - 1;
                while (a < b) {
                    const int64_t mid = (a + b + 1) >> 1;
                    if (raw_tab[mid] <= q) a = mid; else b = mid - 1;
                }
                r_bounds[threadIdx.x] = a;
            }
            __syncthreads();
            const int64_t o = o0 + 16 * (int64_t)threadIdx.x;
            const int64_t a = o < d0 ? d0 : o, e = o + 16 < d1 ? o + 16 : d1;      // the bytes of this granule that are the piece's
            if (a >= e) continue;
            int64_t r = r_bounds[0], rb = r_bounds[1];
            int64_t q = a - shift;
            while (r < rb) {
                const int64_t mid = (r + rb + 1) >> 1;
                if (raw_tab[mid] <= q) r = mid; else rb = mid - 1;
            }
            int64_t rs = raw_tab[r], re = raw_tab[r + 1], p = src_tab[r];
            const bool whole = a == o && e == o + 16;
            const int64_t s16 = p + (q - rs);
            if (whole && q + 16 <= re && s16 >= begin && s16 + 16 <= end) {
                u32x4 v;
                __builtin_memcpy(&v, text + s16, 16);
                *reinterpret_cast<u32x4 *>(out + o) = v;
                continue;
            }
            unsigned long long out_lo = 0, out_hi = 0;    // the 16 bytes of the granule, little-endian (bytes outside [a, e) stay 0)
#pragma unroll 1
            for (int64_t pos = a; pos < e; ++pos, ++q) {
                while (q >= re && r + 1 < hi) {           // (raw_tab[hi] = q1 > q ends it; records of no bytes are stepped over)
                    ++r;
                    rs = re;
                    re = raw_tab[r + 1];
                    p = src_tab[r];
                }
                const int64_t s = p + (q - rs);
                const unsigned long long c = (s >= begin && s < end) ? text[s] : 0;
                const int j = (int)(pos - o);
                if (j < 8) out_lo |= c << (8 * j); else out_hi |= c << (8 * (j - 8));
            }
            if (whole) {
                u32x4 v = {(uint32_t)out_lo, (uint32_t)(out_lo >> 32), (uint32_t)out_hi, (uint32_t)(out_hi >> 32)};
                *reinterpret_cast<u32x4 *>(out + o) = v;
            } else {
                for (int64_t pos = a; pos < e; ++pos) {
                    const int j = (int)(pos - o);
                    out[pos] = (uint8_t)((j < 8 ? out_lo >> (8 * j) : out_hi >> (8 * (j - 8))) & 0xffu);
                }
            }
        }
    }
    for (int64_t i = gtid; i < hi - lo; i += stride) raw_start[i] = raw_tab[lo + i] + shift;
    if (gtid == 0) {
        raw_start[hi - lo] = d1;
        *cursor_out = d1;
    }
}

}  // namespace
