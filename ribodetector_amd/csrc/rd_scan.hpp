// rd_scan.hpp - per-item lengths -> exclusive offsets, the scan under every per-record device output (rd_scan_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, in front of rd_deflate.hpp).
//
// Three passes over n items, 256 x ITEMS of them per workgroup (ITEMS = 8: GZ_SCAN_ITEMS per workgroup; 1: one item per lane):
//   sums      bsum[workgroup] = the sum of its items' lengths: rd_scan_sum_kernel, or the caller's own count pass where the lengths
//             are computed first (it ends in scan_store_sum)
//   base      rd_scan_base_kernel, one workgroup: bsum[] -> exclusive bases in place; the total and the limit check into four words.
//             Word [2], the total in units of `member`, is the gzip path's member count and means something with member =
//             GZ_MEMBER only: every other caller passes 1 and overwrites info[2] in its verdict or never reads it
//   offsets   rd_scan_off_kernel: off[i] = the lengths before item i, entry n = the total; thread 0 of workgroup 0 then runs the
//             caller's verdict, which reads the base pass's words and fills the caller's info[]
// A caller is two by-value functors: len(t, i) = the length of item i < n in table t (T tables are scanned by one offsets launch;
// ScanTab: the lengths stand in the offsets' table, which is scanned in place), and verdict().
#pragma once
#include "rd_common.hpp"

namespace {

constexpr int GZ_SCAN_ITEMS = 2048;   // items per workgroup (256 threads x 8)

__device__ __forceinline__ int64_t gz_block_scan(int64_t v, int64_t *sh, int64_t &total) {   // exclusive scan over the 256 threads
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + inc - v;
}

// the end of a sums pass: s = this thread's share of the workgroup's lengths
__device__ __forceinline__ void scan_store_sum(int64_t s, int64_t *sh, int64_t *__restrict__ bsum) {
    int64_t total;
    gz_block_scan(s, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

template <int T>
struct ScanTab {                       // lengths that stand in a table (in the offsets' own: every thread reads its items before it writes them)
    const int64_t *tab[T];
    __device__ __forceinline__ int64_t operator()(int t, int64_t i) const { return tab[t][i]; }
};
template <int T>
struct ScanOut {                       // per table: the offsets (n + 1 entries) and the workgroups' bases
    int64_t *off[T];
    const int64_t *bbase[T];
};
struct ScanNoVerdict {
    __device__ __forceinline__ void operator()() const {}
};

template <int ITEMS, class Len>
__global__ __launch_bounds__(256) void rd_scan_sum_kernel(Len len, int64_t n, int64_t *__restrict__ bsum) {
    __shared__ int64_t sh[4];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ITEMS;
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s += i0 + k < n ? len(0, i0 + k) : 0;
    scan_store_sum(s, sh, bsum);
}

// one workgroup: bsum[] -> exclusive bases in place; info = {0, total, total in units of `member` (rounded up), 0}, or {0, 0, 0, 1}
// when the total exceeds `limit`: the caller's output or workspace does not hold it, and the passes behind write nothing
__global__ __launch_bounds__(256) void rd_scan_base_kernel(int64_t *__restrict__ bsum, int nb, int64_t *__restrict__ info, int64_t limit, int64_t member) {
    __shared__ int64_t sh[4];
    __shared__ int64_t run_s;
    if (threadIdx.x == 0) run_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int64_t v = b < nb ? bsum[b] : 0;
        int64_t total;
        const int64_t ex = gz_block_scan(v, sh, total);
        const int64_t run = run_s;
        if (b < nb) bsum[b] = run + ex;
        __syncthreads();
        if (threadIdx.x == 0) run_s = run + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool bad = run_s > limit || run_s < 0;
        info[0] = 0;
        info[1] = bad ? 0 : run_s;
        info[2] = bad ? 0 : (run_s + member - 1) / member;
        info[3] = bad ? 1 : 0;
    }
}

// the base pass of a scan of nb workgroups (member: the gzip path's bytes per member; the other callers read no info[2])
inline void scan_base(int64_t *bsum, int nb, int64_t *info, int64_t limit, hipStream_t st, int64_t member = 1) {
    hipLaunchKernelGGL(rd_scan_base_kernel, dim3(1), dim3(256), 0, st, bsum, nb, info, limit, member);
}

template <int ITEMS, int T, class Len, class Verdict>
__global__ __launch_bounds__(256) void rd_scan_off_kernel(Len len, int64_t n, ScanOut<T> o, Verdict verdict) {
    __shared__ int64_t sh[4];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ITEMS;
    int64_t v[T][ITEMS], s[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        s[t] = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { v[t][k] = i0 + k < n ? len(t, i0 + k) : 0; s[t] += v[t][k]; }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        int64_t total;
        int64_t run = o.bbase[t][blockIdx.x] + gz_block_scan(s[t], sh, total);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (i0 + k <= n) o.off[t][i0 + k] = run;      // (entry n = the total)
            run += v[t][k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) verdict();
}

// workgroups of a sums or offsets pass over n items (n + 1 entries), and so the entries of bsum
constexpr int scan_blocks(int64_t n, int items = 8) { return (int)((n + 1 + 256 * items - 1) / (256 * items)); }

}  // namespace
