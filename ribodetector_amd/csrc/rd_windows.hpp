// rd_windows.hpp - reads longer than max_len classified over several windows of max_len bases (`--windows`), on the device (rd_window_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, after rd_scan.hpp, whose scan it uses).
//
// The window rule (one definition: wn_count / wn_start here, ribodetector_amd/windows.py in numpy, README "Windows"): a read of len bases
// with L = max_len, S = stride, K = max_windows has W = 1 window when len <= L, else W = min(K, ceil((len - L) / S) + 1). W == 1: the
// window is the read's own table entry, unchanged. W > 1: window j starts (j (len - L)) / (W - 1) bases in (integer division in int64)
// and has L bases: the first at the read's start, the last at its end, the others evenly between. Integers only, so that the fill pass
// recomputes what the plan pass counted. A window is one more entry of a (seq_off, seq_len) table over the same text: rd_classify takes
// the window table as it takes a read table, and no byte of text is read here.
//
//   rd_window_count_kernel   one thread per 8 reads: W per read, the workgroup's sum (the sums pass of rd_scan.hpp, whose base and
//                            offsets passes make win_first of them: WnLen, WnVerdict); a seq_len < 0 sets the fault word
//   rd_window_fill_kernel    one thread per read: its W table entries from win_first[i] on (W == 1 everywhere: entry i, the stores of a
//                            wave are contiguous). Entries outside [0, total) are not written, whatever win_first says.
//   rd_window_fuse_kernel    one thread per read: its windows' logits in window order -> the read's logits (and label). The order of
//                            the fp32 sum is part of the result (mean), so there is no reduction across lanes.
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"

namespace {

// windows of a read of `len` bases (a negative len counts as one window: the plan's verdict says that nothing is to be trusted)
__device__ __forceinline__ int64_t wn_count(int64_t len, int64_t L, int64_t S, int64_t K) {
    if (len <= L) return 1;
    const int64_t w = (len - L + S - 1) / S + 1;          // (len - L and S are below 2^31: no overflow)
    return w < K ? w : K;
}

// start of window j of a read with W > 1 windows, in bases from the read's start
__device__ __forceinline__ int64_t wn_start(int64_t j, int64_t len, int64_t L, int64_t W) { return j * (len - L) / (W - 1); }

__global__ __launch_bounds__(256) void rd_window_count_kernel(const int32_t *__restrict__ seq_len, int64_t n, int64_t L, int64_t S, int64_t K,
                                                             int64_t *__restrict__ bsum, int32_t *__restrict__ fault) {
    __shared__ int64_t sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * GZ_SCAN_ITEMS + threadIdx.x * 8;
    int64_t s = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (i0 + k < n) {
            const int64_t len = seq_len[i0 + k];
            bad |= len < 0;
            s += wn_count(len, L, S, K);
        }
    if (bad) atomicOr(fault, 1);
    scan_store_sum(s, sh, bsum);
}

// the offsets pass (rd_scan_off_kernel) counts W per read again, then: info = {reads, windows, 0, fault} - the base kernel has set
// info[1] = the total (and info[3] = 0: its limit is INT64_MAX)
struct WnLen {
    const int32_t *seq_len;
    int64_t L, S, K;
    __device__ __forceinline__ int64_t operator()(int, int64_t i) const { return wn_count(seq_len[i], L, S, K); }
};
struct WnVerdict {
    int64_t n;
    const int32_t *fault;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        info[0] = n;
        info[2] = 0;
        if (*fault) info[3] = 1;
    }
};

__global__ __launch_bounds__(256) void rd_window_fill_kernel(const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len,
                                                            const int64_t *__restrict__ win_first, int64_t n, int64_t L, int64_t S, int64_t K,
                                                            int64_t total, int64_t *__restrict__ win_off, int32_t *__restrict__ win_len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t off = seq_off[i], len = seq_len[i], f = win_first[i];
    const int64_t W = wn_count(len, L, S, K);
    if (f < 0 || f > total - W) return;                   // a table that is not this plan's: nothing outside [0, total) is written
    if (W == 1) {
        win_off[f] = off;
        win_len[f] = (int32_t)len;
        return;
    }
#pragma unroll 1
    for (int64_t j = 0; j < W; ++j) {
        win_off[f + j] = off + wn_start(j, len, L, W);
        win_len[f + j] = (int32_t)L;
    }
}

// mode 0 = mean: ((w_0 + w_1) + w_2 + ...) / W, a sequential fp32 sum and one correctly rounded division (W == 1: w_0 bit for bit);
// mode 1 = max: the window with the largest d = w[1] - w[0], the lowest such window on a tie
__global__ __launch_bounds__(256) void rd_window_fuse_kernel(const float2 *__restrict__ win_logits, const int64_t *__restrict__ win_first, int64_t n,
                                                            int mode, int only_multi, float2 *__restrict__ logits, uint8_t *__restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t f = win_first[i], W = win_first[i + 1] - f;
    if (W < 1 || (only_multi && W == 1)) return;
    float2 r = win_logits[f];
    if (mode == 0) {
#pragma unroll 1
        for (int64_t j = 1; j < W; ++j) {
            const float2 w = win_logits[f + j];
            r.x = __fadd_rn(r.x, w.x);
            r.y = __fadd_rn(r.y, w.y);
        }
        const float d = (float)W;
        r.x = __fdiv_rn(r.x, d);
        r.y = __fdiv_rn(r.y, d);
    } else {
        float best = __fsub_rn(r.y, r.x);
#pragma unroll 1
        for (int64_t j = 1; j < W; ++j) {
            const float2 w = win_logits[f + j];
            const float d = __fsub_rn(w.y, w.x);
            if (d > best) { best = d; r = w; }
        }
    }
    logits[i] = r;
    if (labels) labels[i] = r.y > r.x ? 1 : 0;
}

}  // namespace
