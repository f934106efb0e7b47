// rd_summary.hpp - the QC counters of a run (`--summary`), accumulated on the device chunk by chunk (rd_summary_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, after rd_pairs.hpp).
//
// Everything the counters need is in HBM when a chunk's labels exist: the text, the mates' sequence tables, the final logits and the
// int8 labels. The layout of the int64 accumulator (RD_SUM_*) and the meaning of every section are in include/ribodetector_amd.h.
// Integer sums: the result is exact and does not depend on the order of the adds, the chunking or the number of ranks.
//
//   rd_summary_check_kernel  one thread per unit: a label outside -1..1, a seq_len < 0 or a sequence outside its text sets info[0]
//   rd_summary_acc_kernel    returns at once when info[0] is set (a faulty chunk adds nothing). A workgroup takes SM_UNITS consecutive
//                            units and counts them into histograms in LDS laid out like the accumulator; every thread reads its
//                            reads' bytes once, 16 per load, with the base counts in registers. One 64-bit atomicAdd per non-zero bin
//                            moves the histograms to the accumulator.
// The LDS bins are 32 bits wide: every bin but those of `bases` gets at most one count per read, and a workgroup counts at most SM_UNITS
// reads per mate, so none exceeds SM_UNITS. The bins of `bases` (up to 2^31 - 1 per read) are 64 bits wide.
// In a 100 bp run every lane of a wave holds the same length bin and class and one of a few p bins, and same-address LDS atomics of a
// wave serialize. sm_add therefore counts in the wave first: up to SM_AGG rounds, each of which takes the key of the first lane left,
// counts the lanes that hold it with a ballot and adds them with ONE atomic; lanes still left after that (keys of many values: GC,
// lengths of a variable-length run) add one by one. The base counts are summed per class over a thread's units in registers and over
// the wave with shuffles: one 64-bit LDS add per wave, class and code.
#pragma once
#include "rd_common.hpp"

namespace {

constexpr int SM_UPT = 4;                       // units per thread
constexpr int SM_UNITS = 256 * SM_UPT;          // units per workgroup: the bound of every 32-bit LDS bin
constexpr int SM_AGG = 4;                       // rounds of wave-level counting in front of the lane-by-lane adds
constexpr int SM_NBASES = 2 * 3 * 5;

static_assert(RD_SUM_MATE_LABELS == RD_SUM_UNITS + 3 && RD_SUM_LENGTH == RD_SUM_MATE_LABELS + 3 * 2 * 2 &&
              RD_SUM_P_RRNA == RD_SUM_LENGTH + 2 * 3 * RD_SUM_LEN_BINS && RD_SUM_BASES == RD_SUM_P_RRNA + 3 * 3 * RD_SUM_P_BINS &&
              RD_SUM_GC == RD_SUM_BASES + SM_NBASES && RD_SUM_WORDS == RD_SUM_GC + 2 * 3 * RD_SUM_GC_BINS,
              "the RD_SUM_* sections follow each other without gaps");

__global__ __launch_bounds__(256) void rd_summary_check_kernel(int64_t bytes_a, const int64_t *__restrict__ off_a, const int32_t *__restrict__ len_a,
                                                              int64_t bytes_b, const int64_t *__restrict__ off_b, const int32_t *__restrict__ len_b,
                                                              const int8_t *__restrict__ labels, int64_t n, int64_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long f = 0;
    const int l = labels[i];
    if (l < -1 || l > 1) f |= 1;
    {
        const int64_t o = off_a[i], L = len_a[i];
        if (L < 0) f |= 2; else if (o < 0 || o > bytes_a - L) f |= 4;
    }
    if (off_b) {
        const int64_t o = off_b[i], L = len_b[i];
        if (L < 0) f |= 2; else if (o < 0 || o > bytes_b - L) f |= 4;
    }
    if (f) atomicOr((unsigned long long *)info, f);
}

// h[key] += 1 for every lane with `valid`. Every lane of the wave calls it (the ballots need them all); see the head of the file.
__device__ __forceinline__ void sm_add(uint32_t *h, int key, bool valid) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < SM_AGG; ++r) {
        const unsigned long long left = __ballot(valid);
        if (!left) return;
        const int first = __ffsll(left) - 1;
        const int k = __shfl(key, first);
        const bool mine = valid && key == k;
        const unsigned long long same = __ballot(mine);
        if (lane == first) atomicAdd(h + k, (uint32_t)__popcll(same));
        valid = valid && !mine;
    }
    if (valid) atomicAdd(h + key, 1u);
}

// how many of the 4 bytes of w equal the byte that pat repeats
__device__ __forceinline__ uint32_t sm_eq4(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;        // bit 7 of a byte: its low 7 bits are not all zero (no carry leaves a byte)
    return (uint32_t)__popc(~(t | x | 0x7f7f7f7fu));           // 0x80 for every zero byte of x
}

__device__ __forceinline__ int sm_pbin(float d) {
    const uint32_t b = rp_q(d) / 100u;
    return (int)(b < RD_SUM_P_BINS - 1 ? b : RD_SUM_P_BINS - 1);
}

__global__ __launch_bounds__(256) void rd_summary_acc_kernel(const uint8_t *__restrict__ text_a, const int64_t *__restrict__ off_a,
                                                            const int32_t *__restrict__ len_a, const float *__restrict__ la,
                                                            const uint8_t *__restrict__ text_b, const int64_t *__restrict__ off_b,
                                                            const int32_t *__restrict__ len_b, const float *__restrict__ lb,
                                                            const int8_t *__restrict__ labels, int64_t n, int64_t *__restrict__ acc,
                                                            int64_t *__restrict__ info) {
    __shared__ uint32_t h[RD_SUM_WORDS];                  // (the words of `bases` stay unused: those bins are hb's)
    __shared__ unsigned long long hb[SM_NBASES];
    if (info[0]) return;                                  // the check pass found a bad entry: nothing is read, nothing is added
    for (int k = threadIdx.x; k < RD_SUM_WORDS; k += 256) h[k] = 0;
    if (threadIdx.x < SM_NBASES) hb[threadIdx.x] = 0;
    __syncthreads();
    const bool paired = text_b != nullptr;
    const int64_t base = (int64_t)blockIdx.x * SM_UNITS + threadIdx.x;
    // the unit's label and logits: units, mate_labels, p_rrna
#pragma unroll 1
    for (int j = 0; j < SM_UPT; ++j) {
        const int64_t i = base + (int64_t)j * 256;
        const bool valid = i < n;
        int c = 0;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        if (valid) {
            c = labels[i] + 1;
            a0 = la[2 * i];
            a1 = la[2 * i + 1];
            if (paired) {
                b0 = lb[2 * i];
                b1 = lb[2 * i + 1];
            }
        }
        sm_add(h, RD_SUM_UNITS + c, valid);
        sm_add(h, RD_SUM_P_RRNA + c * RD_SUM_P_BINS + sm_pbin(a1 - a0), valid);
        if (paired) {
            sm_add(h, RD_SUM_MATE_LABELS + c * 4 + (a1 > a0 ? 2 : 0) + (b1 > b0 ? 1 : 0), valid);
            sm_add(h, RD_SUM_P_RRNA + (3 + c) * RD_SUM_P_BINS + sm_pbin(b1 - b0), valid);
            sm_add(h, RD_SUM_P_RRNA + (6 + c) * RD_SUM_P_BINS + sm_pbin((a1 + b1) - (a0 + b0)), valid);    // the summed logits, as the report forms them
        }
    }
    // the reads' bytes, mate by mate: length, gc, bases
    for (int m = 0; m < (paired ? 2 : 1); ++m) {
        const uint8_t *__restrict__ text = m ? text_b : text_a;
        const int64_t *__restrict__ off = m ? off_b : off_a;
        const int32_t *__restrict__ len = m ? len_b : len_a;
        unsigned long long bs[3][5] = {};                 // this thread's bases by class and code
#pragma unroll 1
        for (int j = 0; j < SM_UPT; ++j) {
            const int64_t i = base + (int64_t)j * 256;
            const bool valid = i < n;
            int c = 0;
            uint32_t L = 0, cnt[4] = {0u, 0u, 0u, 0u};
            if (valid) {
                c = labels[i] + 1;
                L = (uint32_t)len[i];
                int64_t p = off[i];
                const int64_t e = p + L;
                for (; p + 16 <= e; p += 16) {            // 16 bytes per step while they lie inside the sequence
                    u32x4 v;
                    __builtin_memcpy(&v, text + p, 16);
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        cnt[0] += sm_eq4(v[w], 0x41414141u);
                        cnt[1] += sm_eq4(v[w], 0x43434343u);
                        cnt[2] += sm_eq4(v[w], 0x47474747u);
                        cnt[3] += sm_eq4(v[w], 0x54545454u) + sm_eq4(v[w], 0x55555555u);
                    }
                }
                for (; p < e; ++p) {
                    const int k = rd_code(text[p]);
                    cnt[0] += k == 0;
                    cnt[1] += k == 1;
                    cnt[2] += k == 2;
                    cnt[3] += k == 3;
                }
            }
            const int mc = m * 3 + c;
            sm_add(h, RD_SUM_LENGTH + mc * RD_SUM_LEN_BINS + (int)(L < RD_SUM_LEN_BINS - 1 ? L : RD_SUM_LEN_BINS - 1), valid);
            const uint32_t cg = cnt[1] + cnt[2], tot = cnt[0] + cnt[3] + cg;
            const uint32_t gc = tot == 0 ? 0u : tot <= 0xffffffffu / 100u ? 100u * cg / tot : (uint32_t)(100ull * cg / tot);
            sm_add(h, RD_SUM_GC + mc * RD_SUM_GC_BINS + (int)gc, valid && tot != 0);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
#pragma unroll
                for (int k = 0; k < 4; ++k) bs[cc][k] += c == cc ? cnt[k] : 0u;
                bs[cc][4] += c == cc ? L - tot : 0u;
            }
        }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                unsigned long long v = bs[cc][k];
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
                if ((threadIdx.x & 63) == 0 && v) atomicAdd(hb + (m * 3 + cc) * 5 + k, v);
            }
    }
    __syncthreads();
    unsigned long long *out = (unsigned long long *)acc;
    for (int k = threadIdx.x; k < RD_SUM_WORDS; k += 256) {
        const unsigned long long v = k >= RD_SUM_BASES && k < RD_SUM_BASES + SM_NBASES ? hb[k - RD_SUM_BASES] : h[k];
        if (v) atomicAdd(out + k, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info[1] = n;
}

}  // namespace
