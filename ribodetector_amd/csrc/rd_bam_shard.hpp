// rd_bam_shard.hpp - a BAM file shared by the ranks of a run: a record start behind an arbitrary offset, the records of a share
// Part of the single translation unit rd_kernels.hip (included from there, behind rd_bam_index.hpp); DESIGN.md §3.24. The rule is
// ribodetector_amd/bam.py (plausible / chain_verdict / find_record_start): info[0] and info[1] equal its answer on every input.
//
// BAM records are a length-prefixed chain: nothing in the bytes marks a record start the way '\n@' marks one in FASTQ text. What can be
// tested at an arbitrary offset is the SIGNATURE of a record (bam_plausible, rd_bam_index.hpp), and a signature that is followed, along
// the chain of block_size fields, by RD_BAM_CONFIRM - 1 more: the bytes of a base, quality or tag block imitate one record now and then,
// never a row of them - unless a payload holds records (the documented false hit; the run that cuts there fails at that rank's last
// batch).
//
//   rd_bam_find_kernel   a workgroup takes BAM_FIND_CAND consecutive candidates and stages them, with the BAM_REACH bytes behind them, in
//                        LDS (as the walk kernel stages a segment); a lane per offset tests the signature there, a ballot picks the
//                        hits, and each hit follows its chain in global memory (rare: the true starts and the occasional accident).
//                        The smallest confirmed and the smallest undecided candidate: 64-bit atomic minima (unsigned: -1, "none", is
//                        the largest value). A workgroup whose candidates all lie behind both minima leaves at once.
//
// rd_bam_count is rd_bam_index's walk and stitch instantiated without tables (rd_bam_walk_kernel<false> / rd_bam_stitch_kernel<false>).
//
// Every length is DATA: block_size is compared with `end` in 64-bit arithmetic before the chain moves on, bam_plausible compares
// every offset it reads with `end` first.
#pragma once
#include "rd_bam_index.hpp"

namespace {

constexpr int BAM_FIND_THREADS = 256;
constexpr int BAM_FIND_CAND = 4096;                               // candidates per workgroup
constexpr int BAM_FIND_STAGE = BAM_FIND_CAND + 16 + BAM_REACH;    // (+ 16: the stage starts at the 16-byte boundary in front of them)
enum { BAM_REJECTED = 0, BAM_CONFIRMED = 1, BAM_UNDECIDED = -1 };

// bam.chain_verdict: the chain from q, RD_BAM_CONFIRM records of it
__device__ __forceinline__ int bam_chain_verdict(const BamBytes &g, int64_t q, int64_t end, bool at_eof) {
    int64_t p = q;
    for (int i = 0; i < RD_BAM_CONFIRM; ++i) {
        if (p == end) return at_eof ? BAM_CONFIRMED : BAM_UNDECIDED;
        if (p + 36 > end) return at_eof ? BAM_REJECTED : BAM_UNDECIDED;
        if (!bam_plausible(g, p, end)) return BAM_REJECTED;
        const int64_t block = (int64_t)(int32_t)g.u32(p);         // (33 .. 2^26: plausible)
        if (p + 4 + block > end) return at_eof ? BAM_REJECTED : BAM_UNDECIDED;
        p += 4 + block;
    }
    return BAM_CONFIRMED;
}

__global__ void rd_bam_find_init_kernel(unsigned long long *__restrict__ info, int bad) {
    info[0] = info[1] = ~0ull;
    info[2] = 0;
    info[3] = (unsigned long long)bad;
}

__global__ __launch_bounds__(BAM_FIND_THREADS) void rd_bam_find_kernel(const uint8_t *__restrict__ text, int64_t lo, int64_t hi, int64_t end, int at_eof,
                                                                      unsigned long long *__restrict__ info) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[BAM_FIND_STAGE];
    const int64_t c_lo = lo + (int64_t)blockIdx.x * BAM_FIND_CAND;
    int64_t c_hi = c_lo + BAM_FIND_CAND;
    if (c_hi > hi) c_hi = hi;
    // (unsigned: "none" is larger than every offset. A value read here is a bound: the minima only fall. One thread reads, so that the
    // whole workgroup takes the same way)
    __shared__ int s_leave;
    if (threadIdx.x == 0) {
        const unsigned long long f0 = __hip_atomic_load(&info[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long u0 = __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_leave = (unsigned long long)c_lo > f0 && (unsigned long long)c_lo > u0;
    }
    __syncthreads();
    if (s_leave) return;
    // [a0, stop) -> LDS: aligned 16-byte pieces as long as they lie in front of `end` as a whole, bytes behind
    const int64_t a0 = c_lo & ~(int64_t)15;
    int64_t stop = c_hi + BAM_REACH;
    if (stop > end) stop = end;
    for (int64_t a = a0 + 16 * (int64_t)threadIdx.x; a < stop; a += 16 * BAM_FIND_THREADS) {
        if (a + 16 <= end) {
            *reinterpret_cast<u32x4 *>(stage + (a - a0)) = *reinterpret_cast<const u32x4 *>(text + a);
        } else {
            for (int64_t k = a; k < end; ++k) stage[k - a0] = text[k];
        }
    }
    __syncthreads();
    const BamBytes b = {stage, a0}, g = {text, 0};
    // every read of the stage is of an offset < min(c_hi + BAM_REACH, end): bam_plausible compares with `end` first and reads the 36 fixed
    // bytes and a name of at most 255 behind a candidate < c_hi
    for (int64_t q0 = c_lo + (int64_t)(threadIdx.x & ~63); q0 < c_hi; q0 += BAM_FIND_THREADS) {
        const int64_t q = q0 + (threadIdx.x & 63);
        // a candidate with fewer than 36 bytes in front of `end` cannot be tested: its verdict is the chain's (undecided, or rejected at_eof)
        const bool hit = q < c_hi && (q + 36 > end || bam_plausible(b, q, end));
        if (!__ballot(hit)) continue;
        if (hit) {
            const int v = bam_chain_verdict(g, q, end, at_eof != 0);
            if (v == BAM_CONFIRMED) atomicMin(&info[0], (unsigned long long)q);
            else if (v == BAM_UNDECIDED) atomicMin(&info[1], (unsigned long long)q);
        }
    }
}

struct BamCountWs {
    int nseg;
    BamSeg *seg;
    size_t total;
};
BamCountWs bam_count_ws(void *workspace, int64_t text_end) {
    BamCountWs p;
    Carver c(workspace);
    p.nseg = (int)(text_end / BAM_S) + 1;
    p.seg = c.take<BamSeg>((size_t)p.nseg);
    p.total = c.off;
    return p;
}

}  // namespace
