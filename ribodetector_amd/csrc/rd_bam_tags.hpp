// rd_bam_tags.hpp - the optional fields (tags) of raw BAM records on the device, and the per-read-group counters built on them (rd_bam_tag_* /
// rd_bam_group_* kernels). Part of the single translation unit rd_kernels.hip (included from there, behind rd_summary.hpp); DESIGN.md §3.23.
// The rule is ribodetector_amd/bam.py (find_tag, group_row): every table written here equals that serial walk.
//
//   rd_bam_tag_find_kernel<L>   L lanes (4 or 16; any power of two up to 64 works) per record of a raw view (raw_start[k] .. raw_start[k + 1]). The walk over the tags is
//                               the same in every lane of a group; the search for the NUL of a Z / H value is shared: lane j of the group looks
//                               at bytes [16 j, 16 j + 16) of a step of 16 L bytes with one 16-byte load, and a ballot finds the first NUL. The
//                               loop is a state machine that the whole wave steps together (a group that is done idles), so that the ballot
//                               and the shuffle are executed by all 64 lanes. Every length is data: it is compared in 64-bit arithmetic with the
//                               record's end E before a byte it points to is read, and E itself is clamped by raw_start[k + 1].
//   rd_bam_group_rows_kernel    one thread per record: binary search of the value among the sorted ids (unsigned bytes, a prefix first)
//   rd_bam_group_check_kernel   a label outside -1..1 or a row outside 0..G + 2 (of either mate) sets info[0]
//   rd_bam_group_acc_kernel     returns at once when info[0] is set. A unit's key is row * 3 + class; a wave first counts its lanes per key
//                               (ballot) and sums their bases (shuffles), as rd_summary.hpp's sm_add does - one read group per file is the
//                               common case and then a wave holds at most 3 keys. Up to GR_LDS_KEYS keys (682 groups) the wave's sums go to
//                               the workgroup's LDS bins (32-bit counts: a workgroup counts fewer than 2^32 units; 64-bit bases), and the
//                               non-zero bins to the accumulator with one 64-bit atomic each when the workgroup has walked its share of the
//                               units; with more keys the wave's sums go to the accumulator directly.
#pragma once
#include "rd_common.hpp"

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_LDS_KEYS = 2048;               // keys (row, class) that the workgroup's LDS bins hold: G + 3 <= 682
constexpr int GR_AGG = 4;                       // rounds of wave-level counting in front of the lane-by-lane adds
constexpr int GR_MAX_WGS = 512;                 // workgroups of the accumulate pass: each one flushes its bins once

// index (0..15) of the first zero byte of the 16 bytes v holds, 16 when there is none
__device__ __forceinline__ int tg_first_zero(u32x4 v) {
    int at = 16;
#pragma unroll
    for (int w = 3; w >= 0; --w) {
        const uint32_t x = v[w];
        const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);      // 0x80 in every byte of x that is zero
        if (t) at = 4 * w + ((__ffs((int)t) - 1) >> 3);
    }
    return at;
}

__device__ __forceinline__ int tg_elem_size(uint8_t t) {        // a B array's element, 0: not a subtype
    return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0;
}

template <int L>
__global__ __launch_bounds__(GR_THREADS) void rd_bam_tag_find_kernel(const uint8_t *__restrict__ raw, int64_t raw_bytes, const int64_t *__restrict__ raw_start,
                                                                    int64_t n_rec, uint32_t want, int64_t *__restrict__ val_off, int32_t *__restrict__ val_len,
                                                                    uint8_t *__restrict__ val_type) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1), gbase = lane & ~(L - 1);
    const unsigned long long gmask = L == 64 ? ~0ull : ((1ull << L) - 1ull) << gbase;
    const int64_t k = ((int64_t)blockIdx.x * GR_THREADS + threadIdx.x) / L;
    // state of the group's walk: p = where the next tag starts, or in a search: the next byte to look at
    int64_t p = 0, E = 0, v0 = 0, res_off = -2;
    int res_len = 0, res_type = 0;
    bool done = k >= n_rec, searching = false, hit_tag = false;
    uint8_t cur_type = 0;
    if (!done) {
        const int64_t s = raw_start[k], e = raw_start[k + 1];
        done = true;                                      // (malformed until the fixed fields say otherwise)
        if (s >= 0 && s <= e && e <= raw_bytes && e - s >= 36) {
            uint32_t block, lseq;
            uint16_t ncig;
            __builtin_memcpy(&block, raw + s, 4);
            __builtin_memcpy(&ncig, raw + s + 16, 2);
            __builtin_memcpy(&lseq, raw + s + 20, 4);
            const int64_t bs = (int32_t)block, ls = (int32_t)lseq;
            E = s + 4 + bs;
            p = s + 36 + (int64_t)raw[s + 12] + 4 * (int64_t)ncig + (ls + 1) / 2 + ls;
            if (bs >= 32 && E <= e && ls >= 0 && p <= E) {
                done = false;
                if (p == E) { done = true; res_off = -1; }
            }
        }
    }
    for (;;) {
        if (!__ballot(!done)) break;                      // (wave-uniform: the ballots and the shuffle below are executed by every lane)
        // one step of every group that is searching: 16 L bytes from p
        int z = 16;
        if (!done && searching) {
            const int64_t a = p + 16 * sub;
            if (a + 16 <= E) {
                u32x4 w;
                __builtin_memcpy(&w, raw + a, 16);
                z = tg_first_zero(w);
            } else {
                for (int64_t q = a; q < E; ++q)
                    if (raw[q] == 0) { z = (int)(q - a); break; }
            }
        }
        const unsigned long long found = __ballot(z < 16) & gmask;
        const int first = found ? __ffsll((long long)found) - 1 : gbase;
        const int zf = __shfl(z, first);
        if (!done && searching) {
            if (found) {
                const int64_t q = p + 16 * (int64_t)(first - gbase) + zf;      // the NUL
                searching = false;
                if (hit_tag) { done = true; res_off = v0; res_len = (int)(q - v0); res_type = cur_type; }
                else {
                    p = q + 1;
                    if (p == E) { done = true; res_off = -1; }
                }
            } else {
                p += 16 * L;
                if (p >= E) done = true;                  // no NUL in front of the record's end: malformed (res_off is -2)
            }
        } else if (!done) {                               // the head of the tag at p (p < E)
            if (E - p < 3) { done = true; continue; }
            const uint32_t name = (uint32_t)raw[p] | ((uint32_t)raw[p + 1] << 8);
            const uint8_t t = raw[p + 2];
            const int64_t v = p + 3;
            hit_tag = name == want;
            int64_t size = -1;                            // bytes of a value of known size; -1: malformed
            if (t == 'A' || t == 'c' || t == 'C') size = 1;
            else if (t == 's' || t == 'S') size = 2;
            else if (t == 'i' || t == 'I' || t == 'f') size = 4;
            else if (t == 'Z' || t == 'H') {
                searching = true;
                cur_type = t;
                v0 = p = v;
                if (p >= E) done = true;                  // (no byte left for the NUL)
                continue;
            } else if (t == 'B' && v + 5 <= E) {
                const int es = tg_elem_size(raw[v]);
                uint32_t count;
                __builtin_memcpy(&count, raw + v + 1, 4);
                if (es) size = 5 + (int64_t)count * es;   // (< 2^35: no overflow)
            }
            if (size < 0 || v + size > E) { done = true; continue; }
            if (hit_tag) { done = true; res_off = v; res_len = (int)size; res_type = t; continue; }
            p = v + size;
            if (p == E) { done = true; res_off = -1; }
        }
    }
    if (k < n_rec && sub == 0) {
        val_off[k] = res_off;
        val_len[k] = res_off >= 0 ? res_len : 0;
        val_type[k] = res_off >= 0 ? (uint8_t)res_type : (uint8_t)0;
    }
}

template <int L>
void tag_find_launch(const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start, int64_t n_rec, uint32_t want, int64_t *val_off, int32_t *val_len,
                     uint8_t *val_type, hipStream_t st) {
    const int64_t per = GR_THREADS / L;
    hipLaunchKernelGGL(rd_bam_tag_find_kernel<L>, dim3((unsigned)((n_rec + per - 1) / per)), dim3(GR_THREADS), 0, st, raw, raw_bytes, raw_start, n_rec, want, val_off,
                       val_len, val_type);
}

__global__ __launch_bounds__(GR_THREADS) void rd_bam_group_rows_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ val_off,
                                                                      const int32_t *__restrict__ val_len, const uint8_t *__restrict__ val_type, int64_t n_rec,
                                                                      const uint8_t *__restrict__ dict, const int32_t *__restrict__ dict_off, int32_t G,
                                                                      int32_t *__restrict__ rows) {
    const int64_t k = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    if (k >= n_rec) return;
    const int64_t vo = val_off[k];
    if (vo == -1) { rows[k] = G; return; }
    if (vo < 0 || val_type[k] != 'Z') { rows[k] = G + 2; return; }
    const int32_t vl = val_len[k];
    const uint8_t *__restrict__ val = raw + vo;
    int lo = 0, hi = G - 1, row = G + 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t d0 = dict_off[mid], dl = dict_off[mid + 1] - d0;
        const int32_t m = vl < dl ? vl : dl;
        int cmp = 0;                                      // value <=> ids[mid]: the first differing byte, unsigned; else the shorter one first
        for (int32_t i = 0; i < m; ++i) {
            const int a = val[i], b = dict[d0 + i];
            if (a != b) { cmp = a < b ? -1 : 1; break; }
        }
        if (cmp == 0) cmp = vl < dl ? -1 : vl > dl ? 1 : 0;
        if (cmp == 0) { row = mid; break; }
        if (cmp < 0) hi = mid - 1; else lo = mid + 1;
    }
    rows[k] = row;
}

// bytes [at, at + 8) of a string of len bytes as a big-endian word, zeros behind its end: neither an id (header text) nor a Z value holds
// a NUL, so comparing two strings' words in turn is comparing the strings - unsigned bytes, the shorter one first
__device__ __forceinline__ unsigned long long gr_key8(const uint8_t *__restrict__ s, int len, int at) {
    unsigned long long k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) k = (k << 8) | (at + i < len ? (unsigned long long)s[at + i] : 0ull);
    return k;
}

// the same search with the dictionary in LDS (G <= GR_ROWS_LDS): the first 16 bytes of every id as two big-endian words, so that a step of the
// search is two LDS reads instead of a chain of global byte loads. Only an id and a value that agree in 16 bytes and go on are
// compared further, byte by byte in global memory. A workgroup stages the dictionary once and walks its share of the records.
constexpr int GR_ROWS_LDS = 1024;

__global__ __launch_bounds__(GR_THREADS) void rd_bam_group_rows_lds_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ val_off,
                                                                          const int32_t *__restrict__ val_len, const uint8_t *__restrict__ val_type, int64_t n_rec,
                                                                          const uint8_t *__restrict__ dict, const int32_t *__restrict__ dict_off, int32_t G,
                                                                          int32_t *__restrict__ rows) {
    __shared__ unsigned long long key_hi[GR_ROWS_LDS], key_lo[GR_ROWS_LDS];
    __shared__ int32_t d_off[GR_ROWS_LDS + 1];
    for (int j = threadIdx.x; j <= G; j += GR_THREADS) d_off[j] = dict_off[j];
    __syncthreads();
    for (int j = threadIdx.x; j < G; j += GR_THREADS) {
        const int32_t d0 = d_off[j], dl = d_off[j + 1] - d0;
        key_hi[j] = gr_key8(dict + d0, dl, 0);
        key_lo[j] = gr_key8(dict + d0, dl, 8);
    }
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x; k < n_rec; k += (int64_t)gridDim.x * GR_THREADS) {
        const int64_t vo = val_off[k];
        if (vo == -1) { rows[k] = G; continue; }
        if (vo < 0 || val_type[k] != 'Z') { rows[k] = G + 2; continue; }
        const int32_t vl = val_len[k];
        const uint8_t *__restrict__ val = raw + vo;
        const unsigned long long v_hi = gr_key8(val, vl, 0), v_lo = gr_key8(val, vl, 8);
        int lo = 0, hi = G - 1, row = G + 1;
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            const unsigned long long m_hi = key_hi[mid], m_lo = key_lo[mid];
            int cmp = v_hi != m_hi ? (v_hi < m_hi ? -1 : 1) : v_lo != m_lo ? (v_lo < m_lo ? -1 : 1) : 0;
            if (cmp == 0) {                               // the same first 16 bytes (or the same string of fewer)
                const int32_t d0 = d_off[mid], dl = d_off[mid + 1] - d0;
                const int32_t m = vl < dl ? vl : dl;
                for (int32_t i = 16; i < m; ++i) {
                    const int a = val[i], b = dict[d0 + i];
                    if (a != b) { cmp = a < b ? -1 : 1; break; }
                }
                if (cmp == 0) cmp = vl < dl ? -1 : vl > dl ? 1 : 0;
            }
            if (cmp == 0) { row = mid; break; }
            if (cmp < 0) hi = mid - 1; else lo = mid + 1;
        }
        rows[k] = row;
    }
}

__global__ __launch_bounds__(GR_THREADS) void rd_bam_group_check_kernel(const int32_t *__restrict__ rows_a, int64_t first_a, int64_t stride_a,
                                                                       const int32_t *__restrict__ rows_b, int64_t first_b, int64_t stride_b,
                                                                       const int8_t *__restrict__ labels, int64_t n, int32_t G, int64_t *__restrict__ info) {
    const int64_t u = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    if (u >= n) return;
    unsigned long long f = 0;
    const int l = labels[u];
    if (l < -1 || l > 1) f |= 1;
    const int32_t g = rows_a[first_a + stride_a * u];
    if (g < 0 || g > G + 2) f |= 2;
    if (rows_b) {
        const int32_t h = rows_b[first_b + stride_b * u];
        if (h < 0 || h > G + 2) f |= 2;
    }
    if (f) atomicOr((unsigned long long *)info, f);
}

__device__ __forceinline__ unsigned long long gr_wave_sum(unsigned long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__global__ __launch_bounds__(GR_THREADS) void rd_bam_group_acc_kernel(const uint8_t *__restrict__ raw_a, const int64_t *__restrict__ start_a,
                                                                     const int32_t *__restrict__ rows_a, int64_t first_a, int64_t stride_a,
                                                                     const uint8_t *__restrict__ raw_b, const int64_t *__restrict__ start_b,
                                                                     const int32_t *__restrict__ rows_b, int64_t first_b, int64_t stride_b,
                                                                     const int8_t *__restrict__ labels, int64_t n, int32_t G, int64_t *__restrict__ acc,
                                                                     int64_t *__restrict__ info) {
    __shared__ uint32_t h_units[GR_LDS_KEYS];
    __shared__ unsigned long long h_bases[GR_LDS_KEYS];
    __shared__ uint32_t h_differ;
    if (info[0]) return;                                  // the check pass found a bad entry: nothing is read, nothing is added
    const int nkeys = (G + 3) * 3;
    const bool lds = nkeys <= GR_LDS_KEYS;
    unsigned long long *out = (unsigned long long *)acc;
    if (lds)
        for (int k = threadIdx.x; k < nkeys; k += GR_THREADS) { h_units[k] = 0; h_bases[k] = 0; }
    if (threadIdx.x == 0) h_differ = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t tiles = (n + GR_THREADS - 1) / GR_THREADS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {             // (workgroup-uniform: every lane of a wave takes part in the ballots)
        const int64_t u = t * GR_THREADS + threadIdx.x;
        bool valid = u < n;
        int key = 0;
        unsigned long long bases = 0;
        bool differ = false;
        if (valid) {
            const int64_t ra = first_a + stride_a * u;
            const int32_t g = rows_a[ra];
            key = g * 3 + labels[u] + 1;
            uint32_t l;
            __builtin_memcpy(&l, raw_a + start_a[ra] + 20, 4);
            bases = l;
            if (raw_b) {
                const int64_t rb = first_b + stride_b * u;
                __builtin_memcpy(&l, raw_b + start_b[rb] + 20, 4);
                bases += l;
                differ = rows_b[rb] != g;
            }
        }
        const unsigned long long nd = __ballot(differ);
        if (lane == 0 && nd) atomicAdd(&h_differ, (uint32_t)__popcll(nd));
#pragma unroll 1
        for (int r = 0; r < GR_AGG; ++r) {
            const unsigned long long left = __ballot(valid);
            if (!left) break;
            const int first = __ffsll((long long)left) - 1;
            const int k = __shfl(key, first);
            const bool mine = valid && key == k;
            const unsigned long long same = __ballot(mine);
            const unsigned long long sum = gr_wave_sum(mine ? bases : 0ull);
            if (lane == first) {
                if (lds) {
                    atomicAdd(h_units + k, (uint32_t)__popcll(same));
                    atomicAdd(h_bases + k, sum);
                } else {
                    atomicAdd(out + 2 * (int64_t)k, (unsigned long long)__popcll(same));
                    if (sum) atomicAdd(out + 2 * (int64_t)k + 1, sum);
                }
            }
            valid = valid && !mine;
        }
        if (valid) {
            if (lds) {
                atomicAdd(h_units + key, 1u);
                atomicAdd(h_bases + key, bases);
            } else {
                atomicAdd(out + 2 * (int64_t)key, 1ull);
                if (bases) atomicAdd(out + 2 * (int64_t)key + 1, bases);
            }
        }
    }
    __syncthreads();
    if (lds)
        for (int k = threadIdx.x; k < nkeys; k += GR_THREADS) {
            const unsigned long long c = h_units[k], b = h_bases[k];
            if (c) atomicAdd(out + 2 * k, c);
            if (b) atomicAdd(out + 2 * k + 1, b);
        }
    if (threadIdx.x == 0 && h_differ) atomicAdd(out + 2 * (int64_t)nkeys, (unsigned long long)h_differ);
    if (blockIdx.x == 0 && threadIdx.x == 0) info[1] = n;
}

}  // namespace
