// rd_group_pack.hpp - the records of a chunk partitioned by KEY: one run of text, or of BGZF members, per key (rd_gp_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, behind rd_deflate.hpp); DESIGN.md §3.27.
//
// rd_select_pack / rd_gz_compress_selected select ONE label value per call. A run that writes a set of files per read group has
// (G + 1) x classes files per mate - up to 3,075 - and would make that many calls per chunk, each re-reading the labels. Here every
// record carries a key in -1 .. K - 1 (-1: no file takes it; rd_group_keys makes the keys from the read-group rows and the unit
// labels) and ONE call writes the records of every key, in input order, as a contiguous run per key, in key order. The number of
// launches does not depend on K, and the text is read once and written once in front of the deflate.
//
//   rd_gp_count_kernel     a WAVE per part of the records (at most 1,024 parts of at least 512 records): keys and record table
//                          checked, records per key counted -> cnt[key][part]. The counters are 32-bit words in LDS for K <=
//                          GP_LDS_KEYS (16 KiB per wave; 64-bit words for the CLI's largest K, 3,075, would be 24 KiB per wave and
//                          buy nothing: a chunk has < 2^31 records), else words of the part's own row in HBM.
//   rd_scan_*              cnt, key-major -> pos: where (key, part) starts in the permuted order (rd_scan.hpp, one launch per stage;
//                          no workgroup waits for another one of the same launch)
//   rd_gp_scatter_kernel   the same parts again: perm[pos ...] = the record indices, stable (a strip of 64 records is resolved key
//                          by key from ballots: a lane's rank among the lanes of its key, the key's cursor advanced once per strip)
//   rd_scan_*              the lengths in permuted order -> L (more bytes than the text: the table does not describe it)
//   rd_gp_keytab_kernel    one workgroup: per key its records, bytes and its run's base - each run starts on a multiple of 16 bytes
//                          (text) or of the member size (gzip: member m of the padded stream is still plain + 65,280 m, and only
//                          its LENGTH comes from the per-member table written here)
//   rd_gp_mlen_kernel      gzip: the per-member lengths from the keys' table, a thread per member
//   rd_pack_kernel<GpPermPlaces>   the pack kernel of rd_deflate.hpp over the places of the permuted order: 256 consecutive places per
//                          workgroup, 16-byte pieces by bisection over the staged destinations, nothing written into the gaps between runs
//   rd_gz_deflate_kernel<GzTableLen>, rd_gz_moff_kernel, rd_gz_compact_kernel   the members, as in rd_gz_compress_selected: the
//                          compact stream is in key order already; rd_gp_keytab_gz_kernel turns member offsets into the keys' table
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"
#include "rd_deflate.hpp"

namespace {

constexpr int GP_LDS_KEYS = 4096;       // keys whose counters a wave keeps in LDS
constexpr int GP_MAX_PARTS = 1024;      // parts of a chunk's records: a wave each
constexpr int GP_PART_MIN = 512;        // records per part, at least
constexpr uint32_t GP_FAULT_KEY = 1, GP_FAULT_TABLE = 2, GP_FAULT_CAP = 4;     // info[3] of the two entry points
static_assert(RD_GROUP_KEYS_MAX >= 3 * (RD_SPLIT_GROUPS_MAX + 1) && GP_LDS_KEYS >= 3 * (RD_SPLIT_GROUPS_MAX + 1), "the CLI's keys are counted in LDS");

// ------------------------------------------------------------------------------------------------
// keys from rows and labels
// ------------------------------------------------------------------------------------------------
struct GpSlots { int s[3]; };
__global__ __launch_bounds__(256) void rd_group_keys_kernel(const int32_t *__restrict__ rows, int64_t first, int64_t stride, int mate,
                                                           const int8_t *__restrict__ labels, int64_t n, GpSlots slots, int G,
                                                           int32_t *__restrict__ keys, int64_t *__restrict__ info) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u == 0) info[1] = n;
    if (u >= n) return;
    const int lab = labels[u], row = rows[first + stride * u];
    const unsigned bad = ((lab < -1 || lab > 1) ? 1u : 0u) | ((row < 0 || row > G + 2) ? 2u : 0u);
    int32_t key = -1;
    if (bad) {
        atomicOr(reinterpret_cast<unsigned long long *>(info), (unsigned long long)bad);
    } else {
        const int slot = lab < 0 ? slots.s[0] : lab == 0 ? slots.s[1] : slots.s[2];
        if (slot >= 0) key = slot * (G + 1) + (row < G ? row : G);
    }
    if (mate < 0) {
        keys[u] = key;
    } else {
        keys[2 * u + mate] = key;
        keys[2 * u + 1 - mate] = -1;
    }
}

// ------------------------------------------------------------------------------------------------
// the stable counting partition: counts per (key, part), then - behind their scan - the scatter
// ------------------------------------------------------------------------------------------------
struct GpParts {
    int nb;          // parts
    int64_t per;     // records per part (the last one: the rest)
};

template <bool LDS>
__global__ __launch_bounds__(64) void rd_gp_count_kernel(const int32_t *__restrict__ keys, const int64_t *__restrict__ rec_start, int64_t n,
                                                        int64_t text_bytes, int K, GpParts parts, uint32_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ gcur, uint32_t *__restrict__ flag) {
    __shared__ uint32_t lc[LDS ? GP_LDS_KEYS : 1];
    const int lane = threadIdx.x, b = blockIdx.x;
    uint32_t *c = LDS ? lc : gcur + (size_t)b * K;      // (the rows in HBM were zeroed by the entry point)
    if (LDS) {
        for (int k = lane; k < K; k += 64) lc[k] = 0;
        __syncthreads();
    }
    const int64_t i0 = b * parts.per, i1 = i0 + parts.per < n ? i0 + parts.per : n;
    uint32_t bad = 0;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const int32_t key = keys[i];
        if (key < -1 || key >= K) { bad |= GP_FAULT_KEY; continue; }
        if (key < 0) continue;
        const int64_t s = rec_start[i], e = rec_start[i + 1];
        if (s < 0 || e < s || e > text_bytes) { bad |= GP_FAULT_TABLE; continue; }
        atomicAdd(&c[key], 1u);
    }
    if (bad) atomicOr(flag, bad);
    if (LDS) __syncthreads(); else __threadfence();
    for (int k = lane; k < K; k += 64) cnt[(size_t)k * parts.nb + b] = c[k];
}

struct GpCntLen {                       // rd_scan.hpp's len functor over the counts
    const uint32_t *cnt;
    __device__ __forceinline__ int64_t operator()(int, int64_t i) const { return (int64_t)cnt[i]; }
};

template <bool LDS>
__global__ __launch_bounds__(64) void rd_gp_scatter_kernel(const int32_t *__restrict__ keys, int64_t n, int K, GpParts parts,
                                                          const int64_t *__restrict__ pos, uint32_t *__restrict__ gcur,
                                                          const uint32_t *__restrict__ flag, int32_t *__restrict__ perm) {
    __shared__ uint32_t lc[LDS ? GP_LDS_KEYS : 1];
    if (*flag) return;                   // (a key outside its range, a record outside the text: nothing is permuted)
    const int lane = threadIdx.x, b = blockIdx.x;
    uint32_t *c = LDS ? lc : gcur + (size_t)b * K;
    for (int k = lane; k < K; k += 64) c[k] = (uint32_t)pos[(size_t)k * parts.nb + b];
    if (LDS) __syncthreads(); else __threadfence();
    const int64_t i0 = b * parts.per, i1 = i0 + parts.per < n ? i0 + parts.per : n;
    for (int64_t s0 = i0; s0 < i1; s0 += 64) {
        const int64_t i = s0 + lane;
        const int32_t key = i < i1 ? keys[i] : -1;
        uint64_t todo = __ballot(key >= 0);
        while (todo) {                   // key by key (uniform): the strip's first lane that is still open names the key
            const int l0 = __builtin_ctzll(todo);
            const int32_t k0 = __builtin_amdgcn_readlane(key, l0);
            const uint64_t m = __ballot(key == k0);
            uint32_t old = 0;
            if (lane == l0) old = atomicAdd(&c[k0], (uint32_t)__popcll(m));
            const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)old, l0);
            if (key == k0) perm[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
            todo &= ~m;
        }
    }
}

struct GpPermLen {                      // the length of the record at place j of the permuted order (behind the last one, or flagged: 0)
    const int32_t *perm;
    const int64_t *rec_start;
    const int64_t *placed;              // pos[K * parts]: the records that have a key
    const uint32_t *flag;
    __device__ __forceinline__ int64_t operator()(int, int64_t j) const {
        if (*flag || j >= *placed) return 0;
        const int64_t p = perm[j];
        return rec_start[p + 1] - rec_start[p];
    }
};

// ------------------------------------------------------------------------------------------------
// per key: records, bytes, the base of its run (one workgroup)
// ------------------------------------------------------------------------------------------------
// shift[k] = (base of key k's run) - L[first place of key k]: place j of key k goes to L[j] + shift[k]. GZ: the run's base is a
// multiple of GZ_MEMBER in the padded stream and key_tab[k] = {that base, bytes, records, members} until rd_gp_keytab_gz_kernel
// (rd_gp_mlen_kernel makes the members' lengths from it). Text: the base is a multiple of 16 in `out`, key_tab[k] = {base, bytes, records, 0}.
template <bool GZ>
__global__ __launch_bounds__(256) void rd_gp_keytab_kernel(const int64_t *__restrict__ pos, const int64_t *__restrict__ L, int K, int nb,
                                                          const uint32_t *__restrict__ flag, const int64_t *__restrict__ linfo, int64_t out_cap,
                                                          int64_t *__restrict__ shift, int64_t *__restrict__ key_tab, int64_t *__restrict__ info) {
    __shared__ int64_t sh[4];
    __shared__ int64_t run_s;
    __shared__ unsigned long long need_s;
    const int tid = threadIdx.x;
    const uint32_t fault = *flag | (linfo[3] ? GP_FAULT_TABLE : 0u);
    if (fault) {
        for (int k = tid; k < 4 * K; k += 256) key_tab[k] = 0;
        if (tid == 0) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = fault; }
        return;
    }
    if (tid == 0) { run_s = 0; need_s = 0; }
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + tid;
        int64_t r0 = 0, r1 = 0, l0 = 0, B = 0;
        if (k < K) {
            r0 = pos[(size_t)k * nb];
            r1 = pos[(size_t)(k + 1) * nb];
            l0 = L[r0];
            B = L[r1] - l0;
        }
        const int64_t slot = GZ ? (B + GZ_MEMBER - 1) / GZ_MEMBER * GZ_MEMBER : (B + 15) & ~(int64_t)15;
        int64_t total;
        const int64_t base = gz_block_scan(slot, sh, total) + run_s;
        if (k < K) {
            shift[k] = base - l0;
            key_tab[4 * k] = base;
            key_tab[4 * k + 1] = B;
            key_tab[4 * k + 2] = r1 - r0;
            key_tab[4 * k + 3] = GZ ? slot / GZ_MEMBER : 0;
            if (B > 0) atomicMax(&need_s, (unsigned long long)(base + B));
        }
        __syncthreads();
        if (tid == 0) run_s += total;
        __syncthreads();
    }
    if (tid == 0) {
        if (GZ) {
            info[0] = 0;
            info[1] = linfo[1];
            info[2] = run_s / GZ_MEMBER;
            info[3] = 0;
        } else {
            info[0] = pos[(size_t)K * nb];
            info[1] = (int64_t)need_s;          // the end of the last run that holds a byte
            info[2] = 0;
            info[3] = (int64_t)need_s > out_cap ? GP_FAULT_CAP : 0;
        }
    }
}

// mlen[m] = the bytes of member m of the padded stream, from the keys' table: a workgroup per key, a thread per member (a chunk of
// one or two keys has thousands of members per key: not a loop of one lane)
__global__ __launch_bounds__(256) void rd_gp_mlen_kernel(const int64_t *__restrict__ key_tab, int K, uint32_t *__restrict__ mlen,
                                                        const int64_t *__restrict__ info) {
    if (info[3]) return;                 // (the table was zeroed: no key has a member)
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int64_t m0 = key_tab[4 * k] / GZ_MEMBER, B = key_tab[4 * k + 1], nm = key_tab[4 * k + 3];
        for (int64_t t = threadIdx.x; t < nm; t += 256)
            mlen[m0 + t] = (uint32_t)(B - t * GZ_MEMBER < GZ_MEMBER ? B - t * GZ_MEMBER : GZ_MEMBER);
    }
}

// behind the deflate and rd_gz_moff_kernel: key_tab[k] = {offset of the key's first member in out, compressed bytes, records, members}
__global__ __launch_bounds__(256) void rd_gp_keytab_gz_kernel(const int64_t *__restrict__ moff, int K, int64_t out_cap, int64_t *__restrict__ key_tab,
                                                             int64_t *__restrict__ info) {
    const int64_t nmem = info[2], bytes = info[0];
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        const int64_t m0 = key_tab[4 * k] / GZ_MEMBER, m1 = m0 + key_tab[4 * k + 3];
        const int64_t o0 = m0 < nmem ? moff[m0] : bytes, o1 = m1 < nmem ? moff[m1] : bytes;
        key_tab[4 * k] = o0;
        key_tab[4 * k + 1] = o1 - o0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && bytes > out_cap) info[3] = info[3] | GP_FAULT_CAP;
}

// ------------------------------------------------------------------------------------------------
// the pack: place j of the permuted order -> dst[L[j] + shift[key] ...)
// ------------------------------------------------------------------------------------------------
// rd_pack_kernel's places (rd_deflate.hpp): the records that have a key, read through the permutation. Their destinations ascend, with
// a gap where the key changes (up to the next multiple of 16, or of the member size).
struct GpPermPlaces {
    static constexpr bool GAPS = true;
    const int64_t *rec_start;
    const int32_t *keys, *perm;
    const int64_t *L, *shift;
    const int64_t *placed;              // pos[K * parts]: the records that have a key
    __device__ __forceinline__ int64_t places() const { return *placed; }
    __device__ __forceinline__ int64_t src(int64_t j) const { return rec_start[perm[j]]; }
    __device__ __forceinline__ int64_t begin(int64_t j) const { return L[j] + shift[keys[perm[j]]]; }
    __device__ __forceinline__ int64_t len(int64_t j) const { return rec_start[perm[j] + 1] - rec_start[perm[j]]; }
};

}  // namespace
