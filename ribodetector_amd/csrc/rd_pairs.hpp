// rd_pairs.hpp - paired-end reads from ONE interleaved FASTQ chunk (`--interleaved`), on the device (rd_pair_* kernels)
// Part of the single translation unit rd_kernels.hip (included from there, after rd_report.hpp, whose id rule it shares).
//
// A chunk of 2n records whose records 2k and 2k + 1 are mate 1 and mate 2 of pair k. A pair is eight contiguous lines, so the pairs are
// themselves the records of a table with every second entry: rd_select_pack, rd_gz_compress_selected and rd_report_format work from
// pair_start unchanged, and rd_classify takes the two mates' sequence tables as it takes those of two files.
//
//   rd_pair_split_kernel     one thread per PS_PAIRS pairs (pair k of a workgroup's 1,024 goes to lane k % 256: the table loads and
//                            stores of a wave are contiguous). pair_start and the mates' tables are copies of table entries; the mate
//                            check reads the two header lines: id length with 16-byte loads while they lie inside the record, then the
//                            ids compared in 16-byte pieces, the `/1` - `/2` rule decided on the last two bytes.
//   rd_pair_expand_kernel    pair labels -> record labels for the file of ONE mate: the other mate's records get RD_LABEL_SKIP, a value
//                            no file selects (the selection kernels and the host writer test labels for equality only)
#pragma once
#include "rd_common.hpp"
#include "rd_report.hpp"

namespace {

constexpr int PS_PAIRS = 4;                     // pairs per thread of the split kernel

// length of the id of the record [a, b): the bytes after its first one up to the first white space (rd_report.hpp rp_ws); -1 when the
// header line runs past the record. The caller has checked 0 <= a < b <= text_bytes.
__device__ __forceinline__ int64_t ps_id_len(const uint8_t *__restrict__ text, int64_t a, int64_t b) {
    int64_t p = a + 1;
    for (; p + 16 <= b; p += 16) {              // 16 bytes per step while they lie inside the record
        u32x4 v;
        __builtin_memcpy(&v, text + p, 16);
        int j = 16;
#pragma unroll
        for (int w = 3; w >= 0; --w)
#pragma unroll
            for (int c = 3; c >= 0; --c)
                if (rp_ws((v[w] >> (8 * c)) & 0xffu)) j = 4 * w + c;
        if (j < 16) return p + j - a - 1;
    }
    for (; p < b; ++p)
        if (rp_ws(text[p])) return p - a - 1;
    return -1;
}

// are the ids (L bytes each, at text + x and text + y) those of mates? Equal, or equal up to `/1` in the first and `/2` in the second.
__device__ __forceinline__ bool ps_mates(const uint8_t *__restrict__ text, int64_t x, int64_t y, int64_t L) {
    if (L == 0) return true;
    int64_t i = 0;
    bool same = true;
    for (; i + 16 <= L - 1 && same; i += 16) {  // every byte but the last, in 16-byte pieces (they lie inside the two header lines)
        u32x4 va, vb;
        __builtin_memcpy(&va, text + x + i, 16);
        __builtin_memcpy(&vb, text + y + i, 16);
        same = ((va[0] ^ vb[0]) | (va[1] ^ vb[1]) | (va[2] ^ vb[2]) | (va[3] ^ vb[3])) == 0;
    }
    for (; i < L - 1 && same; ++i) same = text[x + i] == text[y + i];
    if (!same) return false;
    const uint32_t ca = text[x + L - 1], cb = text[y + L - 1];
    return ca == cb || (L >= 2 && ca == '1' && cb == '2' && text[x + L - 2] == '/');      // (byte L - 2 is equal in both)
}

__global__ __launch_bounds__(256) void rd_pair_split_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ rec_start,
                                                           const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len, int64_t n,
                                                           int check_ids, int64_t *__restrict__ pair_start, int64_t *__restrict__ seq_off1,
                                                           int32_t *__restrict__ seq_len1, int64_t *__restrict__ seq_off2, int32_t *__restrict__ seq_len2,
                                                           int64_t *__restrict__ info) {
    const int64_t base = (int64_t)blockIdx.x * (256 * PS_PAIRS) + threadIdx.x;
    bool bad_any = false;
    int64_t first_bad = -1;                     // the first pair of this thread whose ids are not mates (its pairs ascend)
#pragma unroll 1
    for (int j = 0; j < PS_PAIRS; ++j) {
        const int64_t k = base + (int64_t)j * 256;
        if (k > n) break;
        const int64_t a0 = rec_start[2 * k];
        pair_start[k] = a0;
        if (k == n) break;                      // entry n: the end of the last pair
        const int64_t a1 = rec_start[2 * k + 1], a2 = rec_start[2 * k + 2];
        const int64_t o1 = seq_off[2 * k], o2 = seq_off[2 * k + 1];
        const int32_t l1 = seq_len[2 * k], l2 = seq_len[2 * k + 1];
        seq_off1[k] = o1;
        seq_len1[k] = l1;
        seq_off2[k] = o2;
        seq_len2[k] = l2;
        bool bad = !(a0 >= 0 && a0 < a1 && a1 < a2 && a2 <= text_bytes) || l1 < 0 || l2 < 0 || o1 < 0 || o2 < 0 || o1 > text_bytes - l1 || o2 > text_bytes - l2;
        if (!bad && check_ids) {
            bad = text[a0] != '@' || text[a1] != '@';
            if (!bad) {
                const int64_t La = ps_id_len(text, a0, a1), Lb = ps_id_len(text, a1, a2);
                bad = La < 0 || Lb < 0;
                if (!bad && first_bad < 0 && !(La == Lb && ps_mates(text, a0 + 1, a1 + 1, La))) first_bad = k;
            }
        }
        bad_any |= bad;
    }
    // info = {pairs, first pair whose ids are not mates or -1, 0, fault}: the host call has set {0, -1, 0, 0}; -1 is the largest unsigned value
    if (first_bad >= 0) atomicMin((unsigned long long *)(info + 1), (unsigned long long)first_bad);
    if (bad_any) atomicOr((unsigned long long *)(info + 3), 1ull);
    if (base == 0) info[0] = n;
}

// rec_labels[2k + mate] = pair_labels[k], rec_labels[2k + 1 - mate] = RD_LABEL_SKIP: one thread per 8 pairs = 16 bytes of record labels
__global__ __launch_bounds__(256) void rd_pair_expand_kernel(const int8_t *__restrict__ pair_labels, int64_t n, int mate, int8_t *__restrict__ rec_labels) {
    const int64_t k0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (k0 >= n) return;
    if (k0 + 8 <= n) {
        uint64_t v;
        __builtin_memcpy(&v, pair_labels + k0, 8);
        u32x4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t b0 = (uint32_t)(v >> (16 * w)) & 0xffu, b1 = (uint32_t)(v >> (16 * w + 8)) & 0xffu;
            const uint32_t skip = (uint32_t)RD_LABEL_SKIP & 0xffu;
            o[w] = mate ? (skip | (b0 << 8) | (skip << 16) | (b1 << 24)) : (b0 | (skip << 8) | (b1 << 16) | (skip << 24));
        }
        __builtin_memcpy(rec_labels + 2 * k0, &o, 16);
        return;
    }
    for (int64_t k = k0; k < n; ++k) {
        rec_labels[2 * k + mate] = pair_labels[k];
        rec_labels[2 * k + 1 - mate] = (int8_t)RD_LABEL_SKIP;
    }
}

}  // namespace
