// rd_bam_encode.hpp - the records of a FASTQ / FASTA chunk as unaligned BAM records: the RAW view of a chunk that did not come from a
// BAM file (rd_be_* kernels; C ABI rd_bam_encode, the CLI's --ubam_output). Part of the single translation unit rd_kernels.hip (included
// from there, behind rd_report.hpp, whose id rule and tile writer it uses); DESIGN.md §3.28. The rule is ribodetector_amd/bam.py
// (from_fastq): record i becomes bam.encode_record({name, seq, qual, flag}) -
//     block_size:int32 = S - 4, refID -1, pos -1, l_read_name = L + 1, mapq 0, bin 4680, n_cigar_op 0, flag, l_seq, next_refID -1,
//     next_pos -1, tlen 0 (36 bytes), the name and its NUL (L + 1), the bases 4 bits each ((l_seq + 1) / 2), the qualities (l_seq):
//     S = 36 + L + 1 + (l_seq + 1) / 2 + l_seq.
// name = the id of the per-read report (rp_id_len: the header behind '@' / '>' up to the first white space), without a trailing /1 on a
// record whose flag word says mate 1 (0x40) or /2 on one that says mate 2 (0x80); an empty id becomes '*'. A base is the code of its
// letter in "=ACMGRSVTWYHKDBN", either case, U = T, every other byte N (15); an odd l_seq pads with 0. A quality is
// min(max(b, 33), 126) - 33; FASTA: 0xFF.
//
// The raw bytes have a bound linear in the text, so a caller sizes `raw` without a hint and without a second call:
//   FASTQ  a record of the text is '@' header '\n' SEQ '\n' '+'... '\n' QUAL '\n' >= 2 l_seq + idL + 6 bytes (idL = the id, at most the
//          header); its BAM record is 37 + L + (l_seq + 1) / 2 + l_seq bytes with L <= max(idL, 1) and (l_seq + 1) / 2 <= l_seq for
//          l_seq >= 1 (0 for 0): raw - text <= 31 + (L - idL) <= 32 per record.                          raw <= text + 32 n
//   FASTA  a record of the text is '>' header '\n' SEQ '\n' >= l_seq + idL + 3 bytes: raw - text <= 34 + (L - idL) + (l_seq + 1) / 2
//          <= 35 + (l_seq + 1) / 2 per record, and the sum of (l_seq + 1) / 2 is at most (text + n) / 2.    raw <= text + (text + 1) / 2 + 40 n
// (A record whose quality line is not as long as its sequence is laid out with l_seq 0 - it is reported, never delivered - so that the
// bounds hold for every input.)
//
//   rd_be_len_kernel    one thread per 8 records - the sums pass of rd_scan.hpp: every table entry checked against the text, the id's
//                       end (rp_id_len), /1 and /2, '*', the quality line's start; the record's bytes into raw_start, its name length
//                       and quality offset into the workspace; the first record with a name of more than 254 bytes and the first
//                       one with a length mismatch by 64-bit atomic minimum; the names starred, one atomic per workgroup
//   rd_scan_* (rd_scan.hpp)   raw_start -> exclusive offsets in place, entry n = the total; BeVerdict fills info
//   rd_be_write_kernel  a workgroup owns a TILE of 16 KiB of the OUTPUT, whichever records its bytes belong to (a 100 kb read is
//                       spread over seven workgroups): the records that meet the tile are found by bisection in raw_start, their
//                       offsets - clamped to the tile - and sources staged in LDS, and rp_write_tile writes the tile in aligned 16-byte
//                       stores. 16 bytes of a name are one unaligned load; 16 packed-base bytes come from 32 bytes of the text through
//                       a 256-entry table in LDS (code | changed << 4); 16 qualities are shifted and clamped four per 32-bit operation.
//                       Pieces that cross a field or a record go byte by byte. The counters are summed per lane, then per wave, then
//                       in LDS: one 64-bit atomic per workgroup and counter.
// Nothing is written on a fault (info[3]): raw_start is zeroed instead, so that it describes an empty view.
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"
#include "rd_report.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "rd_bam_encode.hpp is written for gfx950 (wave64, 16-byte global stores)"
#endif

namespace {

constexpr int BE_TILE = 16384;                   // bytes of `raw` per workgroup and trip of the write pass
constexpr int BE_MIN_REC = 38;                   // 36 + a name of one byte + its NUL: the least bytes of a record
constexpr int BE_RECS = BE_TILE / BE_MIN_REC + 2;      // the most records that meet a tile (433)
constexpr int BE_MAX_NAME = 254;
constexpr int BE_GRID = 1024;                    // workgroups of the write pass at most (they stride over the tiles)
constexpr uint32_t BE_STAR = 1u << 30;           // meta: the name is '*'
constexpr uint32_t BE_NOSEQ = 1u << 29;          // meta: laid out with l_seq 0 (a length mismatch)

// code (low nibble) and `changed` (bit 4: the BAM letter differs from the byte) of an input byte
__device__ __forceinline__ uint32_t be_code(uint32_t c) {
    const uint32_t u = c >= 'a' && c <= 'z' ? c - 32u : c;
    uint32_t k = 15u;
    switch (u) {
        case '=': k = 0; break;
        case 'A': k = 1; break;
        case 'C': k = 2; break;
        case 'M': k = 3; break;
        case 'G': k = 4; break;
        case 'R': k = 5; break;
        case 'S': k = 6; break;
        case 'V': k = 7; break;
        case 'T': k = 8; break;
        case 'U': k = 8; break;
        case 'W': k = 9; break;
        case 'Y': k = 10; break;
        case 'H': k = 11; break;
        case 'K': k = 12; break;
        case 'D': k = 13; break;
        case 'B': k = 14; break;
        default: break;
    }
    const uint32_t letter = (uint32_t)"=ACMGRSVTWYHKDBN"[k];
    return k | (letter != c ? 16u : 0u);
}

// four quality bytes at once: min(max(b, 33), 126) - 33 per byte; clamped += the bytes outside 33..126
__device__ __forceinline__ uint32_t be_qual4(uint32_t w, uint32_t &clamped) {
    const uint32_t low = w & 0x7f7f7f7fu;
    const uint32_t ge33 = ((low + 0x5f5f5f5fu) | w) & 0x80808080u;      // bit 7 of a byte: b >= 33
    const uint32_t gt126 = ((low + 0x01010101u) | w) & 0x80808080u;     // ... b >= 127
    const uint32_t in = ge33 & ~gt126;
    clamped += 4u - (uint32_t)__popc(in);
    const uint32_t in_m = (in >> 7) * 0xffu, hi_m = (gt126 >> 7) * 0xffu;
    const uint32_t xs = (w & in_m) | (0x21212121u & ~in_m);             // every byte in 33..126: the subtraction borrows nowhere
    return (xs - 0x21212121u) | (0x5d5d5d5du & hi_m);
}

struct BeTabs {                                  // the chunk's tables: record i of the call is entry first + i * stride
    const int64_t *rec_start, *seq_off;
    const int32_t *seq_len;
    int64_t first;
    int32_t stride;
    __device__ __forceinline__ int64_t at(int64_t i) const { return first + i * (int64_t)stride; }
};

__device__ __forceinline__ uint32_t be_flag(uint32_t flags, int64_t i) {      // the record's flag word: even / odd records of the call
    return i & 1 ? (flags >> RD_UBAM_ODD_SHIFT) & 0xfffu : (flags >> RD_UBAM_EVEN_SHIFT) & 0xfffu;
}

__global__ __launch_bounds__(256) void rd_be_len_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, BeTabs t, int64_t n, uint32_t flags,
                                                       int64_t *__restrict__ rec_len, uint32_t *__restrict__ meta, int64_t *__restrict__ qoff,
                                                       int64_t *__restrict__ bsum, unsigned long long *__restrict__ first_bad, int32_t *__restrict__ fault,
                                                       unsigned long long *__restrict__ starred) {
    __shared__ int64_t sh[4];
    __shared__ unsigned int s_star;
    if (threadIdx.x == 0) s_star = 0;
    __syncthreads();
    const bool fasta = flags & RD_UBAM_FASTA;
    const int64_t i0 = (int64_t)blockIdx.x * GZ_SCAN_ITEMS + threadIdx.x * 8;
    int64_t s = 0;
    bool bad_any = false;
    unsigned int stars = 0;
    for (int k = 0; k < 8; ++k) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const int64_t e = t.at(i);
        const int64_t a = t.rec_start[e], b = t.rec_start[e + 1], so = t.seq_off[e];
        int64_t ls = t.seq_len[e];
        bool bad = !(a >= 0 && a < b && b <= text_bytes) || !(ls >= 0 && so > a && so <= b && ls <= b - so);
        int64_t idl = -1;
        if (!bad) {
            const bool no_header = fasta && text[a] != '>';      // (FASTA: sequence lines in front of the first header make a record with an empty one)
            idl = no_header ? 0 : rp_id_len(text, text_bytes, a, b);
            bad = idl < 0 || (!no_header && a + 1 + idl >= so);  // (the id ends in front of the bases)
        }
        uint32_t m = 0;
        int64_t q0 = 0;
        if (!bad) {
            const uint32_t fl = be_flag(flags, i);
            if ((fl & 1u) && idl >= 2 && text[a + idl - 1] == '/' &&
                (((fl & 0x40u) && text[a + idl] == '1') || ((fl & 0x80u) && text[a + idl] == '2'))) idl -= 2;
            if (idl == 0) { m |= BE_STAR; idl = 1; ++stars; }
            if (idl > BE_MAX_NAME) { atomicMin(&first_bad[0], (unsigned long long)i); idl = BE_MAX_NAME; }
            if (!fasta) {
                // the quality line: behind the '\n' of the '+' line, up to the '\n' that ends the record. Every line of a chunk ends in
                // '\n': rd_fq_begin_kernel appends the one a file's last line may lack before the batch is framed, and the host reader's
                // chunks are '\n'.join(lines) + '\n'. A record that is not laid out so is reported as a length mismatch: it cannot be
                // a BAM record either way, and no byte outside [a, b) is read to find out
                int64_t p = so + ls;
                bool ok = p + 2 < b && text[p] == '\n' && text[b - 1] == '\n';
                if (ok) {
                    for (p = p + 1; p < b - 1 && text[p] != '\n'; ++p) {}
                    q0 = p + 1;
                    ok = q0 <= b - 1 && b - 1 - q0 == ls;
                }
                if (!ok) { atomicMin(&first_bad[1], (unsigned long long)i); m |= BE_NOSEQ; ls = 0; q0 = so; }
            }
            m |= (uint32_t)idl;
        }
        bad_any |= bad;
        const int64_t len = bad ? BE_MIN_REC : 36 + idl + 1 + (ls + 1) / 2 + ls;
        rec_len[i] = len;
        meta[i] = bad ? (BE_STAR | BE_NOSEQ | 1u) : m;
        qoff[i] = q0;
        s += len;
    }
    if (bad_any) atomicOr(fault, 1);
    if (stars) atomicAdd(&s_star, stars);
    scan_store_sum(s, sh, bsum);                 // (its barriers stand behind the LDS add)
    if (threadIdx.x == 0 && s_star) atomicAdd(starred, (unsigned long long)s_star);
}

// info = {records, raw bytes, first record whose name is too long or -1, fault, bases changed, qualities clamped, names starred, first
// record with a length mismatch or -1}: the base kernel has set info[1] and info[3] (1: more bytes than raw_cap); a table entry that
// does not describe the text makes it 2. The write pass adds to [4] and [5].
struct BeVerdict {
    int64_t n;
    const int32_t *fault;
    const unsigned long long *first_bad, *starred;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        if (*fault) { info[1] = 0; info[3] = 2; }
        info[0] = info[3] ? 0 : n;
        info[2] = (int64_t)first_bad[0];         // (~0 = -1: none)
        info[6] = (int64_t)*starred;
        info[7] = (int64_t)first_bad[1];
    }
};

struct BeRec {                                   // a staged record of a tile
    int64_t id_src, seq_src, q_src;              // where the name, the bases and the qualities stand in the text
    int32_t name, l_seq;                         // name bytes without the NUL; bases
    uint32_t flag;                               // the flag word | BE_STAR
};

// byte j < 36 of a record's fixed fields
__device__ __forceinline__ uint32_t be_fixed_byte(int64_t size, const BeRec &r, int j) {
    const int w = j >> 2;
    const uint32_t v = w == 0 ? (uint32_t)(size - 4) : w == 3 ? (uint32_t)(r.name + 1) | (4680u << 16) : w == 4 ? (r.flag & 0xffffu) << 16 :
                       w == 5 ? (uint32_t)r.l_seq : w == 8 ? 0u : 0xffffffffu;
    return (v >> (8 * (j & 3))) & 0xffu;
}

__global__ __launch_bounds__(256) void rd_be_write_kernel(const uint8_t *__restrict__ text, BeTabs t, int64_t n, uint32_t flags,
                                                         const uint32_t *__restrict__ meta, const int64_t *__restrict__ qoff,
                                                         int64_t *__restrict__ raw_start, uint8_t *__restrict__ raw, int64_t *__restrict__ info) {
    __shared__ int64_t offs[BE_RECS + 1];
    __shared__ BeRec recs[BE_RECS];
    __shared__ uint8_t code[256];
    __shared__ int64_t r_bounds[2];
    __shared__ unsigned int s_cnt[2];
    if (info[3]) {                               // a fault: nothing is written, and the table describes an empty view
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (int64_t)gridDim.x * 256) raw_start[i] = 0;
        return;
    }
    const int64_t total = info[1];
    const bool fasta = flags & RD_UBAM_FASTA;
    code[threadIdx.x] = (uint8_t)be_code(threadIdx.x);
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    uint32_t changed = 0, clamped = 0;
    for (int64_t lo = (int64_t)blockIdx.x * BE_TILE; lo < total; lo += (int64_t)gridDim.x * BE_TILE) {
        const int64_t hi = lo + BE_TILE < total ? lo + BE_TILE : total;
        __syncthreads();
        if (threadIdx.x < 2) {                   // the records of the tile's first and last byte: raw_start[r] <= q < raw_start[r + 1]
            const int64_t q = threadIdx.x ? hi - 1 : lo;
            int64_t a = 0, b = n - 1;
            while (a < b) {
                const int64_t mid = (a + b + 1) >> 1;
                if (raw_start[mid] <= q) a = mid; else b = mid - 1;
            }
            r_bounds[threadIdx.x] = a;
        }
        __syncthreads();
        const int64_t r0 = r_bounds[0];
        int nr = (int)(r_bounds[1] - r0 + 1);
        if (nr > BE_RECS) nr = BE_RECS;          // (cannot happen: a record has at least BE_MIN_REC bytes)
        const int64_t start0 = raw_start[r0];    // the first record may begin in front of the tile
        for (int k = threadIdx.x; k <= nr; k += 256) {
            const int64_t o = raw_start[r0 + k];
            offs[k] = k == 0 ? lo : o < hi && k < nr ? o : hi;
        }
        for (int k = threadIdx.x; k < nr; k += 256) {
            const int64_t i = r0 + k, e = t.at(i);
            const uint32_t m = meta[i];
            BeRec r;
            r.id_src = t.rec_start[e] + 1;
            r.seq_src = t.seq_off[e];
            r.q_src = qoff[i];
            r.name = (int32_t)(m & 0xffffu);
            r.l_seq = m & BE_NOSEQ ? 0 : t.seq_len[e];
            r.flag = be_flag(flags, i) | (m & BE_STAR);
            recs[k] = r;
        }
        __syncthreads();
        const int64_t skip0 = lo - start0;       // bytes of record r0 in front of the tile
        // j = the byte's offset in its record: 36 fixed, name + NUL, packed bases, qualities
        rp_write_tile(
            offs, nr, raw,
            [&](int k, int64_t j) -> const uint8_t * {
                if (k == 0) j += skip0;
                const BeRec &r = recs[k];
                return j >= 36 && j + 16 <= 36 + r.name && !(r.flag & BE_STAR) ? text + r.id_src + (j - 36) : nullptr;
            },
            [&](int k, int64_t j) -> uint32_t {
                if (k == 0) j += skip0;
                const BeRec &r = recs[k];
                const int64_t size = 36 + r.name + 1 + ((int64_t)r.l_seq + 1) / 2 + r.l_seq;
                if (j < 36) return be_fixed_byte(size, r, (int)j);
                j -= 36;
                if (j < r.name) return r.flag & BE_STAR ? (uint32_t)'*' : text[r.id_src + j];
                if (j == r.name) return 0u;
                j -= r.name + 1;
                const int64_t half = ((int64_t)r.l_seq + 1) / 2;
                if (j < half) {
                    const uint32_t c0 = code[text[r.seq_src + 2 * j]];
                    const uint32_t c1 = 2 * j + 1 < r.l_seq ? code[text[r.seq_src + 2 * j + 1]] : 0u;
                    changed += (c0 >> 4) + (c1 >> 4);
                    return ((c0 & 15u) << 4) | (c1 & 15u);
                }
                j -= half;
                if (fasta) return 0xffu;
                return be_qual4(text[r.q_src + j] | 0x21212100u, clamped);
            },
            [&](int k, int64_t j, u32x4 &v) -> bool {
                if (k == 0) j += skip0;
                const BeRec &r = recs[k];
                const int64_t half = ((int64_t)r.l_seq + 1) / 2;
                j -= 36 + r.name + 1;
                if (j < 0) return false;
                if (j < half) {                  // 16 packed bytes of 32 bases, all of them inside the sequence
                    if (2 * j + 32 > r.l_seq) return false;
                    u32x4 s[2];
                    __builtin_memcpy(s, text + r.seq_src + 2 * j, 32);
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        uint32_t o = 0;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const uint32_t two = (s[w >> 1][2 * (w & 1) + (c >> 1)] >> (16 * (c & 1))) & 0xffffu;
                            const uint32_t c0 = code[two & 0xffu], c1 = code[two >> 8];
                            changed += (c0 >> 4) + (c1 >> 4);
                            o |= (((c0 & 15u) << 4) | (c1 & 15u)) << (8 * c);
                        }
                        v[w] = o;
                    }
                    return true;
                }
                j -= half;
                if (j + 16 > r.l_seq) return false;
                if (fasta) {
                    v = u32x4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                    return true;
                }
                u32x4 q;
                __builtin_memcpy(&q, text + r.q_src + j, 16);
#pragma unroll
                for (int w = 0; w < 4; ++w) v[w] = be_qual4(q[w], clamped);
                return true;
            });
    }
    // the counters: lane -> wave (shuffles) -> LDS -> one 64-bit atomic per workgroup and counter
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        changed += __shfl_xor(changed, o);
        clamped += __shfl_xor(clamped, o);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (changed) atomicAdd(&s_cnt[0], changed);
        if (clamped) atomicAdd(&s_cnt[1], clamped);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd((unsigned long long *)&info[4 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace
