// rd_bam_encode.hpp - the records of a FASTQ / FASTA chunk as unaligned BAM records: the RAW view of a chunk that did not come from a
// BAM file (rd_be_* kernels; C ABI rd_bam_encode, the CLI's --ubam_output). Part of the single translation unit rd_kernels.hip (included
// from there, behind rd_report.hpp, whose id rule and tile writer it uses, and rd_bam_tagtext.hpp, whose lane-group copy the tag pass
// uses); DESIGN.md §3.28. The rule is ribodetector_amd/bam.py
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
//
// Listed names (C ABI rd_bam_encode_ex, the CLI's --ubam_tags; the rule is bam.tags_from_comment): a record ends in the
// listed tags that the comment of its header line holds. Without names the kernels' TAGS = false instances run - the launches above.
//   rd_be_tag_count_kernel<L>   in FRONT of the length pass, L = 4 or 16 lanes per record: the comment's fields in order, every value
//                               validated; per record the bytes of its tags, which the length pass adds to the record's length, and
//                               the mask of the names copied; per copied name where its field stands and where its tag goes
//   rd_be_len_kernel<true>, the scan (without a limit: BeTagVerdict holds the total against raw_cap and REPORTS it, fault 1),
//   rd_be_write_kernel<true>    as above; the tile writer writes the tag bytes as zeros
//   rd_be_tag_write_kernel<L>   behind the tile writer: the tags straight into raw at each record's tag offset, by lane groups
// RD_UBAM_TAG_FLOATS (the CLI's --ubam_tag_floats): the FLOATS = true instances of the two tag kernels turn f and B:f
// values into float32 (rd_float_parse.hpp) instead of leaving them out; the FLOATS = false ones are the code without the flag.
// The bound. A field of t text bytes 'XY:T:value' makes: A 4 of 6; i 3 + 1, 2 or 4 of 5 + digits (a value that needs 4 bytes has 5
// digits); Z / H 3 + (t - 5) + 1 = t - 1; B 8 + es count of t = 6 + the elements' text, each at least ',d' = 2 bytes for es <= 4: at most
// 8 + 2 (t - 6) = 2 t - 4, reached by an I / i array of one-digit values (and by an array without elements: 8 of 6); f 7 of t >= 6, B:f
// 8 + 4 n of t >= 6 + 2 n: inside the same bound. So a field makes at
// most max(t, 2 t - 4) < 2 t bytes, a record's tags at most twice its comment, and - the comment and the byte in front of it are
// part of the text that the bounds above count as header -           raw <= bound above + sum of max(0, tags - comment - 1).
// Real comments shrink (an ML:B:C,255 element is 4 text bytes for 1), so a caller sizes `raw` by the bound above and repeats the
// call once, at the size info[1] reports, in the rare case of fault 1.
#pragma once
#include "rd_common.hpp"
#include "rd_scan.hpp"
#include "rd_report.hpp"
#include "rd_bam_tags.hpp"
#include "rd_bam_tagtext.hpp"
#include "rd_float_parse.hpp"

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

// TAGS (rd_bam_encode_ex with listed names): tagb[i], the bytes of record i's tags (rd_be_tag_count_kernel ran first), are part of its length
template <bool TAGS>
__global__ __launch_bounds__(256) void rd_be_len_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, BeTabs t, int64_t n, uint32_t flags,
                                                       int64_t *__restrict__ rec_len, uint32_t *__restrict__ meta, int64_t *__restrict__ qoff,
                                                       int64_t *__restrict__ bsum, unsigned long long *__restrict__ first_bad, int32_t *__restrict__ fault,
                                                       unsigned long long *__restrict__ starred, const int64_t *__restrict__ tagb) {
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
        int64_t len = bad ? BE_MIN_REC : 36 + idl + 1 + (ls + 1) / 2 + ls;
        if constexpr (TAGS) len += bad ? 0 : tagb[i];
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

// TAGS: a record ends in tagb[i] bytes of tags, which this pass writes as zeros (whole pieces of them as one store) and
// rd_be_tag_write_kernel, behind it on the stream, fills in
template <bool TAGS>
__global__ __launch_bounds__(256) void rd_be_write_kernel(const uint8_t *__restrict__ text, BeTabs t, int64_t n, uint32_t flags,
                                                         const uint32_t *__restrict__ meta, const int64_t *__restrict__ qoff,
                                                         int64_t *__restrict__ raw_start, uint8_t *__restrict__ raw, int64_t *__restrict__ info,
                                                         const int64_t *__restrict__ tagb) {
    __shared__ int64_t offs[BE_RECS + 1];
    __shared__ BeRec recs[BE_RECS];
    __shared__ int64_t tg[TAGS ? BE_RECS : 1];
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
            if constexpr (TAGS) tg[k] = tagb[i];
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
                int64_t size = 36 + r.name + 1 + ((int64_t)r.l_seq + 1) / 2 + r.l_seq;
                if constexpr (TAGS) size += tg[k];
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
                if constexpr (TAGS)
                    if (j >= r.l_seq) return 0u;
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
                if constexpr (TAGS)
                    if (j >= r.l_seq) return j + 16 <= r.l_seq + tg[k];      // (v is zero) 16 bytes of the record's tags
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

// ---- the tags of the header line's comment (rd_bam_encode_ex with listed names; the rule is bam.tags_from_comment) ------------------------
constexpr int BT_THREADS = 256;
constexpr int BT_CNT = 2 + RD_BAM_TAGS_MAX;      // counters: malformed records, float values skipped, records per copied name

__device__ __forceinline__ int bt_first_ws(u32x4 v) {      // index of the first byte of v that ends an id (rp_ws), 16: none
    int j = 16;
#pragma unroll
    for (int w = 3; w >= 0; --w)
#pragma unroll
        for (int c = 3; c >= 0; --c)
            if (rp_ws((v[w] >> (8 * c)) & 0xffu)) j = 4 * w + c;
    return j;
}

__device__ __forceinline__ int bt_first_eq(u32x4 v, uint32_t c) {      // index of the first byte of v equal to c, 16: none
    const uint32_t m = c * 0x01010101u;
    return tg_first_zero(u32x4{v[0] ^ m, v[1] ^ m, v[2] ^ m, v[3] ^ m});
}

// The first byte of text[p, e) that is c - WS: that ends an id -, e when there is none: lane j of a group looks at bytes [16 j, 16 j + 16)
// of a step of 16 L bytes, a ballot finds the first. Called by EVERY lane of the wave (the ballots and the shuffle are executed by all
// 64); on, p and e are the same in the lanes of a group, and a group with on == false idles and gets e. No byte at or behind e is read.
template <int L, bool WS>
__device__ __forceinline__ int64_t bt_find(const uint8_t *__restrict__ text, int64_t p, int64_t e, bool on, int sub, int gbase, unsigned long long gmask,
                                           uint32_t c) {
    int64_t at = e;
    bool searching = on && p < e;
    for (;;) {
        if (!__ballot(searching)) break;
        int z = 16;
        if (searching) {
            const int64_t q0 = p + 16 * sub;
            if (q0 + 16 <= e) {
                u32x4 w;
                __builtin_memcpy(&w, text + q0, 16);
                z = WS ? bt_first_ws(w) : bt_first_eq(w, c);
            } else {
                for (int64_t q = q0; q < e; ++q)
                    if (WS ? rp_ws(text[q]) : text[q] == c) { z = (int)(q - q0); break; }
            }
        }
        const unsigned long long found = __ballot(z < 16) & gmask;
        const int first = found ? __ffsll((long long)found) - 1 : gbase;
        const int zf = __shfl(z, first);
        if (searching) {
            if (found) {
                at = p + 16 * (int64_t)(first - gbase) + zf;
                searching = false;
            } else {
                p += 16 * L;
                if (p >= e) searching = false;
            }
        }
    }
    return at;
}

// [+-]?[0-9]{1,10} at text[p, e): its value and where it ends; false: no digit, or an eleventh one
__device__ __forceinline__ bool bt_int(const uint8_t *__restrict__ text, int64_t p, int64_t e, int64_t &v, int64_t &end) {
    bool neg = false;
    if (p < e && (text[p] == '+' || text[p] == '-')) { neg = text[p] == '-'; ++p; }
    int64_t m = 0;
    int d = 0;
    for (; p < e && d < 11; ++p, ++d) {
        const uint32_t c = text[p];
        if (c < '0' || c > '9') break;
        m = m * 10 + (int64_t)(c - '0');
    }
    v = neg ? -m : m;
    end = p;
    return d >= 1 && d <= 10;
}

__device__ __forceinline__ bool bt_in_range(int64_t v, uint8_t t) {      // may v stand in an element of type t (one of cCsSiI)?
    const int64_t lo = t == 'c' ? -128 : t == 's' ? -32768 : t == 'i' ? -2147483648LL : 0;
    const int64_t hi = t == 'c' ? 127 : t == 'C' ? 255 : t == 's' ? 32767 : t == 'S' ? 65535 : t == 'i' ? 2147483647LL : 4294967295LL;
    return v >= lo && v <= hi;
}

__device__ __forceinline__ uint8_t bt_small_type(int64_t v) {          // the smallest type that holds v in [-2^31, 2^32)
    if (v >= 0) return v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
    return v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
}

// the element behind the comma at text[q] of a B value that ends at fe: its value when it is [+-]?digits up to the next comma or fe
// and lies in the range of subtype st
__device__ __forceinline__ bool bt_element(const uint8_t *__restrict__ text, int64_t q, int64_t fe, uint8_t st, int64_t &v) {
    int64_t end;
    if (!bt_int(text, q + 1, fe, v, end)) return false;
    if (end < fe && text[end] != ',') return false;
    return bt_in_range(v, st);
}

// (RD_UBAM_TAG_FLOATS) the element behind the comma at text[q] of a B:f value that ends at fe: FP_OK when it is of fp_scan's syntax up to
// the next comma or fe, FP_LONG when it is and has more than 17 digits, else FP_BAD
__device__ __forceinline__ int bt_float_element(const uint8_t *__restrict__ text, int64_t q, int64_t fe, FpNum &num) {
    int64_t end;
    const int fs = fp_scan(text, q + 1, fe, num, end);
    return fs == FP_BAD || (end < fe && text[end] != ',') ? FP_BAD : fs;
}

__device__ __forceinline__ int bt_float_element(const uint8_t *__restrict__ text, int64_t q, int64_t fe) {
    FpNum num;
    return bt_float_element(text, q, fe, num);
}

// 16 bytes of a B value at text[i] (fewer at its end fe): a bit per byte that is a comma
__device__ __forceinline__ uint32_t bt_commas(const uint8_t *__restrict__ text, int64_t i, int64_t fe) {
    uint32_t m = 0;
    if (i + 16 <= fe) {
        u32x4 w;
        __builtin_memcpy(&w, text + i, 16);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (((w[c >> 2] >> (8 * (c & 3))) & 0xffu) == ',') m |= 1u << c;
    } else {
        for (int64_t q = i; q < fe; ++q)
            if (text[q] == ',') m |= 1u << (int)(q - i);
    }
    return m;
}

// The count pass: L lanes per record. The header line's end (the first '\n' inside the record; none: the table fault), the id's end, the
// comment behind that one byte up to the line's end (without one '\r' in front of the '\n'); then the fields of the comment in order,
// a step of the loop per field and group: its end (the next '\t'), the five bytes 'XY:T:' and the listed name they hold, the value -
// the lanes stride over the bytes of a Z / H value and over 16-byte pieces of a B value, in which each lane parses the elements whose
// comma stands in its piece. The sums meet in shuffles behind the strided loops. Per record: the bytes of its tags (tagb) and the mask
// of the names that are copied (0 for a malformed record); per copied name: where the field stands in the text (foff, fend) and where
// its tag goes in the record's tag bytes (ooff) - comment order. Every offset is compared with the record's end before it is read.
// FLOATS (RD_UBAM_TAG_FLOATS): an f value is scanned by the group's first lane (fp_scan: the syntax, at most 17 digits) and makes 7
// bytes; the elements of a B:f value are scanned like the integer ones, by the lane in whose piece their comma stands, 4 bytes each. A
// value or element of more than 17 digits leaves the tag out and counts once ("skipped" meets in the same shuffles as "malformed").
// Without FLOATS an f or B:f value is counted and not looked at.
template <int L, bool FLOATS>
__global__ __launch_bounds__(BT_THREADS) void rd_be_tag_count_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, BeTabs t, int64_t n, int n_names,
                                                                    TtNames names, int64_t *__restrict__ tagb, uint32_t *__restrict__ mask,
                                                                    int64_t *__restrict__ foff, int64_t *__restrict__ fend, int64_t *__restrict__ ooff,
                                                                    unsigned long long *__restrict__ cnt, int32_t *__restrict__ fault) {
    __shared__ unsigned int scnt[BT_CNT];
    if (threadIdx.x < BT_CNT) scnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1), gbase = lane & ~(L - 1);
    const unsigned long long gmask = ((1ull << L) - 1ull) << gbase;
    const int64_t k = ((int64_t)blockIdx.x * BT_THREADS + threadIdx.x) / L;
    const bool live = k < n;
    int64_t a = 0, b = 0;
    bool ok = false;                                      // a record with a header line (the length pass judges every other one)
    if (live) {
        const int64_t e = t.at(k);
        a = t.rec_start[e], b = t.rec_start[e + 1];
        ok = a >= 0 && a < b && b <= text_bytes;
        if (ok) ok = text[a] == '@' || text[a] == '>';
    }
    const int64_t nl = bt_find<L, false>(text, a + 1, b, ok, sub, gbase, gmask, '\n');
    if (ok && nl >= b) {                                  // a header line that runs past its record
        if (sub == 0) atomicOr(fault, 1);
        ok = false;
    }
    const int64_t ws = bt_find<L, true>(text, a + 1, nl, ok, sub, gbase, gmask, 0);
    int64_t ce = nl;                                      // the line's end
    if (ok && nl - 1 > a && text[nl - 1] == '\r') ce = nl - 1;
    int64_t p = ws + 1;                                   // the field that the next step takes starts here
    bool more = ok && ws < ce;
    bool mal = false;
    uint32_t seen = 0, copied = 0;
    int floats = 0;
    int64_t tags = 0;
    for (;;) {
        if (!__ballot(more)) break;                       // (wave-uniform: the ballots and shuffles below are executed by every lane)
        const int64_t fe = bt_find<L, false>(text, p, ce, more, sub, gbase, gmask, '\t');
        int j = -1;
        uint8_t ty = 0;
        if (more && fe - p >= 5) {
            const uint32_t c0 = text[p], c1 = text[p + 1], c3 = text[p + 3];
            const bool alpha0 = (c0 >= 'A' && c0 <= 'Z') || (c0 >= 'a' && c0 <= 'z');
            const bool alnum1 = (c1 >= 'A' && c1 <= 'Z') || (c1 >= 'a' && c1 <= 'z') || (c1 >= '0' && c1 <= '9');
            const bool type3 = c3 == 'A' || c3 == 'i' || c3 == 'Z' || c3 == 'H' || c3 == 'B' || c3 == 'f';
            if (alpha0 && alnum1 && type3 && text[p + 2] == ':' && text[p + 4] == ':') {
                for (int q = 0; q < n_names; ++q)
                    if (names.b[2 * q] == c0 && names.b[2 * q + 1] == c1) j = q;
                if (j >= 0 && ((seen >> j) & 1u)) j = -1;             // (only the first field of a name counts)
                ty = (uint8_t)c3;
            }
        }
        int64_t tb = 0;                                   // this lane's share of the tag's bytes
        int lbad = 0;
        int lskip = 0;                                    // (FLOATS) a value of more than 17 digits
        bool is_float = false;
        if (j >= 0) {
            const int64_t v0 = p + 5, vl = fe - v0;
            if (ty == 'A') {
                if (vl != 1 || text[v0] < 0x21u || text[v0] > 0x7eu) lbad = 1;
                if (sub == 0) tb = 4;
            } else if (ty == 'i') {
                if (sub == 0) {
                    int64_t v, end;
                    if (!bt_int(text, v0, fe, v, end) || end != fe || v < -2147483648LL || v > 4294967295LL) lbad = 1;
                    else tb = 3 + tg_elem_size(bt_small_type(v));
                }
            } else if (ty == 'Z' || ty == 'H') {
                const bool hex = ty == 'H';
                if (hex && (vl & 1)) lbad = 1;
                if (sub == 0) tb = 4 + vl;
                for (int64_t i = 16 * (int64_t)sub; i < vl; i += 16 * L) {
                    if (i + 16 <= vl) {
                        u32x4 w;
                        __builtin_memcpy(&w, text + v0 + i, 16);
#pragma unroll
                        for (int c = 0; c < 16; ++c)
                            if (!tt_text_byte((w[c >> 2] >> (8 * (c & 3))) & 0xffu, hex)) lbad = 1;
                    } else {
                        for (int64_t q = i; q < vl; ++q)
                            if (!tt_text_byte(text[v0 + q], hex)) lbad = 1;
                    }
                }
            } else if (ty == 'f') {
                if constexpr (FLOATS) {
                    if (sub == 0) {
                        FpNum num;
                        const int fs = fp_value(text, v0, fe, num);
                        if (fs == FP_BAD) lbad = 1;
                        else if (fs == FP_LONG) lskip = 1;
                        else tb = 7;
                    }
                } else is_float = true;
            } else {                                      // B: a subtype, then ',int' per element
                const uint8_t st = vl >= 1 ? text[v0] : 0;
                if (!FLOATS && st == 'f') is_float = true;
                else if (!(tt_is_int(st) || (FLOATS && st == 'f')) || (vl > 1 && text[v0 + 1] != ',')) lbad = 1;
                else {
                    const int es = tg_elem_size(st);
                    if (sub == 0) tb = 8;
                    for (int64_t i = v0 + 1 + 16 * (int64_t)sub; i < fe; i += 16 * L) {
                        uint32_t m = bt_commas(text, i, fe);
                        while (m) {
                            const int c = __ffs((int)m) - 1;
                            m &= m - 1;
                            if constexpr (FLOATS) {
                                if (st == 'f') {
                                    const int fs = bt_float_element(text, i + c, fe);
                                    if (fs == FP_BAD) lbad = 1;
                                    else if (fs == FP_LONG) lskip = 1;
                                    else tb += 4;
                                    continue;
                                }
                            }
                            int64_t v;
                            if (bt_element(text, i + c, fe, st, v)) tb += es;
                            else lbad = 1;
                        }
                    }
                }
            }
        }
        if constexpr (FLOATS) lbad |= lskip << 1;
#pragma unroll
        for (int o = L / 2; o >= 1; o >>= 1) {
            tb += __shfl_xor(tb, o);
            lbad |= __shfl_xor(lbad, o);
        }
        if constexpr (FLOATS) {
            is_float = (lbad & 2) != 0;                   // the tag is left out and counted once
            lbad &= 1;
        }
        if (j >= 0) {
            seen |= 1u << j;
            if (lbad) mal = true;
            else if (is_float) ++floats;
            else {
                if (sub == 0) {
                    const int64_t at = (int64_t)j * n + k;
                    foff[at] = p;
                    fend[at] = fe;
                    ooff[at] = tags;
                }
                copied |= 1u << j;
                tags += tb;
            }
        }
        if (more) {
            if (fe < ce) p = fe + 1;
            else more = false;
        }
    }
    if (mal) { tags = 0; copied = 0; floats = 0; }
    if (live && sub == 0) {
        tagb[k] = tags;
        mask[k] = copied;
        if (mal) atomicAdd(&scnt[0], 1u);
        if (floats) atomicAdd(&scnt[1], (unsigned int)floats);
    }
    for (int j = 0; j < n_names; ++j) {                   // (uniform) one LDS add per wave and name
        const unsigned long long m = __ballot(sub == 0 && ((copied >> j) & 1u));
        if (lane == 0 && m) atomicAdd(&scnt[2 + j], (unsigned int)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < BT_CNT && scnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// the verdict of a call with listed names: BeVerdict's words, with the bytes the records NEED in info[1] when they are more than raw_cap
// (fault 1), and behind them info[8] = records with malformed tags, [9] = float values skipped, [10 + j] = records in which name j was
// copied. tot: the int64[4] of rd_scan_base_kernel, which ran without a limit
struct BeTagVerdict {
    int64_t n;
    const int32_t *fault;
    const unsigned long long *first_bad, *starred, *cnt;
    const int64_t *tot;
    int64_t raw_cap;
    int n_names;
    int64_t *info;
    __device__ __forceinline__ void operator()() const {
        const int64_t bytes = tot[1];
        const int f = *fault != 0 ? 2 : (tot[3] != 0 || bytes > raw_cap) ? 1 : 0;
        info[0] = f ? 0 : n;
        info[1] = f == 2 ? 0 : bytes;
        info[2] = (int64_t)first_bad[0];
        info[3] = f;
        info[6] = (int64_t)*starred;
        info[7] = (int64_t)first_bad[1];
        for (int j = 0; j < 2 + n_names; ++j) info[8 + j] = f == 2 ? 0 : (int64_t)cnt[j];
    }
};

// The tag pass, behind the tile writer on the stream: L lanes per record write its tags straight into raw, behind the qualities - the
// bytes the tile writer left zero. The names in list order, each at its own offset (ooff). The three bytes 'XY' type and a scalar by
// the group's first lane; a Z / H value as tt_copy copies (aligned 16-byte pieces of the OUTPUT range, the ends bytewise); the elements
// of a B array: a step takes 16 L bytes of the text, a lane counts the commas of its 16, a prefix sum of the counts over the group and a
// running base say which element stands behind a lane's first comma, and the lane parses and stores its elements. That loop is stepped
// by the whole wave (a ballot ends it), so the shuffles are executed by all 64 lanes. Nothing on a fault.
// FLOATS: an f value is converted by the group's first lane (fp_round) and stored as 4 bytes, an element of a B:f array likewise by the
// lane that holds it - a tag offset has no alignment, so the bytes go one by one as the integers' do.
template <int L, bool FLOATS>
__global__ __launch_bounds__(BT_THREADS) void rd_be_tag_write_kernel(const uint8_t *__restrict__ text, int64_t n, int n_names, TtNames names,
                                                                    const int64_t *__restrict__ tagb, const uint32_t *__restrict__ mask,
                                                                    const int64_t *__restrict__ foff, const int64_t *__restrict__ fend,
                                                                    const int64_t *__restrict__ ooff, const int64_t *__restrict__ raw_start,
                                                                    uint8_t *__restrict__ raw, const int64_t *__restrict__ info) {
    if (info[3]) return;                                  // (every lane of the grid)
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1), gbase = lane & ~(L - 1);
    const int64_t k = ((int64_t)blockIdx.x * BT_THREADS + threadIdx.x) / L;
    const bool live = k < n;
    const uint32_t m = live ? mask[k] : 0u;
    const int64_t base = live ? raw_start[k + 1] - tagb[k] : 0;      // where the record's tags begin
    for (int j = 0; j < n_names; ++j) {                   // (uniform)
        const bool on = (m >> j) & 1u;
        int64_t o = 0, fe = 0, i0 = 0, run = 0;
        uint8_t st = 'C';
        bool array = false;
        if (on) {
            const int64_t at = (int64_t)j * n + k;
            const int64_t p = foff[at], v0 = p + 5;
            fe = fend[at];
            o = base + ooff[at];
            const uint8_t ty = text[p + 3];
            if (sub == 0) {
                raw[o] = names.b[2 * j];
                raw[o + 1] = names.b[2 * j + 1];
                raw[o + 2] = ty;
                if (ty == 'A') raw[o + 3] = text[v0];
                else if (ty == 'i') {
                    int64_t v, end;
                    bt_int(text, v0, fe, v, end);
                    const uint8_t small = bt_small_type(v);
                    raw[o + 2] = small;
                    for (int c = 0; c < tg_elem_size(small); ++c) raw[o + 3 + c] = (uint8_t)((uint64_t)v >> (8 * c));
                } else if (FLOATS && ty == 'f') {
                    if constexpr (FLOATS) {
                        FpNum num;
                        fp_value(text, v0, fe, num);      // (FP_OK: the count pass has scanned it)
                        const uint32_t v = fp_bits(num);
                        for (int c = 0; c < 4; ++c) raw[o + 3 + c] = (uint8_t)(v >> (8 * c));
                    }
                } else if (ty == 'B') {
                    raw[o + 3] = text[v0];
                } else {
                    raw[o + 3 + (fe - v0)] = 0;           // Z / H: the NUL
                }
            }
            if (ty == 'Z' || ty == 'H') tt_copy<L>(raw, o + 3, text + v0, fe - v0, sub);
            else if (ty == 'B') {
                array = true;
                st = text[v0];
                i0 = v0 + 1;
            }
        }
        const int es = tg_elem_size(st);
        for (;; i0 += 16 * L) {
            if (!__ballot(array && i0 < fe)) break;       // (wave-uniform)
            const int64_t i = i0 + 16 * (int64_t)sub;
            uint32_t cm = array && i < fe ? bt_commas(text, i, fe) : 0u;
            const int mine = __popc(cm);
            int inc = mine;
#pragma unroll
            for (int d = 1; d < L; d <<= 1) {
                const int up = __shfl_up(inc, d, L);
                if (sub >= d) inc += up;
            }
            const int total = __shfl(inc, gbase + L - 1);
            int64_t idx = run + (inc - mine);
            while (cm) {
                const int c = __ffs((int)cm) - 1;
                cm &= cm - 1;
                int64_t v;
                bool is_f = false;
                if constexpr (FLOATS) {
                    if (st == 'f') {
                        FpNum num;
                        bt_float_element(text, i + c, fe, num);
                        v = (int64_t)fp_bits(num);
                        is_f = true;
                    }
                }
                if (!is_f) bt_element(text, i + c, fe, st, v);       // (valid: the count pass has parsed it)
                uint8_t *__restrict__ q = raw + o + 8 + idx * es;
                for (int w = 0; w < es; ++w) q[w] = (uint8_t)((uint64_t)v >> (8 * w));
                ++idx;
            }
            run += total;
        }
        if (array && sub == 0) {
            for (int c = 0; c < 4; ++c) raw[o + 4 + c] = (uint8_t)((uint64_t)run >> (8 * c));
        }
    }
}


// the tables of a call in its workspace (carved by bam_encode_ws of rd_kernels.hip)
struct BamEncodeWs {
    int nb;
    uint32_t *meta;
    int64_t *qoff, *bsum;
    unsigned long long *first_bad, *starred;     // (first_bad[2], starred and fault lie behind one another: one memset each way)
    int32_t *fault;
    // listed names (rd_bam_encode_ex): the tables of the tag passes, behind the ones every call has
    int64_t *tagb, *foff, *fend, *ooff, *tot;
    uint32_t *mask;
    unsigned long long *cnt;
    size_t total;
};

// the launches of a call with listed names, for one lane mapping of the tag passes (FLOATS: RD_UBAM_TAG_FLOATS)
template <int L, bool FLOATS>
void bam_encode_tags_launch(const uint8_t *text, int64_t text_bytes, const BeTabs &t, int64_t n_rec, uint32_t flags, const TtNames &names, int32_t n_names,
                            uint8_t *raw, int64_t cap, int64_t *raw_start, int64_t *info, const BamEncodeWs &p, unsigned grid, hipStream_t st) {
    const int64_t per = BT_THREADS / L;
    const dim3 tgrid((unsigned)((n_rec + per - 1) / per));
    hipLaunchKernelGGL((rd_be_tag_count_kernel<L, FLOATS>), tgrid, dim3(BT_THREADS), 0, st, text, text_bytes, t, n_rec, (int)n_names, names, p.tagb, p.mask, p.foff, p.fend,
                       p.ooff, p.cnt, p.fault);
    hipLaunchKernelGGL(rd_be_len_kernel<true>, dim3(p.nb), dim3(256), 0, st, text, text_bytes, t, n_rec, flags, raw_start, p.meta, p.qoff, p.bsum, p.first_bad, p.fault,
                       p.starred, (const int64_t *)p.tagb);
    scan_base(p.bsum, p.nb, p.tot, INT64_MAX, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, ScanTab<1>, BeTagVerdict>), dim3(p.nb), dim3(256), 0, st, ScanTab<1>{{raw_start}}, n_rec,
                       ScanOut<1>{{raw_start}, {p.bsum}}, BeTagVerdict{n_rec, p.fault, p.first_bad, p.starred, p.cnt, p.tot, cap, (int)n_names, info});
    hipLaunchKernelGGL(rd_be_write_kernel<true>, dim3(grid), dim3(256), 0, st, text, t, n_rec, flags, (const uint32_t *)p.meta, (const int64_t *)p.qoff, raw_start, raw,
                       info, (const int64_t *)p.tagb);
    hipLaunchKernelGGL((rd_be_tag_write_kernel<L, FLOATS>), tgrid, dim3(BT_THREADS), 0, st, text, n_rec, (int)n_names, names, (const int64_t *)p.tagb, (const uint32_t *)p.mask,
                       (const int64_t *)p.foff, (const int64_t *)p.fend, (const int64_t *)p.ooff, (const int64_t *)raw_start, raw, (const int64_t *)info);
}
}  // namespace
