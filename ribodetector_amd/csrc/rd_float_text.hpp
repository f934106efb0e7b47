// rd_float_text.hpp - a float32 as the text printf("%g") gives it: the correctly rounded 6 significant decimal digits of the EXACT value,
// ties to even, in %g's fixed or exponent form (C ABI rd_float_text; the f and B:f values of rd_bam_tag_splice_ex, rd_bam_tagtext.hpp).
// The rule is ribodetector_amd/bam.py (float_g); DESIGN.md §3.26. Part of the single translation unit rd_kernels.hip; the formatter itself
// (ft_format) is plain C++ over integers and compiles for the host as well (-DRD_FT_HOST, tests/test_float_text_host.py).
//
// v = m 2^e (m < 2^24, -149 <= e <= 104). With E = floor(log2 v), x = floor(E log10 2) is floor(log10 v) or one less, and k = 5 - x
// (-33 <= k <= 50) scales v to v 10^k = m 5^k 2^(e + k) in [10^5, 10^7). That number is the fraction A / D of two integers of at most
// 5 limbs of 32 bits: A = m 5^k (k >= 0) or m, D = 1 or 5^-k, and the power of two on whichever side keeps both whole - the powers of
// five come from a table that holds them exactly (5^50 < 2^117). N = floor(A / D) starts from a float estimate that lies at most 5
// below N and never above (its roundings move v 10^k < 10^7 by less than 2), and is then made exact: r = A - N D in integers, and
// while r >= D one more. The rounding is decided by r alone: 2 r against D, or, when N has 7 digits, its last digit and r != 0. No double,
// no division of limbs, every limb index a constant (registers, no scratch).
#pragma once
#include <stdint.h>

#ifdef RD_FT_HOST
#include <math.h>
#define FT_FN static inline
#define FT_TABLE static const
#define FT_UNROLL
#else
#include "rd_common.hpp"
#define FT_FN __device__ __forceinline__
#define FT_TABLE __device__ const
#define FT_UNROLL _Pragma("unroll")
#endif

namespace {

constexpr int FT_LIMBS = 5;
constexpr int FT_POW5_MAX = 50;
constexpr int FT_SLOT = 16;                     // bytes of a text slot; no text is longer than 12 ("-1.17549e-38")

// 5^i, i = 0..50, little-endian limbs
FT_TABLE uint32_t ft_pow5[FT_POW5_MAX + 1][4] = {
    {0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000005u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000019u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x0000007du, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000271u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000c35u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x00003d09u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x0001312du, 0x00000000u, 0x00000000u, 0x00000000u}, {0x0005f5e1u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x001dcd65u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x009502f9u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x02e90eddu, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x0e8d4a51u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x48c27395u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x6bcc41e9u, 0x00000001u, 0x00000000u, 0x00000000u},
    {0x1afd498du, 0x00000007u, 0x00000000u, 0x00000000u}, {0x86f26fc1u, 0x00000023u, 0x00000000u, 0x00000000u}, {0xa2bc2ec5u, 0x000000b1u, 0x00000000u, 0x00000000u},
    {0x2dace9d9u, 0x00000378u, 0x00000000u, 0x00000000u}, {0xe460913du, 0x00001158u, 0x00000000u, 0x00000000u}, {0x75e2d631u, 0x000056bcu, 0x00000000u, 0x00000000u},
    {0x4d6e2ef5u, 0x0001b1aeu, 0x00000000u, 0x00000000u}, {0x8326eac9u, 0x00087867u, 0x00000000u, 0x00000000u}, {0x8fc295edu, 0x002a5a05u, 0x00000000u, 0x00000000u},
    {0xcecceda1u, 0x00d3c21bu, 0x00000000u, 0x00000000u}, {0x0a00a425u, 0x0422ca8bu, 0x00000000u, 0x00000000u}, {0x320334b9u, 0x14adf4b7u, 0x00000000u, 0x00000000u},
    {0xfa10079du, 0x6765c793u, 0x00000000u, 0x00000000u}, {0xe2502611u, 0x04fce5e3u, 0x00000002u, 0x00000000u}, {0x6b90be55u, 0x18f07d73u, 0x0000000au, 0x00000000u},
    {0x19d3b7a9u, 0x7cb27341u, 0x00000032u, 0x00000000u}, {0x8122964du, 0x6f7c4045u, 0x000000fcu, 0x00000000u}, {0x85acef81u, 0x2d6d415bu, 0x000004eeu, 0x00000000u},
    {0x9c60ad85u, 0xe32246c9u, 0x000018a6u, 0x00000000u}, {0x0de36399u, 0x6fab61f0u, 0x00007b42u, 0x00000000u}, {0x4570f1fdu, 0x2e58e9b0u, 0x0002684cu, 0x00000000u},
    {0x5b34b9f1u, 0xe7bc9071u, 0x000c097cu, 0x00000000u}, {0xc807a1b5u, 0x86aed236u, 0x003c2f70u, 0x00000000u}, {0xe8262889u, 0xa16a1b11u, 0x012ced32u, 0x00000000u},
    {0x88becaadu, 0x27128759u, 0x05e0a1fdu, 0x00000000u}, {0xabb9f561u, 0xc35ca4bfu, 0x1d6329f1u, 0x00000000u}, {0x5aa1cae5u, 0xd0cf37beu, 0x92efd1b8u, 0x00000000u},
    {0xc528f679u, 0x140c16b7u, 0xdeaf189cu, 0x00000002u}, {0xd9ccd05du, 0x643c7196u, 0x596b7b0cu, 0x0000000eu}, {0x410011d1u, 0xf52e37f2u, 0xbf19673du, 0x00000047u},
    {0x45005915u, 0xc9e717bbu, 0xbb7f0435u, 0x00000166u}, {0x5901bd69u, 0xf18376a8u, 0xa97b150cu, 0x00000701u}, {0xbd08b30du, 0xb7915149u, 0x4f676940u, 0x00002308u},
    {0xb12b7f41u, 0x95d69670u, 0x8d050e43u, 0x0000af29u}, {0x75d97c45u, 0xed30f033u, 0xc1194751u, 0x00036bcfu}, {0x4d3f6d59u, 0xa1f4b101u, 0xc57e6499u, 0x00111b0eu},
};

// 5^k rounded to float32, k = -33..50 (entry k + 33): the estimate of N only
FT_TABLE float ft_pow5f[84] = {
    0x1.4c4e98p-77f, 0x1.9f623ep-75f, 0x1.039d66p-72f, 0x1.4484c0p-70f, 0x1.95a5f0p-68f, 0x1.fb0f6cp-66f,
    0x1.3ce9a4p-63f, 0x1.8c240cp-61f, 0x1.ef2d10p-59f, 0x1.357c2ap-56f, 0x1.82db34p-54f, 0x1.e39202p-52f,
    0x1.2e3b40p-49f, 0x1.79ca10p-47f, 0x1.d83c94p-45f, 0x1.2725dep-42f, 0x1.70ef54p-40f, 0x1.cd2b2ap-38f,
    0x1.203afap-35f, 0x1.6849b8p-33f, 0x1.c25c26p-31f, 0x1.197998p-28f, 0x1.5fd7fep-26f, 0x1.b7cdfep-24f,
    0x1.12e0bep-21f, 0x1.5798eep-19f, 0x1.ad7f2ap-17f, 0x1.0c6f7ap-14f, 0x1.4f8b58p-12f, 0x1.a36e2ep-10f,
    0x1.0624dep-7f, 0x1.47ae14p-5f, 0x1.99999ap-3f, 0x1.000000p+0f, 0x1.400000p+2f, 0x1.900000p+4f,
    0x1.f40000p+6f, 0x1.388000p+9f, 0x1.86a000p+11f, 0x1.e84800p+13f, 0x1.312d00p+16f, 0x1.7d7840p+18f,
    0x1.dcd650p+20f, 0x1.2a05f2p+23f, 0x1.74876ep+25f, 0x1.d1a94ap+27f, 0x1.2309cep+30f, 0x1.6bcc42p+32f,
    0x1.c6bf52p+34f, 0x1.1c3794p+37f, 0x1.634578p+39f, 0x1.bc16d6p+41f, 0x1.158e46p+44f, 0x1.5af1d8p+46f,
    0x1.b1ae4ep+48f, 0x1.0f0cf0p+51f, 0x1.52d02cp+53f, 0x1.a78438p+55f, 0x1.08b2a2p+58f, 0x1.4adf4cp+60f,
    0x1.9d971ep+62f, 0x1.027e72p+65f, 0x1.431e10p+67f, 0x1.93e594p+69f, 0x1.f8def8p+71f, 0x1.3b8b5cp+74f,
    0x1.8a6e32p+76f, 0x1.ed09bep+78f, 0x1.342618p+81f, 0x1.812f9cp+83f, 0x1.e17b84p+85f, 0x1.2ced32p+88f,
    0x1.782880p+90f, 0x1.d632a0p+92f, 0x1.25dfa4p+95f, 0x1.6f578cp+97f, 0x1.cb2d70p+99f, 0x1.1efc66p+102f,
    0x1.66bb80p+104f, 0x1.c06a5ep+106f, 0x1.18427cp+109f, 0x1.5e531ap+111f, 0x1.b5e7e0p+113f, 0x1.11b0ecp+116f,
};

struct FtLimbs {
    uint32_t w[FT_LIMBS];
};

// x 2^s for a whole x < 2^32 and 0 <= s < 128
FT_FN FtLimbs ft_place(uint32_t x, int s) {
    const uint64_t v = (uint64_t)x << (s & 31);
    const int q = s >> 5;
    FtLimbs r;
    FT_UNROLL
    for (int i = 0; i < FT_LIMBS; ++i) r.w[i] = i == q ? (uint32_t)v : i == q + 1 ? (uint32_t)(v >> 32) : 0u;
    return r;
}

// a - b; `borrow` says a < b
FT_FN FtLimbs ft_sub(const FtLimbs &a, const FtLimbs &b, bool &borrow) {
    FtLimbs r;
    uint32_t c = 0;
    FT_UNROLL
    for (int i = 0; i < FT_LIMBS; ++i) {
        const uint64_t t = (uint64_t)a.w[i] - b.w[i] - c;
        r.w[i] = (uint32_t)t;
        c = (uint32_t)(t >> 63);
    }
    borrow = c != 0;
    return r;
}

// the text of the float32 with bit pattern `bits` as 16 bytes (t[0]: bytes 0..7, t[1]: bytes 8..15, the bytes behind the text zero);
// returns its length
FT_FN int ft_format(uint32_t bits, uint64_t t[2]) {
    const uint32_t neg = bits >> 31, ef = (bits >> 23) & 0xffu, mf = bits & 0x7fffffu;
    uint64_t lo, hi = 0;
    int len;
    if (ef == 0xffu || (ef | mf) == 0u) {                 // inf, nan, 0
        lo = ef ? (mf ? 0x6e616eull : 0x666e69ull) : 0x30ull;
        len = ef ? 3 : 1;
    } else {
        const uint32_t m = ef ? mf | 0x800000u : mf;
        const int e = (ef ? (int)ef : 1) - 150;
        const int x0 = ((31 - __builtin_clz(m) + e) * 1233) >> 12;      // floor(E log10 2), E = floor(log2 v) in [-149, 127]
        const int k = 5 - x0, s = e + k;
        // A = m 5^k (k >= 0: exact in 5 limbs) or m, times 2^s when s > 0 - then the product is below 2^24 (k >= 0: it is N 2^-s; k < 0: m)
        const uint32_t *pa = ft_pow5[k > 0 ? k : 0], *pd = ft_pow5[k < 0 ? -k : 0];
        FtLimbs A, D;
        uint64_t c = 0;
        FT_UNROLL
        for (int i = 0; i < 4; ++i) {
            c += (uint64_t)m * pa[i];
            A.w[i] = (uint32_t)c;
            c >>= 32;
        }
        A.w[4] = (uint32_t)c;
        if (s > 0) A = ft_place(A.w[0], s);
        // D = 1 or 5^-k (at most 77 bits), times 2^-s when s < 0 - then it is below 2^32 (k >= 0: 1; k < 0: -s <= 5 needs -k <= 3)
        if (s < 0) D = ft_place(pd[0], -s);
        else {
            FT_UNROLL
            for (int i = 0; i < 4; ++i) D.w[i] = pd[i];
            D.w[4] = 0;
        }
        // N: the estimate m 5^k 2^s in float (m exact, two roundings and the table's: off by less than 2), 3 lower, made exact by r
        const float est = ldexpf((float)m * 0x1p-24f * ft_pow5f[k + 33], s + 24);
        uint32_t N = (uint32_t)est;
        N = N > 3u ? N - 3u : 0u;
        FtLimbs P, r;
        c = 0;
        FT_UNROLL
        for (int i = 0; i < FT_LIMBS; ++i) {
            c += (uint64_t)N * D.w[i];
            P.w[i] = (uint32_t)c;
            c >>= 32;
        }
        bool less;
        r = ft_sub(A, P, less);
        FT_UNROLL
        for (int i = 0; i < 5; ++i) {
            const FtLimbs q = ft_sub(r, D, less);
            if (!less) {
                r = q;
                ++N;
            }
        }
        // the 6 digits: round N + r / D to a whole number, or, when N has 7 digits (x0 was one less than floor(log10 v)), to a ten
        int X = x0;
        bool up, tie;
        uint32_t rest = 0;
        FT_UNROLL
        for (int i = 0; i < FT_LIMBS; ++i) rest |= r.w[i];
        if (N >= 1000000u) {
            const uint32_t d = N % 10u;
            N /= 10u;
            ++X;
            up = d > 5u || (d == 5u && rest != 0u);
            tie = d == 5u && rest == 0u;
        } else {
            FtLimbs r2;
            FT_UNROLL
            for (int i = 0; i < FT_LIMBS; ++i) r2.w[i] = (r.w[i] << 1) | (i ? r.w[i - 1] >> 31 : 0u);
            const FtLimbs q = ft_sub(r2, D, less);
            uint32_t any = 0;
            FT_UNROLL
            for (int i = 0; i < FT_LIMBS; ++i) any |= q.w[i];
            up = !less && any != 0u;
            tie = !less && any == 0u;
        }
        if (up || (tie && (N & 1u))) ++N;
        if (N == 1000000u) {
            N = 100000u;
            ++X;
        }
        // the digits as 6 bytes, the first one lowest; P of them are left without the trailing zeros
        uint64_t dig = 0;
        int P6 = 6;
        bool zeros = true;
        FT_UNROLL
        for (int i = 0; i < 6; ++i) {
            const uint32_t d = N % 10u;
            N /= 10u;
            zeros = zeros && d == 0u;
            if (zeros) --P6;
            dig = (dig << 8) | (uint64_t)('0' + d);
        }
        const bool expo = X < -4 || X >= 6;
        if (!expo && X < 0) {                             // 0.000ddd: '0.', -X - 1 zeros, the P digits (at most 11 bytes)
            const int at = 1 - X;                         // 2..5
            lo = 0x3030302e30ull & ((1ull << (8 * at)) - 1ull);
            const uint64_t d = dig & ((1ull << (8 * P6)) - 1ull);
            lo |= d << (8 * at);
            hi = d >> (64 - 8 * at);
            len = at + P6;
        } else {                                          // I digits, then '.' and the rest when there is one; I = 1 in exponent form
            const int I = expo ? 1 : X + 1;               // 1..6
            const uint64_t im = (1ull << (8 * I)) - 1ull;
            len = P6 > I ? P6 + 1 : I;
            lo = (dig & im) | (0x2eull << (8 * I)) | ((dig >> (8 * I)) << (8 * I + 8));
            lo &= (1ull << (8 * len)) - 1ull;             // (len <= 7)
            if (expo) {                                   // e+XX / e-XX behind at most 7 bytes
                const uint32_t ax = (uint32_t)(X < 0 ? -X : X);
                const uint64_t suffix = 0x65ull | ((X < 0 ? 0x2dull : 0x2bull) << 8) | ((uint64_t)('0' + ax / 10u) << 16) | ((uint64_t)('0' + ax % 10u) << 24);
                lo |= suffix << (8 * len);
                hi = len > 4 ? suffix >> (64 - 8 * len) : 0ull;
                len += 4;
            }
        }
    }
    if (neg) {
        hi = (hi << 8) | (lo >> 56);
        lo = (lo << 8) | 0x2dull;
        ++len;
    }
    t[0] = lo;
    t[1] = hi;
    return len;
}

#ifndef RD_FT_HOST
// the length alone (the count pass of the splice)
__device__ __forceinline__ int ft_length(uint32_t bits) {
    uint64_t t[2];
    return ft_format(bits, t);
}

// the text's bytes at p, any alignment (the write pass of the splice: a text ends where the next byte of the line begins)
__device__ __forceinline__ void ft_put(uint8_t *__restrict__ p, const uint64_t t[2], int len) {
#pragma unroll
    for (int i = 0; i < 13; ++i)
        if (i < len) p[i] = (uint8_t)((i < 8 ? t[0] >> (8 * i) : t[1] >> (8 * (i - 8))) & 0xffu);
}

constexpr int FT_THREADS = 256;
constexpr int FT_MAX_WGS = 1024;                // (grid-stride: 4 workgroups per CU)

// one value per lane and step; a slot of 16 bytes is written whole by one store
__global__ __launch_bounds__(FT_THREADS) void rd_float_text_kernel(const uint32_t *__restrict__ bits, int64_t n, uint8_t *__restrict__ text, uint8_t *__restrict__ len) {
    for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FT_THREADS) {
        uint64_t t[2];
        const int l = ft_format(bits[i], t);
        const u32x4 v = {(uint32_t)t[0], (uint32_t)(t[0] >> 32), (uint32_t)t[1], (uint32_t)(t[1] >> 32)};
        *reinterpret_cast<u32x4 *>(text + FT_SLOT * i) = v;
        len[i] = (uint8_t)l;
    }
}
#endif

}  // namespace
