// rd_float_parse.hpp - the text of a float as the float32 nearest to its EXACT decimal value, ties to the even mantissa, denormals
// included, in one rounding (C ABI rd_float_parse; the f and B:f values of rd_bam_encode_ex under RD_UBAM_TAG_FLOATS, rd_bam_encode.hpp):
// the inverse of rd_float_text.hpp. The rule is ribodetector_amd/bam.py (float_from_text); DESIGN.md §3.30. Part of the single
// translation unit rd_kernels.hip; the scanner and the converter (fp_scan, fp_round) are plain C++ over integers and compile for the
// host as well (-DRD_FP_HOST, tests/test_float_parse_host.py).
//
// fp_scan: [+-]? ( D+ | D* '.' D+ ) ( [eE] [+-]? D{1,4} )? or [+-]? inf / nan in any letter case. It takes the LONGEST prefix of
// text[p, e) that is of the syntax and says where it ends: a caller holds that end against the value's own ('5.', '1e', '1e12345' and
// 'infinity' all end early). The digits without their leading and trailing zeros are M of s digits, the value is v = M 10^q. s > 17 is
// not converted (FP_LONG): M < 10^17 < 2^57 is what bounds everything below. q is clamped to [-63, 39]: with M < 10^17, q > 38 is
// v >= 10^39 > 2^128, infinity, and q < -62 is v < 10^-46 < 2^-150, zero - the same as any q further out.
//
// fp_round, -62 <= q <= 38. Both branches end in (X, sticky, ex): v = (X + f) 2^ex with a whole X < 2^32, 0 <= f < 1, sticky = f != 0,
// and X holds at least 25 significant bits whenever f != 0 - then fp_pack rounds once: the ulp's exponent is max(floor(log2 v), -126) - 23.
//   q >= 0  v = P 2^q, P = M 5^q < 2^57 5^38 < 2^146 (5 limbs). P moved up so that its highest bit is bit 191 of 6 limbs: X = limb 5,
//           sticky = the limbs below.
//   q < 0   v = M 2^q / D, D = 5^-q <= 5^62 < 2^144. With a, b the bit lengths of M and D, M / D lies in (2^(a - b - 1), 2^(a - b + 1)), so
//           k = 26 - a + b makes the quotient Q = floor(M 2^k / D) one of 26 or 27 bits: X = Q, sticky = the remainder != 0, ex = q - k.
//           k >= 0: A = M 2^k has a + k = 26 + b <= 170 bits; k < 0 (b < a - 26 <= 31): A = M and D 2^-k of a - 26 bits takes D's place.
//           Q starts from a float estimate: the highest 32 bits of M times the table's 2^b / 5^-q in (1, 2] times 2^-6 - one truncation
//           (2^-31) and three roundings (2^-24 each) move a number below 2^27 by less than 25, the conversion to a whole number by less
//           than 1 - 32 lower, so that R = A - Q D lies in [7 D, 58 D): 6 limbs hold A, Q D < 2^171 and R. Then c = floor(R / D) from the
//           two as floats (the sum of their limbs, relative error far below 1 / 64), one lower, and at most two times D more by compare
//           and subtract (three are coded).
// No double, no division of limbs, every limb index a constant (registers, no scratch): a shift by a variable count is three conditional
// moves by 4, 2 and 1 limbs and a funnel shift.
#pragma once
#include <stdint.h>

#ifdef RD_FP_HOST
#define FP_FN static inline
#define FP_TABLE static const
#define FP_UNROLL
#define FP_CLZ32(x) __builtin_clz(x)
#define FP_CLZ64(x) __builtin_clzll(x)
#else
#include "rd_common.hpp"
#define FP_FN __device__ __forceinline__
#define FP_TABLE __device__ const
#define FP_UNROLL _Pragma("unroll")
#define FP_CLZ32(x) __builtin_clz(x)
#define FP_CLZ64(x) __builtin_clzll(x)
#endif

namespace {

constexpr int FP_LIMBS = 6;
constexpr int FP_POW5_MAX = 62;
constexpr int FP_DIGITS = 17;                   // significant digits at most (bam.FLOAT_DIGITS)
constexpr int FP_Q_MIN = -63, FP_Q_MAX = 39;    // q as fp_scan clamps it: one past what fp_round computes with
constexpr int FP_OK = 0, FP_BAD = 1, FP_LONG = 2;      // the status of rd_float_parse
constexpr uint32_t FP_BITS_INF = 0x7f800000u, FP_BITS_NAN = 0x7fc00000u;

// 5^i, i = 0..62, little-endian limbs (5^62 < 2^144)
FP_TABLE uint32_t fp_pow5[FP_POW5_MAX + 1][5] = {
    {0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000005u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x00000019u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x0000007du, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x00000271u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x00000c35u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x00003d09u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x0001312du, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x0005f5e1u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x001dcd65u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x009502f9u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x02e90eddu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x0e8d4a51u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x48c27395u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x6bcc41e9u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x1afd498du, 0x00000007u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x86f26fc1u, 0x00000023u, 0x00000000u, 0x00000000u, 0x00000000u}, {0xa2bc2ec5u, 0x000000b1u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x2dace9d9u, 0x00000378u, 0x00000000u, 0x00000000u, 0x00000000u}, {0xe460913du, 0x00001158u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x75e2d631u, 0x000056bcu, 0x00000000u, 0x00000000u, 0x00000000u}, {0x4d6e2ef5u, 0x0001b1aeu, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8326eac9u, 0x00087867u, 0x00000000u, 0x00000000u, 0x00000000u}, {0x8fc295edu, 0x002a5a05u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xcecceda1u, 0x00d3c21bu, 0x00000000u, 0x00000000u, 0x00000000u}, {0x0a00a425u, 0x0422ca8bu, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x320334b9u, 0x14adf4b7u, 0x00000000u, 0x00000000u, 0x00000000u}, {0xfa10079du, 0x6765c793u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xe2502611u, 0x04fce5e3u, 0x00000002u, 0x00000000u, 0x00000000u}, {0x6b90be55u, 0x18f07d73u, 0x0000000au, 0x00000000u, 0x00000000u},
    {0x19d3b7a9u, 0x7cb27341u, 0x00000032u, 0x00000000u, 0x00000000u}, {0x8122964du, 0x6f7c4045u, 0x000000fcu, 0x00000000u, 0x00000000u},
    {0x85acef81u, 0x2d6d415bu, 0x000004eeu, 0x00000000u, 0x00000000u}, {0x9c60ad85u, 0xe32246c9u, 0x000018a6u, 0x00000000u, 0x00000000u},
    {0x0de36399u, 0x6fab61f0u, 0x00007b42u, 0x00000000u, 0x00000000u}, {0x4570f1fdu, 0x2e58e9b0u, 0x0002684cu, 0x00000000u, 0x00000000u},
    {0x5b34b9f1u, 0xe7bc9071u, 0x000c097cu, 0x00000000u, 0x00000000u}, {0xc807a1b5u, 0x86aed236u, 0x003c2f70u, 0x00000000u, 0x00000000u},
    {0xe8262889u, 0xa16a1b11u, 0x012ced32u, 0x00000000u, 0x00000000u}, {0x88becaadu, 0x27128759u, 0x05e0a1fdu, 0x00000000u, 0x00000000u},
    {0xabb9f561u, 0xc35ca4bfu, 0x1d6329f1u, 0x00000000u, 0x00000000u}, {0x5aa1cae5u, 0xd0cf37beu, 0x92efd1b8u, 0x00000000u, 0x00000000u},
    {0xc528f679u, 0x140c16b7u, 0xdeaf189cu, 0x00000002u, 0x00000000u}, {0xd9ccd05du, 0x643c7196u, 0x596b7b0cu, 0x0000000eu, 0x00000000u},
    {0x410011d1u, 0xf52e37f2u, 0xbf19673du, 0x00000047u, 0x00000000u}, {0x45005915u, 0xc9e717bbu, 0xbb7f0435u, 0x00000166u, 0x00000000u},
    {0x5901bd69u, 0xf18376a8u, 0xa97b150cu, 0x00000701u, 0x00000000u}, {0xbd08b30du, 0xb7915149u, 0x4f676940u, 0x00002308u, 0x00000000u},
    {0xb12b7f41u, 0x95d69670u, 0x8d050e43u, 0x0000af29u, 0x00000000u}, {0x75d97c45u, 0xed30f033u, 0xc1194751u, 0x00036bcfu, 0x00000000u},
    {0x4d3f6d59u, 0xa1f4b101u, 0xc57e6499u, 0x00111b0eu, 0x00000000u}, {0x823d22bdu, 0x29c77506u, 0xdb77f700u, 0x00558749u, 0x00000000u},
    {0x8b31adb1u, 0xd0e54920u, 0x4957d300u, 0x01aba471u, 0x00000000u}, {0xb7f86475u, 0x147a6da2u, 0x6eb71f04u, 0x085a3636u, 0x00000000u},
    {0x97d9f649u, 0x6664242du, 0x29939b14u, 0x29c30f10u, 0x00000000u}, {0xf741cf6du, 0xfff4b4e3u, 0xcfe20765u, 0xd0cf4b50u, 0x00000000u},
    {0xd4490d21u, 0xffc78873u, 0x0f6a24fdu, 0x140c7894u, 0x00000004u}, {0x256d41a5u, 0xfee5aa43u, 0x4d12b8f5u, 0x643e5ae4u, 0x00000014u},
    {0xbb224839u, 0xfa7c534fu, 0x815d9ccdu, 0xf537c675u, 0x00000065u}, {0xa7ab691du, 0xe46da08eu, 0x86d41005u, 0xca16e04bu, 0x000001fdu},
    {0x46590d91u, 0x762422c9u, 0xa224501du, 0xf2726179u, 0x000009f4u}, {0x5fbd43d5u, 0x4eb4adeeu, 0x2ab59093u, 0xbc3be760u, 0x000031c8u},
    {0xdeb25329u, 0x898765a7u, 0xd58bd2e0u, 0xad2b84e0u, 0x0000f8ebu},
};

// the bit length of 5^i
FP_TABLE uint8_t fp_pow5_bits[FP_POW5_MAX + 1] = {
    1, 3, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, 31, 33, 35, 38, 40, 42, 45, 47,
    49, 52, 54, 56, 59, 61, 63, 66, 68, 70, 72, 75, 77, 79, 82, 84, 86, 89, 91, 93, 96,
    98, 100, 103, 105, 107, 110, 112, 114, 117, 119, 121, 124, 126, 128, 131, 133, 135, 137, 140, 142, 144,
};

// 2^(bit length of 5^i) / 5^i rounded to float32, in (1, 2]: the estimate of Q only
FP_TABLE float fp_inv5f[FP_POW5_MAX + 1] = {
    0x1.000000p+1f, 0x1.99999ap+0f, 0x1.47ae14p+0f, 0x1.0624dep+0f, 0x1.a36e2ep+0f, 0x1.4f8b58p+0f,
    0x1.0c6f7ap+0f, 0x1.ad7f2ap+0f, 0x1.5798eep+0f, 0x1.12e0bep+0f, 0x1.b7cdfep+0f, 0x1.5fd7fep+0f,
    0x1.197998p+0f, 0x1.c25c26p+0f, 0x1.6849b8p+0f, 0x1.203afap+0f, 0x1.cd2b2ap+0f, 0x1.70ef54p+0f,
    0x1.2725dep+0f, 0x1.d83c94p+0f, 0x1.79ca10p+0f, 0x1.2e3b40p+0f, 0x1.e39202p+0f, 0x1.82db34p+0f,
    0x1.357c2ap+0f, 0x1.ef2d10p+0f, 0x1.8c240cp+0f, 0x1.3ce9a4p+0f, 0x1.fb0f6cp+0f, 0x1.95a5f0p+0f,
    0x1.4484c0p+0f, 0x1.039d66p+0f, 0x1.9f623ep+0f, 0x1.4c4e98p+0f, 0x1.09d87ap+0f, 0x1.a95a5cp+0f,
    0x1.54484ap+0f, 0x1.1039d4p+0f, 0x1.b38fbap+0f, 0x1.5c72fcp+0f, 0x1.16c262p+0f, 0x1.be03d0p+0f,
    0x1.64cfdap+0f, 0x1.1d7314p+0f, 0x1.c8b822p+0f, 0x1.6d601ap+0f, 0x1.244ce2p+0f, 0x1.d3ae36p+0f,
    0x1.7624f8p+0f, 0x1.2b50c6p+0f, 0x1.dee7a4p+0f, 0x1.7f1fb6p+0f, 0x1.327fc6p+0f, 0x1.ea6608p+0f,
    0x1.8851a0p+0f, 0x1.39dae6p+0f, 0x1.f62b0cp+0f, 0x1.91bc08p+0f, 0x1.41633ap+0f, 0x1.011c2ep+0f,
    0x1.9b604ap+0f, 0x1.4919d6p+0f, 0x1.0747dep+0f,
};

struct FpLimbs {
    uint32_t w[FP_LIMBS];
};

struct FpNum {                                  // what fp_scan read
    uint64_t M;                                 // the significant digits (0: the value is zero)
    int32_t q;                                  // v = M 10^q, clamped to [FP_Q_MIN, FP_Q_MAX]
    uint32_t sign;                              // 0 or 0x80000000
    uint32_t special;                           // 0, FP_BITS_INF or FP_BITS_NAN
};

template <int N>
FP_FN FpLimbs fp_up_limbs(const FpLimbs &x, bool on) {  // x 2^(32 N) when `on`
    FpLimbs r;
    FP_UNROLL
    for (int i = 0; i < FP_LIMBS; ++i) r.w[i] = !on ? x.w[i] : i >= N ? x.w[i >= N ? i - N : 0] : 0u;
    return r;
}

// x 2^s, 0 <= s < 192; the bits above limb 5 are lost
FP_FN FpLimbs fp_shl(const FpLimbs &x, int s) {
    const int ws = s >> 5, bs = s & 31;
    FpLimbs r = fp_up_limbs<4>(x, ws & 4);
    r = fp_up_limbs<2>(r, ws & 2);
    r = fp_up_limbs<1>(r, ws & 1);
    FpLimbs o;
    FP_UNROLL
    for (int i = 0; i < FP_LIMBS; ++i) o.w[i] = (uint32_t)(((((uint64_t)r.w[i] << 32) | (i ? r.w[i ? i - 1 : 0] : 0u)) << bs) >> 32);
    return o;
}

// a - b; `borrow` says a < b
FP_FN FpLimbs fp_sub(const FpLimbs &a, const FpLimbs &b, bool &borrow) {
    FpLimbs r;
    uint32_t c = 0;
    FP_UNROLL
    for (int i = 0; i < FP_LIMBS; ++i) {
        const uint64_t t = (uint64_t)a.w[i] - b.w[i] - c;
        r.w[i] = (uint32_t)t;
        c = (uint32_t)(t >> 63);
    }
    borrow = c != 0;
    return r;
}

// x m (the product fits 6 limbs)
FP_FN FpLimbs fp_mul(const FpLimbs &x, uint32_t m) {
    FpLimbs r;
    uint64_t c = 0;
    FP_UNROLL
    for (int i = 0; i < FP_LIMBS; ++i) {
        c += (uint64_t)m * x.w[i];
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}

// x 2^-64 as a float, relative error below 2^-20 (x < 2^171)
FP_FN float fp_float(const FpLimbs &x) {
    return (((float)x.w[0] * 0x1p-64f + (float)x.w[1] * 0x1p-32f) + ((float)x.w[2] + (float)x.w[3] * 0x1p32f)) +
           ((float)x.w[4] * 0x1p64f + (float)x.w[5] * 0x1p96f);
}

FP_FN int fp_bit_length(const FpLimbs &x) {      // of x != 0
    uint32_t top = x.w[0];
    int at = 0;
    FP_UNROLL
    for (int i = 1; i < FP_LIMBS; ++i)
        if (x.w[i]) {
            top = x.w[i];
            at = i;
        }
    return 32 * at + 32 - FP_CLZ32(top | 1u);
}

// the float32 nearest to (X + f) 2^ex, X != 0, sticky = f != 0 (header comment), ties to even
FP_FN uint32_t fp_pack(uint32_t X, bool sticky, int ex, uint32_t sign) {
    const int lz = FP_CLZ32(X);
    const uint64_t Y = (uint64_t)(X << lz);      // bit 31 set: the value lies in [2^(31 + ex), 2^(32 + ex))
    ex -= lz;
    const int e = 31 + ex, E = e > -126 ? e : -126;
    const int t = E - 23 - ex;                   // the ulp is 2^t of Y's: 8, more for a denormal
    if (t > 33) return sign;                     // below 2^-151
    uint32_t n = (uint32_t)(Y >> t);
    const bool half = (Y >> (t - 1)) & 1u;
    const bool low = (Y & ((1ull << (t - 1)) - 1ull)) != 0 || sticky;
    if (half && (low || (n & 1u))) ++n;
    const uint32_t bits = ((uint32_t)(E + 126) << 23) + n;      // n < 2^23: a denormal; n == 2^24: the next exponent
    return sign | (bits < FP_BITS_INF ? bits : FP_BITS_INF);
}

// the bits of v = M 10^q, 0 < M < 10^17
FP_FN uint32_t fp_round(uint64_t M, int q, uint32_t sign) {
    if (q > 38) return sign | FP_BITS_INF;
    if (q < -62) return sign;
    const uint32_t m0 = (uint32_t)M, m1 = (uint32_t)(M >> 32);
    if (q >= 0) {
        const uint32_t *pw = fp_pow5[q];         // q <= 38: 3 limbs
        uint32_t lo[4];
        FpLimbs P;
        uint64_t c = 0;
        FP_UNROLL
        for (int i = 0; i < 3; ++i) {
            c += (uint64_t)m0 * pw[i];
            lo[i] = (uint32_t)c;
            c >>= 32;
        }
        lo[3] = (uint32_t)c;
        P.w[0] = lo[0];
        c = 0;
        FP_UNROLL
        for (int i = 0; i < 3; ++i) {
            c += (uint64_t)m1 * pw[i] + lo[i + 1];
            P.w[i + 1] = (uint32_t)c;
            c >>= 32;
        }
        P.w[4] = (uint32_t)c;
        P.w[5] = 0;
        const int L = fp_bit_length(P);
        const FpLimbs S = fp_shl(P, 32 * FP_LIMBS - L);
        return fp_pack(S.w[5], (S.w[0] | S.w[1] | S.w[2] | S.w[3] | S.w[4]) != 0u, L - 32 + q, sign);
    }
    const int n5 = -q;
    const int a = 64 - FP_CLZ64(M), b = fp_pow5_bits[n5], k = 26 - a + b;
    FpLimbs A, D;
    FP_UNROLL
    for (int i = 0; i < FP_LIMBS; ++i) {
        A.w[i] = i == 0 ? m0 : i == 1 ? m1 : 0u;
        D.w[i] = i < 5 ? fp_pow5[n5][i < 5 ? i : 0] : 0u;
    }
    if (k >= 0) A = fp_shl(A, k);
    else D = fp_shl(D, -k);
    const uint32_t mtop = (uint32_t)((M << (64 - a)) >> 32);
    uint32_t Q = (uint32_t)((float)mtop * fp_inv5f[n5] * 0x1p-6f) - 32u;
    bool less;
    FpLimbs R = fp_sub(A, fp_mul(D, Q), less);
    uint32_t cq = (uint32_t)(fp_float(R) / fp_float(D));
    cq = cq ? cq - 1u : 0u;
    R = fp_sub(R, fp_mul(D, cq), less);
    Q += cq;
    FP_UNROLL
    for (int i = 0; i < 3; ++i) {
        const FpLimbs T = fp_sub(R, D, less);
        if (!less) {
            R = T;
            ++Q;
        }
    }
    return fp_pack(Q, (R.w[0] | R.w[1] | R.w[2] | R.w[3] | R.w[4] | R.w[5]) != 0u, q - k, sign);
}

// The longest prefix of text[p, e) that is of the syntax: FP_BAD when there is none, else `end` = where it stops, num = what it says, and
// FP_LONG when it has more than FP_DIGITS significant digits (num.M is not its value then). No byte at or behind e is read.
FP_FN int fp_scan(const uint8_t *text, int64_t p, int64_t e, FpNum &num, int64_t &end) {
    num.M = 0;
    num.q = 0;
    num.sign = 0;
    num.special = 0;
    end = p;
    if (p < e && (text[p] == '+' || text[p] == '-')) {
        num.sign = text[p] == '-' ? 0x80000000u : 0u;
        ++p;
    }
    if (p + 3 <= e) {
        const uint32_t c0 = text[p] | 0x20u, c1 = text[p + 1] | 0x20u, c2 = text[p + 2] | 0x20u;
        const bool inf = c0 == 'i' && c1 == 'n' && c2 == 'f', nan = c0 == 'n' && c1 == 'a' && c2 == 'n';
        if (inf || nan) {
            num.special = inf ? FP_BITS_INF : FP_BITS_NAN;
            end = p + 3;
            return FP_OK;
        }
    }
    uint64_t M = 0;
    int s = 0;                                   // digits of M
    int64_t zeros = 0, frac = 0, whole = 0;      // zeros behind M's last digit so far; digits behind the point; digits in front of it
    bool over = false;
    int64_t stop = p;                            // the end of the mantissa found so far
    bool point = false;
    for (; p < e; ++p) {
        const uint32_t c = text[p];
        if (c == '.' && !point) {
            point = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        if (point) ++frac;
        else ++whole;
        stop = p + 1;
        if (c == '0') {
            if (s) ++zeros;
            continue;
        }
        if ((int64_t)s + zeros + 1 > FP_DIGITS) over = true;
        else {
            for (; zeros > 0; --zeros, ++s) M *= 10u;
            M = M * 10u + (c - '0');
            ++s;
        }
        if (over) {                              // (the count alone goes on: it stays above FP_DIGITS)
            s = FP_DIGITS + 1;
            zeros = 0;
        }
    }
    if (whole + frac == 0) return FP_BAD;
    p = stop;                                    // ('D+.' : the digits in front of the point are the prefix)
    int64_t q = zeros - frac;
    if (p < e && (text[p] | 0x20u) == 'e') {      // an exponent counts when it has a digit; four of them are taken
        int64_t x = p + 1;
        bool neg = false;
        if (x < e && (text[x] == '+' || text[x] == '-')) {
            neg = text[x] == '-';
            ++x;
        }
        int v = 0, d = 0;
        for (; x < e && d < 4 && text[x] >= '0' && text[x] <= '9'; ++x, ++d) v = v * 10 + (int)(text[x] - '0');
        if (d) {
            q += neg ? -v : v;
            p = x;
        }
    }
    end = p;
    num.M = M;
    num.q = (int32_t)(q < FP_Q_MIN ? FP_Q_MIN : q > FP_Q_MAX ? FP_Q_MAX : q);
    return over ? FP_LONG : FP_OK;
}

// the bits of a value that fp_scan read with FP_OK
FP_FN uint32_t fp_bits(const FpNum &num) {
    if (num.special) return num.sign | num.special;
    if (num.M == 0) return num.sign;
    return fp_round(num.M, num.q, num.sign);
}

// text[p, e) as ONE value: the status of rd_float_parse
FP_FN int fp_value(const uint8_t *text, int64_t p, int64_t e, FpNum &num) {
    int64_t end;
    const int st = fp_scan(text, p, e, num, end);
    return st == FP_BAD || end != e ? FP_BAD : st;
}

#ifndef RD_FP_HOST
constexpr int FP_THREADS = 256;
constexpr int FP_MAX_WGS = 1024;                // (grid-stride: 4 workgroups per CU)

// one value per lane and step: value k is text[start[k], start[k + 1]), every offset held against start[n] before it is read
__global__ __launch_bounds__(FP_THREADS) void rd_float_parse_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ start, int64_t n,
                                                                   uint32_t *__restrict__ bits, uint8_t *__restrict__ status) {
    const int64_t total = start[n];
    for (int64_t i = (int64_t)blockIdx.x * FP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FP_THREADS) {
        const int64_t a = start[i], b = start[i + 1];
        int st = FP_BAD;
        uint32_t v = 0;
        if (a >= 0 && a <= b && b <= total) {
            FpNum num;
            st = fp_value(text, a, b, num);
            if (st == FP_OK) v = fp_bits(num);
        }
        bits[i] = v;
        status[i] = (uint8_t)st;
    }
}
#endif

}  // namespace
