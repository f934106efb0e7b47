// The scanner and the converter of csrc/rd_float_parse.hpp compiled for the host (tests/test_float_parse_host.py): the same integer
// arithmetic the kernels run, checked without a GPU.
//   float_parse_host IN OUT             IN: values as length:uint32 and the text's bytes; OUT: 5 bytes per value - bits:uint32 and the
//                                       status (0 converted, 1 not of the syntax, 2 more than 17 significant digits; bits 0 for 1 and 2)
//   float_parse_host --self LO HI STEP  every STEP-th finite pattern of [LO, HI) printed with "%.9g" and with "%g", parsed, and held
//                                       against this C library's strtof of the same text; prints the mismatches
#define RD_FP_HOST 1
#include "../ribodetector_amd/csrc/rd_float_parse.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static int parse(const uint8_t *text, size_t len, uint32_t &bits) {
    FpNum num;
    const int st = fp_value(text, 0, (int64_t)len, num);
    bits = st == FP_OK ? fp_bits(num) : 0u;
    return st;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "--self")) {
        const uint64_t lo = strtoull(argv[2], nullptr, 0), hi = strtoull(argv[3], nullptr, 0), step = strtoull(argv[4], nullptr, 0);
        uint64_t bad = 0, n = 0;
        for (uint64_t b = lo; b < hi; b += step) {
            const uint32_t pattern = (uint32_t)b;
            if (((pattern >> 23) & 0xffu) == 0xffu) continue;
            float f;
            memcpy(&f, &pattern, 4);
            for (int form = 0; form < 2; ++form, ++n) {
                char text[40];
                const int l = snprintf(text, sizeof(text), form ? "%g" : "%.9g", (double)f);
                const float w = strtof(text, nullptr);
                uint32_t want, got;
                memcpy(&want, &w, 4);
                const int st = parse((const uint8_t *)text, (size_t)l, got);
                const bool ok = st == FP_OK && got == want && (form || got == pattern);
                if (!ok && ++bad <= 20) printf("'%s': got 0x%08x (status %d), want 0x%08x\n", text, got, st, want);
            }
        }
        printf("%llu texts, %llu mismatches\n", (unsigned long long)n, (unsigned long long)bad);
        return bad != 0;
    }
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        std::vector<uint8_t> text(len);          // the text and not a byte more: a sanitizer sees a read at or behind the value's end
        if (len && fread(text.data(), 1, len, in) != len) return 2;
        uint32_t bits;
        const uint8_t st = (uint8_t)parse(text.data(), len, bits);
        fwrite(&bits, 4, 1, out);
        fwrite(&st, 1, 1, out);
    }
    return fclose(out) != 0;
}
