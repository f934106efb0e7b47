// The formatter of csrc/rd_float_text.hpp compiled for the host (tests/test_float_text_host.py): the same integer arithmetic the kernels
// run, checked without a GPU.
//   float_text_host IN OUT          IN: uint32 bit patterns; OUT: 17 bytes per value - the 16-byte slot and the length
//   float_text_host --self LO HI STEP    every STEP-th pattern of [LO, HI) against this C library's snprintf("%g"); prints the mismatches
#define RD_FT_HOST 1
#include "../ribodetector_amd/csrc/rd_float_text.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "--self")) {
        const uint64_t lo = strtoull(argv[2], nullptr, 0), hi = strtoull(argv[3], nullptr, 0), step = strtoull(argv[4], nullptr, 0);
        uint64_t bad = 0, n = 0;
        int longest = 0;
        for (uint64_t b = lo; b < hi; b += step, ++n) {
            const uint32_t bits = (uint32_t)b;
            float f;
            memcpy(&f, &bits, 4);
            char want[32];
            const int wl = snprintf(want, sizeof(want), "%g", (double)f);
            uint64_t t[2];
            const int l = ft_format(bits, t);
            char got[17] = {0};
            memcpy(got, t, 16);
            longest = l > longest ? l : longest;
            bool ok = l == wl && !memcmp(got, want, (size_t)wl);
            for (int i = l; i < 16 && ok; ++i) ok = got[i] == 0;
            if (!ok && ++bad <= 20) printf("0x%08x: got '%s' (%d), want '%s'\n", bits, got, l, want);
        }
        printf("%llu values, %llu mismatches, longest %d\n", (unsigned long long)n, (unsigned long long)bad, longest);
        return bad != 0;
    }
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t bits;
    while (fread(&bits, 4, 1, in) == 1) {
        uint64_t t[2];
        const uint8_t l = (uint8_t)ft_format(bits, t);
        fwrite(t, 16, 1, out);
        fwrite(&l, 1, 1, out);
    }
    return fclose(out) != 0;
}
