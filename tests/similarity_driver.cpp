// The driver of tests/test_similarity.py: frog_amd/csrc/device/similarity.h by itself, with no library of the project's.
// Reads cases from stdin until it ends.  A case is
//   n  <n * 6 words>
// one correspondence per 6 words: source x y z, target x y z, each float as the 8 hex digits of its bits (the words of a case
// may follow one another without blanks).
// Prints one line per case: similarity_fit's return value, the 16 doubles of `out` and the two largest eigenvalues of N
// (0 0 when no N was formed), all as hex floats.
#include "similarity.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    size_t n;
    std::vector<float> words;
    while (std::scanf("%zu", &n) == 1) {
        words.resize(6 * n);
        for (float &w : words) {
            uint32_t bits;
            if (std::scanf("%8" SCNx32, &bits) != 1) return 3;
            std::memcpy(&w, &bits, sizeof bits);
        }
        double out[16], top2[2];
        const bool ok = frog::similarity_fit(n, [&](size_t i, double a[3], double b[3]) {
            for (int k = 0; k < 3; k++) { a[k] = words[6 * i + k]; b[k] = words[6 * i + 3 + k]; }
        }, out, top2);
        std::printf("%d", (int)ok);
        for (double v : out) std::printf(" %a", v);
        std::printf(" %a %a\n", top2[0], top2[1]);
    }
    return 0;
}
