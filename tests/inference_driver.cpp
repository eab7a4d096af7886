// The driver of tests/test_inference_host.py: frog_amd/csrc/host/inference.h by itself, with no library of the project's.
// Reads cases from stdin until it ends.  A case is
//   f|u  sides  rows  <rows * sides null values>  m  <m values>
// with f: floats, each as the 8 hex digits of its bits; u: uint32_t in decimal.  A null row's sides are reduced by sides_max.
// Prints per value "<p> <significant>", p as a hex float, then the case's threshold_p05 as a hex float.
#include "inference.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

template <class T>
bool read_value(T *v);

template <>
bool read_value<float>(float *v)
{
    uint32_t bits;
    if (std::scanf("%" SCNx32, &bits) != 1) return false;
    std::memcpy(v, &bits, sizeof bits);
    return true;
}

template <>
bool read_value<uint32_t>(uint32_t *v)
{
    return std::scanf("%" SCNu32, v) == 1;
}

template <class T>
bool run_case(uint32_t sides)
{
    size_t rows = 0, m = 0;
    if (std::scanf("%zu", &rows) != 1) return false;
    std::vector<T> row(sides), null(rows);
    for (size_t k = 0; k < rows; k++) {
        for (uint32_t s = 0; s < sides; s++)
            if (!read_value(&row[s])) return false;
        null[k] = frog::sides_max(row.data(), sides);
    }
    const frog::NullDistribution<T> dist(std::move(null));
    if (std::scanf("%zu", &m) != 1) return false;
    for (size_t i = 0; i < m; i++) {
        T v;
        if (!read_value(&v)) return false;
        std::printf("%a %d\n", (double)dist.p(v), (int)dist.significant(v));
    }
    std::printf("%a\n", dist.threshold_p05());
    return true;
}

int main()
{
    char type;
    uint32_t sides;
    while (std::scanf(" %c %" SCNu32, &type, &sides) == 2) {
        if ((type != 'f' && type != 'u') || sides < 1 || sides > 2) return 2;
        if (!(type == 'f' ? run_case<float>(sides) : run_case<uint32_t>(sides))) return 3;
    }
    return 0;
}
