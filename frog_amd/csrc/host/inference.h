// inference.h -- the inference of GroupStats' permutation test, stated once for its three statistics (the voxel's t, the
// cluster's extent, the voxel's tfce): the null distribution of one contrast with its corrected p and its p < 0.05 rule, the
// reduction of a slot's sides, and the csv pieces the tool's tables share.  Plain C++17 with no header of the project's, so a
// test compiles it alone (tests/inference_driver.cpp).
#ifndef FROG_INFERENCE_H
#define FROG_INFERENCE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <ostream>
#include <string>
#include <vector>

namespace frog {

// The larger of a slot row's sides: row[0], or with two sides max(row[0], row[1]).  The t-test's row is { max_t, -min_t }.
template <class T>
T sides_max(const T *row, uint32_t sides)
{
    return sides == 2 ? std::max(row[0], row[1]) : row[0];
}

// The null distribution of one contrast: the statistic's largest value under permutations 1..nPerms-1 (permutation 0 is the
// design itself and is not part of it), sorted.  T is the statistic's own type -- float, or uint32_t for extents -- and every
// comparison is made in it.
template <class T>
class NullDistribution {
public:
    explicit NullDistribution(std::vector<T> values) : null(std::move(values)), nPerms((long)null.size() + 1) { std::sort(null.begin(), null.end()); }

    // The family-wise corrected p of a value, (float)((1 + #{k >= 1 : null[k] >= value}) / (double)nPerms), and whether it is
    // below 0.05, in integers.  Nothing is below a NaN, so every null value counts against it: p = 1.
    struct Verdict {
        float p;
        bool significant;
    };
    Verdict test(T value) const
    {
        const size_t exceed = null.end() - std::lower_bound(null.begin(), null.end(), value);
        return Verdict{ (float)((double)(1 + exceed) / (double)nPerms), 20 * (1 + (long)exceed) < nPerms };
    }
    float p(T value) const { return test(value).p; }
    bool significant(T value) const { return test(value).significant; }

    // The largest null value a statistic must exceed for p < 0.05, so that significant(v) == (v > threshold_p05()):
    // (nPerms - 1) / 20 - 1 exceedances are allowed; fewer than 0 means that no value gets there (+inf).
    double threshold_p05() const
    {
        const long allowed = (nPerms - 1) / 20 - 1;
        return allowed < 0 ? INFINITY : (allowed >= (long)null.size() ? -INFINITY : (double)null[null.size() - 1 - allowed]);
    }

private:
    std::vector<T> null;
    long nPerms;
};

inline std::string csv_float(float v)
{
    if (std::isnan(v)) return "nan";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.9g", (double)v);
    return buf;
}

// "value,x,y,z" of the peak at voxel index `peak` of a grid of dims, or "nan,,," where there is none (peak == the grid's voxels)
inline void write_peak(std::ostream &csv, const float *map, size_t peak, const uint32_t dims[3])
{
    const size_t plane = (size_t)dims[0] * dims[1];
    if (peak < plane * dims[2]) csv << csv_float(map[peak]) << "," << peak % dims[0] << "," << (peak / dims[0]) % dims[1] << "," << peak / plane;
    else csv << "nan,,,";
}

// closes the file; false if that or any write before it failed
inline bool csv_close(std::ofstream &csv)
{
    csv.close();
    return (bool)csv;
}

} // namespace frog

#endif
