// score_metrics.cpp -- frog_score_metrics_from (include/frog_host.h): normalised cross-correlation, mean absolute difference,
// RMSE, mutual information and its normalised form from the sums and the joint histogram of frog_cover_score.  Plain f64 in
// the order the header states; x86-64 without -mfma contracts nothing.
#include "frog_host.h"

#include <cmath>
#include <limits>
#include <vector>

namespace {

// -(sum of p log p) over the non-empty counts, ascending
double entropy(const uint64_t *counts, size_t n_counts, double n)
{
    double acc = 0.0;
    for (size_t i = 0; i < n_counts; i++) {
        if (!counts[i]) continue;
        const double p = (double)counts[i] / n;
        const double t = p * std::log(p);
        acc = acc + t;
    }
    return -acc;
}

} // namespace

extern "C" int frog_score_metrics_from(const frog_score_sums *s, const uint64_t *histogram, uint32_t bins, frog_score_metrics *out)
{
    if (!s || !out || (histogram && (bins < 2 || bins > 64))) return FROG_E_INVALID;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->ncc = out->mean_abs_diff = out->rmse = out->mi = out->nmi = nan;
    if (!s->n) return FROG_OK;
    const double n = (double)s->n;
    const double xx = s->sx * s->sx, yy = s->sy * s->sy, xy = s->sx * s->sy;
    const double cx = s->sxx - xx / n, cy = s->syy - yy / n, cxy = s->sxy - xy / n;
    if (cx > 0 && cy > 0) {
        const double v = cx * cy;
        out->ncc = cxy / std::sqrt(v);
    }
    out->mean_abs_diff = s->sad / n;
    const double twice = 2 * s->sxy;
    const double r = ((s->sxx - twice) + s->syy) / n;
    out->rmse = r < 0 ? 0.0 : std::sqrt(r);
    if (!histogram) return FROG_OK;
    std::vector<uint64_t> rx(bins, 0), ry(bins, 0);
    for (uint32_t i = 0; i < bins; i++)
        for (uint32_t j = 0; j < bins; j++) { rx[i] += histogram[(size_t)i * bins + j]; ry[j] += histogram[(size_t)i * bins + j]; }
    const double hx = entropy(rx.data(), bins, n), hy = entropy(ry.data(), bins, n), hxy = entropy(histogram, (size_t)bins * bins, n);
    const double both = hx + hy;
    out->mi = both - hxy;
    out->nmi = hxy == 0 ? 1.0 : both / hxy;
    return FROG_OK;
}
