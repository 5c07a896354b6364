// apd_knn_math.h -- the mean distance to a point's k nearest neighbours and the statistical threshold on it (arithmetic contract
// C12): the relation under apd_points_knn_mean_distances and apd_points_remove_statistical, written once and compiled
// by hipcc into the kernels (apd_points_knn.hip) and by the host compiler into whoever restates it.  As in apd_radius_math.h:
// -ffp-contract=off, no fast-math, every operation an IEEE binary32 operation in a fixed order unless binary64 is stated; sqrtf
// correctly rounded (C4).
//
// Neighbours.  Those of contract C11 (apd_radius_math.h), unchanged, on the grid of cell size `radius` at `origin`: other indices,
// both points inside the grid, adjacent cells, radius_d2 <= r2.  The search is bounded by the radius on purpose: the 27-cell
// search stays the definition, and an isolated point costs nothing.
//
// Score.  d_i of point i for a given k in 1 .. kKnnMaxK: with at least k neighbours, the k smallest radius_d2(i, j) over its
// neighbours -- a multiset, ties need no rule --, sqrtf of each, summed in ascending order from 0.0f, divided by (float)k
// (knn_score).  With fewer than k neighbours, an isolated point and a point outside the grid included, d_i = +inf (knn_none).
// A score is never NaN and never negative: a neighbour's d2 is at most r2, which is finite.
//
// Threshold.  Over the FULL points, those with a finite d_i (knn_full), in input-index order, in binary64: n_f their number,
// S1 = sum (double)d_i, S2 = sum (double)d_i * (double)d_i, each taken in chunks of kKnnChunk consecutive input indices -- a
// chunk's sum sequential and ascending from 0.0, the others contributing nothing (knn_chunk_sums), the total the sequential
// ascending sum of the chunk sums -- so that a device reduction and a host loop give the same bits.  Then (knn_threshold)
//   mu = S1 / n_f, var = (S2 - S1 * S1 / n_f) / (n_f - 1) clamped below at 0.0 (n_f < 2: var = 0), sigma = sqrt(var),
//   T = mu + (double)std_ratio * sigma; n_f == 0: T = 0.
// Removal.  Point i is kept when d_i is finite and (double)d_i <= T (knn_kept); with n_f == 0 nothing is kept.
#pragma once

#include <math.h>
#include <stddef.h>

#include "apd_radius_math.h"

namespace apd_fusion {

constexpr unsigned kKnnMaxK = 64;  // the largest k
constexpr int kKnnChunk = 256;     // input indices per chunk of the threshold's sums

APD_HD float knn_none() { return INFINITY; }

// The score from the k smallest d2 of a point's neighbours; at(s): the s-th of them in ascending order, s < k
template <typename At> APD_HD float knn_score(At &&at, unsigned k)
{
    float sum = 0.0f;
    for (unsigned s = 0; s < k; ++s) {
        const float d = sqrtf(at(s));
        sum = sum + d;
    }
    return sum / (float)k;
}

APD_HD bool knn_full(float d) { return fabsf(d) <= 3.402823466e+38f; }  // finite; a score is never NaN

// One chunk: scores d[0 .. count), count <= kKnnChunk consecutive input indices
APD_HD void knn_chunk_sums(const float *d, size_t count, double &s1, double &s2, unsigned &full)
{
    s1 = 0.0;
    s2 = 0.0;
    full = 0;
    for (size_t j = 0; j < count; ++j) {
        if (knn_full(d[j])) {
            const double v = (double)d[j];
            const double vv = v * v;
            s1 = s1 + v;
            s2 = s2 + vv;
            ++full;
        }
    }
}

// T from the totals of the chunk sums.  Host arithmetic: the device never computes it
inline double knn_threshold(unsigned long long n_f, double S1, double S2, float std_ratio)
{
    if (n_f == 0) {
        return 0.0;
    }
    const double nf = (double)n_f;
    const double mu = S1 / nf;
    double var = 0.0;
    if (n_f >= 2) {
        const double sq = S1 * S1;
        const double part = sq / nf;
        const double diff = S2 - part;
        var = diff / (nf - 1.0);
        if (!(var > 0.0)) {
            var = 0.0;
        }
    }
    const double sigma = sqrt(var);
    const double spread = (double)std_ratio * sigma;
    return mu + spread;
}

APD_HD bool knn_kept(float d, double T) { return knn_full(d) && (double)d <= T; }

}  // namespace apd_fusion
