// apd_nearest_math.h -- the nearest point of another cloud within a radius, and precision / recall / F-score at a threshold
// (arithmetic contract C17): the relation under apd_points_nearest and apd_points_score, written once and compiled by
// hipcc into the kernel (apd_points_nearest.hip) and by the host compiler into whoever restates it.  As in apd_radius_math.h:
// -ffp-contract=off, no fast-math, every operation an IEEE binary32 operation in a fixed order unless binary64 is stated; sqrtf
// correctly rounded (C4).
//
// Grid.  That of contract C11 (apd_radius_math.h), cell size `radius`, origin `origin`; the query cloud P and the target cloud Q
// stand on the same grid.  A point outside the grid (radius_cells false) has no nearest point and is nobody's nearest point.
//
// Candidates.  Those of query point i of P are the points j of Q inside the grid whose cell differs from i's by at most 1 on
// every axis (radius_cells_adjacent) and for which radius_d2(P_i, Q_j) <= r2, r2 = radius * radius.  As in C11 the cell condition
// is part of the definition: a loop over all pairs that applies it gives the same bits as the search of the 27 cells.  P and Q
// may be the same cloud; a point is then its own candidate, at d2 = 0.
//
// Nearest.  The candidate with the least d2; among candidates with equal d2 the one with the smallest index j in Q
// (nearest_takes: it does not depend on the order in which the candidates are met).
// Results.  distance_i = sqrtf(d2) (nearest_distance), index_i = j as a 32-bit signed integer; without a candidate +inf
// (nearest_no_distance) and -1 (kNearestNoIndex).  A distance is never NaN and never negative, and it is finite exactly when a
// candidate exists: d2 <= r2, which is finite.
//
// Score at threshold tau: radius = tau, so "finite" is "within tau".  a = the number of finite distances from P to Q, b = that
// from Q to P; n_P and n_Q count every point of a cloud, those outside the grid too (nearest_score):
//   precision = (double)a / (double)n_P, recall = (double)b / (double)n_Q, each 0 when its denominator is 0;
//   fscore = 2 * precision * recall / (precision + recall), the product taken left to right, 0 when the sum is 0;
//   mean_p = S / (double)a with S the binary64 sum of the finite distances from P to Q in contract C12's fixed order -- chunks of
//   kKnnChunk consecutive input indices, each summed ascending from 0.0 (knn_chunk_sums), the chunk sums added ascending --,
//   0 when a is 0; mean_q the same for the distances from Q to P and b.
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_knn_math.h"

namespace apd_fusion {

constexpr int32_t kNearestNoIndex = -1;

APD_HD float nearest_no_distance() { return INFINITY; }

// Whether candidate j at squared distance d2 (<= r2 already) replaces the best so far, (best_d2, best_j); have: there is one
APD_HD bool nearest_takes(float d2, uint32_t j, bool have, float best_d2, uint32_t best_j)
{
    return !have || d2 < best_d2 || (d2 == best_d2 && j < best_j);
}

APD_HD float nearest_distance(float d2) { return sqrtf(d2); }

// The nine numbers of a score; the layout of apd_points_score_t (include/apd_mi355x.h)
struct NearestScore {
    long long n_p, n_q, p_within, q_within;
    double precision, recall, fscore, mean_p, mean_q;
};

// From the counts and the totals of the chunk sums.  Host arithmetic: the device never computes it
inline NearestScore nearest_score(unsigned long long n_p, unsigned long long n_q, unsigned long long a, unsigned long long b, double sum_p, double sum_q)
{
    NearestScore s;
    s.n_p = (long long)n_p;
    s.n_q = (long long)n_q;
    s.p_within = (long long)a;
    s.q_within = (long long)b;
    s.precision = n_p > 0 ? (double)a / (double)n_p : 0.0;
    s.recall = n_q > 0 ? (double)b / (double)n_q : 0.0;
    const double sum = s.precision + s.recall;
    const double twice = 2.0 * s.precision;
    const double product = twice * s.recall;
    s.fscore = sum > 0.0 ? product / sum : 0.0;
    s.mean_p = a > 0 ? sum_p / (double)a : 0.0;
    s.mean_q = b > 0 ? sum_q / (double)b : 0.0;
    return s;
}

}  // namespace apd_fusion
