// apd_smooth_math.h -- a point's position projected on the weighted least-squares plane of its neighbourhood (arithmetic contract
// C16): the relation under apd_points_smoothed_positions and apd_points_with_smoothed_positions, written once and
// compiled by hipcc into the kernel (apd_points_smooth.hip) and by the host compiler into whoever restates it.  As in
// apd_normal_math.h, which it includes and reuses unchanged: -ffp-contract=off, no fast-math, every operation an IEEE operation in a
// fixed order; binary32 where the positions are subtracted and the squared distance is formed, binary64 from there on.
//
// Neighbours.  Those of contract C11 (apd_radius_math.h), unchanged, on the grid of cell size `radius` at `origin`.  Point i at P
// with c neighbours -- the point itself is not counted in c -- has an estimate when c >= min_neighbours, min_neighbours in
// kNormalMinNeighbours .. kNormalMaxNeighbours.
//
// Weight of a term at Q seen from P (smooth_weight).  d2 = radius_d2(P, Q) in binary32, r2 = radius * radius in binary32;
// t = 1.0 - (double)d2 / (double)r2;  w = t * t.  The point's own term has d2 = +0 and so w = 1.0 exactly (as has a neighbour at
// the same position); a neighbour at exactly the radius has d2 == r2 and w = 0.0, and still counts in c.  0 <= w <= 1.
//
// Sums (smooth_add).  Over the point and its neighbours in the walk's order, ascending (cell key, input index); binary64,
// sequentially from 0.0.  d = Q - P as in normal_add: three binary32 subtractions, each converted.  W += w; for each a:
// wd_a = w * d_a, then s[a] += wd_a; for the six a <= b: S_ab += wd_a * d_b, every product rounded before it is added.  They
// are kept in a NormalSums with n = W, and normal_solve(sums, N, ...) of contract C14 gives the weighted plane's normal as
// binary32, signed like the stored normal N, with `sweeps` and `capped`: W >= 1 (the own term), so its precondition holds.  A
// capped solve is a defined result like any other; the cap is C14's and is not raised here.
//
// Projection (smooth_project).  m_a = s[a] / W;  n_a = (double)normal_a, the binary32 result converted back;
// h = (m_0 * n_0 + m_1 * n_1) + m_2 * n_2, every product rounded;  X_a = (float)((double)P_a + h * n_a);  offset = (float)h,
// signed along the returned normal.  h * n does not depend on the sign rule.  |h| <= |m| <= radius: a step never exceeds a cell.
//
// No estimate.  c < min_neighbours, or a point outside the grid: the position is copied bit for bit and the offset is +inf
// (smooth_none).
//
// Iterations.  Simultaneous: iteration k computes every point's result from the positions after iteration k - 1, on the grid and
// in the cell order rebuilt from those positions, ties broken by input index as ever; the stored normal stays the object's own
// in every iteration.  A point that leaves the grid by moving has no estimate from then on and stays where it is.
#pragma once

#include <math.h>

#include "apd_normal_math.h"

namespace apd_fusion {

constexpr unsigned kSmoothMaxIterations = 16;  // iterations of apd_points_with_smoothed_positions at most

APD_HD float smooth_none() { return INFINITY; }

// The weight of the term at squared distance d2 <= r2
APD_HD double smooth_weight(float d2, float r2)
{
    const double q = (double)d2 / (double)r2;
    const double t = 1.0 - q;
    return t * t;
}

// One term: the point at Q, within the radius of P, seen from P
APD_HD_FLAT void smooth_add(NormalSums &m, const float P[3], const float Q[3], float r2)
{
    const double w = smooth_weight(radius_d2(P, Q), r2);
    const float fx = Q[0] - P[0], fy = Q[1] - P[1], fz = Q[2] - P[2];
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double wx = w * x, wy = w * y, wz = w * z;
    const double xx = wx * x, xy = wx * y, xz = wx * z, yy = wy * y, yz = wy * z, zz = wz * z;
    m.n = m.n + w;
    m.s[0] = m.s[0] + wx;
    m.s[1] = m.s[1] + wy;
    m.s[2] = m.s[2] + wz;
    m.xx = m.xx + xx;
    m.xy = m.xy + xy;
    m.xz = m.xz + xz;
    m.yy = m.yy + yy;
    m.yz = m.yz + yz;
    m.zz = m.zz + zz;
}

// The new position X and the offset of the point at P with the weighted sums m (m.n >= 1) and the stored normal N; normal: the
// weighted plane's, as the offset is signed along it
APD_HD_FLAT void smooth_project(const NormalSums &m, const float N[3], const float P[3], float X[3], float &offset, float normal[3], unsigned &sweeps,
                                bool &capped)
{
    float variation = 0.0f;
    normal_solve(m, N, normal, variation, sweeps, capped);
    const double mx = m.s[0] / m.n, my = m.s[1] / m.n, mz = m.s[2] / m.n;
    const double nx = (double)normal[0], ny = (double)normal[1], nz = (double)normal[2];
    const double hx = mx * nx, hy = my * ny, hz = mz * nz;
    const double hxy = hx + hy;
    const double h = hxy + hz;
    const double sx = h * nx, sy = h * ny, sz = h * nz;
    X[0] = (float)((double)P[0] + sx);
    X[1] = (float)((double)P[1] + sy);
    X[2] = (float)((double)P[2] + sz);
    offset = (float)h;
}

}  // namespace apd_fusion
