// apd_simplify_math.h -- what simplifying an indexed triangle mesh by vertex clustering computes (arithmetic contract C23):
// the rules under apd_mesh_simplify, written once and compiled by hipcc into the kernels (apd_mesh_simplify.hip) and by the host
// compiler into the sequential checker (tests/helpers/mesh_simplify_ref.cpp).  As in apd_mesh_math.h: -ffp-contract=off, no
// fast-math, every operation an IEEE operation in a fixed order.
//
// Clusters.  Vertex v is inside the grid when voxel_key(P_v, origin, cell) of contract C10 (apd_voxel_math.h) succeeds.  A cluster is
// the set of inside vertices with one key, its members in ascending vertex index; the clusters are ordered by ascending key.  A
// vertex outside the grid (a non-finite coordinate, a cell beyond +-2^20) belongs to no cluster.
//
// Faces.  A face that names an outside vertex is dropped.  Every other face has each index replaced by its cluster; a face for which
// mesh_face_degenerate holds afterwards is dropped.  Of the faces that remain, two are duplicates when their triples are equal after
// each is rotated (not reflected) so that its smallest cluster comes first (simplify_rotated); reflected triples are different faces
// and both stay.  Of a set of duplicates the face with the smallest input index survives.  Surviving faces keep the input order and
// their own corner order.  A cluster survives when a surviving face names it; surviving clusters are numbered in key order and the
// faces renumbered.
//
// Colour (both placements).  C10's rule over the members: (sum + m / 2) / m per channel in unsigned 64-bit (simplify_colour).
// Normals.  The result has none, whatever the input had.
//
// Placement MEAN.  C10's position rule over the members: a binary32 sum per component in member order from the first member's value,
// divided by (float)m.
//
// Placement QUADRIC.  All in binary64; every product and every sum is one IEEE operation in the order written.
//   1. Centre of the cluster's cell (ix, iy, iz signed; simplify_cell, simplify_centre): c_a = (double)origin_a + ((double)i_a + 0.5) *
//      (double)cell.
//   2. Mean: mu_a = (the sum over the members of ((double)P_a - c_a), from +0.0) / (double)m.
//   3. Sums (simplify_add) over the corners (f, k) of the input faces whose three vertices are all inside the grid, whether or not
//      the face survives; a corner counts when index[3 f + k] is a member of the cluster; corners in ascending 3 f + k.  A face with
//      two corners in the cluster therefore adds twice.  The term of a corner: g = mesh_face_normal(A, B, C) of face f (contract C22,
//      area-weighted); a_a = (double)A_a - c_a with A the face's first corner; d = -((g0 * a0 + g1 * a1) + g2 * a2); g_i * g_j is added
//      to S_ij for the six i <= j and g_a * d to t_a, each from +0.0.
//   4. Residual at the mean: q_a = (S_a0 * mu0 + S_a1 * mu1) + S_a2 * mu2, r_a = (-t_a) - q_a.
//   5. Eigen-solve: normal_jacobi of contract C14 (apd_normal_math.h) on S with V = I: the same settle rule, sweep order and
//      kNormalSweepCap.  The diagonal entries are lambda_k, unclamped; column k of V is e_k; lmax = lambda_0, replaced by lambda_1 when
//      lambda_1 > lmax, then by lambda_2 when lambda_2 > lmax.
//   6. Truncated pseudo-inverse step from the mean: x = mu; for k = 0, 1, 2 in that order, where lambda_k > 0.0 and lambda_k >
//      kSimplifyRankCut * lmax: p = ((e_0k * r0 + e_1k * r1) + e_2k * r2) / lambda_k, then x_a = x_a + e_ak * p.  The vertex moves only
//      along the directions the faces constrain: a flat neighbourhood gets its mean projected on the plane, a crease its mean
//      projected on the line, a corner the intersection point.
//   7. x is accepted when every x_a is finite and |x_a| <= (double)cell -- at most half a cell outside its own cell.  Otherwise, or
//      when one of the nine sums is not finite or lmax is not > 0.0, x = mu.
//   8. Position: (float)(c_a + x_a).
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_mesh_math.h"
#include "apd_normal_math.h"
#include "apd_voxel_math.h"

namespace apd_fusion {

constexpr double kSimplifyRankCut = 1e-3;  // Lindstrom's: an eigenvalue at or below this share of the largest constrains nothing

// (a, b, c) rotated so that its smallest entry comes first; a face that is not degenerate has one smallest
APD_HD void simplify_rotated(int32_t a, int32_t b, int32_t c, int32_t r[3])
{
    if (a < b && a < c) {
        r[0] = a, r[1] = b, r[2] = c;
    } else if (b < c) {
        r[0] = b, r[1] = c, r[2] = a;
    } else {
        r[0] = c, r[1] = a, r[2] = b;
    }
}

// The signed cell of a key of voxel_key
APD_HD void simplify_cell(uint64_t key, int cell[3])
{
    for (int a = 0; a < 3; ++a) {
        cell[a] = (int)((key >> (a * kVoxelAxisBits)) & (((uint64_t)1 << kVoxelAxisBits) - 1)) - kVoxelHalf;
    }
}

APD_HD double simplify_centre(float origin, int i, float cell)
{
    const double steps = (double)i + 0.5;
    const double along = steps * (double)cell;
    return (double)origin + along;
}

APD_HD uint8_t simplify_colour(uint64_t sum, uint64_t m) { return (uint8_t)((sum + m / 2) / m); }

// The nine sums of a cluster
struct SimplifySums {
    double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
};

// One corner's term: the face (A, B, C) seen from the centre c
APD_HD_FLAT void simplify_add(SimplifySums &m, const float A[3], const float B[3], const float C[3], double c0, double c1, double c2)
{
    double g[3];
    mesh_face_normal(A, B, C, g);
    const double a0 = (double)A[0] - c0, a1 = (double)A[1] - c1, a2 = (double)A[2] - c2;
    const double p0 = g[0] * a0, p1 = g[1] * a1, p2 = g[2] * a2;
    const double p01 = p0 + p1;
    const double d = -(p01 + p2);
    const double g00 = g[0] * g[0], g01 = g[0] * g[1], g02 = g[0] * g[2], g11 = g[1] * g[1], g12 = g[1] * g[2], g22 = g[2] * g[2];
    const double gd0 = g[0] * d, gd1 = g[1] * d, gd2 = g[2] * d;
    m.s00 = m.s00 + g00;
    m.s01 = m.s01 + g01;
    m.s02 = m.s02 + g02;
    m.s11 = m.s11 + g11;
    m.s12 = m.s12 + g12;
    m.s22 = m.s22 + g22;
    m.t0 = m.t0 + gd0;
    m.t1 = m.t1 + gd1;
    m.t2 = m.t2 + gd2;
}

APD_HD bool simplify_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // a NaN fails the test

APD_HD double simplify_row(double a, double b, double c, double x, double y, double z)
{
    const double ax = a * x, by = b * y, cz = c * z;
    const double two = ax + by;
    return two + cz;
}

// Steps 4 to 7: the offset x from the centre, given the sums and the mean offset mu
APD_HD_FLAT void simplify_place(const SimplifySums &m, double mu0, double mu1, double mu2, float cell, double &x0, double &x1, double &x2)
{
    x0 = mu0, x1 = mu1, x2 = mu2;
    if (!(simplify_finite(m.s00) && simplify_finite(m.s01) && simplify_finite(m.s02) && simplify_finite(m.s11) && simplify_finite(m.s12) &&
          simplify_finite(m.s22) && simplify_finite(m.t0) && simplify_finite(m.t1) && simplify_finite(m.t2))) {
        return;
    }
    const double r0 = (-m.t0) - simplify_row(m.s00, m.s01, m.s02, mu0, mu1, mu2);
    const double r1 = (-m.t1) - simplify_row(m.s01, m.s11, m.s12, mu0, mu1, mu2);
    const double r2 = (-m.t2) - simplify_row(m.s02, m.s12, m.s22, mu0, mu1, mu2);
    double a00 = m.s00, a01 = m.s01, a02 = m.s02, a11 = m.s11, a12 = m.s12, a22 = m.s22;
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    unsigned sweeps;
    bool capped;
    normal_jacobi(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22, sweeps, capped);
    double lmax = a00;
    lmax = a11 > lmax ? a11 : lmax;
    lmax = a22 > lmax ? a22 : lmax;
    if (!(lmax > 0.0)) {
        return;
    }
    const double cut = kSimplifyRankCut * lmax;
    double y0 = mu0, y1 = mu1, y2 = mu2;
    if (a00 > 0.0 && a00 > cut) {
        const double p = simplify_row(v00, v10, v20, r0, r1, r2) / a00;
        const double s0 = v00 * p, s1 = v10 * p, s2 = v20 * p;
        y0 = y0 + s0, y1 = y1 + s1, y2 = y2 + s2;
    }
    if (a11 > 0.0 && a11 > cut) {
        const double p = simplify_row(v01, v11, v21, r0, r1, r2) / a11;
        const double s0 = v01 * p, s1 = v11 * p, s2 = v21 * p;
        y0 = y0 + s0, y1 = y1 + s1, y2 = y2 + s2;
    }
    if (a22 > 0.0 && a22 > cut) {
        const double p = simplify_row(v02, v12, v22, r0, r1, r2) / a22;
        const double s0 = v02 * p, s1 = v12 * p, s2 = v22 * p;
        y0 = y0 + s0, y1 = y1 + s1, y2 = y2 + s2;
    }
    const double bound = (double)cell;
    if (fabs(y0) <= bound && fabs(y1) <= bound && fabs(y2) <= bound) {  // a NaN or an infinity fails: cell is finite
        x0 = y0, x1 = y1, x2 = y2;
    }
}

}  // namespace apd_fusion
