// apd_normal_math.h -- a point's normal and surface variation from the second moments of its neighbourhood (arithmetic contract
// C14): the relation under apd_points_estimate_normals and apd_points_with_estimated_normals, written once and compiled
// by hipcc into the kernel (apd_points_normals.hip) and by the host compiler into whoever restates it.  As in apd_knn_math.h:
// -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order; binary32 where the positions are subtracted,
// binary64 from there on; the binary64 division and sqrt correctly rounded.
//
// Neighbours.  Those of contract C11 (apd_radius_math.h), unchanged, on the grid of cell size `radius` at `origin`: other indices,
// both points inside the grid, adjacent cells, radius_d2 <= r2.
//
// Sums.  Point i at P with c neighbours -- the point itself is not counted in c -- has an estimate when c >= min_neighbours,
// min_neighbours in kNormalMinNeighbours .. kNormalMaxNeighbours (below 2 there is no plane; a cloud has fewer than 2^31 points).  The
// sums then run over the point itself and its neighbours in ascending (cell key, input index), the order in which the 9-row walk
// meets them and the stable sort gives them.  A term at Q is d = Q - P, three binary32 subtractions (the exact negations of the
// components radius_d2 forms; the point's own term is +0, +0, +0), each converted to binary64.  In binary64, sequentially from
// 0.0 (normal_add): n (one per term), s[a] the sums of d_a, and xx, xy, xz, yy, yz, zz the sums of the products d_a * d_b, a
// product rounded before it is added.
// Covariance (normal_solve): m_a = s[a] / n;  C_ab = q - r with q = S_ab / n and r = m_a * m_b, for the six a <= b.
//
// Eigen-solve (normal_jacobi, which contract C23 calls on its own matrix).  Cyclic Jacobi on the symmetric 3 x 3 matrix A = C with
// V = I, in binary64, with + - * / and sqrt alone.  An
// off-diagonal A_pq is SETTLED when g = |A_pq| changes neither diagonal: |A_pp| + g == |A_pp| and |A_qq| + g == |A_qq| (zero
// is settled).  Before every sweep: if all three are settled, stop; if kNormalSweepCap sweeps are done, stop (`capped`, which
// no point of the tests' clouds reaches: DESIGN.md section 4).  A sweep visits (0,1), (0,2), (1,2) in that order; a settled entry
// is set to 0.0 and left, any other is rotated away (normal_rotate):
//   h = A_qq - A_pp, theta = h / (2.0 * A_pq), t = +-1.0 / (|theta| + sqrt(theta * theta + 1.0)) with the sign of theta (+ for
//   theta == 0), c = 1.0 / sqrt(t * t + 1.0), s = t * c, u = t * A_pq;
//   A_pp -= u, A_qq += u, A_pq = 0.0; for the third index r: (A_rp, A_rq) = (c * A_rp - s * A_rq, s * A_rp + c * A_rq); and the
//   same for (V_kp, V_kq), k = 0, 1, 2.
// A theta whose square overflows gives t = 0 and changes nothing but A_pq.
//
// Result.  The diagonal, each entry clamped below at 0.0 (`!(x > 0.0)` gives 0.0), sorted: l0 <= l1 <= l2.  The normal is the
// column of V that belongs to the smallest clamped entry, the lowest column among equals.  It IS renormalised: len =
// sqrt((x * x + y * y) + z * z), and each component divided by len when len > 0.0 (V is orthogonal up to rounding, so len is 1
// within a few units in the last place).  Sign: dot = (x * (double)N_x + y * (double)N_y) + z * (double)N_z with N the point's
// stored normal; dot < 0 flips the vector; when dot is neither < 0 nor > 0 (a zero, NaN or orthogonal N) the vector is flipped
// when its first non-zero component is negative.  The three components are converted to binary32 last.
// Variation.  sum = (l0 + l1) + l2;  (float)(l0 / sum), and 0.0f when sum is not > 0.0 (coincident points).
//
// No estimate.  c < min_neighbours, or a point outside the grid: the normal is the stored normal, copied bit for bit, and the
// variation +inf (normal_none).  A result with an estimate is never NaN: the terms are finite (|d_a| <= radius).
#pragma once

#include <math.h>
#include <stddef.h>

#include "apd_radius_math.h"

// The rotation and the solve take their matrix by reference: inlined always, so that on the device it stays in registers
#define APD_HD_FLAT APD_HD __attribute__((always_inline))

namespace apd_fusion {

constexpr unsigned kNormalMinNeighbours = 2;            // the smallest min_neighbours
constexpr unsigned kNormalMaxNeighbours = 0x7fffffffu;  // the largest: a cloud has fewer than 2^31 points
constexpr unsigned kNormalSweepCap = 5;                 // Jacobi sweeps at most

APD_HD float normal_none() { return INFINITY; }

// The ten sums of a point
struct NormalSums {
    double n = 0.0, s[3] = {0.0, 0.0, 0.0};
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
};

// One term: the point at Q seen from P
APD_HD_FLAT void normal_add(NormalSums &m, const float P[3], const float Q[3])
{
    const float fx = Q[0] - P[0], fy = Q[1] - P[1], fz = Q[2] - P[2];
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double xx = x * x, xy = x * y, xz = x * z, yy = y * y, yz = y * z, zz = z * z;
    m.n = m.n + 1.0;
    m.s[0] = m.s[0] + x;
    m.s[1] = m.s[1] + y;
    m.s[2] = m.s[2] + z;
    m.xx = m.xx + xx;
    m.xy = m.xy + xy;
    m.xz = m.xz + xz;
    m.yy = m.yy + yy;
    m.yz = m.yz + yz;
    m.zz = m.zz + zz;
}

APD_HD double normal_covariance(double sab, double ma, double mb, double n)
{
    const double q = sab / n;
    const double r = ma * mb;
    return q - r;
}

APD_HD bool normal_settled(double apq, double app, double aqq)
{
    const double g = fabs(apq), p = fabs(app), q = fabs(aqq);
    return p + g == p && q + g == q;
}

// The rotation that takes A_pq to 0; (arp, arq): the third row's entries in columns p and q; (vkp, vkq): V's columns p and q
APD_HD_FLAT void normal_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p, double &v1q,
                          double &v2p, double &v2q)
{
    const double h = aqq - app;
    const double twice = 2.0 * apq;
    const double theta = h / twice;
    const double square = theta * theta;
    const double root = sqrt(square + 1.0);
    const double below = fabs(theta) + root;
    const double size = 1.0 / below;
    const double t = theta < 0.0 ? -size : size;
    const double tt = t * t;
    const double c = 1.0 / sqrt(tt + 1.0);
    const double s = t * c;
    const double u = t * apq;
    app = app - u;
    aqq = aqq + u;
    apq = 0.0;
    const double rp = arp, rq = arq;
    const double rp_c = c * rp, rq_s = s * rq, rp_s = s * rp, rq_c = c * rq;
    arp = rp_c - rq_s;
    arq = rp_s + rq_c;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    const double a0c = c * a0, b0s = s * b0, a0s = s * a0, b0c = c * b0;
    v0p = a0c - b0s;
    v0q = a0s + b0c;
    const double a1c = c * a1, b1s = s * b1, a1s = s * a1, b1c = c * b1;
    v1p = a1c - b1s;
    v1q = a1s + b1c;
    const double a2c = c * a2, b2s = s * b2, a2s = s * a2, b2c = c * b2;
    v2p = a2c - b2s;
    v2q = a2s + b2c;
}

APD_HD double normal_clamped(double x) { return x > 0.0 ? x : 0.0; }

// The cyclic Jacobi of the contract on the symmetric matrix A (its six entries a_pq, p <= q) with V = I: on return the diagonal of A
// holds the eigenvalues, unclamped and unsorted, and column k of V (v0k, v1k, v2k) the vector of a_kk.  The one loop of normal_solve
// and of simplify_place (apd_simplify_math.h, contract C23).  sweeps: the sweeps taken; capped: stopped by the cap
APD_HD_FLAT void normal_jacobi(double &a00, double &a01, double &a02, double &a11, double &a12, double &a22, double &v00, double &v01, double &v02,
                               double &v10, double &v11, double &v12, double &v20, double &v21, double &v22, unsigned &sweeps, bool &capped)
{
    v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    sweeps = 0;
    capped = false;
    for (;;) {
        if (normal_settled(a01, a00, a11) && normal_settled(a02, a00, a22) && normal_settled(a12, a11, a22)) {
            break;
        }
        if (sweeps == kNormalSweepCap) {
            capped = true;
            break;
        }
        if (normal_settled(a01, a00, a11)) {
            a01 = 0.0;
        } else {
            normal_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        }
        if (normal_settled(a02, a00, a22)) {
            a02 = 0.0;
        } else {
            normal_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        }
        if (normal_settled(a12, a11, a22)) {
            a12 = 0.0;
        } else {
            normal_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        ++sweeps;
    }
}

// The estimate of a point with the sums m (m.n >= 1) and the stored normal N.  sweeps: the sweeps taken; capped: stopped by the cap
APD_HD_FLAT void normal_solve(const NormalSums &m, const float N[3], float normal[3], float &variation, unsigned &sweeps, bool &capped)
{
    const double mx = m.s[0] / m.n, my = m.s[1] / m.n, mz = m.s[2] / m.n;
    double a00 = normal_covariance(m.xx, mx, mx, m.n), a01 = normal_covariance(m.xy, mx, my, m.n), a02 = normal_covariance(m.xz, mx, mz, m.n);
    double a11 = normal_covariance(m.yy, my, my, m.n), a12 = normal_covariance(m.yz, my, mz, m.n), a22 = normal_covariance(m.zz, mz, mz, m.n);
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    normal_jacobi(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22, sweeps, capped);
    const double e0 = normal_clamped(a00), e1 = normal_clamped(a11), e2 = normal_clamped(a22);
    // the column of the smallest, the lowest among equals
    const bool second = e1 < e0;
    const double first_two = second ? e1 : e0;
    const bool third = e2 < first_two;
    double x = third ? v02 : (second ? v01 : v00);
    double y = third ? v12 : (second ? v11 : v10);
    double z = third ? v22 : (second ? v21 : v20);
    // l0 <= l1 <= l2: none of the three is NaN
    const double other_two = second ? e0 : e1;                 // max(e0, e1)
    const double l0 = third ? e2 : first_two;                  // min of the three
    const double l2 = e2 > other_two ? e2 : other_two;         // max of the three
    const double below_top = e2 < other_two ? e2 : other_two;  // min(max(e0, e1), e2)
    const double l1 = below_top > first_two ? below_top : first_two;
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = xx + yy;
    const double len = sqrt(xy + zz);
    if (len > 0.0) {
        x = x / len;
        y = y / len;
        z = z / len;
    }
    const double px = x * (double)N[0], py = y * (double)N[1], pz = z * (double)N[2];
    const double pxy = px + py;
    const double dot = pxy + pz;
    bool flip = false;
    if (dot < 0.0) {
        flip = true;
    } else if (!(dot > 0.0)) {
        flip = x != 0.0 ? x < 0.0 : (y != 0.0 ? y < 0.0 : z < 0.0);
    }
    normal[0] = (float)(flip ? -x : x);
    normal[1] = (float)(flip ? -y : y);
    normal[2] = (float)(flip ? -z : z);
    const double low = l0 + l1;
    const double sum = low + l2;
    variation = sum > 0.0 ? (float)(l0 / sum) : 0.0f;
}

}  // namespace apd_fusion
