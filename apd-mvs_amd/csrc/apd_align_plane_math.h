// apd_align_plane_math.h -- rigid alignment of one cloud to another by point-to-plane ICP onto the other cloud's stored normals
// (arithmetic contract C20): the relation under apd_points_align_planes, written once and compiled by hipcc into the
// kernel (apd_points_align_planes.hip) and by the host compiler into whoever restates it.  As in apd_align_math.h:
// -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order; binary64 from the point where a float is
// read, with + - * / and sqrt alone (both correctly rounded): no sin, cos or atan anywhere.
//
// A STEP k = 0, 1, .. works on the positions X_k of P; X_0 is P's own positions, X_k for k > 0 is X_0 moved by the total, exactly
// as in contract C18 (apd_align_math.h).
//
// 1. Correspondences.  Contract C17 (apd_nearest_math.h) as it stands, as C18 uses it.
//
// 2. Pass 1.  That of C18 unchanged (align_terms1, kAlignSums1 = 8 sums, THE TREE over chunks of 256, chunk sums added ascending):
//    m = [0], the means pm and qm, the point rms prms_k = sqrt([7] / m), 0.0 when m is 0.
//
// 3. Pass 2, the normal equations (align_plane_terms).  The centre is c = qm.  A matched point is USABLE when its match's stored
//    normal n, three floats converted to double, gives s = (nx * nx + ny * ny) + nz * nz with s > 0.0 and s < +inf (false for a
//    NaN); then len = sqrt(s) and u = (nx / len, ny / len, nz / len).  The sign of n plays no part: every sum below is even in u.
//    For a usable point, p its position in X_k and q its match's in Q, each float converted to double:
//      x = p - c;  y = q - c;  a0 = x1 * u2 - x2 * u1;  a1 = x2 * u0 - x0 * u2;  a2 = x0 * u1 - x1 * u0;
//      g = (a0, a1, a2, u0, u1, u2);  e = x - y;  r = (e0 * u0 + e1 * u1) + e2 * u2.
//    kAlignPlaneSums = 30 sums through C18's tree over 256-slot chunks; a slot holds +0.0 when the point is unmatched, unusable or
//    past the end; chunk sums are added ascending from 0.0:
//      [0 .. 20]  g_i * g_j for i <= j, row-major upper triangle (index align_plane_at(i, j)): the matrix A;
//      [21 .. 26] g_i * r: the vector b;   [27] r * r;   [28] 1.0: m_plane, exact;   [29] (x0 * x0 + x1 * x1) + x2 * x2: S_xx.
//    The plane rms is sqrt([27] / [28]), 0.0 when m_plane is 0 (align_rms).
//
// 4. Solve (align_plane_solve; host arithmetic, the device never computes it).  Minimise sum (r + g . z)^2 over z = (omega, tau):
//    A z = -b, by LDL^T without pivoting.  For the columns j = 0 .. 5 in turn:
//      w_k = L_jk * d_k for k < j;
//      d_j = (..((A_jj - L_j0 * w_0) - L_j1 * w_1) .. - L_j,j-1 * w_j-1): every product rounded, subtracted for ascending k;
//      the geometry is DEGENERATE when !(d_j > kAlignPlanePivot * bound_j), bound_j = S_xx for j < 3 and m_plane for j >= 3, and
//      the factorisation ends there (the later d are reported as 0.0);
//      L_ij = ((..((A_ij - L_i0 * w_0) - L_i1 * w_1) .. - L_i,j-1 * w_j-1)) / d_j for i = j + 1 .. 5.
//    Forward, i = 0 .. 5: f_i = (..((-b_i - L_i0 * f_0) - L_i1 * f_1) .. - L_i,i-1 * f_i-1), ascending k.  Then h_i = f_i / d_i.
//    Back, i = 5 .. 0: z_i = (..((h_i - L_5i * z_5) - L_4i * z_4) .. - L_i+1,i * z_i+1), descending k.
//    Why these bounds: |a|^2 <= |x|^2 |u|^2 = |x|^2, so A_jj <= S_xx for j < 3; |u|^2 = 1, so A_jj <= m_plane for j >= 3; and a
//    pivot d_j is what column j adds to the constraint after the columns before it.  kAlignPlanePivot = 2^-20 is then the share of
//    the largest possible constraint that a direction must reach: binary32 coordinates carry about 2^-24 of relative noise, so a
//    constraint a million times weaker than the strongest possible one is sampling noise and not shape.
//    The rotation, without trigonometry: the quaternion (w, x, y, z) = (1.0, omega_0 / 2.0, omega_1 / 2.0, omega_2 / 2.0),
//    len = sqrt(((w * w + x * x) + y * y) + z * z), each divided by len (len >= 1), then the nine expressions of C18 step 4
//    (align_rotation_of): a proper rotation by construction, of angle 2 atan(|omega| / 2).  The translation
//    t_a = (c_a + tau_a) - align_row_dot(R, a, c): the rotation is about c.  The scale is 1.0: there is no similarity variant.
//
// 5. Compose and move.  align_compose, align_move_of and align_moved of C18, unchanged; positions are moved from X_0.
//
// 6. Stopping (align_plane_run).  For k = 0, 1, ..: search and pass 1 on X_k; (m, prms_k) are matched_after and rms_after, and
//    for k = 0 also the _before ones; steps = k.  Pass 2 runs on X_k whenever m >= 1 (it needs the centre), also where the
//    iteration ends before it would be used -- at k == iterations and at m < 3 -- so that planes_after and plane_rms_after always
//    describe the returned positions; with m == 0 they are 0 and 0.0.  For k = 0 they are also the _before ones.  That extra
//    pass 2 is for the figures alone: the step count and the transform do not depend on it.  Then, in this order:
//      k == iterations (1 .. kAlignMaxIterations = 64): stopped = kAlignIterations;
//      m < 3: kAlignTooFew;  m_plane < 6: kAlignTooFew;
//      k > 0 and |prms_k - prms_{k-1}| <= tolerance * prms_{k-1}: kAlignConverged;
//      the solve; degenerate, or a component of z that is not finite: kAlignDegenerate;
//    otherwise the step joins the total and k + 1 follows.  What is returned is the total of the `steps` steps taken -- the
//    identity when that is none.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "apd_align_math.h"

namespace apd_fusion {

constexpr int kAlignPlaneSums = 30;
constexpr int kAlignPlaneB = 21, kAlignPlaneRr = 27, kAlignPlaneCount = 28, kAlignPlaneSxx = 29;  // where b, r r, m_plane and S_xx stand
constexpr double kAlignPlanePivot = 1.0 / 1048576.0;  // 2^-20
constexpr double kAlignPlaneMinimum = 6.0;            // usable matches a step needs
enum : int { kAlignDegenerate = 3 };                  // APD_ALIGN_DEGENERATE of include/apd_mi355x.h

// The fields of apd_points_plane_alignment_t (include/apd_mi355x.h), in its layout
struct PlaneAlignment {
    Alignment points;
    long long planes_before, planes_after;
    double plane_rms_before, plane_rms_after;
};

// Where g_i * g_j, i <= j, stands among the sums
constexpr int align_plane_at(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }
static_assert(align_plane_at(0, 0) == 0 && align_plane_at(1, 1) == 6 && align_plane_at(5, 5) == 20, "row-major upper triangle");

// The terms of a matched point at P with its match at Q, whose stored normal is N, about the centre c.  false: not usable, and v
// is left as it is
APD_HD bool align_plane_terms(const float P[3], const float Q[3], const float N[3], const double c[3], double v[kAlignPlaneSums])
{
    const double nx = (double)N[0], ny = (double)N[1], nz = (double)N[2];
    const double nxx = nx * nx, nyy = ny * ny, nzz = nz * nz;
    const double nxy = nxx + nyy;
    const double s = nxy + nzz;
    if (!(s > 0.0 && s < (double)INFINITY)) {  // false for a NaN
        return false;
    }
    const double len = sqrt(s);
    const double u0 = nx / len, u1 = ny / len, u2 = nz / len;
    const double x0 = (double)P[0] - c[0], x1 = (double)P[1] - c[1], x2 = (double)P[2] - c[2];
    const double y0 = (double)Q[0] - c[0], y1 = (double)Q[1] - c[1], y2 = (double)Q[2] - c[2];
    const double x1u2 = x1 * u2, x2u1 = x2 * u1, x2u0 = x2 * u0, x0u2 = x0 * u2, x0u1 = x0 * u1, x1u0 = x1 * u0;
    const double g0 = x1u2 - x2u1, g1 = x2u0 - x0u2, g2 = x0u1 - x1u0;
    const double e0 = x0 - y0, e1 = x1 - y1, e2 = x2 - y2;
    const double r0 = e0 * u0, r1 = e1 * u1, r2 = e2 * u2;
    const double r01 = r0 + r1;
    const double r = r01 + r2;
    v[0] = g0 * g0;
    v[1] = g0 * g1;
    v[2] = g0 * g2;
    v[3] = g0 * u0;
    v[4] = g0 * u1;
    v[5] = g0 * u2;
    v[6] = g1 * g1;
    v[7] = g1 * g2;
    v[8] = g1 * u0;
    v[9] = g1 * u1;
    v[10] = g1 * u2;
    v[11] = g2 * g2;
    v[12] = g2 * u0;
    v[13] = g2 * u1;
    v[14] = g2 * u2;
    v[15] = u0 * u0;
    v[16] = u0 * u1;
    v[17] = u0 * u2;
    v[18] = u1 * u1;
    v[19] = u1 * u2;
    v[20] = u2 * u2;
    v[21] = g0 * r;
    v[22] = g1 * r;
    v[23] = g2 * r;
    v[24] = u0 * r;
    v[25] = u1 * r;
    v[26] = u2 * r;
    v[27] = r * r;
    v[28] = 1.0;
    const double xx = x0 * x0, yy = x1 * x1, zz = x2 * x2;
    const double xy = xx + yy;
    v[29] = xy + zz;
    return true;
}

// One step's solve.  degenerate: z is zeros and the step the identity; d: the pivots found, 0.0 from the failing column's successor on
struct AlignPlaneSolve {
    bool degenerate = false;
    double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    AlignTransform step;
};

// From the centre c and the thirty sums of pass 2
inline AlignPlaneSolve align_plane_solve(const double c[3], const double S[kAlignPlaneSums])
{
    AlignPlaneSolve out;
    double L[6][6] = {}, w[6];
    for (int j = 0; j < 6; ++j) {
        for (int k = 0; k < j; ++k) {
            w[k] = L[j][k] * out.d[k];
        }
        double pivot = S[align_plane_at(j, j)];
        for (int k = 0; k < j; ++k) {
            const double product = L[j][k] * w[k];
            pivot = pivot - product;
        }
        out.d[j] = pivot;
        const double least = kAlignPlanePivot * (j < 3 ? S[kAlignPlaneSxx] : S[kAlignPlaneCount]);
        if (!(pivot > least)) {
            out.degenerate = true;
            return out;
        }
        for (int i = j + 1; i < 6; ++i) {
            double entry = S[align_plane_at(j, i)];
            for (int k = 0; k < j; ++k) {
                const double product = L[i][k] * w[k];
                entry = entry - product;
            }
            L[i][j] = entry / pivot;
        }
    }
    double f[6];
    for (int i = 0; i < 6; ++i) {
        double left = -S[kAlignPlaneB + i];
        for (int k = 0; k < i; ++k) {
            const double product = L[i][k] * f[k];
            left = left - product;
        }
        f[i] = left;
    }
    for (int i = 5; i >= 0; --i) {
        double left = f[i] / out.d[i];
        for (int k = 5; k > i; --k) {
            const double product = L[k][i] * out.z[k];
            left = left - product;
        }
        out.z[i] = left;
    }
    for (int i = 0; i < 6; ++i) {
        if (!isfinite(out.z[i])) {
            out.degenerate = true;
            return out;
        }
    }
    double q0 = 1.0, q1 = out.z[0] / 2.0, q2 = out.z[1] / 2.0, q3 = out.z[2] / 2.0;
    align_unit_quaternion(q0, q1, q2, q3);
    align_rotation_of(q0, q1, q2, q3, out.step.R);
    for (int a = 0; a < 3; ++a) {
        const double to = c[a] + out.z[3 + a];
        out.step.t[a] = to - align_row_dot(out.step.R, a, c[0], c[1], c[2]);
    }
    return out;
}

inline PlaneAlignment align_plane_identity()
{
    PlaneAlignment a = {};
    a.points = align_identity();
    return a;
}

// The iteration.  pass1(k, total, sums[8]) as align_run's; pass2(centre, sums[30]): the totals of pass 2 on the same positions
// and matches.  Either returns 0 or what align_plane_run then returns at once
template <typename Pass1, typename Pass2>
inline int align_plane_run(unsigned iterations, double tolerance, Pass1 &&pass1, Pass2 &&pass2, PlaneAlignment &out)
{
    AlignTransform total;
    out = align_plane_identity();
    Alignment &points = out.points;
    double previous = 0.0;
    for (unsigned k = 0;; ++k) {
        double s1[kAlignSums1];
        if (const int rc = pass1(k, total, s1); rc != 0) {
            return rc;
        }
        const double m = s1[0];
        const double rms = align_rms(s1[7], m);
        double s2[kAlignPlaneSums] = {};
        const double centre[3] = {m > 0.0 ? s1[4] / m : 0.0, m > 0.0 ? s1[5] / m : 0.0, m > 0.0 ? s1[6] / m : 0.0};
        if (m > 0.0) {
            if (const int rc = pass2(centre, s2); rc != 0) {
                return rc;
            }
        }
        const double usable = s2[kAlignPlaneCount];
        const double plane_rms = align_rms(s2[kAlignPlaneRr], usable);
        if (k == 0) {
            points.matched_before = (long long)m;
            points.rms_before = rms;
            out.planes_before = (long long)usable;
            out.plane_rms_before = plane_rms;
        }
        points.matched_after = (long long)m;
        points.rms_after = rms;
        out.planes_after = (long long)usable;
        out.plane_rms_after = plane_rms;
        points.steps = (int)k;
        if (k == iterations) {
            points.stopped = kAlignIterations;
            break;
        }
        points.stopped = kAlignTooFew;
        if (m < 3.0 || usable < kAlignPlaneMinimum) {
            break;
        }
        if (k > 0 && fabs(rms - previous) <= tolerance * previous) {
            points.stopped = kAlignConverged;
            break;
        }
        const AlignPlaneSolve solved = align_plane_solve(centre, s2);
        if (solved.degenerate) {
            points.stopped = kAlignDegenerate;
            break;
        }
        total = align_compose(solved.step, total);
        previous = rms;
    }
    points.scale = total.scale;
    for (int e = 0; e < 9; ++e) {
        points.rotation[e] = total.R[e];
    }
    for (int a = 0; a < 3; ++a) {
        points.translation[a] = total.t[a];
    }
    return 0;
}

}  // namespace apd_fusion
