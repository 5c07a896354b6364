// apd_align_math.h -- rigid or similarity alignment of one cloud to another by point-to-point ICP, and the move of a cloud by a
// similarity transform (arithmetic contract C18): the relation under apd_points_align and apd_points_transformed,
// written once and compiled by hipcc into the kernels (apd_points_align.hip) and by the host compiler into whoever restates it.
// As in apd_nearest_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order; binary64 from the
// point where a coordinate is read, with + - * / and sqrt alone (both correctly rounded): no sin, cos or atan anywhere.
//
// A STEP k = 0, 1, .. works on the positions X_k of P; X_0 is P's own positions, X_k for k > 0 is X_0 moved by the total (below).
//
// 1. Correspondences.  Contract C17 (apd_nearest_math.h) as it stands, for X_k in Q on the grid (radius, origin): point i is
//    MATCHED to the index that search gives it, among equally near ones the smallest; a point without a candidate is unmatched.
//    P and Q may be the same cloud: nothing is special about it.
//
// 2. Pass 1, means.  Per chunk of kKnnChunk = 256 consecutive input indices of P, kAlignSums1 = 8 binary64 sums over the chunk's
//    matched points (align_terms1), p the point's position in X_k and q its match's in Q, each float coordinate converted to double:
//      [0] 1.0;  [1..3] p;  [4..6] q;  [7] ((dx * dx + dy * dy) + dz * dz) with d = p - q in binary64.
//    THE TREE (align_tree): slot s of the chunk's 256 holds the point's term, or +0.0 if the point is unmatched or past the end.
//    Inside each group of 64 consecutive slots, for d = 32, 16, 8, 4, 2, 1: v[s] = v[s] + v[s + d] for s < d.  With g0 .. g3 the
//    first slot of each group, the chunk sum is (g0 + g1) + (g2 + g3).  The chunk sums are added in ascending order from 0.0.
//    m = [0] (exact), the means pm_a = [1 + a] / m and qm_a = [4 + a] / m, rms_k = sqrt([7] / m), 0.0 when m is 0 (align_rms).
//
// 3. Pass 2, moments.  The same tree and order for kAlignSums2 = 10 sums over the matched points (align_terms2): with
//    u = p - pm and w = q - qm in binary64, [3 * a + b] = u_a * w_b for a, b = 0 .. 2 -- the entries of sum u w^T, row-major --
//    and [9] = ((u_0 * u_0 + u_1 * u_1) + u_2 * u_2).
//
// 4. Solve (align_solve; host arithmetic, the device never computes it).  With S_ab = [3 * a + b], Horn's symmetric matrix
//      N = | (S00 + S11) + S22   S12 - S21            S20 - S02            S01 - S10          |
//          |                     (S00 - S11) - S22    S01 + S10            S20 + S02          |
//          |                                          (S11 - S00) - S22    S12 + S21          |
//          |                                                               (S22 - S00) - S11  |
//    is diagonalised by cyclic Jacobi with V = I: the settled test and the rotation of contract C14 (apd_normal_math.h: h, theta,
//    t, c, s, u; A_pp -= u, A_qq += u, A_pq = 0; (A_rp, A_rq) = (c * A_rp - s * A_rq, s * A_rp + c * A_rq) for BOTH other indices
//    r in ascending order; the same for (V_kp, V_kq), k = 0 .. 3), the pairs of a sweep in the order (0,1) (0,2) (0,3) (1,2) (1,3)
//    (2,3); before every sweep: stop if all six are settled, stop if kAlignSweepCap = 16 sweeps are done.  The quaternion
//    (w, x, y, z) is the column of V under the largest diagonal entry, the lowest column among equals; all four negated when
//    w < 0.0; len = sqrt(((w * w + x * x) + y * y) + z * z) and each divided by len when len > 0.0.  Then, every product rounded:
//      R00 = (ww + xx) - (yy + zz)   R01 = 2.0 * (xy - wz)         R02 = 2.0 * (xz + wy)
//      R10 = 2.0 * (xy + wz)         R11 = (ww - xx) + (yy - zz)   R12 = 2.0 * (yz - wx)
//      R20 = 2.0 * (xz - wy)         R21 = 2.0 * (yz + wx)         R22 = (ww - xx) - (yy - zz)
//    a proper rotation by construction: there is no reflection case.  scale = 1.0; with_scale: with r_a = (R_a0 * S_0a + R_a1 *
//    S_1a) + R_a2 * S_2a, scale = ((r_0 + r_1) + r_2) / [9].  t_a = qm_a - scale * ((R_a0 * pm_0 + R_a1 * pm_1) + R_a2 * pm_2).
//
// 5. Compose and move.  The total (S, R, T) starts as (1.0, I, 0).  The step (s, r, t) applied AFTER it (align_compose):
//    S' = s * S;  R'_ab = (r_a0 * R_0b + r_a1 * R_1b) + r_a2 * R_2b;  T'_a = s * ((r_a0 * T_0 + r_a1 * T_1) + r_a2 * T_2) + t_a.
//    X_{k+1} comes from X_0 and the total, never from X_k: with m_ab = S * R_ab formed once on the host (align_move_of),
//    x'_a = (float)(((m_a0 * x + m_a1 * y) + m_a2 * z) + T_a), x y z converted to double (align_moved).  A normal is moved by the
//    same expression with m = R, unscaled, and T = +0.0, and is not renormalised.
//
// 6. Stopping (align_run).  For k = 0, 1, ..: search and pass 1 on X_k; (m, rms_k) are matched_after and rms_after, and for
//    k = 0 also matched_before and rms_before; steps = k.  Then, in this order:
//      k == iterations (1 .. kAlignMaxIterations = 64): stopped = kAlignIterations;
//      m < 3: kAlignTooFew;  pass 2, and [9] == 0.0: kAlignTooFew;
//      k > 0 and |rms_k - rms_{k-1}| <= tolerance * rms_{k-1}: kAlignConverged;
//      the solve, and with_scale with a scale that is not finite or not > 0.0 (every moment zero): kAlignTooFew;
//    otherwise the step joins the total and k + 1 follows.  What is returned is the total of the `steps` steps taken -- the
//    identity when that is none -- and the last search describes it: K steps take K + 1 searches.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "apd_nearest_math.h"
#include "apd_normal_math.h"

namespace apd_fusion {

constexpr unsigned kAlignMaxIterations = 64;  // the largest `iterations`
constexpr unsigned kAlignSweepCap = 16;       // Jacobi sweeps of the 4 x 4 solve at most
constexpr int kAlignSums1 = 8, kAlignSums2 = 10;
enum : int { kAlignIterations = 0, kAlignConverged = 1, kAlignTooFew = 2 };  // APD_ALIGN_* of include/apd_mi355x.h

// x' = scale * R x + t; R row-major
struct AlignTransform {
    double scale = 1.0;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double t[3] = {0.0, 0.0, 0.0};
};

// What the move reads: m = scale * R
struct AlignMove {
    double m[9], t[3];
};

// The fields of apd_points_alignment_t (include/apd_mi355x.h), in its layout
struct Alignment {
    double scale, rotation[9], translation[3];
    long long matched_before, matched_after;
    double rms_before, rms_after;
    int steps, stopped;
};

// The terms of a matched point at P with its match at Q
APD_HD void align_terms1(const float P[3], const float Q[3], double v[kAlignSums1])
{
    const double px = (double)P[0], py = (double)P[1], pz = (double)P[2];
    const double qx = (double)Q[0], qy = (double)Q[1], qz = (double)Q[2];
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    v[0] = 1.0;
    v[1] = px;
    v[2] = py;
    v[3] = pz;
    v[4] = qx;
    v[5] = qy;
    v[6] = qz;
    v[7] = xy + zz;
}

// mean: pm, then qm
APD_HD void align_terms2(const float P[3], const float Q[3], const double mean[6], double v[kAlignSums2])
{
    const double ux = (double)P[0] - mean[0], uy = (double)P[1] - mean[1], uz = (double)P[2] - mean[2];
    const double wx = (double)Q[0] - mean[3], wy = (double)Q[1] - mean[4], wz = (double)Q[2] - mean[5];
    v[0] = ux * wx;
    v[1] = ux * wy;
    v[2] = ux * wz;
    v[3] = uy * wx;
    v[4] = uy * wy;
    v[5] = uy * wz;
    v[6] = uz * wx;
    v[7] = uz * wy;
    v[8] = uz * wz;
    const double xx = ux * ux, yy = uy * uy, zz = uz * uz;
    const double xy = xx + yy;
    v[9] = xy + zz;
}

APD_HD float align_moved_component(double m0, double m1, double m2, double t, double x, double y, double z)
{
    const double a = m0 * x, b = m1 * y, c = m2 * z;
    const double ab = a + b;
    const double abc = ab + c;
    return (float)(abc + t);
}

APD_HD void align_moved(const AlignMove &by, const float X[3], float out[3])
{
    const double x = (double)X[0], y = (double)X[1], z = (double)X[2];
    out[0] = align_moved_component(by.m[0], by.m[1], by.m[2], by.t[0], x, y, z);
    out[1] = align_moved_component(by.m[3], by.m[4], by.m[5], by.t[1], x, y, z);
    out[2] = align_moved_component(by.m[6], by.m[7], by.m[8], by.t[2], x, y, z);
}

// The tree over one chunk's kKnnChunk slots of one sum; v is used up
inline double align_tree(double v[kKnnChunk])
{
    for (int g = 0; g < kKnnChunk; g += 64) {
        for (int d = 32; d >= 1; d /= 2) {
            for (int s = 0; s < d; ++s) {
                v[g + s] = v[g + s] + v[g + s + d];
            }
        }
    }
    const double low = v[0] + v[64], high = v[128] + v[192];
    return low + high;
}

inline double align_rms(double sum, double m) { return m > 0.0 ? sqrt(sum / m) : 0.0; }

// How positions move under a transform; scaled false: a normal's move
inline AlignMove align_move_of(const AlignTransform &by, bool scaled)
{
    AlignMove move;
    for (int e = 0; e < 9; ++e) {
        move.m[e] = scaled ? by.scale * by.R[e] : by.R[e];
    }
    for (int a = 0; a < 3; ++a) {
        move.t[a] = scaled ? by.t[a] : 0.0;
    }
    return move;
}

// (row a of R) . v
inline double align_row_dot(const double R[9], int a, double v0, double v1, double v2)
{
    const double x = R[3 * a] * v0, y = R[3 * a + 1] * v1, z = R[3 * a + 2] * v2;
    const double xy = x + y;
    return xy + z;
}

// The Jacobi rotation of contract C14 on the symmetric 4 x 4 matrix A (both halves kept) and V, for the pair p < q
inline void align_rotate(double A[4][4], double V[4][4], int p, int q)
{
    const double apq = A[p][q];
    const double h = A[q][q] - A[p][p];
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
    A[p][p] = A[p][p] - u;
    A[q][q] = A[q][q] + u;
    A[p][q] = 0.0;
    A[q][p] = 0.0;
    for (int r = 0; r < 4; ++r) {
        if (r == p || r == q) {
            continue;
        }
        const double rp = A[r][p], rq = A[r][q];
        const double rp_c = c * rp, rq_s = s * rq, rp_s = s * rp, rq_c = c * rq;
        A[r][p] = A[p][r] = rp_c - rq_s;
        A[r][q] = A[q][r] = rp_s + rq_c;
    }
    for (int k = 0; k < 4; ++k) {
        const double a = V[k][p], b = V[k][q];
        const double ac = c * a, bs = s * b, as = s * a, bc = c * b;
        V[k][p] = ac - bs;
        V[k][q] = as + bc;
    }
}

// The quaternion (w, x, y, z) divided by its length, when that is > 0.0 (contract C18, step 4)
inline void align_unit_quaternion(double &w, double &x, double &y, double &z)
{
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double len = sqrt(((ww + xx) + yy) + zz);
    if (len > 0.0) {
        w = w / len;
        x = x / len;
        y = y / len;
        z = z / len;
    }
}

// The nine expressions of contract C18, step 4: R, row-major, from the unit quaternion (w, x, y, z)
inline void align_rotation_of(double w, double x, double y, double z, double R[9])
{
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = (ww + xx) - (yy + zz);
    R[1] = 2.0 * (xy - wz);
    R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);
    R[4] = (ww - xx) + (yy - zz);
    R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);
    R[7] = 2.0 * (yz + wx);
    R[8] = (ww - xx) - (yy - zz);
}

// The step from the means (pm, then qm) and the ten sums of pass 2 (S[9] > 0).  sweeps (may be null): the sweeps taken;
// quaternion (may be null): w, x, y, z as the rotation was expanded from them
inline AlignTransform align_solve(const double mean[6], const double S[kAlignSums2], bool with_scale, unsigned *sweeps = nullptr,
                                  double *quaternion = nullptr)
{
    double A[4][4], V[4][4];
    A[0][0] = (S[0] + S[4]) + S[8];
    A[1][1] = (S[0] - S[4]) - S[8];
    A[2][2] = (S[4] - S[0]) - S[8];
    A[3][3] = (S[8] - S[0]) - S[4];
    A[0][1] = A[1][0] = S[5] - S[7];
    A[0][2] = A[2][0] = S[6] - S[2];
    A[0][3] = A[3][0] = S[1] - S[3];
    A[1][2] = A[2][1] = S[1] + S[3];
    A[1][3] = A[3][1] = S[6] + S[2];
    A[2][3] = A[3][2] = S[5] + S[7];
    for (int r = 0; r < 4; ++r) {
        for (int c = 0; c < 4; ++c) {
            V[r][c] = r == c ? 1.0 : 0.0;
        }
    }
    unsigned done = 0;
    for (;;) {
        bool settled = true;
        for (int p = 0; p < 4; ++p) {
            for (int q = p + 1; q < 4; ++q) {
                settled = settled && normal_settled(A[p][q], A[p][p], A[q][q]);
            }
        }
        if (settled || done == kAlignSweepCap) {
            break;
        }
        for (int p = 0; p < 4; ++p) {
            for (int q = p + 1; q < 4; ++q) {
                if (normal_settled(A[p][q], A[p][p], A[q][q])) {
                    A[p][q] = A[q][p] = 0.0;
                } else {
                    align_rotate(A, V, p, q);
                }
            }
        }
        ++done;
    }
    if (sweeps) {
        *sweeps = done;
    }
    int top = 0;
    for (int c = 1; c < 4; ++c) {
        top = A[c][c] > A[top][top] ? c : top;
    }
    double w = V[0][top], x = V[1][top], y = V[2][top], z = V[3][top];
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    align_unit_quaternion(w, x, y, z);
    if (quaternion) {
        quaternion[0] = w;
        quaternion[1] = x;
        quaternion[2] = y;
        quaternion[3] = z;
    }
    AlignTransform step;
    align_rotation_of(w, x, y, z, step.R);
    if (with_scale) {
        const double r0 = align_row_dot(step.R, 0, S[0], S[3], S[6]);
        const double r1 = align_row_dot(step.R, 1, S[1], S[4], S[7]);
        const double r2 = align_row_dot(step.R, 2, S[2], S[5], S[8]);
        const double r01 = r0 + r1;
        step.scale = (r01 + r2) / S[9];
    }
    for (int a = 0; a < 3; ++a) {
        const double moved = step.scale * align_row_dot(step.R, a, mean[0], mean[1], mean[2]);
        step.t[a] = mean[3 + a] - moved;
    }
    return step;
}

// `step` applied after `total`
inline AlignTransform align_compose(const AlignTransform &step, const AlignTransform &total)
{
    AlignTransform both;
    both.scale = step.scale * total.scale;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            both.R[3 * a + b] = align_row_dot(step.R, a, total.R[b], total.R[3 + b], total.R[6 + b]);
        }
        const double turned = step.scale * align_row_dot(step.R, a, total.t[0], total.t[1], total.t[2]);
        both.t[a] = turned + step.t[a];
    }
    return both;
}

inline Alignment align_identity()
{
    const AlignTransform none;
    Alignment a = {};
    a.scale = none.scale;
    for (int e = 0; e < 9; ++e) {
        a.rotation[e] = none.R[e];
    }
    a.stopped = kAlignTooFew;
    return a;
}

// The iteration.  pass1(k, total, sums[8]): the totals of pass 1 on X_k (X_0 when k is 0, X_0 moved by `total` otherwise), after
// the search that matches it; pass2(mean, sums[10]): those of pass 2 on the same positions and matches.  Either returns 0 or
// what align_run then returns at once
template <typename Pass1, typename Pass2>
inline int align_run(unsigned iterations, double tolerance, bool with_scale, Pass1 &&pass1, Pass2 &&pass2, Alignment &out)
{
    AlignTransform total;
    out = align_identity();
    double previous = 0.0;
    for (unsigned k = 0;; ++k) {
        double s1[kAlignSums1];
        if (const int rc = pass1(k, total, s1); rc != 0) {
            return rc;
        }
        const double m = s1[0];
        const double rms = align_rms(s1[7], m);
        if (k == 0) {
            out.matched_before = (long long)m;
            out.rms_before = rms;
        }
        out.matched_after = (long long)m;
        out.rms_after = rms;
        out.steps = (int)k;
        if (k == iterations) {
            out.stopped = kAlignIterations;
            break;
        }
        out.stopped = kAlignTooFew;
        if (m < 3.0) {
            break;
        }
        const double mean[6] = {s1[1] / m, s1[2] / m, s1[3] / m, s1[4] / m, s1[5] / m, s1[6] / m};
        double s2[kAlignSums2];
        if (const int rc = pass2(mean, s2); rc != 0) {
            return rc;
        }
        if (s2[9] == 0.0) {
            break;
        }
        if (k > 0 && fabs(rms - previous) <= tolerance * previous) {
            out.stopped = kAlignConverged;
            break;
        }
        const AlignTransform step = align_solve(mean, s2, with_scale);
        if (!(isfinite(step.scale) && step.scale > 0.0)) {
            break;
        }
        total = align_compose(step, total);
        previous = rms;
    }
    out.scale = total.scale;
    for (int e = 0; e < 9; ++e) {
        out.rotation[e] = total.R[e];
    }
    for (int a = 0; a < 3; ++a) {
        out.translation[a] = total.t[a];
    }
    return 0;
}

}  // namespace apd_fusion
