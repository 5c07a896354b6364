// apd_register_math.h -- global registration of one cloud to another by FPFH descriptors, nearest descriptors and RANSAC
// (arithmetic contract C19): the relation under apd_points_features, apd_points_match_features and apd_points_register,
// written once and compiled by hipcc into the kernels (apd_points_register.hip) and by the host compiler into whoever restates
// it.  As in apd_align_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order, + - * / and
// sqrt alone (both correctly rounded) and conversions: no acos, atan2, sin or cos anywhere, on the host or the device.
//
// 1. DESCRIPTORS (per cloud; binary64 from the point where a coordinate or a normal is read).
//    Frame.  The unit normal of a point is its stored normal, each component converted to double, divided by len =
//    sqrt((nx * nx + ny * ny) + nz * nz) (register_unit_normal).  A point HAS A FRAME when len is finite and > 0.0 and the point
//    lies inside the grid of contract C11 (cell size `radius`, origin `origin`).  Only points with a frame take part.
//    Pair (register_pair).  For a centre c and a neighbour q of it by contract C11, both with a frame: d = x_q - x_c per axis,
//    d2 = (dx * dx + dy * dy) + dz * dz.  d2 == 0.0 (the two positions are equal): the pair is skipped.  a1 = n_c . d, a2 = n_q . d
//    (every dot product here is (x + y) + z of the three rounded products).  The SOURCE is the member whose normal makes the smaller
//    angle with the connecting line, decided on the dot products: |a1| < |a2| makes q the source -- n1 = n_q, n2 = n_c, d negated,
//    f = -a2 --, otherwise c is -- n1 = n_c, n2 = n_q, f = a1.  With dist = sqrt(d2): phi = f / dist.  v = d x n1 (each component
//    the difference of two rounded products), vv = v . v; vv == 0.0 (d parallel to n1): the pair is skipped; v is divided by
//    sqrt(vv); w = n1 x v; alpha = v . n2; the pair (y, x) = (w . n2, n1 . n2) stands for theta = atan2(y, x), which is never
//    computed.  These are the u = n1, v, w and the three features of PCL's computePairFeatures.  A pair that is not skipped is
//    ADMITTED, and q is then an admitted neighbour of c; the relation is symmetric but for the sign conventions, which are the
//    centre's.
//    Bins, kRegisterBins = 11 per feature.  alpha and phi (cosines in [-1, 1]): s = 11.0 * ((value + 1.0) * 0.5); the bin is 0
//    when !(s >= 0.0), 10 when s >= 11.0, else s truncated to an integer (register_linear_bin).  theta over [-pi, pi), bin b =
//    [-pi + 2 pi b / 11, -pi + 2 pi (b + 1) / 11), found by comparing (y, x) with the ten edge directions E_k = (cos, sin)(-pi +
//    2 pi k / 11), k = 1 .. 10, whose components are the literals of APD_REGISTER_EDGES and APD_REGISTER_EDGES_UP (register_theta_bin): the vector is at or past
//    edge k when cross_k = c_k * y - s_k * x (two rounded products, one difference) is >= 0.0.  y < 0.0 (the lower half plane,
//    where edges 1 .. 5 lie): the bin is the number of k = 1 .. 5 with cross_k >= 0.0.  Otherwise (y >= 0.0, which includes y =
//    -0.0): 5 + the number of k = 6 .. 10 with cross_k >= 0.0.
//    EXACTLY ON AN EDGE (cross_k == 0.0) a vector belongs to the upper bin, as floor would put it.  The direction (-1, 0) (y == 0.0
//    or -0.0, x < 0.0) falls into bin 10: theta = +pi, clamped as PCL clamps it; a y of -0.0 is not the lower half plane.  (y, x) =
//    (0, 0) -- n2 parallel to v -- falls into bin 5, where atan2's 0 would: it is tested first.
//    SPFH.  k_c = the number of admitted neighbours of c.  k_c < min_neighbours (>= 3): c has NO DESCRIPTOR.  Otherwise SPFH(c) is
//    the three count histograms, 33 binary64 numbers (double)count_b / (double)k_c: alpha at 0 .. 10, phi at 11 .. 21, theta at
//    22 .. 32.
//    FPFH (register_fpfh).  acc_b = 0.0, then over the admitted neighbours q of c that have an SPFH, in THE WALK'S ASCENDING ORDER
//    (apd_points_search.h: ascending cell key, equal keys by ascending input index): acc_b = acc_b + SPFH(q)_b / d2(c, q).  f_b =
//    SPFH(c)_b + acc_b / (double)k_c.  Each block of 11 is divided by its own sum, ((f_0 + f_1) + ..) + f_10 taken ascending, and
//    stored as binary32: (float)(f_b / sum).  The sum is at least the SPFH block's, which is about 1.  A point without a
//    descriptor gets 33 zeros; `has` says which points have one.
//
// 2. MATCHES.  For every point i of P with a descriptor: the point j of Q with a descriptor whose register_distance2 -- binary32:
//    from 0.0f, for b = 0 .. 32 ascending, diff = a_b - c_b, sq = diff * diff, sum = sum + sq, no fma -- is smallest; among equal
//    ones the smallest j.  `mutual`: the pair is kept only when i is in turn the match of j by the same rule with the roles
//    swapped.  The M matches are kept in ascending i.  The reported distance is sqrtf of the sum.
//
// 3. TRIALS, t = 0 .. trials - 1 (1 .. kRegisterMaxTrials), M >= 3.  The generator is counter-based, in unsigned 64-bit arithmetic
//    modulo 2^64 (register_draw): key = seed + (t + 1) * 0x9E3779B97F4A7C15; draw number c = 0, 1, ..: z = key + c *
//    0xD1B54A32D192ED03; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z = z ^ (z >> 31);
//    position = ((z >> 32) * M) >> 32 (M < 2^31).  Three distinct positions (register_three): the first is draw 0; each further
//    one takes the following draws until one differs from those already taken; after kRegisterDrawCap = 16 draws in all the
//    rejection loop ends and a missing position is (the position taken last + 1) mod M, advanced by 1 mod M while it equals one
//    already taken.
//    The trial is ADMITTED (register_trial) when for each edge (0, 1), (1, 2), (2, 0) of the triangle the squared lengths lp and
//    lq on the two sides (binary64 of the float coordinates, (dx * dx + dy * dy) + dz * dz) satisfy lp >= e2 * lq and lq >= e2 * lp
//    with e2 = (double)edge_ratio * (double)edge_ratio -- no square root --, and neither triangle is degenerate: the sum |u|^2 of
//    pass 2 of contract C18 about its own mean is not 0.0, on P's side as align_run tests it and on Q's side with the roles
//    swapped.  The trial's transform is align_solve (apd_align_math.h, rigid) on the three pairs through its own means and
//    moments: the pairs stand in slots 0, 1, 2 of one chunk of contract C18's tree (align_tree), the other slots +0.0.
//    INLIERS.  A match is an inlier of a transform when radius_d2(align_moved(P point), Q point) <= inlier_distance *
//    inlier_distance in binary32 (contract C17's comparison).  The best trial is the admitted one with the most inliers, the
//    lowest t among equals.
//
// 4. REFIT (register_run).  index[i] = the match of i when it is an inlier of the best trial, -1 otherwise; steps 2 - 4 of
//    contract C18 over P's own positions and that index, with_scale the caller's choice.  If the moment [9] is 0.0 or the scale
//    is not finite or not > 0.0 the best trial's transform stands; otherwise the refit is what is returned.  Under what is
//    returned the inliers are marked once more and pass 1 of C18 over P moved (align_moved) gives inliers_after = [0] and
//    rms_after = sqrt([7] / [0]) (align_rms).
//    STOPS.  kRegisterOk; kRegisterTooFewMatches when M < 3; kRegisterNoTrial when no trial is admitted or the best has fewer
//    than 3 inliers.  Both failures return the identity.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "apd_align_math.h"
#include "apd_nearest_math.h"
#include "apd_radius_math.h"

// The loops over a descriptor have constant bounds: unrolled, a lane's 33 numbers are registers and not an indexed array
#if defined(__HIPCC__)
#define APD_REGISTER_UNROLL _Pragma("unroll")
#else
#define APD_REGISTER_UNROLL
#endif

namespace apd_fusion {

constexpr int kRegisterBins = 11;                    // per feature
constexpr int kRegisterWidth = 3 * kRegisterBins;    // numbers of a descriptor
constexpr unsigned kRegisterMinNeighbours = 3;       // the least min_neighbours
constexpr unsigned kRegisterMaxTrials = 65536;       // the largest `trials`
constexpr unsigned kRegisterDrawCap = 16;            // draws of a trial's rejection loop at most
constexpr long long kRegisterMaxPoints = 1LL << 18;  // on either side of a match: its cost is quadratic
enum : int { kRegisterOk = 0, kRegisterTooFewMatches = 1, kRegisterNoTrial = 2 };  // APD_REGISTER_* of include/apd_mi355x.h

// apd_points_register_options (include/apd_mi355x.h), in its layout
struct RegisterOptions {
    unsigned trials;
    unsigned long long seed;
    float inlier_distance, edge_ratio;
    unsigned min_neighbours;
    int mutual, with_scale;
};

// The fields of apd_points_registration_t (include/apd_mi355x.h), in its layout
struct Registration {
    double scale, rotation[9], translation[3];
    long long features_p, features_q, matches, trials_admitted, best_trial, inliers, inliers_after;
    double rms_after;
    int stopped;
};

APD_HD double register_dot(const double a[3], const double b[3])
{
    const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    const double xy = x + y;
    return xy + z;
}

// out = a x b
APD_HD void register_cross(const double a[3], const double b[3], double out[3])
{
    const double yz = a[1] * b[2], zy = a[2] * b[1], zx = a[2] * b[0], xz = a[0] * b[2], xy = a[0] * b[1], yx = a[1] * b[0];
    out[0] = yz - zy;
    out[1] = zx - xz;
    out[2] = xy - yx;
}

// The unit normal of a stored normal; false (and zeros): none.  Whether the point lies inside the grid is the caller's to add
APD_HD bool register_unit_normal(const float N[3], double unit[3])
{
    const double n[3] = {(double)N[0], (double)N[1], (double)N[2]};
    const double len = sqrt(register_dot(n, n));
    const bool have = len > 0.0 && len < (double)INFINITY;  // false for a NaN
    unit[0] = have ? n[0] / len : 0.0;
    unit[1] = have ? n[1] / len : 0.0;
    unit[2] = have ? n[2] / len : 0.0;
    return have;
}

// A unit normal as register_unit_normal left it: zeros stand for "no frame" (a unit vector has a component of at least 0.5)
APD_HD bool register_has_frame(const double unit[3]) { return unit[0] != 0.0 || unit[1] != 0.0 || unit[2] != 0.0; }

APD_HD int register_linear_bin(double value)
{
    const double s = 11.0 * ((value + 1.0) * 0.5);
    if (!(s >= 0.0)) {
        return 0;
    }
    return s >= 11.0 ? kRegisterBins - 1 : (int)s;
}

// (cos, sin) of the edges -pi + 2 pi k / 11, k = 1 .. 10: the edges of the lower half plane, then those of the upper
#define APD_REGISTER_EDGES(F)                                                                                                        \
    F(-0.8412535328311811, -0.5406408174555978)                                                                                      \
    F(-0.4154150130018863, -0.9096319953545184)                                                                                      \
    F(0.14231483827328512, -0.9898214418809327)                                                                                      \
    F(0.6548607339452851, -0.7557495743542583)                                                                                       \
    F(0.9594929736144975, -0.2817325568414295)
#define APD_REGISTER_EDGES_UP(F)                                                                                                     \
    F(0.9594929736144975, 0.2817325568414295)                                                                                        \
    F(0.6548607339452851, 0.7557495743542583)                                                                                        \
    F(0.14231483827328512, 0.9898214418809327)                                                                                       \
    F(-0.4154150130018863, 0.9096319953545184)                                                                                       \
    F(-0.8412535328311811, 0.5406408174555978)

// 1 when (x, y) is at or past the edge direction (c, s)
APD_HD int register_past_edge(double c, double s, double y, double x)
{
    const double cy = c * y, sx = s * x;
    return cy - sx >= 0.0 ? 1 : 0;
}

// The bin of theta = atan2(y, x), by comparisons alone
APD_HD int register_theta_bin(double y, double x)
{
    if (y == 0.0 && x == 0.0) {
        return 5;
    }
    int bin = 0;
#define APD_REGISTER_COUNT(c, s) bin += register_past_edge(c, s, y, x);
    if (y < 0.0) {
        APD_REGISTER_EDGES(APD_REGISTER_COUNT)
    } else {
        bin = 5;
        APD_REGISTER_EDGES_UP(APD_REGISTER_COUNT)
    }
#undef APD_REGISTER_COUNT
    return bin;
}

// The pair of a centre at C with unit normal nc and a neighbour at Q with unit normal nq, both with a frame.  false: skipped.
// d2: the squared distance; bins: those of alpha, phi and theta, each 0 .. 10
APD_HD bool register_pair(const float C[3], const double nc[3], const float Q[3], const double nq[3], double &d2, int bins[3])
{
    double d[3] = {(double)Q[0] - (double)C[0], (double)Q[1] - (double)C[1], (double)Q[2] - (double)C[2]};
    d2 = register_dot(d, d);
    if (d2 == 0.0) {
        return false;
    }
    const double a1 = register_dot(nc, d), a2 = register_dot(nq, d);
    const bool swap = fabs(a1) < fabs(a2);
    double n1[3], n2[3];
    for (int a = 0; a < 3; ++a) {
        n1[a] = swap ? nq[a] : nc[a];
        n2[a] = swap ? nc[a] : nq[a];
        d[a] = swap ? -d[a] : d[a];
    }
    const double f = swap ? -a2 : a1;
    const double phi = f / sqrt(d2);
    double v[3], w[3];
    register_cross(d, n1, v);
    const double vv = register_dot(v, v);
    if (vv == 0.0) {
        return false;
    }
    const double len = sqrt(vv);
    v[0] = v[0] / len;
    v[1] = v[1] / len;
    v[2] = v[2] / len;
    register_cross(n1, v, w);
    bins[0] = register_linear_bin(register_dot(v, n2));
    bins[1] = register_linear_bin(phi);
    bins[2] = register_theta_bin(register_dot(w, n2), register_dot(n1, n2));
    return true;
}

// The descriptor of a point with k admitted neighbours: own, its SPFH; acc, the weighted sum over its neighbours' (used up)
APD_HD void register_fpfh(const double own[kRegisterWidth], double acc[kRegisterWidth], unsigned k, float out[kRegisterWidth])
{
    const double count = (double)k;
    APD_REGISTER_UNROLL
    for (int block = 0; block < kRegisterWidth; block += kRegisterBins) {
        double sum = 0.0;
        APD_REGISTER_UNROLL
        for (int b = 0; b < kRegisterBins; ++b) {
            const double share = acc[block + b] / count;
            acc[block + b] = own[block + b] + share;
            sum = b == 0 ? acc[block + b] : sum + acc[block + b];
        }
        APD_REGISTER_UNROLL
        for (int b = 0; b < kRegisterBins; ++b) {
            out[block + b] = (float)(acc[block + b] / sum);
        }
    }
}

// The squared distance of two descriptors
APD_HD float register_distance2(const float a[kRegisterWidth], const float c[kRegisterWidth])
{
    float sum = 0.0f;
    APD_REGISTER_UNROLL
    for (int b = 0; b < kRegisterWidth; ++b) {
        const float diff = a[b] - c[b];
        const float sq = diff * diff;
        sum = sum + sq;
    }
    return sum;
}

// Draw number c of trial t among M positions
inline uint32_t register_draw(unsigned long long seed, unsigned t, unsigned c, uint32_t M)
{
    const uint64_t key = (uint64_t)seed + ((uint64_t)t + 1) * 0x9E3779B97F4A7C15ull;
    uint64_t z = key + (uint64_t)c * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(((z >> 32) * (uint64_t)M) >> 32);
}

// The three distinct positions of trial t, M >= 3
inline void register_three(unsigned long long seed, unsigned t, uint32_t M, uint32_t at[3])
{
    unsigned c = 0;
    for (int have = 0; have < 3; ++have) {
        bool found = false;
        while (!found && c < kRegisterDrawCap) {
            at[have] = register_draw(seed, t, c++, M);
            found = (have < 1 || at[have] != at[0]) && (have < 2 || at[have] != at[1]);
        }
        if (!found) {  // have > 0: draw 0 is always taken
            at[have] = (at[have - 1] + 1) % M;
            for (int step = 0; step < 2; ++step) {
                if (at[have] == at[0] || (have == 2 && at[have] == at[1])) {
                    at[have] = (at[have] + 1) % M;
                }
            }
        }
    }
}

inline double register_length2(const float *a, const float *b)
{
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz;
}

// The totals of pass 1 or pass 2 of contract C18 for three pairs in slots 0 .. 2 of one chunk; terms(slot, v)
template <int N, typename Terms> inline void register_sums3(Terms &&terms, double total[N])
{
    double slots[N][kKnnChunk];
    for (int s = 0; s < kKnnChunk; ++s) {
        double v[N];
        for (int j = 0; j < N; ++j) {
            v[j] = 0.0;
        }
        if (s < 3) {
            terms(s, v);
        }
        for (int j = 0; j < N; ++j) {
            slots[j][s] = v[j];
        }
    }
    for (int j = 0; j < N; ++j) {
        total[j] = 0.0 + align_tree(slots[j]);
    }
}

// Whether the trial on the pairs (P[e], Q[e]), e = 0 .. 2 (three floats each) is admitted, and then its transform
inline bool register_trial(const float *const P[3], const float *const Q[3], float edge_ratio, AlignTransform &step)
{
    const double e2 = (double)edge_ratio * (double)edge_ratio;
    for (int e = 0; e < 3; ++e) {
        const int f = (e + 1) % 3;
        const double lp = register_length2(P[e], P[f]), lq = register_length2(Q[e], Q[f]);
        if (!(lp >= e2 * lq && lq >= e2 * lp)) {
            return false;
        }
    }
    double s1[kAlignSums1], s2[kAlignSums2], other[kAlignSums2];
    register_sums3<kAlignSums1>([&](int s, double *v) { align_terms1(P[s], Q[s], v); }, s1);
    const double m = s1[0];
    const double mean[6] = {s1[1] / m, s1[2] / m, s1[3] / m, s1[4] / m, s1[5] / m, s1[6] / m};
    const double swapped[6] = {mean[3], mean[4], mean[5], mean[0], mean[1], mean[2]};
    register_sums3<kAlignSums2>([&](int s, double *v) { align_terms2(P[s], Q[s], mean, v); }, s2);
    register_sums3<kAlignSums2>([&](int s, double *v) { align_terms2(Q[s], P[s], swapped, v); }, other);
    if (s2[9] == 0.0 || other[9] == 0.0) {
        return false;
    }
    step = align_solve(mean, s2, false);
    return true;
}

inline Registration register_identity(int stopped)
{
    const AlignTransform none;
    Registration r = {};
    r.scale = none.scale;
    for (int e = 0; e < 9; ++e) {
        r.rotation[e] = none.R[e];
    }
    r.best_trial = -1;
    r.stopped = stopped;
    return r;
}

// Trials, best trial and refit over the M matches, whose positions stand at mp and mq (three floats per match, P's and Q's).
//   count(moves, counts): counts[a] = the inliers of admitted trial a's move;
//   mark(move): index[] = the match of every inlier of `move`, -1 for every other point of P;
//   pass1(move or null, sums[8]): the totals of pass 1 of C18 over P's positions -- moved by *move, or its own -- and index[];
//   pass2(mean, sums[10]): those of pass 2 over P's own positions and index[].
// Each returns 0 or what register_run then returns at once.  out: features_p and features_q are the caller's to set
template <typename Count, typename Mark, typename Pass1, typename Pass2>
inline int register_run(const RegisterOptions &o, size_t M, const float *mp, const float *mq, Count &&count, Mark &&mark, Pass1 &&pass1, Pass2 &&pass2,
                        Registration &out)
{
    const long long features_p = out.features_p, features_q = out.features_q;
    out = register_identity(kRegisterTooFewMatches);
    out.features_p = features_p;
    out.features_q = features_q;
    out.matches = (long long)M;
    if (M < 3) {
        return 0;
    }
    out.stopped = kRegisterNoTrial;
    std::vector<unsigned> trial;
    std::vector<AlignTransform> steps;
    std::vector<AlignMove> moves;
    for (unsigned t = 0; t < o.trials; ++t) {
        uint32_t at[3];
        register_three(o.seed, t, (uint32_t)M, at);
        const float *const P[3] = {mp + 3 * (size_t)at[0], mp + 3 * (size_t)at[1], mp + 3 * (size_t)at[2]};
        const float *const Q[3] = {mq + 3 * (size_t)at[0], mq + 3 * (size_t)at[1], mq + 3 * (size_t)at[2]};
        AlignTransform step;
        if (register_trial(P, Q, o.edge_ratio, step)) {
            trial.push_back(t);
            steps.push_back(step);
            moves.push_back(align_move_of(step, true));
        }
    }
    out.trials_admitted = (long long)trial.size();
    if (trial.empty()) {
        return 0;
    }
    std::vector<uint32_t> counts(trial.size(), 0);
    if (const int rc = count(moves, counts); rc != 0) {
        return rc;
    }
    size_t best = 0;
    for (size_t a = 1; a < counts.size(); ++a) {
        best = counts[a] > counts[best] ? a : best;
    }
    out.best_trial = (long long)trial[best];
    out.inliers = (long long)counts[best];
    if (counts[best] < 3) {
        return 0;
    }
    AlignTransform result = steps[best];
    if (const int rc = mark(moves[best]); rc != 0) {
        return rc;
    }
    double s1[kAlignSums1], s2[kAlignSums2];
    if (const int rc = pass1((const AlignMove *)nullptr, s1); rc != 0) {
        return rc;
    }
    const double m = s1[0];
    if (m >= 3.0) {
        const double mean[6] = {s1[1] / m, s1[2] / m, s1[3] / m, s1[4] / m, s1[5] / m, s1[6] / m};
        if (const int rc = pass2(mean, s2); rc != 0) {
            return rc;
        }
        if (s2[9] != 0.0) {
            const AlignTransform refit = align_solve(mean, s2, o.with_scale != 0);
            if (isfinite(refit.scale) && refit.scale > 0.0) {
                result = refit;
            }
        }
    }
    const AlignMove by = align_move_of(result, true);
    if (const int rc = mark(by); rc != 0) {
        return rc;
    }
    if (const int rc = pass1(&by, s1); rc != 0) {
        return rc;
    }
    out.inliers_after = (long long)s1[0];
    out.rms_after = align_rms(s1[7], s1[0]);
    out.scale = result.scale;
    for (int e = 0; e < 9; ++e) {
        out.rotation[e] = result.R[e];
    }
    for (int a = 0; a < 3; ++a) {
        out.translation[a] = result.t[a];
    }
    out.stopped = kRegisterOk;
    return 0;
}

// Whether the match (P, Q) is an inlier of `by` at the squared distance r2
APD_HD bool register_inlier(const AlignMove &by, const float P[3], const float Q[3], float r2)
{
    float moved[3];
    align_moved(by, P, moved);
    return radius_d2(moved, Q) <= r2;
}

}  // namespace apd_fusion
