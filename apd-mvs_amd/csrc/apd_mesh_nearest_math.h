// apd_mesh_nearest_math.h -- the closest point of a mesh's surface to a point, points drawn on the surface by area, and from the two the
// score of a mesh against a cloud (arithmetic contract C27): the rules under apd_mesh_nearest, apd_mesh_sample_points and
// apd_mesh_score, written once and compiled by hipcc into the kernels (apd_mesh_nearest.hip) and by the host compiler into whoever
// restates them.  As in apd_nearest_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in the order given;
// binary64 on the binary32 inputs widened unless binary32 is stated; sqrt correctly rounded (C4).
//
// CLOSEST POINT.  Grid: that of contract C11 (apd_radius_math.h), cell size `radius`, origin `origin`.  Face f with corners a, b, c
// is a CANDIDATE of query P when
//   its three indices are distinct,
//   its nine coordinates are finite and each has a cell (voxel_cell true: within +-2^20 cells of the origin)  [mesh_face_on_grid],
//   n2 = |(b - a) x (c - a)|^2 > 0  [mesh_face_area2],
//   P is inside the grid (radius_cells true),
//   d2 <= (double)radius * (double)radius, d2 the squared distance from P to its closest point X on the face  [mesh_closest_point].
// Unlike C17 no cell condition is part of the definition: a loop over all faces gives the same bits as any search that meets every
// candidate at least once.  A NaN d2 fails the comparison.
// Every dot product is (x * x' + y * y') + z * z'  [mesh_dot].  The cross product of u and v is (uy * vz - uz * vy, uz * vx - ux * vz,
// ux * vy - uy * vx), each a difference of two rounded products.
// X is the Voronoi-region method of Ericson, Real-Time Collision Detection, section 5.1.5, with ab = b - a, ac = c - a, bc = c - b,
// ap = P - a, bp = P - b, cp = P - c and, as printed there,
//   d1 = ab . ap, d2 = ac . ap, d3 = ab . bp, d4 = ac . bp, d5 = ab . cp, d6 = ac . cp,
//   vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4  (each a difference of two rounded products),
// the regions tested in this order, the first that holds decides:
//   vertex a:  d1 <= 0 and d2 <= 0                                X = a
//   vertex b:  d3 >= 0 and d4 <= d3                               X = b
//   vertex c:  d6 >= 0 and d5 <= d6                               X = c
//   edge ab:   vc <= 0 and d1 >= 0 and d3 <= 0                    v = d1 / (d1 - d3),       X = a + v * ab
//   edge ac:   vb <= 0 and d2 >= 0 and d6 <= 0                    w = d2 / (d2 - d6),       X = a + w * ac
//   edge bc:   va <= 0 and s = d4 - d3 >= 0 and t = d5 - d6 >= 0  w = s / (s + t),          X = b + w * bc
//   interior:  otherwise                                          D = (va + vb) + vc, v = vb / D, w = vc / D, X = (a + v * ab) + w * ac
// (per coordinate; a vertex region gives the vertex's own bits).  Then every coordinate of X is held between the least and the largest
// of the three corners' (comparisons only: it changes X where rounding, or the cancellation in va, vb, vc of a sliver, put it
// outside the face's bounding box, where no closest point is).  A NaN X stays NaN.  d2 = mesh_dot(P - X, P - X).
// NEAREST.  The candidate of least d2; among equal d2 the smallest face index  [mesh_nearest_takes: it does not depend on the order
// in which the candidates are met, nor on how often].  distance = (float)sqrt(d2), closest = X rounded to binary32 per coordinate;
// without a candidate +inf, -1 and three NaNs.
//
// SAMPLES.  A face with a repeated index, a non-finite coordinate or n2 not > 0 gets none (no grid is involved).  Otherwise
//   area = 0.5 * sqrt(n2),  n_f = floor(area * density + u(seed, f))  [mesh_sample_count],
// stochastic rounding: the expected number is area * density.  The random numbers are counter-based  [mesh_sample_unit]: with
// mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31) (the splitmix64
// finaliser, modulo 2^64),
//   h = mix(seed + (f + 1) * 0x9E3779B97F4A7C15),  z = mix(h + k * 0xD1B54A32D192ED03 + c * 0x8CB92BA72F3D8DD7),
//   the number = (double)(z >> 11) * 2^-53, in [0, 1);
// u(seed, f) is (k, c) = (0, 0); sample k of face f takes r1 = (k, 1) and r2 = (k, 2).  When r1 + r2 > 1 they become 1 - r1 and
// 1 - r2.  Position: (a + r1 * ab) + r2 * ac per coordinate, rounded to binary32.  Normal: the cross product (b - a) x (c - a)
// divided per coordinate by sqrt(n2), rounded to binary32.  Colour per channel: w0 = (1 - r1) - r2, m = (w0 * ca + r1 * cb) + r2 * cc,
// the byte (int)floor(m + 0.5) held to 0 .. 255; 0 for a mesh without colours.  Order: faces ascending, k ascending within a face.
//
// SCORE at threshold tau with samples S of the mesh and a truth cloud T: a = the finite distances of contract C17's search of S in T
// at radius tau (binary32, its cell condition included), b = the finite distances of the closest-point search above of T against the
// mesh at radius tau; n_p = |S|, n_q = |T|; the nine numbers are nearest_score's (apd_nearest_math.h) with the binary64 chunk sums
// of contract C12 over the two lists of distances.
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_radius_math.h"

namespace apd_fusion {

constexpr int32_t kMeshNearestNoFace = -1;
constexpr uint32_t kMeshSampleCap = 0x80000000u;  // what mesh_sample_count gives for 2^31 samples or more, a NaN included

APD_HD double mesh_dot(const double u[3], const double v[3])
{
    const double xx = u[0] * v[0], yy = u[1] * v[1], zz = u[2] * v[2];
    const double xy = xx + yy;
    return xy + zz;
}

APD_HD void mesh_cross(const double u[3], const double v[3], double out[3])
{
    const double a0 = u[1] * v[2], b0 = u[2] * v[1];
    const double a1 = u[2] * v[0], b1 = u[0] * v[2];
    const double a2 = u[0] * v[1], b2 = u[1] * v[0];
    out[0] = a0 - b0;
    out[1] = a1 - b1;
    out[2] = a2 - b2;
}

// The nine coordinates of a face widened, corner after corner
struct MeshFace {
    double a[3], b[3], c[3];
};

APD_HD MeshFace mesh_face_of(const float A[3], const float B[3], const float C[3])
{
    MeshFace f;
    for (int k = 0; k < 3; ++k) {
        f.a[k] = (double)A[k];
        f.b[k] = (double)B[k];
        f.c[k] = (double)C[k];
    }
    return f;
}

APD_HD bool mesh_face_finite(const float A[3], const float B[3], const float C[3])
{
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        ok = ok && isfinite(A[k]) && isfinite(B[k]) && isfinite(C[k]);
    }
    return ok;
}

// normal = (b - a) x (c - a); returns its squared length n2
APD_HD double mesh_face_area2(const MeshFace &f, double normal[3])
{
    double ab[3], ac[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = f.b[k] - f.a[k];
        ac[k] = f.c[k] - f.a[k];
    }
    mesh_cross(ab, ac, normal);
    return mesh_dot(normal, normal);
}

// Whether a face with these indices and corners can give anything at all: distinct indices, finite corners, n2 > 0
APD_HD bool mesh_face_proper(const int32_t index[3], const float A[3], const float B[3], const float C[3])
{
    if (index[0] == index[1] || index[1] == index[2] || index[0] == index[2] || !mesh_face_finite(A, B, C)) {
        return false;
    }
    double normal[3];
    return mesh_face_area2(mesh_face_of(A, B, C), normal) > 0.0;
}

// How far the binary32 cell of a coordinate can be from where real arithmetic puts it, as a share of a cell: with u = 2^-24 the
// quotient t = fl(fl(x - origin) / radius) of voxel_cell differs from q = (x - origin) / radius by at most |q| (2 u + u^2) (and
// 2^-150 where the division underflows).  For a query P and a point X of a face's bounding box with |P.x - X.x| <= radius (1 +
// 2^-50) -- what d2 <= r2 gives after the roundings of d2 -- and xmax the box's largest x: q(P.x) <= q(xmax) + 1 + 2^-50, so
// t(P.x) <= t(xmax) + 1 + E with E = 2^-21 (|t(xmax)| + 2), which is more than twice the sum of the two quotients' errors and
// the distance's.  P's cell floor(t(P.x)) therefore exceeds the box's last cell floor(t(xmax)) by 2 or more only if the
// fraction of t(xmax) is >= 1 - E; on the other side it falls 2 or more below floor(t(xmin)) only if the fraction of t(xmin) is
// <= E.  In exactly these cases the box's cell range is widened by one cell (mesh_cell_range), and then every query within the
// radius of a point of the box has one of its three cells of that axis in the range: the search of the 27 cells is complete
// for the definition above, whatever the rounding does.  The closest point itself is held inside the box (mesh_closest_point).
// At cell 2^20 E is 1/2 and half the faces are widened; near the origin none but those whose corner stands on a cell boundary.
APD_HD double mesh_cell_margin(float t) { return 0x1p-21 * (fabs((double)t) + 2.0); }

// The cells lo .. hi that the coordinates least <= most of one axis are binned into: their own cells, widened by one where
// mesh_cell_margin asks for it, held to the grid; false: a coordinate has no cell
APD_HD bool mesh_cell_range(float least, float most, float origin, float radius, int &lo, int &hi)
{
    if (!voxel_cell(least, origin, radius, lo) || !voxel_cell(most, origin, radius, hi)) {
        return false;
    }
    const float t_lo = (least - origin) / radius, t_hi = (most - origin) / radius;  // voxel_cell's quotients, bit for bit
    if ((double)t_lo - (double)lo <= mesh_cell_margin(t_lo) && lo > -kVoxelHalf) {
        lo -= 1;
    }
    if ((double)t_hi - (double)hi >= 1.0 - mesh_cell_margin(t_hi) && hi < kVoxelHalf - 1) {
        hi += 1;
    }
    return true;
}

// The cells of the grid a face is binned into: those of its bounding box, lo[k] <= hi[k], by mesh_cell_range; false: a coordinate
// has no cell.  voxel_cell is monotonic in its coordinate, so the cells of the least and the largest coordinate bound every corner's
APD_HD bool mesh_face_on_grid(const float A[3], const float B[3], const float C[3], const float origin[3], float radius, int lo[3], int hi[3])
{
    for (int k = 0; k < 3; ++k) {
        int cell = 0;
        if (!voxel_cell(A[k], origin[k], radius, cell) || !voxel_cell(B[k], origin[k], radius, cell) || !voxel_cell(C[k], origin[k], radius, cell)) {
            return false;
        }
        const float ab_least = A[k] < B[k] ? A[k] : B[k], ab_most = A[k] > B[k] ? A[k] : B[k];
        const float least = ab_least < C[k] ? ab_least : C[k], most = ab_most > C[k] ? ab_most : C[k];
        if (!mesh_cell_range(least, most, origin[k], radius, lo[k], hi[k])) {
            return false;
        }
    }
    return true;
}

// The cells of that box, capped at 2^31: each axis spans at most 2^21 cells, so two axes fit 64 bits and the third is tested first
APD_HD uint32_t mesh_face_cells(const int lo[3], const int hi[3])
{
    const uint64_t nx = (uint64_t)(hi[0] - lo[0]) + 1, ny = (uint64_t)(hi[1] - lo[1]) + 1, nz = (uint64_t)(hi[2] - lo[2]) + 1;
    const uint64_t xy = nx * ny;  // <= 2^42
    if (xy >= (uint64_t)kMeshSampleCap) {
        return kMeshSampleCap;
    }
    const uint64_t all = xy * nz;  // < 2^31 * 2^21
    return all >= (uint64_t)kMeshSampleCap ? kMeshSampleCap : (uint32_t)all;
}

// X, the closest point of the face to P, and the squared distance to it
APD_HD double mesh_closest_point(const MeshFace &f, const double P[3], double X[3])
{
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = f.b[k] - f.a[k];
        ac[k] = f.c[k] - f.a[k];
        ap[k] = P[k] - f.a[k];
        bp[k] = P[k] - f.b[k];
        cp[k] = P[k] - f.c[k];
    }
    const double d1 = mesh_dot(ab, ap), d2 = mesh_dot(ac, ap);
    const double d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp);
    const double d5 = mesh_dot(ab, cp), d6 = mesh_dot(ac, cp);
    if (d1 <= 0.0 && d2 <= 0.0) {
        X[0] = f.a[0], X[1] = f.a[1], X[2] = f.a[2];
    } else if (d3 >= 0.0 && d4 <= d3) {
        X[0] = f.b[0], X[1] = f.b[1], X[2] = f.b[2];
    } else if (d6 >= 0.0 && d5 <= d6) {
        X[0] = f.c[0], X[1] = f.c[1], X[2] = f.c[2];
    } else {
        const double p14 = d1 * d4, p32 = d3 * d2, p52 = d5 * d2, p16 = d1 * d6, p36 = d3 * d6, p54 = d5 * d4;
        const double vc = p14 - p32, vb = p52 - p16, va = p36 - p54;
        const double s = d4 - d3, t = d5 - d6;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double v = d1 / (d1 - d3);
            for (int k = 0; k < 3; ++k) {
                const double step = v * ab[k];
                X[k] = f.a[k] + step;
            }
        } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            for (int k = 0; k < 3; ++k) {
                const double step = w * ac[k];
                X[k] = f.a[k] + step;
            }
        } else if (va <= 0.0 && s >= 0.0 && t >= 0.0) {
            const double w = s / (s + t);
            for (int k = 0; k < 3; ++k) {
                const double bc = f.c[k] - f.b[k];
                const double step = w * bc;
                X[k] = f.b[k] + step;
            }
        } else {
            const double D = (va + vb) + vc;
            const double v = vb / D, w = vc / D;
            for (int k = 0; k < 3; ++k) {
                const double sv = v * ab[k], sw = w * ac[k];
                const double along = f.a[k] + sv;
                X[k] = along + sw;
            }
        }
    }
    for (int k = 0; k < 3; ++k) {  // inside the face's bounding box, where the closest point of real arithmetic is: an ill-conditioned sliver cannot leave it
        const double ab_least = f.a[k] < f.b[k] ? f.a[k] : f.b[k], ab_most = f.a[k] > f.b[k] ? f.a[k] : f.b[k];
        const double least = ab_least < f.c[k] ? ab_least : f.c[k], most = ab_most > f.c[k] ? ab_most : f.c[k];
        X[k] = X[k] < least ? least : X[k] > most ? most : X[k];
    }
    const double off[3] = {P[0] - X[0], P[1] - X[1], P[2] - X[2]};
    return mesh_dot(off, off);
}

// Whether face j at squared distance d2 (<= r2 already) replaces the best so far, (best_d2, best_j); have: there is one
APD_HD bool mesh_nearest_takes(double d2, uint32_t j, bool have, double best_d2, uint32_t best_j)
{
    return !have || d2 < best_d2 || (d2 == best_d2 && j < best_j);
}

APD_HD double mesh_nearest_r2(float radius) { return (double)radius * (double)radius; }

APD_HD float mesh_nearest_distance(double d2) { return (float)sqrt(d2); }

// ---- samples ----

APD_HD uint64_t mesh_sample_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The number (k, c) of face f under `seed`, in [0, 1)
APD_HD double mesh_sample_unit(unsigned long long seed, uint64_t f, uint64_t k, uint64_t c)
{
    const uint64_t h = mesh_sample_mix((uint64_t)seed + (f + 1) * 0x9E3779B97F4A7C15ull);
    const uint64_t z = mesh_sample_mix(h + k * 0xD1B54A32D192ED03ull + c * 0x8CB92BA72F3D8DD7ull);
    return (double)(z >> 11) * 0x1p-53;
}

// n_f of a proper face with squared normal length n2; kMeshSampleCap for 2^31 or more
APD_HD uint32_t mesh_sample_count(double n2, double density, double u)
{
    const double area = 0.5 * sqrt(n2);
    const double wanted = area * density;
    const double n = floor(wanted + u);
    if (!(n < 2147483648.0)) {
        return kMeshSampleCap;
    }
    return n > 0.0 ? (uint32_t)n : 0u;
}

// Sample k of face f: position and normal (binary32), colour from the corners' colours (null: 0, 0, 0)
APD_HD void mesh_sample_point(const MeshFace &face, unsigned long long seed, uint64_t f, uint64_t k, const uint8_t *ca, const uint8_t *cb,
                              const uint8_t *cc, float xyz[3], float normal[3], uint8_t bgr[3])
{
    double r1 = mesh_sample_unit(seed, f, k, 1), r2 = mesh_sample_unit(seed, f, k, 2);
    if (r1 + r2 > 1.0) {
        r1 = 1.0 - r1;
        r2 = 1.0 - r2;
    }
    double n[3];
    const double length = sqrt(mesh_face_area2(face, n));
    for (int a = 0; a < 3; ++a) {
        const double ab = face.b[a] - face.a[a], ac = face.c[a] - face.a[a];
        const double s1 = r1 * ab, s2 = r2 * ac;
        const double along = face.a[a] + s1;
        xyz[a] = (float)(along + s2);
        normal[a] = (float)(n[a] / length);
    }
    const double w0 = (1.0 - r1) - r2;
    for (int a = 0; a < 3; ++a) {
        if (!ca) {
            bgr[a] = 0;
            continue;
        }
        const double ta = w0 * (double)ca[a], tb = r1 * (double)cb[a], tc = r2 * (double)cc[a];
        const double m = floor(((ta + tb) + tc) + 0.5);
        bgr[a] = m >= 255.0 ? (uint8_t)255 : m > 0.0 ? (uint8_t)(int)m : (uint8_t)0;
    }
}

}  // namespace apd_fusion
