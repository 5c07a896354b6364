// The sequential checker of apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score (contract C27): plain loops over
// all faces and all points, no grid search, with the rules of csrc/apd_mesh_nearest_math.h, which the kernels compile too.  Built by
// tests/mesh_nearest_checker.py with the host compiler and -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../apd-mvs_amd/csrc/apd_mesh_nearest_math.h"
#include "../../apd-mvs_amd/csrc/apd_nearest_math.h"

using namespace apd_fusion;

namespace {

struct Corners {
    int32_t id[3];
    float A[3], B[3], C[3];
};

Corners corners_of(const float *xyz, const int32_t *index, long long f)
{
    Corners c;
    for (int k = 0; k < 3; ++k) {
        c.id[k] = index[3 * f + k];
    }
    for (int a = 0; a < 3; ++a) {
        c.A[a] = xyz[3 * (size_t)c.id[0] + a];
        c.B[a] = xyz[3 * (size_t)c.id[1] + a];
        c.C[a] = xyz[3 * (size_t)c.id[2] + a];
    }
    return c;
}

// the faces that can be a candidate at all on this grid
std::vector<char> usable_faces(const float *xyz, long long faces, const int32_t *index, const float *origin, float radius)
{
    std::vector<char> usable((size_t)faces, 0);
    for (long long f = 0; f < faces; ++f) {
        const Corners c = corners_of(xyz, index, f);
        int lo[3], hi[3];
        usable[(size_t)f] = mesh_face_proper(c.id, c.A, c.B, c.C) && mesh_face_on_grid(c.A, c.B, c.C, origin, radius, lo, hi);
    }
    return usable;
}

void nearest(const float *xyz, long long faces, const int32_t *index, long long n, const float *points, float radius, const float *origin,
             float *distance, int32_t *face, float *closest, double *d2_out)
{
    const std::vector<char> usable = usable_faces(xyz, faces, index, origin, radius);
    const double r2 = mesh_nearest_r2(radius);
    for (long long i = 0; i < n; ++i) {
        distance[i] = nearest_no_distance();
        face[i] = kMeshNearestNoFace;
        closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = NAN;
        if (d2_out) {
            d2_out[i] = INFINITY;
        }
        int cell[3];
        if (!radius_cells(points + 3 * i, origin, radius, cell)) {
            continue;
        }
        const double P[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
        bool have = false;
        double best = 0.0, best_x[3] = {0.0, 0.0, 0.0};
        uint32_t best_f = 0;
        for (long long f = 0; f < faces; ++f) {
            if (!usable[(size_t)f]) {
                continue;
            }
            const Corners c = corners_of(xyz, index, f);
            double X[3];
            const double d2 = mesh_closest_point(mesh_face_of(c.A, c.B, c.C), P, X);
            if (d2 <= r2 && mesh_nearest_takes(d2, (uint32_t)f, have, best, best_f)) {
                have = true;
                best = d2;
                best_f = (uint32_t)f;
                best_x[0] = X[0], best_x[1] = X[1], best_x[2] = X[2];
            }
        }
        if (have) {
            distance[i] = mesh_nearest_distance(best);
            face[i] = (int32_t)best_f;
            for (int a = 0; a < 3; ++a) {
                closest[3 * i + a] = (float)best_x[a];
            }
            if (d2_out) {
                d2_out[i] = best;
            }
        }
    }
}

// the finite ones of n distances: contract C12's chunk sums, added ascending
void finite_totals(const float *distance, size_t n, unsigned long long *count, double *sum)
{
    double total = 0.0;
    unsigned long long found = 0;
    for (size_t first = 0; first < n; first += (size_t)kKnnChunk) {
        const size_t m = n - first < (size_t)kKnnChunk ? n - first : (size_t)kKnnChunk;
        double a = 0.0, b = 0.0;
        unsigned f = 0;
        knn_chunk_sums(distance + first, m, a, b, f);
        total = total + a;
        found += f;
    }
    *count = found;
    *sum = total;
}

}  // namespace

extern "C" {

// (cell, face) pairs of the search: what the pair limit is held against
long long mesh_nearest_pairs(const float *xyz, long long faces, const int32_t *index, float radius, const float *origin)
{
    long long pairs = 0;
    for (long long f = 0; f < faces; ++f) {
        const Corners c = corners_of(xyz, index, f);
        int lo[3], hi[3];
        if (mesh_face_proper(c.id, c.A, c.B, c.C) && mesh_face_on_grid(c.A, c.B, c.C, origin, radius, lo, hi)) {
            pairs += (long long)mesh_face_cells(lo, hi);
        }
    }
    return pairs;
}

// The cells face 0 of the mesh is binned into, lo[3] then hi[3], and the cell[3] of `point`: what the grid search rests on, for the test
// that every candidate is met.  Returns 1 when both are on the grid
int mesh_nearest_cells(const float *xyz, const int32_t *index, const float *point, float radius, const float *origin, int *box, int *cell)
{
    const Corners c = corners_of(xyz, index, 0);
    return mesh_face_on_grid(c.A, c.B, c.C, origin, radius, box, box + 3) && radius_cells(point, origin, radius, cell) ? 1 : 0;
}

// d2 (may be null): the binary64 squared distance of the answer, +inf without one
void mesh_nearest(const float *xyz, long long faces, const int32_t *index, long long n, const float *points, float radius, const float *origin,
                  float *distance, int32_t *face, float *closest, double *d2)
{
    nearest(xyz, faces, index, n, points, radius, origin, distance, face, closest, d2);
}

// The samples; with out_xyz null only their number.  bgr null: a mesh without colours
long long mesh_sample_points(const float *xyz, const uint8_t *bgr, long long faces, const int32_t *index, double density, unsigned long long seed,
                             float *out_xyz, float *out_normal, uint8_t *out_bgr, int32_t *out_face)
{
    long long total = 0;
    for (long long f = 0; f < faces; ++f) {
        const Corners c = corners_of(xyz, index, f);
        if (!mesh_face_proper(c.id, c.A, c.B, c.C)) {
            continue;
        }
        const MeshFace face = mesh_face_of(c.A, c.B, c.C);
        double normal[3];
        const double n2 = mesh_face_area2(face, normal);
        const uint32_t n = mesh_sample_count(n2, density, mesh_sample_unit(seed, (uint64_t)f, 0, 0));
        for (uint32_t k = 0; k < n && out_xyz; ++k) {
            const size_t s = (size_t)total + k;
            mesh_sample_point(face, seed, (uint64_t)f, k, bgr ? bgr + 3 * (size_t)c.id[0] : nullptr, bgr ? bgr + 3 * (size_t)c.id[1] : nullptr,
                              bgr ? bgr + 3 * (size_t)c.id[2] : nullptr, out_xyz + 3 * s, out_normal + 3 * s, out_bgr + 3 * s);
            out_face[s] = (int32_t)f;
        }
        total += n;
    }
    return total;
}

// The nine numbers of apd_mesh_score as nine doubles (the counts are exact in them), density > 0
void mesh_score(const float *xyz, long long faces, const int32_t *index, long long nt, const float *truth, float threshold, const float *origin,
                double density, unsigned long long seed, double *out)
{
    const long long ns = mesh_sample_points(xyz, nullptr, faces, index, density, seed, nullptr, nullptr, nullptr, nullptr);
    std::vector<float> s((size_t)ns * 3 + 1), normal((size_t)ns * 3 + 1);
    std::vector<uint8_t> bgr((size_t)ns * 3 + 1);
    std::vector<int32_t> on((size_t)ns + 1);
    mesh_sample_points(xyz, nullptr, faces, index, density, seed, s.data(), normal.data(), bgr.data(), on.data());
    // precision side: contract C17, every pair
    const float r2 = threshold * threshold;
    std::vector<float> dp((size_t)ns + 1), dq((size_t)nt + 1);
    std::vector<int> cells((size_t)nt * 3 + 1);
    std::vector<char> inside((size_t)nt + 1, 0);
    for (long long j = 0; j < nt; ++j) {
        inside[(size_t)j] = radius_cells(truth + 3 * j, origin, threshold, &cells[3 * (size_t)j]);
    }
    for (long long i = 0; i < ns; ++i) {
        dp[(size_t)i] = nearest_no_distance();
        int cell[3];
        if (!radius_cells(&s[3 * (size_t)i], origin, threshold, cell)) {
            continue;
        }
        bool have = false;
        float best = 0.0f;
        uint32_t best_j = 0;
        for (long long j = 0; j < nt; ++j) {
            if (!inside[(size_t)j] || !radius_cells_adjacent(cell, &cells[3 * (size_t)j])) {
                continue;
            }
            const float d2 = radius_d2(&s[3 * (size_t)i], truth + 3 * j);
            if (d2 <= r2 && nearest_takes(d2, (uint32_t)j, have, best, best_j)) {
                have = true;
                best = d2;
                best_j = (uint32_t)j;
            }
        }
        if (have) {
            dp[(size_t)i] = nearest_distance(best);
        }
    }
    std::vector<int32_t> face((size_t)nt + 1);
    std::vector<float> closest((size_t)nt * 3 + 1);
    nearest(xyz, faces, index, nt, truth, threshold, origin, dq.data(), face.data(), closest.data(), nullptr);
    unsigned long long a = 0, b = 0;
    double sum_p = 0.0, sum_q = 0.0;
    finite_totals(dp.data(), (size_t)ns, &a, &sum_p);
    finite_totals(dq.data(), (size_t)nt, &b, &sum_q);
    const NearestScore r = nearest_score((unsigned long long)ns, (unsigned long long)nt, a, b, sum_p, sum_q);
    out[0] = (double)r.n_p, out[1] = (double)r.n_q, out[2] = (double)r.p_within, out[3] = (double)r.q_within;
    out[4] = r.precision, out[5] = r.recall, out[6] = r.fscore, out[7] = r.mean_p, out[8] = r.mean_q;
}

// the number (k, c) of face f: for the count rule's test
double mesh_sample_number(unsigned long long seed, unsigned long long f, unsigned long long k, unsigned long long c) { return mesh_sample_unit(seed, f, k, c); }

}  // extern "C"
