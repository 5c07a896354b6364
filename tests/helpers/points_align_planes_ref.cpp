// points_align_planes_ref.cpp -- the alignment of one cloud to another cloud's tangent planes, as a sequential restatement of
// arithmetic contract C20, with the search of contract C17 under it in two ways:
//   mode 0, brute: every step's matches by the double loop over all (point of P, point of Q) pairs, the cell condition and the
//                  distance of the relation applied to each;
//   mode 1, grid:  a std::map from cell key to Q's indices of the cell, built once, the 27 cells of a point looked up.
// The two must agree in every bit of every field.  The sums are taken as the contract words them: an array of 256 slots per
// chunk and per sum, +0.0 where a point is unmatched, unusable or past the end, and the tree over it (align_tree); the chunk
// sums added ascending.  The positions of step k > 0 are X_0 moved by the total.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_align_planes (apd-mvs_amd/csrc/apd_points_align_planes.hip), compiled by
// tests/points_align_planes_checker.py with -ffp-contract=off.  It shares the contract's headers with the product (the terms, the
// tree, the solve, the composition, the stopping rule, the move; the cell, the key, the distance and the rule for ties of the
// search) and nothing else: no sort of cells, no kernel, no shuffle.
#include <algorithm>
#include <cstdint>
#include <map>
#include <thread>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_align_math.h"
#include "../../apd-mvs_amd/csrc/apd_align_plane_math.h"
#include "../../apd-mvs_amd/csrc/apd_nearest_math.h"

namespace {

struct Located {
    bool inside;
    int cell[3];
};

using Cells = std::map<uint64_t, std::vector<long long>>;

Located locate(const float *at, float radius, const float *origin)
{
    Located w;
    w.inside = apd_fusion::radius_cells(at, origin, radius, w.cell);
    return w;
}

struct Target {
    long long n;
    const float *xyz;
    std::vector<Located> where;
    Cells cells;  // mode 1
};

// The index in q of the match of the point at P, -1 without one
int32_t match_of(int mode, const float *P, const Target &q, float radius, const float *origin)
{
    const Located w = locate(P, radius, origin);
    const float r2 = radius * radius;
    bool have = false;
    float best = 0.0f;
    uint32_t best_j = 0;
    const auto offer = [&](long long j) {
        const float d = apd_fusion::radius_d2(P, q.xyz + 3 * j);
        if (d <= r2 && apd_fusion::nearest_takes(d, (uint32_t)j, have, best, best_j)) {
            have = true;
            best = d;
            best_j = (uint32_t)j;
        }
    };
    if (w.inside && mode == 0) {
        for (long long j = 0; j < q.n; ++j) {
            if (q.where[(size_t)j].inside && apd_fusion::radius_cells_adjacent(w.cell, q.where[(size_t)j].cell)) {
                offer(j);
            }
        }
    } else if (w.inside) {
        const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
        for (int d = 0; d < 27; ++d) {
            const int x = w.cell[0] + d % 3 - 1, y = w.cell[1] + d / 3 % 3 - 1, z = w.cell[2] + d / 9 - 1;
            if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) {
                continue;
            }
            const auto found = q.cells.find(apd_fusion::radius_key(x, y, z));
            if (found != q.cells.end()) {
                for (long long j : found->second) {
                    offer(j);
                }
            }
        }
    }
    return have ? (int32_t)best_j : apd_fusion::kNearestNoIndex;
}

void match_all(int mode, const std::vector<float> &x, const Target &q, float radius, const float *origin, std::vector<int32_t> &index)
{
    const long long n = (long long)index.size();
    const long long threads = n < 4096 ? 1 : std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 8);
    const auto part = [&](long long first) {
        for (long long i = first; i < n; i += threads) {
            index[(size_t)i] = match_of(mode, x.data() + 3 * i, q, radius, origin);
        }
    };
    std::vector<std::thread> pool;
    for (long long t = 1; t < threads; ++t) {
        pool.emplace_back(part, t);
    }
    part(0);
    for (std::thread &t : pool) {
        t.join();
    }
}

// The totals of `width` sums over the n points at x with the matches `index`; terms(k, j, v) fills a matched point's (v is zeros)
template <typename Terms> void totals(const std::vector<int32_t> &index, int width, Terms &&terms, double *total)
{
    const size_t n = index.size();
    for (int j = 0; j < width; ++j) {
        total[j] = 0.0;
    }
    for (size_t first = 0; first < n; first += apd_fusion::kKnnChunk) {
        double slots[apd_fusion::kAlignPlaneSums][apd_fusion::kKnnChunk];
        for (int s = 0; s < apd_fusion::kKnnChunk; ++s) {
            double v[apd_fusion::kAlignPlaneSums] = {};
            const size_t k = first + (size_t)s;
            if (k < n && index[k] >= 0) {
                terms(k, (size_t)index[k], v);
            }
            for (int j = 0; j < width; ++j) {
                slots[j][s] = v[j];
            }
        }
        for (int j = 0; j < width; ++j) {
            total[j] = total[j] + apd_fusion::align_tree(slots[j]);
        }
    }
}

}  // namespace

extern "C" {

// out: apd_fusion::PlaneAlignment
int points_align_planes(int mode, long long n_p, const float *p, long long n_q, const float *q, const float *normal, float radius, const float *origin,
                        unsigned iterations, double tolerance, apd_fusion::PlaneAlignment *out)
{
    *out = apd_fusion::align_plane_identity();
    if (n_p == 0 || n_q == 0) {
        return 0;
    }
    Target target = {n_q, q, {}, {}};
    for (long long j = 0; j < n_q; ++j) {
        const Located w = locate(q + 3 * j, radius, origin);
        target.where.push_back(w);
        if (w.inside && mode != 0) {
            target.cells[apd_fusion::radius_key(w.cell[0], w.cell[1], w.cell[2])].push_back(j);
        }
    }
    const std::vector<float> own(p, p + 3 * n_p);
    std::vector<float> x = own;
    std::vector<int32_t> index((size_t)n_p);
    const auto pass1 = [&](unsigned k, const apd_fusion::AlignTransform &total, double *s) {
        if (k > 0) {
            const apd_fusion::AlignMove by = apd_fusion::align_move_of(total, true);
            for (long long i = 0; i < n_p; ++i) {
                apd_fusion::align_moved(by, own.data() + 3 * i, x.data() + 3 * i);
            }
        }
        match_all(mode, x, target, radius, origin, index);
        totals(index, apd_fusion::kAlignSums1, [&](size_t at, size_t j, double *v) { apd_fusion::align_terms1(x.data() + 3 * at, q + 3 * j, v); }, s);
        return 0;
    };
    const auto pass2 = [&](const double centre[3], double *s) {
        totals(index, apd_fusion::kAlignPlaneSums,
               [&](size_t at, size_t j, double *v) { apd_fusion::align_plane_terms(x.data() + 3 * at, q + 3 * j, normal + 3 * j, centre, v); }, s);
        return 0;
    };
    return apd_fusion::align_plane_run(iterations, tolerance, pass1, pass2, *out);
}

// The thirty sums of pass 2 over the n pairs (p_i, q_i) with the normals n_i, all matched, about the mean of the q_i as pass 1
// gives it; centre3: that mean
void points_align_planes_sums(long long n, const float *p, const float *q, const float *normal, double *centre3, double *sums30)
{
    std::vector<int32_t> index((size_t)n);
    for (long long i = 0; i < n; ++i) {
        index[(size_t)i] = (int32_t)i;
    }
    double s1[apd_fusion::kAlignSums1];
    totals(index, apd_fusion::kAlignSums1, [&](size_t at, size_t j, double *v) { apd_fusion::align_terms1(p + 3 * at, q + 3 * j, v); }, s1);
    for (int a = 0; a < 3; ++a) {
        centre3[a] = s1[0] > 0.0 ? s1[4 + a] / s1[0] : 0.0;
    }
    totals(index, apd_fusion::kAlignPlaneSums,
           [&](size_t at, size_t j, double *v) { apd_fusion::align_plane_terms(p + 3 * at, q + 3 * j, normal + 3 * j, centre3, v); }, sums30);
}

// One step's solve from given sums: z, the six pivots d_j, the step (R, t); returns whether the geometry is degenerate
int points_align_planes_solve(const double *centre3, const double *sums30, double *z6, double *d6, double *rotation9, double *translation3)
{
    const apd_fusion::AlignPlaneSolve solved = apd_fusion::align_plane_solve(centre3, sums30);
    std::copy(solved.z, solved.z + 6, z6);
    std::copy(solved.d, solved.d + 6, d6);
    std::copy(solved.step.R, solved.step.R + 9, rotation9);
    std::copy(solved.step.t, solved.step.t + 3, translation3);
    return solved.degenerate ? 1 : 0;
}

}  // extern "C"
