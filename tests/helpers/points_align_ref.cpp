// points_align_ref.cpp -- the alignment of one cloud to another and the move of a cloud by a transform, as a sequential
// restatement of arithmetic contract C18, with the search of contract C17 under it in two ways:
//   mode 0, brute: every step's matches by the double loop over all (point of P, point of Q) pairs, the cell condition and the
//                  distance of the relation applied to each;
//   mode 1, grid:  a std::map from cell key to Q's indices of the cell, built once, the 27 cells of a point looked up.
// The two must agree in every bit of every field.  The sums are taken as the contract words them: an array of 256 slots per
// chunk and per sum, +0.0 where a point is unmatched or past the end, and the tree over it (align_tree); the chunk sums added
// ascending.  The positions of step k > 0 are X_0 moved by the total.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_align and apd_points_transformed (apd-mvs_amd/csrc/apd_points_align.hip),
// compiled by tests/points_align_checker.py with -ffp-contract=off.  It shares the contract's headers with the product (the terms,
// the tree, the solve, the composition, the stopping rule, the move; the cell, the key, the distance and the rule for ties of the
// search) and nothing else: no sort of cells, no kernel, no shuffle.
#include <algorithm>
#include <cstdint>
#include <map>
#include <thread>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_align_math.h"
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

// The totals of `width` sums over the points at x with the matches `index`; terms(P, Q, v) gives a matched point's
template <typename Terms> void totals(const std::vector<float> &x, const std::vector<int32_t> &index, const float *q, int width, Terms &&terms, double *total)
{
    const size_t n = index.size();
    for (int j = 0; j < width; ++j) {
        total[j] = 0.0;
    }
    for (size_t first = 0; first < n; first += apd_fusion::kKnnChunk) {
        double slots[apd_fusion::kAlignSums2][apd_fusion::kKnnChunk];
        for (int s = 0; s < apd_fusion::kKnnChunk; ++s) {
            double v[apd_fusion::kAlignSums2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const size_t k = first + (size_t)s;
            if (k < n && index[k] >= 0) {
                terms(x.data() + 3 * k, q + 3 * (size_t)index[k], v);
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

// out: apd_fusion::Alignment; rms (may be null): rms_k of every search made, 65 entries at most, and *searches their number
int points_align(int mode, long long n_p, const float *p, long long n_q, const float *q, float radius, const float *origin, unsigned iterations,
                 double tolerance, int with_scale, apd_fusion::Alignment *out, double *rms, int *searches)
{
    *out = apd_fusion::align_identity();
    if (searches) {
        *searches = 0;
    }
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
        totals(x, index, q, apd_fusion::kAlignSums1, [](const float *P, const float *Q, double *v) { apd_fusion::align_terms1(P, Q, v); }, s);
        if (rms && searches) {
            rms[(*searches)++] = apd_fusion::align_rms(s[7], s[0]);
        }
        return 0;
    };
    const auto pass2 = [&](const double mean[6], double *s) {
        totals(x, index, q, apd_fusion::kAlignSums2, [&](const float *P, const float *Q, double *v) { apd_fusion::align_terms2(P, Q, mean, v); }, s);
        return 0;
    };
    return apd_fusion::align_run(iterations, tolerance, with_scale != 0, pass1, pass2, *out);
}

// One step's solve from given pairs: the step (scale, R, t) of the n pairs (p_i, q_i), all matched, its quaternion (w, x, y, z)
// and the Jacobi sweeps it took
void points_align_solve_pairs(long long n, const float *p, const float *q, int with_scale, double *scale, double *rotation9, double *translation3,
                              double *quaternion4, unsigned *sweeps)
{
    const std::vector<float> x(p, p + 3 * n);
    std::vector<float> y(q, q + 3 * n);
    std::vector<int32_t> index((size_t)n);
    for (long long i = 0; i < n; ++i) {
        index[(size_t)i] = (int32_t)i;
    }
    double s1[apd_fusion::kAlignSums1], s2[apd_fusion::kAlignSums2];
    totals(x, index, y.data(), apd_fusion::kAlignSums1, [](const float *P, const float *Q, double *v) { apd_fusion::align_terms1(P, Q, v); }, s1);
    const double m = s1[0];
    const double mean[6] = {s1[1] / m, s1[2] / m, s1[3] / m, s1[4] / m, s1[5] / m, s1[6] / m};
    totals(x, index, y.data(), apd_fusion::kAlignSums2, [&](const float *P, const float *Q, double *v) { apd_fusion::align_terms2(P, Q, mean, v); }, s2);
    const apd_fusion::AlignTransform step = apd_fusion::align_solve(mean, s2, with_scale != 0, sweeps, quaternion4);
    *scale = step.scale;
    std::copy(step.R, step.R + 9, rotation9);
    std::copy(step.t, step.t + 3, translation3);
}

// xyz and normal (n points each) moved as apd_points_transformed moves them
void points_transformed(long long n, const float *xyz, const float *normal, double scale, const double *rotation9, const double *translation3,
                        float *out_xyz, float *out_normal)
{
    apd_fusion::AlignTransform by;
    by.scale = scale;
    std::copy(rotation9, rotation9 + 9, by.R);
    std::copy(translation3, translation3 + 3, by.t);
    const apd_fusion::AlignMove positions = apd_fusion::align_move_of(by, true), normals = apd_fusion::align_move_of(by, false);
    for (long long i = 0; i < n; ++i) {
        apd_fusion::align_moved(positions, xyz + 3 * i, out_xyz + 3 * i);
        apd_fusion::align_moved(normals, normal + 3 * i, out_normal + 3 * i);
    }
}

}  // extern "C"
