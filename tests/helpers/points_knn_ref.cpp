// points_knn_ref.cpp -- the mean distance to the k nearest neighbours and the statistical removal, as a sequential restatement of
// arithmetic contract C12 in two ways:
//   mode 0, brute: the double loop over all pairs of points, the relation of apd_radius_math.h applied to each, and a full sort of
//                  each point's neighbour distances;
//   mode 1, grid:  a std::map from cell key to the member indices of the cell, 27 lookups per point, and a partial sort.
// The two must agree: the cell condition of the relation makes the 27-cell search the definition, and the k smallest values are a
// multiset.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_knn_mean_distances and apd_points_remove_statistical
// (apd-mvs_amd/csrc/apd_points_knn.hip), compiled by tests/points_knn_checker.py with -ffp-contract=off.  It shares the contract's
// headers with the product (the cell, the key, the squared distance, the score, the chunk sums, the threshold) and nothing else:
// no sort of cells, no scan, no kernel, no LDS.
#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <thread>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_knn_math.h"

namespace {

struct Located {
    bool inside;
    int cell[3];
};

std::vector<Located> locate(long long n, const float *xyz, float radius, const float *origin)
{
    std::vector<Located> where((size_t)n);
    for (long long k = 0; k < n; ++k) {
        where[(size_t)k].inside = apd_fusion::radius_cells(xyz + 3 * k, origin, radius, where[(size_t)k].cell);
    }
    return where;
}

float score_of(const std::vector<float> &ascending, uint32_t k)
{
    return apd_fusion::knn_score([&](unsigned s) { return ascending[s]; }, k);
}

// Points i of [first, n) in steps of `step`: a point's score depends on no other's, so the double loop is shared out to threads
void scores_brute_part(long long first, long long step, long long n, const float *xyz, const std::vector<Located> &where, float r2, uint32_t k,
                       float *scores)
{
    std::vector<float> d2;
    for (long long i = first; i < n; i += step) {
        d2.clear();
        for (long long j = 0; j < n && where[(size_t)i].inside; ++j) {
            if (j != i && where[(size_t)j].inside &&
                apd_fusion::radius_neighbour(xyz + 3 * i, where[(size_t)i].cell, xyz + 3 * j, where[(size_t)j].cell, r2)) {
                d2.push_back(apd_fusion::radius_d2(xyz + 3 * i, xyz + 3 * j));
            }
        }
        std::sort(d2.begin(), d2.end());
        scores[i] = d2.size() >= k ? score_of(d2, k) : apd_fusion::knn_none();
    }
}

void scores_brute(long long n, const float *xyz, const std::vector<Located> &where, float r2, uint32_t k, float *scores)
{
    const long long threads = n < 4096 ? 1 : std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 8);
    std::vector<std::thread> pool;
    for (long long t = 1; t < threads; ++t) {
        pool.emplace_back(scores_brute_part, t, threads, n, xyz, std::cref(where), r2, k, scores);
    }
    scores_brute_part(0, threads, n, xyz, where, r2, k, scores);
    for (std::thread &t : pool) {
        t.join();
    }
}

void scores_grid(long long n, const float *xyz, const std::vector<Located> &where, float r2, uint32_t k, float *scores)
{
    std::map<uint64_t, std::vector<long long>> cells;
    for (long long j = 0; j < n; ++j) {
        if (where[(size_t)j].inside) {
            const int *c = where[(size_t)j].cell;
            cells[apd_fusion::radius_key(c[0], c[1], c[2])].push_back(j);
        }
    }
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    std::vector<float> d2;
    for (long long i = 0; i < n; ++i) {
        d2.clear();
        const int *ci = where[(size_t)i].cell;
        for (int d = 0; d < 27 && where[(size_t)i].inside; ++d) {
            const int x = ci[0] + d % 3 - 1, y = ci[1] + d / 3 % 3 - 1, z = ci[2] + d / 9 - 1;
            if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) {
                continue;
            }
            const auto found = cells.find(apd_fusion::radius_key(x, y, z));
            if (found == cells.end()) {
                continue;
            }
            for (long long j : found->second) {
                if (j != i && apd_fusion::radius_within(xyz + 3 * i, xyz + 3 * j, r2)) {
                    d2.push_back(apd_fusion::radius_d2(xyz + 3 * i, xyz + 3 * j));
                }
            }
        }
        if (d2.size() < k) {
            scores[i] = apd_fusion::knn_none();
            continue;
        }
        std::partial_sort(d2.begin(), d2.begin() + k, d2.end());
        scores[i] = score_of(d2, k);
    }
}

}  // namespace

extern "C" {

// T of contract C12 for n scores in input order; *full: n_f, *s1, *s2: the totals
double knn_threshold_of(long long n, const float *scores, float std_ratio, long long *full, double *s1, double *s2)
{
    double S1 = 0.0, S2 = 0.0;
    unsigned long long n_f = 0;
    for (long long first = 0; first < n; first += apd_fusion::kKnnChunk) {
        const long long count = n - first < apd_fusion::kKnnChunk ? n - first : apd_fusion::kKnnChunk;
        double a = 0.0, b = 0.0;
        unsigned f = 0;
        apd_fusion::knn_chunk_sums(scores + first, (size_t)count, a, b, f);
        S1 = S1 + a;
        S2 = S2 + b;
        n_f += f;
    }
    *full = (long long)n_f;
    *s1 = S1;
    *s2 = S2;
    return apd_fusion::knn_threshold(n_f, S1, S2, std_ratio);
}

// Points j < n with the lists views[offsets[j] .. offsets[j + 1]).  scores: n entries.  kept_index: room for n; the out_* arrays
// have room for n points, out_offsets for n + 1 entries, out_views for offsets[n] entries: the points kept, in input order, with
// their lists.  Returns their number; *removed: the others; *threshold: T.
long long points_knn(int mode, long long n, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                     const int32_t *pixel, const uint32_t *sources, const long long *offsets, const int32_t *views, float radius, const float *origin,
                     uint32_t k, float std_ratio, float *scores, double *threshold, long long *kept_index, float *out_xyz, float *out_normal,
                     uint8_t *out_bgr, uint8_t *out_support, int32_t *out_view, int32_t *out_pixel, uint32_t *out_sources, long long *out_offsets,
                     int32_t *out_views, long long *removed)
{
    const std::vector<Located> where = locate(n, xyz, radius, origin);
    const float r2 = radius * radius;
    (mode == 0 ? scores_brute : scores_grid)(n, xyz, where, r2, k, scores);
    long long full = 0;
    double s1 = 0.0, s2 = 0.0;
    const double T = knn_threshold_of(n, scores, std_ratio, &full, &s1, &s2);
    *threshold = T;
    long long kept = 0, entries = 0;
    out_offsets[0] = 0;
    for (long long j = 0; j < n; ++j) {
        if (!apd_fusion::knn_kept(scores[j], T)) {
            continue;
        }
        kept_index[kept] = j;
        for (int c = 0; c < 3; ++c) {
            out_xyz[3 * kept + c] = xyz[3 * j + c];
            out_normal[3 * kept + c] = normal[3 * j + c];
            out_bgr[3 * kept + c] = bgr[3 * j + c];
        }
        out_support[kept] = support[j];
        out_view[kept] = view[j];
        out_pixel[kept] = pixel[j];
        out_sources[kept] = sources[j];
        for (long long e = offsets[j]; e < offsets[j + 1]; ++e) {
            out_views[entries++] = views[e];
        }
        ++kept;
        out_offsets[kept] = entries;
    }
    *removed = n - kept;
    return kept;
}

}  // extern "C"
