// points_normals_ref.cpp -- normals and surface variation from each point's neighbourhood, as a sequential restatement of arithmetic
// contract C14 in two ways:
//   mode 0, brute: the double loop over all pairs of points, the relation of apd_radius_math.h applied to each, and a sort of each
//                  point's terms (itself and its neighbours) by (cell key, input index);
//   mode 1, grid:  a std::map from cell key to the member indices of the cell in input order, the 27 cells of a point looked up
//                  in ascending key order, the point's own term where that order meets it.
// The two must agree bit for bit: the cell condition of the relation makes the 27-cell search the definition, and the order of the
// binary64 sums is the same ascending (cell key, input index) in both.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_estimate_normals and apd_points_with_estimated_normals
// (apd-mvs_amd/csrc/apd_points_normals.hip), compiled by tests/points_normals_checker.py with -ffp-contract=off.  It shares the
// contract's headers with the product (the cell, the key, the squared distance, the sums, the solve) and nothing else: no sort of
// cells, no scan, no kernel.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_normal_math.h"

namespace {

struct Located {
    bool inside;
    int cell[3];
    uint64_t key;
};

std::vector<Located> locate(long long n, const float *xyz, float radius, const float *origin)
{
    std::vector<Located> where((size_t)n);
    for (long long k = 0; k < n; ++k) {
        Located &w = where[(size_t)k];
        w.inside = apd_fusion::radius_cells(xyz + 3 * k, origin, radius, w.cell);
        w.key = w.inside ? apd_fusion::radius_key(w.cell[0], w.cell[1], w.cell[2]) : 0;
    }
    return where;
}

struct Out {
    float *normal, *variation;
    uint32_t *sweeps;
    uint8_t *estimated, *capped;
};

// Point i from its terms in order: `terms` holds the indices of the point itself and its neighbours
void finish(long long i, const std::vector<long long> &terms, const float *xyz, const float *stored, uint32_t min_neighbours, const Out &out)
{
    for (int a = 0; a < 3; ++a) {
        memcpy(out.normal + 3 * i + a, stored + 3 * i + a, sizeof(float));  // bit for bit, a NaN's payload too
    }
    out.variation[i] = apd_fusion::normal_none();
    out.sweeps[i] = 0;
    out.estimated[i] = 0;
    out.capped[i] = 0;
    if (terms.empty() || terms.size() - 1 < min_neighbours) {
        return;
    }
    apd_fusion::NormalSums sums;
    for (long long j : terms) {
        apd_fusion::normal_add(sums, xyz + 3 * i, xyz + 3 * j);
    }
    unsigned sweeps = 0;
    bool capped = false;
    apd_fusion::normal_solve(sums, stored + 3 * i, out.normal + 3 * i, out.variation[i], sweeps, capped);
    out.sweeps[i] = sweeps;
    out.estimated[i] = 1;
    out.capped[i] = capped ? 1 : 0;
}

// Points i of [first, n) in steps of `step`: a point's estimate depends on no other's, so the double loop is shared out to threads
void brute_part(long long first, long long step, long long n, const float *xyz, const float *stored, const std::vector<Located> &where, float r2,
                uint32_t min_neighbours, const Out &out)
{
    std::vector<std::pair<uint64_t, long long>> found;
    std::vector<long long> terms;
    for (long long i = first; i < n; i += step) {
        found.clear();
        terms.clear();
        for (long long j = 0; j < n && where[(size_t)i].inside; ++j) {
            if (j == i || (where[(size_t)j].inside &&
                           apd_fusion::radius_neighbour(xyz + 3 * i, where[(size_t)i].cell, xyz + 3 * j, where[(size_t)j].cell, r2))) {
                found.emplace_back(where[(size_t)j].key, j);
            }
        }
        std::sort(found.begin(), found.end());
        for (const auto &f : found) {
            terms.push_back(f.second);
        }
        finish(i, terms, xyz, stored, min_neighbours, out);
    }
}

void brute(long long n, const float *xyz, const float *stored, const std::vector<Located> &where, float r2, uint32_t min_neighbours, const Out &out)
{
    const long long threads = n < 4096 ? 1 : std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 8);
    std::vector<std::thread> pool;
    for (long long t = 1; t < threads; ++t) {
        pool.emplace_back(brute_part, t, threads, n, xyz, stored, std::cref(where), r2, min_neighbours, std::cref(out));
    }
    brute_part(0, threads, n, xyz, stored, where, r2, min_neighbours, out);
    for (std::thread &t : pool) {
        t.join();
    }
}

void grid(long long n, const float *xyz, const float *stored, const std::vector<Located> &where, float r2, uint32_t min_neighbours, const Out &out)
{
    std::map<uint64_t, std::vector<long long>> cells;
    for (long long j = 0; j < n; ++j) {
        if (where[(size_t)j].inside) {
            cells[where[(size_t)j].key].push_back(j);
        }
    }
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    std::vector<long long> terms;
    for (long long i = 0; i < n; ++i) {
        terms.clear();
        const int *ci = where[(size_t)i].cell;
        for (int d = 0; d < 27 && where[(size_t)i].inside; ++d) {  // x fastest, then y, then z: ascending keys
            const int x = ci[0] + d % 3 - 1, y = ci[1] + d / 3 % 3 - 1, z = ci[2] + d / 9 - 1;
            if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) {
                continue;
            }
            const auto found = cells.find(apd_fusion::radius_key(x, y, z));
            if (found == cells.end()) {
                continue;
            }
            for (long long j : found->second) {
                if (j == i || apd_fusion::radius_within(xyz + 3 * i, xyz + 3 * j, r2)) {
                    terms.push_back(j);
                }
            }
        }
        finish(i, terms, xyz, stored, min_neighbours, out);
    }
}

}  // namespace

extern "C" {

unsigned points_normals_sweep_cap() { return apd_fusion::kNormalSweepCap; }

// Points j < n at xyz with the stored normals `stored`: normal (3 n), variation, sweeps, estimated, capped (n each).  Returns the
// number of points with an estimate.
long long points_normals(int mode, long long n, const float *xyz, const float *stored, float radius, const float *origin, uint32_t min_neighbours,
                         float *normal, float *variation, uint32_t *sweeps, uint8_t *estimated, uint8_t *capped)
{
    const std::vector<Located> where = locate(n, xyz, radius, origin);
    const float r2 = radius * radius;
    const Out out = {normal, variation, sweeps, estimated, capped};
    (mode == 0 ? brute : grid)(n, xyz, stored, where, r2, min_neighbours, out);
    long long count = 0;
    for (long long j = 0; j < n; ++j) {
        count += estimated[j];
    }
    return count;
}

}  // extern "C"
