// points_smooth_ref.cpp -- positions smoothed by projection on each neighbourhood's weighted plane, as a sequential restatement of
// arithmetic contract C16 in two ways:
//   mode 0, brute: the double loop over all pairs of points, the relation of apd_radius_math.h applied to each, and a sort of each
//                  point's terms (itself and its neighbours) by (cell key, input index);
//   mode 1, grid:  a std::map from cell key to the member indices of the cell in input order, the 27 cells of a point looked up
//                  in ascending key order, the point's own term where that order meets it;
//                  a point's result depends on no other's, so both modes share the points out to threads.
// The two must agree bit for bit: the cell condition of the relation makes the 27-cell search the definition, and the order of the
// binary64 sums is the same ascending (cell key, input index) in both.  Iterations are simultaneous: every point of iteration k
// is computed from the positions after iteration k - 1, located anew.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_smoothed_positions and apd_points_with_smoothed_positions
// (apd-mvs_amd/csrc/apd_points_smooth.hip), compiled by tests/points_smooth_checker.py with -ffp-contract=off.  It shares the
// contract's headers with the product (the cell, the key, the squared distance, the weight, the sums, the solve, the projection)
// and nothing else: no sort of cells, no scan, no kernel.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_smooth_math.h"

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

// One iteration's results
struct Out {
    float *smoothed, *offset, *normal;
    uint32_t *sweeps;
    uint8_t *estimated, *capped;
};

// Point i from its terms in order: `terms` holds the indices of the point itself and its neighbours
void finish(long long i, const std::vector<long long> &terms, const float *xyz, const float *stored, float r2, uint32_t min_neighbours, const Out &out)
{
    memcpy(out.smoothed + 3 * i, xyz + 3 * i, 3 * sizeof(float));  // bit for bit, a NaN's payload too
    out.offset[i] = apd_fusion::smooth_none();
    memcpy(out.normal + 3 * i, stored + 3 * i, 3 * sizeof(float));
    out.sweeps[i] = 0;
    out.estimated[i] = 0;
    out.capped[i] = 0;
    if (terms.empty() || terms.size() - 1 < min_neighbours) {
        return;
    }
    apd_fusion::NormalSums sums;
    for (long long j : terms) {
        apd_fusion::smooth_add(sums, xyz + 3 * i, xyz + 3 * j, r2);
    }
    unsigned sweeps = 0;
    bool capped = false;
    apd_fusion::smooth_project(sums, stored + 3 * i, xyz + 3 * i, out.smoothed + 3 * i, out.offset[i], out.normal + 3 * i, sweeps, capped);
    out.sweeps[i] = sweeps;
    out.estimated[i] = 1;
    out.capped[i] = capped ? 1 : 0;
}

// Points i of [first, n) in steps of `step`: a point's result depends on no other's, so the double loop is shared out to threads
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
        finish(i, terms, xyz, stored, r2, min_neighbours, out);
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

using Cells = std::map<uint64_t, std::vector<long long>>;

// Points i of [first, n) in steps of `step`, like brute_part
void grid_part(long long first, long long step, long long n, const float *xyz, const float *stored, const std::vector<Located> &where, const Cells &cells,
               float r2, uint32_t min_neighbours, const Out &out)
{
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    std::vector<long long> terms;
    for (long long i = first; i < n; i += step) {
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
        finish(i, terms, xyz, stored, r2, min_neighbours, out);
    }
}

void grid(long long n, const float *xyz, const float *stored, const std::vector<Located> &where, float r2, uint32_t min_neighbours, const Out &out)
{
    Cells cells;
    for (long long j = 0; j < n; ++j) {
        if (where[(size_t)j].inside) {
            cells[where[(size_t)j].key].push_back(j);
        }
    }
    const long long threads = n < 4096 ? 1 : std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 8);
    std::vector<std::thread> pool;
    for (long long t = 1; t < threads; ++t) {
        pool.emplace_back(grid_part, t, threads, n, xyz, stored, std::cref(where), std::cref(cells), r2, min_neighbours, std::cref(out));
    }
    grid_part(0, threads, n, xyz, stored, where, cells, r2, min_neighbours, out);
    for (std::thread &t : pool) {
        t.join();
    }
}

}  // namespace

extern "C" {

unsigned points_smooth_max_iterations() { return apd_fusion::kSmoothMaxIterations; }

// Points j < n at xyz with the stored normals `stored`, `iterations` >= 1 times: smoothed (3 n) the positions after the last
// iteration; offset, sweeps, estimated, capped (n each) and normal (3 n: the weighted plane's, the stored one where there is no
// estimate) those of the last iteration; ever (n): estimated in at least one iteration.  Returns `moved`, the number of points with ever[j] set.
long long points_smooth(int mode, long long n, const float *xyz, const float *stored, float radius, const float *origin, uint32_t min_neighbours,
                        uint32_t iterations, float *smoothed, float *offset, float *normal, uint32_t *sweeps, uint8_t *estimated, uint8_t *capped, uint8_t *ever)
{
    const float r2 = radius * radius;
    std::vector<float> from(xyz, xyz + 3 * n), to((size_t)(3 * n));
    std::fill(ever, ever + n, (uint8_t)0);
    for (uint32_t k = 0; k < iterations; ++k) {
        const Out out = {to.data(), offset, normal, sweeps, estimated, capped};
        const std::vector<Located> where = locate(n, from.data(), radius, origin);
        (mode == 0 ? brute : grid)(n, from.data(), stored, where, r2, min_neighbours, out);
        for (long long j = 0; j < n; ++j) {
            ever[j] |= estimated[j];
        }
        from.swap(to);  // what was computed is what the next iteration reads
    }
    if (n > 0) {
        memcpy(smoothed, from.data(), (size_t)(3 * n) * sizeof(float));
    }
    long long moved = 0;
    for (long long j = 0; j < n; ++j) {
        moved += ever[j];
    }
    return moved;
}

}  // extern "C"
