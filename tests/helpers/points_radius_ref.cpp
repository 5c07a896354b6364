// points_radius_ref.cpp -- neighbours within a radius and the removal of sparse points, as a sequential restatement of arithmetic
// contract C11 in two ways:
//   mode 0, brute: the double loop over all pairs of points, the relation of apd_radius_math.h applied to each;
//   mode 1, grid:  a std::map from cell key to the member indices of the cell, 27 lookups per point.
// The two must agree: the cell condition of the relation makes the 27-cell search the definition.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_neighbour_counts and apd_points_remove_sparse
// (apd-mvs_amd/csrc/apd_points_radius.hip), compiled by tests/points_radius_checker.py with -ffp-contract=off.  It shares the
// contract's header with the product (the cell, the key, the squared distance) and nothing else: no sort, no scan, no kernel.
#include <cstdint>
#include <map>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_radius_math.h"

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

void count_brute(long long n, const float *xyz, const std::vector<Located> &where, float r2, uint32_t cap, uint32_t *counts)
{
    for (long long i = 0; i < n; ++i) {
        uint64_t c = 0;
        for (long long j = 0; j < n && where[(size_t)i].inside; ++j) {
            if (j != i && where[(size_t)j].inside &&
                apd_fusion::radius_neighbour(xyz + 3 * i, where[(size_t)i].cell, xyz + 3 * j, where[(size_t)j].cell, r2)) {
                ++c;
            }
        }
        counts[i] = (uint32_t)(cap != 0 && c > cap ? cap : c);
    }
}

void count_grid(long long n, const float *xyz, const std::vector<Located> &where, float r2, uint32_t cap, uint32_t *counts)
{
    std::map<uint64_t, std::vector<long long>> cells;
    for (long long k = 0; k < n; ++k) {
        if (where[(size_t)k].inside) {
            const int *c = where[(size_t)k].cell;
            cells[apd_fusion::radius_key(c[0], c[1], c[2])].push_back(k);
        }
    }
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    for (long long i = 0; i < n; ++i) {
        uint64_t c = 0;
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
                    ++c;
                }
            }
        }
        counts[i] = (uint32_t)(cap != 0 && c > cap ? cap : c);
    }
}

}  // namespace

extern "C" {

// Points k < n with the lists views[offsets[k] .. offsets[k + 1]).  counts: n entries, min(neighbours, cap), cap == 0: no cap.
// kept_index: room for n; the out_* arrays have room for n points, out_offsets for n + 1 entries, out_views for offsets[n]
// entries: the points with at least min_neighbours neighbours, in input order, with their lists.  Returns their number;
// *removed: the others.
long long points_radius(int mode, long long n, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                        const int32_t *pixel, const uint32_t *sources, const long long *offsets, const int32_t *views, float radius,
                        const float *origin, uint32_t cap, uint32_t min_neighbours, uint32_t *counts, long long *kept_index, float *out_xyz,
                        float *out_normal, uint8_t *out_bgr, uint8_t *out_support, int32_t *out_view, int32_t *out_pixel, uint32_t *out_sources,
                        long long *out_offsets, int32_t *out_views, long long *removed)
{
    const std::vector<Located> where = locate(n, xyz, radius, origin);
    const float r2 = radius * radius;
    std::vector<uint32_t> uncapped((size_t)n);
    (mode == 0 ? count_brute : count_grid)(n, xyz, where, r2, 0, uncapped.data());
    for (long long k = 0; k < n; ++k) {
        counts[k] = cap != 0 && uncapped[(size_t)k] > cap ? cap : uncapped[(size_t)k];
    }
    long long kept = 0, entries = 0;
    out_offsets[0] = 0;
    for (long long k = 0; k < n; ++k) {
        if (uncapped[(size_t)k] < min_neighbours) {
            continue;
        }
        kept_index[kept] = k;
        for (int c = 0; c < 3; ++c) {
            out_xyz[3 * kept + c] = xyz[3 * k + c];
            out_normal[3 * kept + c] = normal[3 * k + c];
            out_bgr[3 * kept + c] = bgr[3 * k + c];
        }
        out_support[kept] = support[k];
        out_view[kept] = view[k];
        out_pixel[kept] = pixel[k];
        out_sources[kept] = sources[k];
        for (long long e = offsets[k]; e < offsets[k + 1]; ++e) {
            out_views[entries++] = views[e];
        }
        ++kept;
        out_offsets[kept] = entries;
    }
    *removed = n - kept;
    return kept;
}

}  // extern "C"
