// points_cluster_ref.cpp -- connected components within a radius and the removal of small ones, as a sequential restatement of
// contract C13 in two ways:
//   mode 0, brute: the double loop over all pairs of points, the relation of apd_radius_math.h applied to each, a sequential
//                  union-find (union by index, path compression) over the pairs it holds for;
//   mode 1, grid:  a std::map from cell key to the member indices of the cell, and a breadth-first search from every point not
//                  reached yet, 27 lookups per point taken off the queue.
// The two must agree: the cell condition of the relation makes the 27-cell search the definition.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_components and apd_points_remove_small_components
// (apd-mvs_amd/csrc/apd_points_clusters.hip), compiled by tests/points_cluster_checker.py with -ffp-contract=off.  It shares the
// contract's header with the product (the cell, the key, the squared distance) and nothing else: no sort, no scan, no kernel, no
// atomic.
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

long long find(std::vector<long long> &parent, long long v)
{
    long long r = v;
    while (parent[(size_t)r] != r) {
        r = parent[(size_t)r];
    }
    while (parent[(size_t)v] != r) {
        const long long next = parent[(size_t)v];
        parent[(size_t)v] = r;
        v = next;
    }
    return r;
}

// group[k]: a number that the points of one component share and no others
void group_brute(long long n, const float *xyz, const std::vector<Located> &where, float r2, std::vector<long long> &group)
{
    for (long long k = 0; k < n; ++k) {
        group[(size_t)k] = k;
    }
    for (long long i = 0; i < n; ++i) {
        for (long long j = 0; j < i && where[(size_t)i].inside; ++j) {
            if (where[(size_t)j].inside && apd_fusion::radius_neighbour(xyz + 3 * i, where[(size_t)i].cell, xyz + 3 * j, where[(size_t)j].cell, r2)) {
                const long long a = find(group, i), b = find(group, j);
                if (a != b) {
                    group[(size_t)(a > b ? a : b)] = a > b ? b : a;
                }
            }
        }
    }
    for (long long k = 0; k < n; ++k) {
        group[(size_t)k] = find(group, k);
    }
}

void group_grid(long long n, const float *xyz, const std::vector<Located> &where, float r2, std::vector<long long> &group)
{
    std::map<uint64_t, std::vector<long long>> cells;
    for (long long k = 0; k < n; ++k) {
        group[(size_t)k] = -1;
        if (where[(size_t)k].inside) {
            const int *c = where[(size_t)k].cell;
            cells[apd_fusion::radius_key(c[0], c[1], c[2])].push_back(k);
        }
    }
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    std::vector<long long> queue;
    for (long long start = 0; start < n; ++start) {
        if (group[(size_t)start] >= 0) {
            continue;
        }
        group[(size_t)start] = start;
        queue.assign(1, start);
        for (size_t head = 0; head < queue.size(); ++head) {
            const long long i = queue[head];
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
                    if (group[(size_t)j] < 0 && apd_fusion::radius_within(xyz + 3 * i, xyz + 3 * j, r2)) {
                        group[(size_t)j] = start;
                        queue.push_back(j);
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

// Points k < n with the lists views[offsets[k] .. offsets[k + 1]).  label, size: n entries each; *components: their number.
// kept_index: room for n; the out_* arrays have room for n points, out_offsets for n + 1 entries, out_views for offsets[n]
// entries: the points of the components with at least min_size points, in input order, with their lists.  Returns their number;
// *removed: the others.
long long points_clusters(int mode, long long n, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                          const int32_t *pixel, const uint32_t *sources, const long long *offsets, const int32_t *views, float radius,
                          const float *origin, uint32_t min_size, uint32_t *label, uint32_t *size, long long *components, long long *kept_index,
                          float *out_xyz, float *out_normal, uint8_t *out_bgr, uint8_t *out_support, int32_t *out_view, int32_t *out_pixel,
                          uint32_t *out_sources, long long *out_offsets, int32_t *out_views, long long *removed)
{
    const std::vector<Located> where = locate(n, xyz, radius, origin);
    const float r2 = radius * radius;
    std::vector<long long> group((size_t)n);
    (mode == 0 ? group_brute : group_grid)(n, xyz, where, r2, group);
    // the smallest index and the number of every group, whatever number the mode gave it
    std::map<long long, std::pair<long long, long long>> seen;
    for (long long k = 0; k < n; ++k) {
        auto at = seen.find(group[(size_t)k]);
        if (at == seen.end()) {
            seen[group[(size_t)k]] = {k, 1};
        } else {
            ++at->second.second;
        }
    }
    *components = (long long)seen.size();
    for (long long k = 0; k < n; ++k) {
        const auto &g = seen[group[(size_t)k]];
        label[k] = (uint32_t)g.first;
        size[k] = (uint32_t)g.second;
    }
    long long kept = 0, entries = 0;
    out_offsets[0] = 0;
    for (long long k = 0; k < n; ++k) {
        if (size[k] < min_size) {
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
