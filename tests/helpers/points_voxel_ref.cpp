// points_voxel_ref.cpp -- the voxel-grid merge of a point cloud with the union of the members' visibility lists, as a sequential
// restatement of arithmetic contract C10: the cell and the key of every point, std::stable_sort on (key, index), one
// loop per cell over its members in that order, std::set for the union of their lists.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_merge_voxels (apd-mvs_amd/csrc/apd_points_merge.hip), compiled by
// tests/points_voxel_checker.py with -ffp-contract=off.  It takes nothing from the product: the cell, the key, the sums, the
// renormalisation and the colour rounding are all written out here, and neither the product's sort nor its merge is called.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

extern "C" {

// Points k < n with the lists views[offsets[k] .. offsets[k + 1]).  The out_* arrays have room for n points, out_offsets for n + 1
// entries, out_views for offsets[n] entries.  Returns the number of cells; *dropped: the points without a cell.
long long points_voxel(long long n, const float *xyz, const float *normal, const uint8_t *bgr, const int32_t *view, const int32_t *pixel,
                       const uint32_t *sources, const long long *offsets, const int32_t *views, float voxel_size, const float *origin,
                       float *out_xyz, float *out_normal, uint8_t *out_bgr, uint8_t *out_support, int32_t *out_view, int32_t *out_pixel,
                       uint32_t *out_sources, long long *out_offsets, int32_t *out_views, long long *dropped)
{
    std::vector<std::pair<uint64_t, long long>> kept;  // (key, input index)
    *dropped = 0;
    for (long long k = 0; k < n; ++k) {
        uint64_t biased[3];
        bool in_range = true;
        for (int c = 0; c < 3; ++c) {
            const float difference = xyz[3 * k + c] - origin[c];
            const float t = difference / voxel_size;
            const float f = floorf(t);
            if (f >= -1048576.0f && f < 1048576.0f) {
                biased[c] = (uint64_t)((long long)f + 1048576);
            } else {  // too far out, infinite or NaN
                in_range = false;
            }
        }
        if (!in_range) {
            *dropped += 1;
            continue;
        }
        kept.push_back({(biased[2] << 42) | (biased[1] << 21) | biased[0], k});
    }
    std::stable_sort(kept.begin(), kept.end(),
                     [](const std::pair<uint64_t, long long> &a, const std::pair<uint64_t, long long> &b) { return a.first < b.first; });
    long long cells = 0, entries = 0;
    out_offsets[0] = 0;
    for (size_t first = 0; first < kept.size();) {
        size_t end = first;
        while (end < kept.size() && kept[end].first == kept[first].first) {
            ++end;
        }
        const long long r = kept[first].second;  // the representative
        float sum_p[3], sum_n[3];
        uint64_t sum_c[3];
        for (int c = 0; c < 3; ++c) {
            sum_p[c] = xyz[3 * r + c];
            sum_n[c] = normal[3 * r + c];
            sum_c[c] = bgr[3 * r + c];
        }
        std::set<int32_t> seen(views + offsets[r], views + offsets[r + 1]);
        for (size_t e = first + 1; e < end; ++e) {
            const long long k = kept[e].second;
            for (int c = 0; c < 3; ++c) {
                sum_p[c] = sum_p[c] + xyz[3 * k + c];
                sum_n[c] = sum_n[c] + normal[3 * k + c];
                sum_c[c] = sum_c[c] + bgr[3 * k + c];
            }
            seen.insert(views + offsets[k], views + offsets[k + 1]);
        }
        const uint64_t m = end - first;
        const float count = (float)m;
        float t[3];
        for (int c = 0; c < 3; ++c) {
            out_xyz[3 * cells + c] = sum_p[c] / count;
            t[c] = sum_n[c] / count;
            out_bgr[3 * cells + c] = (uint8_t)((sum_c[c] + m / 2) / m);
        }
        const float squares = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        const float len = sqrtf(squares);
        for (int c = 0; c < 3; ++c) {
            out_normal[3 * cells + c] = len > 0.0f ? t[c] / len : 0.0f;
        }
        out_view[cells] = view[r];
        out_pixel[cells] = pixel[r];
        out_sources[cells] = sources[r];
        for (int32_t v : seen) {  // ascending
            out_views[entries++] = v;
        }
        const long long others = (long long)seen.size() - 1;
        out_support[cells] = (uint8_t)(others < 255 ? others : 255);
        ++cells;
        out_offsets[cells] = entries;
        first = end;
    }
    return cells;
}

}  // extern "C"
