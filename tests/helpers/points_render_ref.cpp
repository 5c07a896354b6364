// points_render_ref.cpp -- the z-buffered rendering of a cloud into a camera and the visibility lists that follow from it, as a
// sequential restatement of arithmetic contract C15: a loop over the points in index order and over the pixels of each
// footprint that keeps the smaller key in a plain array, then the resolve; for the lists a loop over the cameras, then over the points.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_render and apd_points_rendered_visibility
// (apd-mvs_amd/csrc/apd_points_render.hip), compiled by tests/points_render_checker.py with -ffp-contract=off.  It shares the
// contract's header with the product (the projection, the draw rule, the key, the seen test) and nothing else: no threads, no
// atomics, no shortcut.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_render_math.h"

namespace {

// camera: K (9), R (9), t (3); the centre is not read by the projection
apd_fusion::View view_of(const float *camera, int width, int height)
{
    apd_fusion::View v;
    memset(&v, 0, sizeof(v));
    memcpy(v.K, camera, sizeof(v.K));
    memcpy(v.R, camera + 9, sizeof(v.R));
    memcpy(v.t, camera + 18, sizeof(v.t));
    v.rows = height;
    v.cols = width;
    return v;
}

std::vector<uint64_t> key_image(long long n, const float *xyz, const apd_fusion::View &view, int splat)
{
    std::vector<uint64_t> keys((size_t)view.rows * (size_t)view.cols, apd_fusion::kRenderEmptyKey);
    for (long long k = 0; k < n; ++k) {
        int c, r;
        float d;
        if (!apd_fusion::render_draw(view, xyz + 3 * k, c, r, d)) {
            continue;
        }
        const uint64_t key = apd_fusion::render_key(d, (uint32_t)k);
        for (long long y = (long long)r - splat; y <= (long long)r + splat; ++y) {
            for (long long x = (long long)c - splat; x <= (long long)c + splat; ++x) {
                if (x < 0 || x >= view.cols || y < 0 || y >= view.rows) {
                    continue;
                }
                uint64_t &held = keys[(size_t)y * (size_t)view.cols + (size_t)x];
                if (key < held) {
                    held = key;
                }
            }
        }
    }
    return keys;
}

}  // namespace

extern "C" {

// depth and index: width * height entries each
void points_render(long long n, const float *xyz, const float *camera, int width, int height, int splat, float *depth, uint32_t *index)
{
    const std::vector<uint64_t> keys = key_image(n, xyz, view_of(camera, width, height), splat);
    for (size_t i = 0; i < keys.size(); ++i) {
        depth[i] = apd_fusion::render_depth(keys[i]);
        index[i] = apd_fusion::render_index(keys[i]);
    }
}

// cameras: 21 floats each; sizes: width, height each.  offsets: n + 1 entries, views: room for n * num_views, support: n.  Returns
// the number of points with an empty list.
long long points_rendered_visibility(long long n, const float *xyz, int num_views, const float *cameras, const int *sizes, int splat,
                                     float rel_tolerance, long long *offsets, int32_t *views, uint8_t *support)
{
    std::vector<uint8_t> seen((size_t)n * (size_t)num_views, 0);
    for (int s = 0; s < num_views; ++s) {
        const apd_fusion::View view = view_of(cameras + 21 * s, sizes[2 * s], sizes[2 * s + 1]);
        const std::vector<uint64_t> keys = key_image(n, xyz, view, splat);
        for (long long k = 0; k < n; ++k) {
            int c, r;
            float d;
            if (!apd_fusion::render_draw(view, xyz + 3 * k, c, r, d)) {
                continue;
            }
            const float z = apd_fusion::render_depth(keys[(size_t)r * (size_t)view.cols + (size_t)c]);
            if (apd_fusion::render_seen(d, z, rel_tolerance)) {
                seen[(size_t)k * (size_t)num_views + (size_t)s] = 1;
            }
        }
    }
    long long total = 0, unseen = 0;
    for (long long k = 0; k < n; ++k) {
        offsets[k] = total;
        for (int s = 0; s < num_views; ++s) {
            if (seen[(size_t)k * (size_t)num_views + (size_t)s]) {
                views[total++] = s;
            }
        }
        const long long entries = total - offsets[k];
        support[k] = (uint8_t)(entries == 0 ? 0 : (entries - 1 < 255 ? entries - 1 : 255));
        unseen += entries == 0 ? 1 : 0;
    }
    offsets[n] = total;
    return unseen;
}

}  // extern "C"
