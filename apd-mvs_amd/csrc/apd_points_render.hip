// apd_points_render.hip -- apd_points_render and apd_points_rendered_visibility of include/apd_mi355x.h: the cloud drawn into a
// camera with a z-buffer -- per pixel the depth and the index of the nearest point -- and, from such maps of every camera of a call,
// the views that see each point, occlusion included, as the lists of a merged object (arithmetic contract C15; the
// relation: apd_render_math.h).
//
// On the points' device, on its null stream, per camera:
//   1. k_render_clear: the key image of the camera, width * height 64-bit keys, to the empty key (apd_render_device.h, shared with
//      the mesh's rasteriser, as are render_offer and k_render_resolve).
//   2. k_render_scatter: one lane per point; the point's key (depth bits, index) goes to every pixel of its footprint with a 64-bit
//      unsigned atomic min, relaxed, agent scope, after a relaxed load that skips it where the pixel already holds a smaller key
//      (render_offer).  The min of integers does not depend on the order of arrival: the image is a function of the input.  In a
//      cloud many layers deep all but the lanes of the front layer then end in a load.
//   3. apd_points_render: k_render_resolve turns the keys into the depth and the index map.
//      apd_points_rendered_visibility: k_render_test repeats the projection of every point, reads the key at its centre pixel and
//      sets bit s of the point's row of a bitset (ceil(num_views / 32) words a point) when camera s sees it.  A row belongs to one
//      lane and the cameras follow each other on one stream: no atomics.
// After the last camera k_seen_lengths counts each row's bits (and the rows without any), the scan of apd_sort.h turns the lengths
// into 64-bit offsets, and k_seen_emit writes each point's views in ascending order and its support.
// One key image is alive at a time, allocated once per call at the largest camera of the call.
// There is no host path: host-resident points go up, the maps or the result come down.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_lab.h"
#include "apd_points_grid.h"
#include "apd_points_host.h"
#include "apd_render_device.h"
#include "apd_render_math.h"
#include "apd_sort.h"

namespace {

using apd_fusion::PointArrays;
using apd_fusion::View;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_render_device::k_render_clear;
using apd_render_device::k_render_resolve;
using apd_render_device::render_offer;

// Point k < n: its key to the pixels of its footprint.  keys: view.rows x view.cols, cleared.
__global__ __launch_bounds__(256) void k_render_scatter(const float *__restrict__ xyz, uint32_t n, View view, int splat, uint64_t *keys)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;  // n < 2^31
    if (k >= n) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2]};
    int c, r;
    float d;
    if (!apd_fusion::render_draw(view, P, c, r, d)) {
        return;
    }
    const uint64_t key = apd_fusion::render_key(d, k);
    int c0, c1, r0, r1;
    apd_fusion::render_span(c, splat, view.cols, c0, c1);
    apd_fusion::render_span(r, splat, view.rows, r0, r1);
    for (int y = r0; y <= r1; ++y) {
        uint64_t *row = keys + (size_t)y * (size_t)view.cols;
        for (int x = c0; x <= c1; ++x) {
            render_offer(row + x, key);
        }
    }
}

// Point k < n against the finished key image of camera s: bit s of its row of `seen` (words per point) is set when it is seen
__global__ __launch_bounds__(256) void k_render_test(const float *__restrict__ xyz, uint32_t n, View view, float rel_tolerance,
                                                      const uint64_t *__restrict__ keys, int s, uint32_t words, uint32_t *__restrict__ seen)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2]};
    int c, r;
    float d;
    if (!apd_fusion::render_draw(view, P, c, r, d)) {
        return;
    }
    const float z = apd_fusion::render_depth(keys[(size_t)r * (size_t)view.cols + (size_t)c]);
    if (apd_fusion::render_seen(d, z, rel_tolerance)) {
        seen[(size_t)k * words + (uint32_t)s / 32u] |= 1u << ((uint32_t)s % 32u);
    }
}

// length[k]: the set bits of row k; *unseen: the rows without one (an integer sum: the order of arrival does not show)
__global__ __launch_bounds__(256) void k_seen_lengths(const uint32_t *__restrict__ seen, uint32_t n, uint32_t words, uint32_t *__restrict__ length,
                                                       unsigned long long *__restrict__ unseen)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    uint32_t bits = 0;
    for (uint32_t w = 0; w < words; ++w) {
        bits += (uint32_t)__popc(seen[(size_t)k * words + w]);
    }
    length[k] = bits;
    if (bits == 0) {
        atomicAdd(unseen, 1ull);
    }
}

// The list of point k starts at entry at[k]: its views ascending; support[k] = 0 for an empty list, else min(255, L - 1)
__global__ __launch_bounds__(256) void k_seen_emit(const uint32_t *__restrict__ seen, uint32_t n, uint32_t words, const uint64_t *__restrict__ at,
                                                    long long *__restrict__ offsets, int32_t *__restrict__ views, uint8_t *__restrict__ support)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    offsets[k] = (long long)at[k];
    int32_t *list = views + at[k];
    for (uint32_t w = 0; w < words; ++w) {
        uint32_t m = seen[(size_t)k * words + w];
        while (m) {
            *list++ = (int32_t)(w * 32u + (uint32_t)(__ffs((int)m) - 1));
            m &= m - 1;
        }
    }
    const uint64_t entries = at[k + 1] - at[k];
    support[k] = (uint8_t)(entries == 0 ? 0 : (entries - 1 < 255 ? entries - 1 : 255));
    if (k == 0) {
        offsets[n] = (long long)at[n];
    }
}

std::string &err() { return apd_fusion::g_fusion_error; }

constexpr long long kMaxEntries = 1LL << 32;

// One call of either entry point: its name, which starts every message, and what both share
struct Call {
    const char *const who;

    int hip_failed(const char *expr, hipError_t e, const char *, int) const  // what HIP_TRY returns
    {
        return apd::set_error(err(), APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
    }

    // What both calls refuse of the points, the footprint and their cameras, before any device is touched
    int check(apd_points_t p, const void *cameras, const void *output, int splat) const
    {
        err().clear();
        if (!p || !cameras || !output) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: null argument", who);
        }
        if (splat < 0 || splat > apd_fusion::kRenderMaxSplat) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: splat = %d, not in 0 .. %d", who, splat, apd_fusion::kRenderMaxSplat);
        }
        return APD_OK;
    }

    int check_camera(const apd_camera &c, int s) const
    {
        if (c.width <= 0 || c.height <= 0) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels", who, s, c.width, c.height);
        }
        if ((long long)c.width * c.height >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels, 2^31 or more", who, s, c.width, c.height);
        }
        return APD_OK;
    }

    int check_count(apd_points_t p) const
    {
        if (p->count >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld points, 2^31 or more (a key carries a 32-bit index)", who, p->count);
        }
        return APD_OK;
    }

    // The key image of `camera` from the n points at xyz (n may be 0) with footprints of `splat`, into keys (room for the camera's
    // pixels); launches only
    int draw(const float *xyz, size_t n, const apd_camera &camera, int splat, uint64_t *keys, View &view) const
    {
        apd_fusion::view_geometry(camera, camera.height, camera.width, view);
        const size_t px = (size_t)camera.width * (size_t)camera.height;
        hipLaunchKernelGGL(k_render_clear, grid_of(px), dim3(256), 0, 0, keys, px);
        if (n > 0) {
            hipLaunchKernelGGL(k_render_scatter, grid_of(n), dim3(256), 0, 0, xyz, (uint32_t)n, view, splat, keys);
        }
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // apd_points_render of p on its device: device-resident points, or host-resident ones with at least one point
    int render(apd_points_t p, const apd_camera &camera, int splat, float *depth, uint32_t *index) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t n = (size_t)p->count, px = (size_t)camera.width * (size_t)camera.height;
        Scratch scratch;
        HIP_TRY(hipSetDevice(p->device));
        const float *xyz = p->arrays.xyz;
        float *device_depth = depth;
        uint32_t *device_index = index;
        if (!p->on_device) {
            HIP_TRY(scratch.upload((const float *)p->arrays.xyz, n * 12, &xyz));
            if (depth) {
                HIP_TRY(scratch.alloc(px * 4, &device_depth));
            }
            if (index) {
                HIP_TRY(scratch.alloc(px * 4, &device_index));
            }
        }
        uint64_t *keys = nullptr;
        HIP_TRY(scratch.alloc(px * 8, &keys));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        View view;
        if (const int rc = draw(xyz, n, camera, splat, keys, view); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_render_resolve, grid_of(px), dim3(256), 0, 0, (const uint64_t *)keys, px, device_depth, device_index);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        if (!p->on_device) {
            if (depth) {
                HIP_TRY(hipMemcpy(depth, device_depth, px * 4, hipMemcpyDeviceToHost));
            }
            if (index) {
                HIP_TRY(hipMemcpy(index, device_index, px * 4, hipMemcpyDeviceToHost));
            }
        }
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // `bytes` device bytes at `from` as host memory (malloc) in *to
    template <typename T> int download(const T *from, size_t bytes, T **to) const
    {
        *to = static_cast<T *>(malloc(bytes > 0 ? bytes : 1));
        if (!*to) {
            return apd::set_error(err(), APD_ERR_HIP, "%s: out of host memory", who);
        }
        HIP_TRY(hipMemcpy(*to, from, bytes, hipMemcpyDeviceToHost));
        return APD_OK;
    }

    // apd_points_rendered_visibility of p (count > 0) into `result` (where p lives, without arrays so far)
    int visibility(apd_points_t p, int num_views, const apd_camera *cameras, int splat, float rel_tolerance, apd_points *result, long long *unseen) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t n = (size_t)p->count;
        const uint32_t words = ((uint32_t)num_views + 31u) / 32u;
        size_t max_px = 0;
        for (int s = 0; s < num_views; ++s) {
            max_px = std::max(max_px, (size_t)cameras[s].width * (size_t)cameras[s].height);
        }
        Scratch scratch;
        HIP_TRY(hipSetDevice(p->device));
        const float *xyz = p->arrays.xyz;
        if (!p->on_device) {
            HIP_TRY(scratch.upload((const float *)p->arrays.xyz, n * 12, &xyz));
        }
        uint64_t *keys = nullptr, *at = nullptr;
        uint32_t *seen = nullptr, *length = nullptr;
        unsigned long long *empty = nullptr;
        HIP_TRY(scratch.alloc(max_px * 8, &keys));
        HIP_TRY(scratch.alloc(n * words * 4, &seen));
        HIP_TRY(scratch.alloc(n * 4, &length));
        HIP_TRY(scratch.alloc((n + 1) * 8, &at));
        HIP_TRY(scratch.alloc(8, &empty));
        HIP_TRY(hipMemsetAsync(seen, 0, n * words * 4, 0));
        HIP_TRY(hipMemsetAsync(empty, 0, 8, 0));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        for (int s = 0; s < num_views; ++s) {
            View view;
            if (const int rc = draw(xyz, n, cameras[s], splat, keys, view); rc != APD_OK) {
                return rc;
            }
            hipLaunchKernelGGL(k_render_test, grid_of(n), dim3(256), 0, 0, xyz, (uint32_t)n, view, rel_tolerance, (const uint64_t *)keys, s, words, seen);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_seen_lengths, grid_of(n), dim3(256), 0, 0, (const uint32_t *)seen, (uint32_t)n, words, length, empty);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(length, at, n));
        uint64_t total = 0;
        unsigned long long none = 0;
        HIP_TRY(hipMemcpy(&total, at + n, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&none, empty, 8, hipMemcpyDeviceToHost));
        if (total >= (uint64_t)kMaxEntries) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %llu visibility entries, 2^32 or more", who, (unsigned long long)total);
        }
        const size_t entries = (size_t)total;
        long long *vis_offsets = nullptr;
        int32_t *vis_views = nullptr;
        PointArrays out;
        HIP_TRY(scratch.alloc((n + 1) * sizeof(long long), &vis_offsets));
        HIP_TRY(scratch.alloc(entries * sizeof(int32_t), &vis_views));
        // device-resident points: every array of the result at once; host-resident ones: the support alone, which comes down
        HIP_TRY(alloc_arrays(scratch, out, n, p->on_device ? apd_fusion::kAllArrays : apd_fusion::kSupport));
        hipLaunchKernelGGL(k_seen_emit, grid_of(n), dim3(256), 0, 0, (const uint32_t *)seen, (uint32_t)n, words, (const uint64_t *)at, vis_offsets, vis_views,
                           out.support);
        HIP_TRY(hipGetLastError());
        constexpr unsigned kCopied = apd_fusion::kAllArrays & ~apd_fusion::kSupport;
        if (p->on_device) {
            HIP_TRY(copy_arrays(out, p->arrays, n, hipMemcpyDeviceToDevice, kCopied));
            HIP_TRY(hipDeviceSynchronize());
            keep_arrays(scratch, out);
            scratch.keep(vis_offsets);
            scratch.keep(vis_views);
            result->arrays = out;
            result->vis_offsets = vis_offsets;
            result->vis_views = vis_views;
        } else {  // freed with `result` by the caller if anything below fails
            if (!alloc_host_arrays(result->arrays, n)) {
                return apd::set_error(err(), APD_ERR_HIP, "%s: out of host memory", who);
            }
            HIP_TRY(copy_arrays(result->arrays, p->arrays, n, hipMemcpyHostToHost, kCopied));
            HIP_TRY(copy_arrays(result->arrays, out, n, hipMemcpyDeviceToHost, apd_fusion::kSupport));
            int rc = download(vis_offsets, (n + 1) * sizeof(long long), &result->vis_offsets);
            rc = rc != APD_OK ? rc : download(vis_views, entries * sizeof(int32_t), &result->vis_views);
            if (rc != APD_OK) {
                return rc;
            }
        }
        result->count = p->count;
        *unseen = (long long)none;
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }
};

// A new object like p that names at least num_views views: the lists of the result index the cameras of the call, which may be
// more than the fusion of p had.  A view past p's own has the size of its camera and no sources.
apd_points *new_result(const apd_points *p, int num_views, const apd_camera *cameras)
{
    apd_points *q = apd_points_host::new_points_like(p);
    for (int s = (int)q->rows.size(); s < num_views; ++s) {
        q->rows.push_back(cameras[s].height);
        q->cols.push_back(cameras[s].width);
        q->pair_offsets.push_back(q->pair_offsets.back());
    }
    q->merged = 1;
    return q;
}

}  // namespace

extern "C" int apd_points_render(apd_points_t p, const apd_camera *camera, int splat, float *depth, uint32_t *index)
{
    const Call call{"apd_points_render"};
    if (const int rc = call.check(p, camera, depth ? (const void *)depth : (const void *)index, splat); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_camera(*camera, 0); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_count(p); rc != APD_OK) {
        return rc;
    }
    apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0;
    if (p->count == 0 && !p->on_device) {  // all-empty host maps: no device is touched
        const size_t px = (size_t)camera->width * (size_t)camera->height;
        if (depth) {
            std::fill(depth, depth + px, 0.0f);
        }
        if (index) {
            std::fill(index, index + px, apd_fusion::kRenderNoIndex);
        }
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.render(p, *camera, splat, depth, index);
}

extern "C" int apd_points_rendered_visibility(apd_points_t p, int num_views, const apd_camera *cameras, int splat, float rel_tolerance,
                                              apd_points_t *out, long long *unseen)
{
    const Call call{"apd_points_rendered_visibility"};
    if (const int rc = call.check(p, cameras, out, splat); rc != APD_OK) {
        return rc;
    }
    if (num_views < 1) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d views", call.who, num_views);
    }
    if (!(isfinite(rel_tolerance) && rel_tolerance >= 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a relative tolerance of %g, not a non-negative finite number", call.who, (double)rel_tolerance);
    }
    for (int s = 0; s < num_views; ++s) {
        if (const int rc = call.check_camera(cameras[s], s); rc != APD_OK) {
            return rc;
        }
    }
    if (const int rc = call.check_count(p); rc != APD_OK) {
        return rc;
    }
    apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0;
    apd_points *result = new_result(p, num_views, cameras);
    long long none = 0;
    if (p->count > 0) {
        DeviceScope scope(true);
        if (const int rc = call.visibility(p, num_views, cameras, splat, rel_tolerance, result, &none); rc != APD_OK) {
            const std::string why = err();
            apd_points_destroy(result);  // its arrays are host memory, or none yet
            err() = why;
            return rc;
        }
    }
    *out = result;
    if (unseen) {
        *unseen = none;
    }
    return APD_OK;
}
