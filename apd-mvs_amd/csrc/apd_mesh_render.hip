// apd_mesh_render.hip -- apd_mesh_render, apd_mesh_face_visibility and apd_mesh_remove_unseen of include/apd_mi355x.h: the mesh drawn
// into a camera with a z-buffer -- per pixel the depth and the index of the nearest face --, from such maps of every camera of a call
// the number of cameras that see each face and the pixels it owns, and the mesh without the faces too few cameras see (arithmetic
// contract C25; the rules: apd_mesh_render_math.h).  On the mesh's device, on its null stream; the input stays as it is;
// there is no host path.  Per camera:
//   1. k_mesh_project: one lane per vertex, its fixed-point position, depth and usable flag, 16 bytes.
//   2. k_render_clear (apd_render_device.h, shared with the points' renderer): the key image to the empty key.
//   3. k_mesh_raster_small: one lane per face.  A drawn, unculled face whose clipped bounding box has at most `split` pixels is drawn
//      by its lane, which loops over the box; a larger one writes slices[f], the waves that will share its box: one per 256 of its
//      8 x 8 tiles, 1 to 64.  Every other face has slices[f] = 0.
//   4. apd_sort::exclusive_scan of the slice counts (the scan of apd_scan.h): at[f] = the first wave of face f; the total, the number
//      of waves, is read back: the one read-back a camera costs besides the scan's own, which makes the host wait for the device
//      once per camera.
//   5. k_mesh_raster_large: one wave per large face and slice.  Wave w finds its face, the last f with at[f] <= w, by bisection
//      (the same steps in every lane), and is slice w - at[f] of slices[f].  The 64 lanes take the 8 x 8 pixels of one tile of the
//      box at a time, a slice every slices[f]-th tile; a tile that lies wholly outside one edge (the edge function is linear: its
//      largest value over the tile is at a corner) is skipped by the whole wave, so the loop does not diverge.  The slices are per
//      face: a face that fills the frame is shared by 64 waves instead of serialising 10^5 tiles on one, and a face of a few tiles
//      beside it still costs one wave.
//   Steps 1, 3 and 5 and their launches are apd_mesh_render_device.h's, shared with apd_mesh_colour.hip.
//   Both write the one image of 64-bit keys with render_offer: a 64-bit unsigned atomic min, relaxed, agent scope, after the relaxed
//   load that skips losers.  The minimum does not depend on who drew a pixel or when: the image is a function of the input, the same
//   for every split.
//   6. apd_mesh_render: k_render_resolve turns the keys into the depth and the face map.
//      The visibility: k_mesh_owned, one lane per pixel, adds the pixels to their owners' counters (32-bit integer atomic adds, one
//      per run of equal owners within a wave: integer sums do not depend on the order); k_mesh_face_seen, one lane per face, applies
//      the two rules, adds 1 to the face's view count and its pixels to its total, and zeroes its counter for the next camera: one
//      writer per face, the cameras follow each other on one stream.
// No floating-point atomic, no LDS, no scratch memory (profiles/mesh_render/kres.txt).  One key image is alive at a time, allocated
// once per call at the largest camera of the call.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_mesh_render_device.h"
#include "apd_mesh_render_math.h"
#include "apd_points_host.h"
#include "apd_render_device.h"
#include "apd_sort.h"
#include "apd_tuning.h"

namespace {

using apd_fusion::RenderFace;
using apd_fusion::RenderVertex;
using apd_fusion::View;
using apd_mesh_compact::clear_timing;
using apd_mesh_compact::err;
using apd_mesh_compact::MeshCall;
using apd_mesh_compact::new_mesh_like;
using apd_mesh_render_device::Canvas;
using apd_mesh_render_device::face_of;
using apd_mesh_render_device::g_render_split;
using apd_mesh_render_device::RenderCall;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_render_device::k_render_clear;
using apd_render_device::k_render_resolve;
using apd_render_device::render_offer;

static_assert(APD_RENDER_CULL_NONE == apd_fusion::kRenderCullNone && APD_RENDER_CULL_BACK == apd_fusion::kRenderCullBack,
              "the modes of the header are the modes of the rules");

// Pixel i < px: one more for the counter of its owner.  The lanes of a wave that follow each other with one owner add their number
// once, by the first of them.  owned: a 32-bit counter a face (a camera has fewer than 2^31 pixels)
__global__ __launch_bounds__(256) void k_mesh_owned(const uint64_t *__restrict__ keys, size_t px, uint32_t *owned)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t f = i < px ? apd_fusion::render_index(keys[i]) : apd_fusion::kRenderNoIndex;  // every lane stays for the exchange
    const uint32_t before = __shfl_up(f, 1);
    const bool head = lane == 0 || before != f;
    const uint64_t heads = __ballot(head);
    if (head && f != apd_fusion::kRenderNoIndex) {
        const uint64_t later = lane == 63 ? 0ull : heads >> (lane + 1);
        const uint32_t run = later ? (uint32_t)__ffsll((unsigned long long)later) : (uint32_t)(64 - lane);
        atomicAdd(owned + f, run);
    }
}

// Face f < faces against the finished key image of one camera: views[f] + 1 when the camera sees it, pixels[f] + the pixels it owns;
// owned[f] back to 0.  xyz: the world positions, for the corners' own pixels
__global__ __launch_bounds__(256) void k_mesh_face_seen(const RenderVertex *__restrict__ verts, const int32_t *__restrict__ index,
                                                         const float *__restrict__ xyz, size_t faces, View view, int cull, uint32_t min_pixels,
                                                         float rel_tolerance, const uint64_t *__restrict__ keys, uint32_t *__restrict__ owned,
                                                         uint32_t *__restrict__ views, uint64_t *__restrict__ pixels)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    const uint32_t mine = owned[f];
    RenderFace face;
    if (!face_of(verts, index, f, cull, view.cols, view.rows, face)) {
        return;  // it owns nothing
    }
    bool seen = mine >= min_pixels;
    if (!seen) {
        seen = true;
        for (int c = 0; c < 3 && seen; ++c) {
            const size_t v = (size_t)index[3 * f + c];
            const float P[3] = {xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]};
            seen = apd_fusion::mesh_render_corner_seen(view, P, rel_tolerance, [&](int x, int y) {
                return apd_fusion::render_depth(keys[(size_t)y * (size_t)view.cols + (size_t)x]);
            });
        }
    }
    if (seen) {
        views[f] += 1u;
    }
    if (mine) {
        pixels[f] += (uint64_t)mine;
        owned[f] = 0u;
    }
}

// keep[f] = 1 where views[f] >= min_views; *unseen (zero before) + 1 where views[f] == 0: an integer sum
__global__ __launch_bounds__(256) void k_mesh_seen_flags(const uint32_t *__restrict__ views, size_t faces, uint32_t min_views, uint32_t *__restrict__ keep,
                                                          unsigned long long *unseen)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    keep[f] = views[f] >= min_views ? 1u : 0u;
    if (views[f] == 0u) {
        atomicAdd(unseen, 1ull);
    }
}

template <typename T> __global__ __launch_bounds__(256) void k_mesh_render_fill(T *__restrict__ out, size_t n, T value)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out[i] = value;
    }
}

struct Call : RenderCall {
    int bad_cull(int cull) const
    {
        if (cull != APD_RENDER_CULL_NONE && cull != APD_RENDER_CULL_BACK) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: cull mode %d, neither APD_RENDER_CULL_NONE nor APD_RENDER_CULL_BACK", who, cull);
        }
        return APD_OK;
    }

    // What the two visibility calls refuse of their arguments besides their outputs
    int bad_visibility(int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance) const
    {
        if (const int rc = bad_cull(cull); rc != APD_OK) {
            return rc;
        }
        if (min_pixels < 1) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: min_pixels = 0, not at least 1", who);
        }
        if (!(isfinite(rel_tolerance) && rel_tolerance >= 0.0f)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a relative tolerance of %g, not a non-negative finite number", who, (double)rel_tolerance);
        }
        if (num_views < 1) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: %d views", who, num_views);
        }
        for (int s = 0; s < num_views; ++s) {
            if (const int rc = bad_camera(cameras[s], s); rc != APD_OK) {
                return rc;
            }
        }
        return APD_OK;
    }

    // apd_mesh_render of m (with faces) into host maps
    int render(const apd_mesh *m, const apd_camera &camera, int cull, float *depth, uint32_t *face) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t px = (size_t)camera.width * (size_t)camera.height;
        Scratch scratch;
        Canvas c;
        if (const int rc = canvas(scratch, m, px, c); rc != APD_OK) {
            return rc;
        }
        float *device_depth = nullptr;
        uint32_t *device_face = nullptr;
        if (depth) {
            HIP_TRY(scratch.alloc(px * 4, &device_depth));
        }
        if (face) {
            HIP_TRY(scratch.alloc(px * 4, &device_face));
        }
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        View view;
        if (const int rc = draw(m, camera, cull, c, view); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_render_resolve, grid_of(px), dim3(256), 0, 0, (const uint64_t *)c.keys, px, device_depth, device_face);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        std::vector<float> got_depth(depth ? px : 0);
        std::vector<uint32_t> got_face(face ? px : 0);
        if (depth) {
            HIP_TRY(hipMemcpy(got_depth.data(), device_depth, px * 4, hipMemcpyDeviceToHost));
        }
        if (face) {
            HIP_TRY(hipMemcpy(got_face.data(), device_face, px * 4, hipMemcpyDeviceToHost));
        }
        std::copy(got_depth.begin(), got_depth.end(), depth);  // both or neither: outputs are untouched on failure
        std::copy(got_face.begin(), got_face.end(), face);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // The view count and the owned pixels of every face of m (with faces) over the cameras, in device arrays of `scratch`; launches
    // and the read-backs of draw()
    int visibility(Scratch &scratch, const apd_mesh *m, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance,
                   uint32_t **views, uint64_t **pixels) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t nf = (size_t)m->faces;
        size_t max_px = 0;
        for (int s = 0; s < num_views; ++s) {
            max_px = std::max(max_px, (size_t)cameras[s].width * (size_t)cameras[s].height);
        }
        Canvas c;
        if (const int rc = canvas(scratch, m, max_px, c); rc != APD_OK) {
            return rc;
        }
        uint32_t *owned = nullptr;
        HIP_TRY(scratch.alloc(nf * 4, &owned));
        HIP_TRY(scratch.alloc(nf * 4, views));
        HIP_TRY(scratch.alloc(nf * 8, pixels));
        HIP_TRY(hipMemsetAsync(owned, 0, nf * 4, 0));
        HIP_TRY(hipMemsetAsync(*views, 0, nf * 4, 0));
        HIP_TRY(hipMemsetAsync(*pixels, 0, nf * 8, 0));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        for (int s = 0; s < num_views; ++s) {
            View view;
            if (const int rc = draw(m, cameras[s], cull, c, view); rc != APD_OK) {
                return rc;
            }
            const size_t px = (size_t)view.cols * (size_t)view.rows;
            hipLaunchKernelGGL(k_mesh_owned, grid_of(px), dim3(256), 0, 0, (const uint64_t *)c.keys, px, owned);
            hipLaunchKernelGGL(k_mesh_face_seen, grid_of(nf), dim3(256), 0, 0, (const RenderVertex *)c.verts, (const int32_t *)m->index, (const float *)m->xyz,
                               nf, view, cull, (uint32_t)min_pixels, rel_tolerance, (const uint64_t *)c.keys, owned, *views, *pixels);
            HIP_TRY(hipGetLastError());
        }
        return APD_OK;
    }

    // keep[f] for views[f] >= min_views in a device array of `scratch`, and the faces no camera sees
    int flags(Scratch &scratch, const uint32_t *views, size_t nf, unsigned min_views, uint32_t **keep, long long *unseen) const
    {
        unsigned long long *none = nullptr, found = 0;
        HIP_TRY(scratch.alloc(nf * 4, keep));
        HIP_TRY(scratch.alloc(8, &none));
        HIP_TRY(hipMemsetAsync(none, 0, 8, 0));
        hipLaunchKernelGGL(k_mesh_seen_flags, grid_of(nf), dim3(256), 0, 0, views, nf, (uint32_t)min_views, *keep, none);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&found, none, 8, hipMemcpyDeviceToHost));
        *unseen = (long long)found;
        return APD_OK;
    }

    // apd_mesh_face_visibility of m (with faces) into host arrays of the call's own
    int face_visibility(const apd_mesh *m, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance, uint32_t *views,
                        uint64_t *pixels, long long *unseen) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *device_views = nullptr, *keep = nullptr;
        uint64_t *device_pixels = nullptr;
        if (const int rc = visibility(scratch, m, num_views, cameras, cull, min_pixels, rel_tolerance, &device_views, &device_pixels); rc != APD_OK) {
            return rc;
        }
        if (const int rc = flags(scratch, device_views, nf, 1, &keep, unseen); rc != APD_OK) {
            return rc;
        }
        if (views) {
            HIP_TRY(hipMemcpy(views, device_views, nf * 4, hipMemcpyDeviceToHost));
        }
        if (pixels) {
            HIP_TRY(hipMemcpy(pixels, device_pixels, nf * 8, hipMemcpyDeviceToHost));
        }
        apd_fusion::g_fusion_ms[1] = ms_since(t0) - apd_fusion::g_fusion_ms[0];  // [0]: the allocations, set by visibility()
        return APD_OK;
    }

    // apd_mesh_remove_unseen of m (with faces) into `out`, which has colour and normals as m
    int remove_unseen(const apd_mesh *m, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance, unsigned min_views,
                      apd_mesh *out) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *keep = nullptr;
        if (min_views == 0) {  // every face stays: nothing is drawn
            HIP_TRY(scratch.alloc(nf * 4, &keep));
            hipLaunchKernelGGL(k_mesh_render_fill<uint32_t>, grid_of(nf), dim3(256), 0, 0, keep, nf, 1u);
            HIP_TRY(hipGetLastError());
        } else {
            uint32_t *views = nullptr;
            uint64_t *pixels = nullptr;
            long long unseen = 0;
            if (const int rc = visibility(scratch, m, num_views, cameras, cull, min_pixels, rel_tolerance, &views, &pixels); rc != APD_OK) {
                return rc;
            }
            if (const int rc = flags(scratch, views, nf, min_views, &keep, &unseen); rc != APD_OK) {
                return rc;
            }
        }
        const int rc = compact(scratch, m, m->index, keep, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t0) - apd_fusion::g_fusion_ms[0];  // [0]: the allocations, set by visibility()
        return rc;
    }
};

}  // namespace

std::atomic<int> apd_mesh_render_device::g_render_split{0};

// The box size, in pixels, above which a face is drawn by a wave instead of a lane: box_pixels > 0 sets it, 0 restores
// APD_MESH_RENDER_SPLIT.  The maps do not depend on it; tools/mesh_render_time.py times three values and
// tests/test_gpu_mesh_render.py compares their bytes
extern "C" void apd_mesh_render_split(int box_pixels) { g_render_split.store(box_pixels > 0 ? box_pixels : 0); }

extern "C" int apd_mesh_render(apd_mesh_t m, const apd_camera *camera, int cull, float *depth, uint32_t *face)
{
    const Call call{{{{"apd_mesh_render"}}}};
    err().clear();
    if (!m || !camera) {
        return call.invalid("null argument");
    }
    if (!depth && !face) {
        return call.invalid("every output is null");
    }
    if (const int rc = call.bad_cull(cull); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.bad_camera(*camera, 0); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    if (m->faces == 0) {  // empty maps: no device is touched
        const size_t px = (size_t)camera->width * (size_t)camera->height;
        if (depth) {
            std::fill(depth, depth + px, 0.0f);
        }
        if (face) {
            std::fill(face, face + px, apd_fusion::kRenderNoIndex);
        }
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.render(m, *camera, cull, depth, face);
}

extern "C" int apd_mesh_face_visibility(apd_mesh_t m, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance,
                                        uint32_t *views, uint64_t *pixels, long long *unseen)
{
    const Call call{{{{"apd_mesh_face_visibility"}}}};
    err().clear();
    if (!m || !cameras) {
        return call.invalid("null argument");
    }
    if (!views && !pixels && !unseen) {
        return call.invalid("every output is null");
    }
    if (const int rc = call.bad_visibility(num_views, cameras, cull, min_pixels, rel_tolerance); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    const size_t nf = (size_t)m->faces;
    long long none = 0;
    std::vector<uint32_t> seen(views ? nf : 0, 0u);
    std::vector<uint64_t> owned(pixels ? nf : 0, 0ull);
    if (nf > 0) {
        DeviceScope scope(true);
        if (const int rc = call.face_visibility(m, num_views, cameras, cull, min_pixels, rel_tolerance, views ? seen.data() : nullptr,
                                                pixels ? owned.data() : nullptr, &none);
            rc != APD_OK) {
            return rc;
        }
    }
    std::copy(seen.begin(), seen.end(), views);
    std::copy(owned.begin(), owned.end(), pixels);
    if (unseen) {
        *unseen = none;
    }
    return APD_OK;
}

extern "C" int apd_mesh_remove_unseen(apd_mesh_t m, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance,
                                      unsigned min_views, apd_mesh_t *out, long long *removed_faces, long long *removed_vertices)
{
    const Call call{{{{"apd_mesh_remove_unseen"}}}};
    err().clear();
    if (!m || !cameras || !out) {
        return call.invalid("null argument");
    }
    if (const int rc = call.bad_visibility(num_views, cameras, cull, min_pixels, rel_tolerance); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    apd_mesh *result = new_mesh_like(m);
    if (m->faces > 0) {  // a mesh without faces keeps none and so no vertex: no device is touched
        DeviceScope scope(true);
        if (const int rc = call.remove_unseen(m, num_views, cameras, cull, min_pixels, rel_tolerance, min_views, result); rc != APD_OK) {
            delete result;  // it holds nothing: what the call allocated went with its scratch
            return rc;
        }
    }
    *out = result;
    if (removed_faces) {
        *removed_faces = m->faces - result->faces;
    }
    if (removed_vertices) {
        *removed_vertices = m->vertices - result->vertices;
    }
    return APD_OK;
}
