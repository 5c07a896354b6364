// apd_mesh_colour.hip -- apd_mesh_colour_from_views of include/apd_mi355x.h: the vertices of a mesh coloured from the images of the
// cameras that see them, through the mesh's own z-buffer (arithmetic contract C26; the rules: apd_mesh_colour_math.h).  On
// the mesh's device, on its null stream; the input stays as it is; there is no host path.  A mesh without normals first gets them
// by contract C22 (apd_mesh_with_vertex_normals: the same bits).  Then per camera, in the call's order:
//   1. an image in host memory is copied into the one image buffer of the call;
//   2. the rasteriser of contract C25 (apd_mesh_render_device.h: project, clear, small and large raster) with APD_RENDER_CULL_NONE,
//      then k_render_resolve into the one depth map of the call, which stays on the device;
//   3. k_mesh_colour_view: one lane per vertex.  drop, the four depth taps, the facing test, the 4 x (1 or 3) image taps, and the
//      vertex's four binary64 sums and its count in global memory: one writer per vertex, the cameras follow each other on one stream.
//      The two pixels of a footprint's row are neighbours in memory: a lane reads 2 or 6 consecutive floats per row, as dword loads
//      (an interleaved pixel is 12 bytes at a 4-byte alignment, so no wider load is possible); the lanes of a wave read the pixels
//      their vertices project to, which for the vertices of a surface in index order are near each other.
// After the last camera k_mesh_colour_finish, one lane per vertex: the division, the conversion, the fallback colour, the count as the
// caller's `views`, and one integer atomic add per uncoloured vertex.
// No floating-point atomic, no LDS, no scratch memory (profiles/mesh_colour/kres.txt).  Alive at a time: one key image, one depth
// map and, for host images, one image buffer, each allocated once per call at the largest camera, and 36 bytes a vertex (four
// binary64 sums and a 32-bit count); for a mesh without normals also the mesh with them.
// The host copies are not overlapped with the raster of the view before: at 3200 x 2400 x 3 a copy takes 1.65 ms and the kernels of a
// view 0.25 ms, so a second stream and a second image buffer could hide at most 13 % of the call (profiles/mesh_colour/timing.txt).
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_colour_math.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_mesh_render_device.h"
#include "apd_points_host.h"
#include "apd_render_device.h"

namespace {

using apd_fusion::ColourSample;
using apd_fusion::View;
using apd_mesh_compact::clear_timing;
using apd_mesh_compact::err;
using apd_mesh_compact::new_mesh_like;
using apd_mesh_render_device::Canvas;
using apd_mesh_render_device::RenderCall;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_render_device::k_render_resolve;

// Vertex v < vertices against one camera: depth, the C25 depth map, and image, rows x cols x channels floats, both of view's size.
// sums: S_blue, S_green, S_red, W, `vertices` entries each; count: one entry a vertex
template <int kChannels>
__global__ __launch_bounds__(256) void k_mesh_colour_view(const float *__restrict__ xyz, const float *__restrict__ normal, size_t vertices, View view,
                                                           float rel_tolerance, float min_cos, const float *__restrict__ depth,
                                                           const float *__restrict__ image, double *__restrict__ sums, uint32_t *__restrict__ count)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    const float P[3] = {xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]};
    const float n[3] = {normal[3 * v], normal[3 * v + 1], normal[3 * v + 2]};
    const size_t cols = (size_t)view.cols;
    ColourSample s;
    if (!apd_fusion::colour_sample(view, P, n, rel_tolerance, min_cos, [&](int c, int r) { return depth[(size_t)r * cols + (size_t)c]; }, s)) {
        return;
    }
    // rule 3: 0 <= c0, c0 + 1 < cols, 0 <= r0, r0 + 1 < rows: the two rows of 2 * kChannels floats are inside the image
    const float *top = image + ((size_t)s.r0 * cols + (size_t)s.c0) * kChannels;
    const float *bot = top + cols * kChannels;
    float value[3];
    for (int k = 0; k < kChannels; ++k) {
        value[k] = apd_fusion::colour_bilinear(top[k], top[kChannels + k], bot[k], bot[kChannels + k], s.fu, s.fw);
    }
    if (kChannels == 1) {
        value[1] = value[2] = value[0];
    }
    for (int k = 0; k < 3; ++k) {
        sums[(size_t)k * vertices + v] = apd_fusion::colour_add(sums[(size_t)k * vertices + v], s.c, value[k]);
    }
    sums[3 * vertices + v] = sums[3 * vertices + v] + s.c;
    count[v] += 1u;
}

// Vertex v < vertices: its colour from its sums, or from bgr (null: a mesh without colour) where no camera gave a sample;
// *uncoloured (zero before) + 1 for each of those: an integer sum
__global__ __launch_bounds__(256) void k_mesh_colour_finish(const double *__restrict__ sums, const uint32_t *__restrict__ count, size_t vertices,
                                                             const uint8_t *__restrict__ bgr, uint8_t *__restrict__ out_bgr,
                                                             unsigned long long *uncoloured)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    if (count[v] > 0u) {
        const double W = sums[3 * vertices + v];
        for (int k = 0; k < 3; ++k) {
            out_bgr[3 * v + k] = apd_fusion::colour_byte(sums[(size_t)k * vertices + v], W);
        }
        return;
    }
    for (int k = 0; k < 3; ++k) {
        out_bgr[3 * v + k] = bgr ? bgr[3 * v + k] : (uint8_t)0;
    }
    atomicAdd(uncoloured, 1ull);
}

struct Call : RenderCall {
    // apd_mesh_colour_from_views of m (with vertices) into `out`, which has colour, and normals as m; views: null or a host array of
    // the call's own
    int colour(const apd_mesh *m, int num_views, const apd_camera *cameras, const float *const *images, int channels, bool on_device, float rel_tolerance,
               float min_cos, apd_mesh *out, uint32_t *views, long long *uncoloured) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        apd_mesh_t with_normals = nullptr;  // where m has none: freed on every path
        struct Release {
            apd_mesh_t &mesh;
            ~Release()
            {
                if (mesh) {
                    apd_mesh_destroy(mesh);
                }
            }
        } release{with_normals};
        if (!m->normals && nf > 0) {
            if (const int rc = apd_mesh_with_vertex_normals(const_cast<apd_mesh *>(m), &with_normals); rc != APD_OK) {
                return rc;  // its message
            }
            HIP_TRY(hipSetDevice(m->device));
        }
        const float *normal = m->normals ? m->normal : with_normals ? with_normals->normal : nullptr;
        size_t max_px = 0;
        for (int s = 0; s < num_views; ++s) {
            max_px = std::max(max_px, (size_t)cameras[s].width * (size_t)cameras[s].height);
        }
        Scratch scratch, made;
        if (const int rc = alloc(made, out, nv, nf); rc != APD_OK) {
            return rc;
        }
        double *sums = nullptr;
        uint32_t *count = nullptr;
        unsigned long long *none = nullptr, found = 0;
        HIP_TRY(scratch.alloc(nv * 32, &sums));
        HIP_TRY(scratch.alloc(nv * 4, &count));
        HIP_TRY(scratch.alloc(8, &none));
        Canvas c;
        float *depth = nullptr, *staged = nullptr;
        if (nf > 0) {  // without faces nothing is drawn and no vertex has a normal: every vertex keeps its colour
            if (const int rc = canvas(scratch, m, max_px, c); rc != APD_OK) {
                return rc;
            }
            HIP_TRY(scratch.alloc(max_px * 4, &depth));
            if (!on_device) {
                HIP_TRY(scratch.alloc(max_px * 4 * (size_t)channels, &staged));
            }
        }
        HIP_TRY(hipMemsetAsync(sums, 0, nv * 32, 0));
        HIP_TRY(hipMemsetAsync(count, 0, nv * 4, 0));
        HIP_TRY(hipMemsetAsync(none, 0, 8, 0));
        const double setup = ms_since(t0);
        for (int s = 0; s < num_views && nf > 0; ++s) {
            const size_t px = (size_t)cameras[s].width * (size_t)cameras[s].height;
            const float *image = images[s];
            if (!on_device) {
                HIP_TRY(hipMemcpy(staged, images[s], px * 4 * (size_t)channels, hipMemcpyHostToDevice));  // after the kernel that read it last
                image = staged;
            }
            View view;
            if (const int rc = draw(m, cameras[s], APD_RENDER_CULL_NONE, c, view); rc != APD_OK) {
                return rc;
            }
            hipLaunchKernelGGL(k_render_resolve, grid_of(px), dim3(256), 0, 0, (const uint64_t *)c.keys, px, depth, (uint32_t *)nullptr);
            if (channels == 3) {
                hipLaunchKernelGGL(k_mesh_colour_view<3>, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, normal, nv, view, rel_tolerance, min_cos,
                                   (const float *)depth, image, sums, count);
            } else {
                hipLaunchKernelGGL(k_mesh_colour_view<1>, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, normal, nv, view, rel_tolerance, min_cos,
                                   (const float *)depth, image, sums, count);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(out->xyz, m->xyz, nv * 12, hipMemcpyDeviceToDevice, 0));
        if (m->normals) {
            HIP_TRY(hipMemcpyAsync(out->normal, m->normal, nv * 12, hipMemcpyDeviceToDevice, 0));
        }
        if (nf > 0) {
            HIP_TRY(hipMemcpyAsync(out->index, m->index, nf * 12, hipMemcpyDeviceToDevice, 0));
        }
        hipLaunchKernelGGL(k_mesh_colour_finish, grid_of(nv), dim3(256), 0, 0, (const double *)sums, (const uint32_t *)count, nv, (const uint8_t *)m->bgr,
                           out->bgr, none);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&found, none, 8, hipMemcpyDeviceToHost));
        if (views) {
            HIP_TRY(hipMemcpy(views, count, nv * 4, hipMemcpyDeviceToHost));
        }
        HIP_TRY(hipDeviceSynchronize());
        keep(made, out);
        *uncoloured = (long long)found;
        clear_timing();  // what the normals reported
        apd_fusion::g_fusion_ms[0] = setup;
        apd_fusion::g_fusion_ms[1] = ms_since(t0) - setup;
        return APD_OK;
    }
};

}  // namespace

extern "C" int apd_mesh_colour_from_views(apd_mesh_t m, int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                                          int maps_on_device, float rel_tolerance, float min_cos, apd_mesh_t *out, uint32_t *views, long long *uncoloured)
{
    const Call call{{{{"apd_mesh_colour_from_views"}}}};
    err().clear();
    if (!m || !cameras || !images || !out) {
        return call.invalid("null argument");
    }
    if (num_views < 1) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d views", call.who, num_views);
    }
    if (image_channels != 1 && image_channels != 3) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: images of %d channels, not 1 or 3", call.who, image_channels);
    }
    if (!(isfinite(rel_tolerance) && rel_tolerance >= 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a relative tolerance of %g, not a non-negative finite number", call.who, (double)rel_tolerance);
    }
    if (!(min_cos >= 0.0f && min_cos < 1.0f)) {  // a NaN fails both
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a min_cos of %g, not in [0, 1)", call.who, (double)min_cos);
    }
    for (int s = 0; s < num_views; ++s) {
        if (!images[s]) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: view %d has no image", call.who, s);
        }
        if (const int rc = call.bad_camera(cameras[s], s); rc != APD_OK) {
            return rc;
        }
    }
    if (3 * m->faces >= (1LL << 32) && !m->normals) {
        return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld faces without normals, whose 3 corners each are 2^32 or more", call.who, m->faces);
    }
    clear_timing();
    apd_mesh *result = new_mesh_like(m);
    result->colour = 1;
    const size_t nv = (size_t)m->vertices;
    std::vector<uint32_t> seen(views ? nv : 0, 0u);
    long long none = 0;
    if (nv > 0) {  // a mesh without vertices gives one without: no device is touched
        DeviceScope scope(true);
        if (const int rc = call.colour(m, num_views, cameras, images, image_channels, maps_on_device != 0, rel_tolerance, min_cos, result,
                                       views ? seen.data() : nullptr, &none);
            rc != APD_OK) {
            delete result;  // it holds nothing: what the call allocated went with its scratch
            return rc;
        }
    }
    *out = result;
    std::copy(seen.begin(), seen.end(), views);
    if (uncoloured) {
        *uncoloured = none;
    }
    return APD_OK;
}
