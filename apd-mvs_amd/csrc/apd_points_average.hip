// apd_points_average.hip -- apd_points_average of include/apd_mi355x.h: the mean position and normal of every point over its own
// view and its agreeing sources (apd_fusion::mean_point, apd_fusion_math.h: contract C9).  A pure function of (points, maps): a
// point names its view and its agreeing sources, its stored xyz is the very P the fusion projected into them, and the source
// pixel is a function of P (vote_target) -- so the mean is computed after the fact, one lane per point, in no order, by
// k_points_average.  There is no host path: host-resident points and host maps go up, the kernel runs on the points' device, the
// four arrays it writes come down.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_fusion_math.h"
#include "apd_points_host.h"

namespace {

using apd_fusion::MapView;
using apd_fusion::PointArrays;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;

// Point k < n of `in` averaged into `out` (xyz, normal, sources = the sources that contributed, support = their number).  One lane
// per point; each lane walks its mask (mean_point: at most 32 rounds) and gathers up to 32 x (4 + 12) bytes from the maps.  No
// LDS, no atomics; every offset is a size_t.
__global__ __launch_bounds__(256) void k_points_average(const MapView *__restrict__ views, const int *__restrict__ pair_offsets,
                                                         const int *__restrict__ pair_indices, size_t n, const float *__restrict__ xyz,
                                                         const float *__restrict__ normal, const int32_t *__restrict__ view,
                                                         const uint32_t *__restrict__ sources, PointArrays out)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    const int v = view[k];
    const int first = pair_offsets[v];
    const float P[3] = {xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]};
    const float nr[3] = {normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]};
    float meanP[3], meanN[3];
    uint32_t kept;
    int used;
    apd_fusion::mean_point(views, pair_indices + first, pair_offsets[v + 1] - first, P, nr, sources[k], meanP, meanN, kept, used);
    for (int c = 0; c < 3; ++c) {
        out.xyz[3 * k + c] = meanP[c];
        out.normal[3 * k + c] = meanN[c];
    }
    out.sources[k] = kept;
    out.support[k] = (uint8_t)used;
}

std::string &err() { return apd_fusion::g_fusion_error; }

int hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(err(), APD_ERR_HIP, "apd_points_average: %s: %s", expr, hipGetErrorString(e));
}

// What apd_points_average refuses, before any device call
int check_average(apd_points_t p, int num_views, const apd_camera *cameras, const float *const *depths, const float *const *normals,
                  const int *rows, const int *cols, apd_points_t *out)
{
    if (!p || !cameras || !depths || !normals || !rows || !cols || !out) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_average: null argument");
    }
    if (p->merged) {  // its sources are its representative's: there is no list of maps to average a merged point over
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_average: merged points name no sources");
    }
    if (num_views != (int)p->rows.size()) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_average: %d views, the fusion of the points had %d", num_views, (int)p->rows.size());
    }
    for (int i = 0; i < num_views; ++i) {
        if (rows[i] != p->rows[(size_t)i] || cols[i] != p->cols[(size_t)i]) {
            return apd::set_error(err(), APD_ERR_INVALID, "apd_points_average: view %d has %d x %d pixels, in the fusion of the points it had %d x %d", i,
                                  cols[i], rows[i], p->cols[(size_t)i], p->rows[(size_t)i]);
        }
    }
    for (int s : p->pair_indices) {
        if (!depths[s] || !normals[s]) {
            return apd::set_error(err(), APD_ERR_INVALID, "apd_points_average: view %d is a source and has no %s map", s, depths[s] ? "normal" : "depth");
        }
    }
    return APD_OK;
}

int average(apd_points_t p, int num_views, const apd_camera *cameras, const float *const *depths, const float *const *normals,
            int maps_on_device, apd_points *result)
{
    const size_t n = (size_t)p->count;
    const size_t nblocks = (n + 255) / 256;
    if (nblocks > 0x7fffffffull) {
        return apd::set_error(err(), APD_ERR_UNSUPPORTED, "apd_points_average: %lld points are more than one launch takes", p->count);
    }
    HIP_TRY(hipSetDevice(p->device));
    Scratch scratch;
    // the view table, built and uploaded once: geometry, and the maps of the views some list names
    std::vector<char> named((size_t)num_views, 0);
    for (int s : p->pair_indices) {
        named[(size_t)s] = 1;
    }
    std::vector<MapView> hv((size_t)num_views);
    for (int i = 0; i < num_views; ++i) {
        MapView &v = hv[(size_t)i];
        apd_fusion::view_geometry(cameras[i], p->rows[(size_t)i], p->cols[(size_t)i], v.geo);
        v.depth = nullptr;
        v.normal = nullptr;
        if (!named[(size_t)i]) {
            continue;
        }
        if (maps_on_device) {
            v.depth = depths[i];
            v.normal = normals[i];
        } else {
            const size_t px = (size_t)p->rows[(size_t)i] * (size_t)p->cols[(size_t)i];
            HIP_TRY(scratch.upload(depths[i], px * 4, &v.depth));
            HIP_TRY(scratch.upload(normals[i], px * 12, &v.normal));
        }
    }
    const MapView *dviews = nullptr;
    const int *pair_offsets = nullptr, *pair_indices = nullptr;
    HIP_TRY(scratch.upload(hv.data(), sizeof(MapView) * hv.size(), &dviews));
    HIP_TRY(scratch.upload(p->pair_offsets.data(), p->pair_offsets.size() * sizeof(int), &pair_offsets));
    HIP_TRY(scratch.upload(p->pair_indices.data(), p->pair_indices.size() * sizeof(int), &pair_indices));
    // the points the kernel reads, and the arrays it writes at their final size; the other three are copied as they are
    constexpr unsigned kRead = apd_fusion::kXyz | apd_fusion::kNormal | apd_fusion::kView | apd_fusion::kSources;
    constexpr unsigned kWritten = apd_fusion::kXyz | apd_fusion::kNormal | apd_fusion::kSources | apd_fusion::kSupport;
    constexpr unsigned kCopied = apd_fusion::kAllArrays & ~kWritten;
    PointArrays in = p->arrays, dev;
    if (!p->on_device) {
        HIP_TRY(alloc_arrays(scratch, in, n, kRead));
        HIP_TRY(copy_arrays(in, p->arrays, n, hipMemcpyHostToDevice, kRead));
    }
    HIP_TRY(alloc_arrays(scratch, dev, n, p->on_device ? apd_fusion::kAllArrays : kWritten));
    if (p->on_device) {
        HIP_TRY(copy_arrays(dev, in, n, hipMemcpyDeviceToDevice, kCopied));
    }
    hipLaunchKernelGGL(k_points_average, dim3((unsigned)nblocks), dim3(256), 0, 0, dviews, pair_offsets, pair_indices, n, (const float *)in.xyz,
                       (const float *)in.normal, (const int32_t *)in.view, (const uint32_t *)in.sources, dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (p->on_device) {
        keep_arrays(scratch, dev);
        result->arrays = dev;
        return APD_OK;
    }
    PointArrays &h = result->arrays;  // freed with `result` by the caller if anything below fails
    if (!alloc_host_arrays(h, n)) {
        return apd::set_error(err(), APD_ERR_HIP, "apd_points_average: out of host memory");
    }
    HIP_TRY(copy_arrays(h, dev, n, hipMemcpyDeviceToHost, kWritten));
    HIP_TRY(copy_arrays(h, p->arrays, n, hipMemcpyHostToHost, kCopied));
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_average(apd_points_t p, int num_views, const apd_camera *cameras, const float *const *depths,
                                  const float *const *normals, const int *rows, const int *cols, int maps_on_device, apd_points_t *out)
{
    err().clear();
    if (const int rc = check_average(p, num_views, cameras, depths, normals, rows, cols, out); rc != APD_OK) {
        return rc;
    }
    apd_points *result = apd_points_host::new_points_like(p);
    result->count = p->count;
    if (p->count > 0) {
        DeviceScope scope(true);
        const int rc = average(p, num_views, cameras, depths, normals, maps_on_device, result);
        if (rc != APD_OK) {
            apd_points_destroy(result);  // its arrays are host memory, or none yet
            return rc;
        }
    }
    *out = result;
    return APD_OK;
}
