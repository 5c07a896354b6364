// apd_points.hip -- what is done with a fusion's points after the fusion: apd_points_average and apd_points_write_ply of
// include/apd_mi355x.h, and apd_points_create, which makes a points object of a caller's arrays.  (apd_points_merge_voxels:
// apd_points_merge.hip.)
//
// apd_points_create: the checks that make the arrays a cloud some fusion could have made (every later call relies on them: a
// view indexes the source lists, a bit of `sources` indexes a list), then one copy of each array, to host memory or to the device.
//
// apd_points_average: the mean position and normal of every point over its own view and its agreeing sources
// (apd_fusion::mean_point, apd_fusion_math.h: contract C9).  A pure function of (points, maps): a point names its view and its
// agreeing sources, its stored xyz is the very P the fusion projected into them, and the source pixel is a function of P
// (vote_target) -- so the mean is computed after the fact, one lane per point, in no order, by k_points_average.  There is no host
// path: host-resident points and host maps go up, the kernel runs on the points' device, the four arrays it writes come down.
//
// apd_points_write_ply: ExportPointCloud's file (APD.cpp:214-254) of any points object, the fusion's own or an averaged one: the
// header, then the 15-byte or 27-byte records k_fusion_compact packs (apd_fusion.hip), packed here on the host from the arrays
// (device-resident points come down in chunks).
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

// The object apd_points_average returns, without its arrays: where p lives, with p's source lists and view sizes
apd_points *like(const apd_points *p)
{
    apd_points *q = new apd_points();
    q->device = p->device;
    q->on_device = p->on_device;
    q->count = p->count;
    q->pair_offsets = p->pair_offsets;
    q->pair_indices = p->pair_indices;
    q->rows = p->rows;
    q->cols = p->cols;
    return q;
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
    // the points the kernel reads, and the arrays it writes at their final size
    const PointArrays &in = p->arrays;
    const float *xyz = in.xyz, *normal = in.normal;
    const int32_t *view = in.view;
    const uint32_t *sources = in.sources;
    if (!p->on_device) {
        HIP_TRY(scratch.upload(in.xyz, n * 12, &xyz));
        HIP_TRY(scratch.upload(in.normal, n * 12, &normal));
        HIP_TRY(scratch.upload(in.view, n * 4, &view));
        HIP_TRY(scratch.upload(in.sources, n * 4, &sources));
    }
    PointArrays dev;
    HIP_TRY(scratch.alloc(n * 12, &dev.xyz));
    HIP_TRY(scratch.alloc(n * 12, &dev.normal));
    HIP_TRY(scratch.alloc(n * 4, &dev.sources));
    HIP_TRY(scratch.alloc(n, &dev.support));
    if (p->on_device) {  // what is copied, device to device
        HIP_TRY(scratch.alloc(n * 3, &dev.bgr));
        HIP_TRY(scratch.alloc(n * 4, &dev.view));
        HIP_TRY(scratch.alloc(n * 4, &dev.pixel));
        HIP_TRY(hipMemcpy(dev.bgr, in.bgr, n * 3, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(dev.view, in.view, n * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(dev.pixel, in.pixel, n * 4, hipMemcpyDeviceToDevice));
    }
    hipLaunchKernelGGL(k_points_average, dim3((unsigned)nblocks), dim3(256), 0, 0, dviews, pair_offsets, pair_indices, n, xyz, normal, view, sources,
                       dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (p->on_device) {
        for (void *q : {(void *)dev.xyz, (void *)dev.normal, (void *)dev.sources, (void *)dev.support, (void *)dev.bgr, (void *)dev.view, (void *)dev.pixel}) {
            scratch.keep(q);
        }
        result->arrays = dev;
        return APD_OK;
    }
    PointArrays &h = result->arrays;  // freed with `result` by the caller if anything below fails
    h.xyz = (float *)malloc(n * 12);
    h.normal = (float *)malloc(n * 12);
    h.bgr = (uint8_t *)malloc(n * 3);
    h.support = (uint8_t *)malloc(n);
    h.view = (int32_t *)malloc(n * 4);
    h.pixel = (int32_t *)malloc(n * 4);
    h.sources = (uint32_t *)malloc(n * 4);
    if (!(h.xyz && h.normal && h.bgr && h.support && h.view && h.pixel && h.sources)) {
        return apd::set_error(err(), APD_ERR_HIP, "apd_points_average: out of host memory");
    }
    HIP_TRY(hipMemcpy(h.xyz, dev.xyz, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.normal, dev.normal, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.sources, dev.sources, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h.support, dev.support, n, hipMemcpyDeviceToHost));
    memcpy(h.bgr, in.bgr, n * 3);
    memcpy(h.view, in.view, n * 4);
    memcpy(h.pixel, in.pixel, n * 4);
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
    apd_points *result = like(p);
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

namespace {

int create_hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(err(), APD_ERR_HIP, "apd_points_create: %s: %s", expr, hipGetErrorString(e));
}

#define CREATE_REFUSE(...) return apd::set_error(err(), APD_ERR_INVALID, "apd_points_create: " __VA_ARGS__)

// What apd_points_create refuses, before anything is allocated
int check_create(long long count, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                 const int32_t *pixel, const uint32_t *sources, int num_views, const int *rows, const int *cols, const int *pair_offsets,
                 const int *pair_indices, apd_points_t *out)
{
    if (!rows || !cols || !pair_offsets || !out) {
        CREATE_REFUSE("null argument");
    }
    if (count < 0) {
        CREATE_REFUSE("a count of %lld points", count);
    }
    if (count > 0 && !(xyz && normal && bgr && support && view && pixel && sources)) {
        CREATE_REFUSE("null argument");
    }
    if (num_views < 1) {
        CREATE_REFUSE("%d views", num_views);
    }
    for (int i = 0; i < num_views; ++i) {
        if (rows[i] <= 0 || cols[i] <= 0) {
            CREATE_REFUSE("view %d has %d x %d pixels", i, cols[i], rows[i]);
        }
        if ((long long)rows[i] * cols[i] > 0x7fffffffLL) {
            CREATE_REFUSE("view %d has %d x %d pixels, more than a pixel index holds", i, cols[i], rows[i]);
        }
    }
    if (pair_offsets[0] != 0) {
        CREATE_REFUSE("pair_offsets starts at %d, not at 0", pair_offsets[0]);
    }
    for (int i = 0; i < num_views; ++i) {
        const int len = pair_offsets[i + 1] - pair_offsets[i];
        if (pair_offsets[i + 1] < pair_offsets[i]) {
            CREATE_REFUSE("pair_offsets descends at view %d", i);
        }
        if (len > APD_MAX_IMAGES) {
            CREATE_REFUSE("view %d has %d sources, more than %d", i, len, APD_MAX_IMAGES);
        }
    }
    if (pair_offsets[num_views] > 0 && !pair_indices) {
        CREATE_REFUSE("null argument");
    }
    for (int i = 0; i < num_views; ++i) {
        for (int e = pair_offsets[i]; e < pair_offsets[i + 1]; ++e) {
            if (pair_indices[e] < 0 || pair_indices[e] >= num_views) {
                CREATE_REFUSE("source %d of view %d is view %d of %d", e - pair_offsets[i], i, pair_indices[e], num_views);
            }
            if (pair_indices[e] == i) {
                CREATE_REFUSE("view %d is its own source", i);
            }
        }
    }
    for (long long k = 0; k < count; ++k) {
        const int v = view[k];
        if (v < 0 || v >= num_views) {
            CREATE_REFUSE("point %lld is of view %d of %d", k, v, num_views);
        }
        if (pixel[k] < 0 || pixel[k] >= rows[v] * cols[v]) {
            CREATE_REFUSE("point %lld is pixel %d of view %d, which has %d", k, pixel[k], v, rows[v] * cols[v]);
        }
        const int len = pair_offsets[v + 1] - pair_offsets[v];
        if (len < 32 && (sources[k] >> len) != 0) {
            CREATE_REFUSE("point %lld names sources 0x%x, its view %d has %d", k, sources[k], v, len);
        }
        if (__builtin_popcount(sources[k]) != (int)support[k]) {
            CREATE_REFUSE("point %lld names %d sources and has a support of %d", k, __builtin_popcount(sources[k]), (int)support[k]);
        }
    }
    return APD_OK;
}

#undef CREATE_REFUSE

// a copy of `bytes` caller bytes where the object lives
template <typename T> int create_copy(bool on_device, const T *from, size_t bytes, T **to)
{
    const auto hip_failed = create_hip_failed;
    if (on_device) {
        void *q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes));
        *to = static_cast<T *>(q);  // the object's from here on: apd_points_destroy frees it
        HIP_TRY(hipMemcpy(q, from, bytes, hipMemcpyHostToDevice));
        return APD_OK;
    }
    *to = static_cast<T *>(malloc(bytes));
    if (!*to) {
        return apd::set_error(err(), APD_ERR_HIP, "apd_points_create: out of host memory");
    }
    memcpy(*to, from, bytes);
    return APD_OK;
}

int create_arrays(apd_points *q, const float *xyz, const float *normal, const uint8_t *bgr, const uint8_t *support, const int32_t *view,
                  const int32_t *pixel, const uint32_t *sources)
{
    const auto hip_failed = create_hip_failed;
    const size_t n = (size_t)q->count;
    const bool dev = q->on_device != 0;
    if (dev) {
        HIP_TRY(hipSetDevice(q->device));
    }
    PointArrays &a = q->arrays;
    int rc = create_copy(dev, xyz, n * 12, &a.xyz);
    rc = rc != APD_OK ? rc : create_copy(dev, normal, n * 12, &a.normal);
    rc = rc != APD_OK ? rc : create_copy(dev, bgr, n * 3, &a.bgr);
    rc = rc != APD_OK ? rc : create_copy(dev, support, n, &a.support);
    rc = rc != APD_OK ? rc : create_copy(dev, view, n * 4, &a.view);
    rc = rc != APD_OK ? rc : create_copy(dev, pixel, n * 4, &a.pixel);
    return rc != APD_OK ? rc : create_copy(dev, sources, n * 4, &a.sources);
}

}  // namespace

extern "C" int apd_points_create(int device, int on_device, long long count, const float *xyz, const float *normal, const uint8_t *bgr,
                                 const uint8_t *support, const int32_t *view, const int32_t *pixel, const uint32_t *sources, int num_views,
                                 const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, apd_points_t *out)
{
    err().clear();
    if (const int rc = check_create(count, xyz, normal, bgr, support, view, pixel, sources, num_views, rows, cols, pair_offsets, pair_indices, out);
        rc != APD_OK) {
        return rc;
    }
    apd_points *q = new apd_points();
    q->device = device;
    q->on_device = on_device ? 1 : 0;
    q->count = count;
    q->pair_offsets.assign(pair_offsets, pair_offsets + num_views + 1);
    q->pair_indices.assign(pair_indices, pair_indices + pair_offsets[num_views]);
    q->rows.assign(rows, rows + num_views);
    q->cols.assign(cols, cols + num_views);
    if (count > 0) {
        DeviceScope scope(q->on_device != 0);
        if (const int rc = create_arrays(q, xyz, normal, bgr, support, view, pixel, sources); rc != APD_OK) {
            const std::string why = err();
            apd_points_destroy(q);  // the arrays made so far
            err() = why;
            return rc;
        }
    }
    *out = q;
    return APD_OK;
}

extern "C" int apd_points_write_ply(apd_points_t p, const char *path, int with_normals)
{
    err().clear();
    if (!p || !path) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_write_ply: null argument");
    }
    const size_t n = (size_t)p->count;
    const size_t floats = with_normals ? 6 : 3, record = 4 * floats + 3;
    const size_t kChunk = 1u << 20;  // points per download and per fwrite
    const PointArrays &a = p->arrays;
    std::vector<float> xyz, normal;
    std::vector<uint8_t> bgr, packed;
    DeviceScope scope(p->on_device && n > 0);
    if (p->on_device && n > 0) {
        const hipError_t e = hipSetDevice(p->device);
        if (e != hipSuccess) {
            return apd::set_error(err(), APD_ERR_HIP, "apd_points_write_ply: hipSetDevice: %s", hipGetErrorString(e));
        }
        xyz.resize(3 * std::min(n, kChunk));
        normal.resize(with_normals ? xyz.size() : 0);
        bgr.resize(xyz.size());
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        err() = std::string("apd_points_write_ply: cannot write ") + path;  // no length limit: not through set_error
        return APD_ERR_IO;
    }
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n%s"
               "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n", p->count,
            with_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "");
    bool ok = true;
    for (size_t k0 = 0; k0 < n && ok; k0 += kChunk) {
        const size_t m = std::min(n - k0, kChunk);
        const float *cx = a.xyz + 3 * k0, *cn = a.normal + 3 * k0;
        const uint8_t *cb = a.bgr + 3 * k0;
        if (p->on_device) {
            hipError_t e = hipMemcpy(xyz.data(), cx, m * 12, hipMemcpyDeviceToHost);
            e = e != hipSuccess || !with_normals ? e : hipMemcpy(normal.data(), cn, m * 12, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(bgr.data(), cb, m * 3, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                fclose(f);
                return apd::set_error(err(), APD_ERR_HIP, "apd_points_write_ply: download of the points: %s", hipGetErrorString(e));
            }
            cx = xyz.data();
            cn = normal.data();
            cb = bgr.data();
        }
        packed.resize(m * record);
        for (size_t k = 0; k < m; ++k) {  // little endian floats, as the host's memcpy writes them
            uint8_t *rec = packed.data() + k * record;
            memcpy(rec, cx + 3 * k, 12);
            if (with_normals) {
                memcpy(rec + 12, cn + 3 * k, 12);
            }
            memcpy(rec + 4 * floats, cb + 3 * k, 3);
        }
        ok = fwrite(packed.data(), 1, packed.size(), f) == packed.size();
    }
    if (fclose(f) != 0 || !ok) {
        err() = std::string("apd_points_write_ply: short write to ") + path;
        return APD_ERR_IO;
    }
    return APD_OK;
}
