// apd_points_host.h -- the points object (apd_points_t of include/apd_mi355x.h) and what the host side of every call on one
// shares: its arrays and the one table of them, the device of one call, the device memory of one call.  The object's life and its
// files: apd_points.hip.  Who fills one: the fusions (apd_fusion_call.hip), apd_points_average.hip, apd_points_merge.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <vector>

namespace apd_points_host {

inline double ms_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// Selects a device for one call and puts the caller's back
struct DeviceScope {
    int previous = -1;
    explicit DeviceScope(bool active)
    {
        if (active && hipGetDevice(&previous) != hipSuccess) {
            previous = -1;
        }
    }
    ~DeviceScope()
    {
        if (previous >= 0) {
            hipSetDevice(previous);
        }
    }
};

// Device memory of one call: freed when the call returns, in the order it was made, but for what it hands over
struct Scratch {
    std::vector<void *> owned;
    ~Scratch() { release(); }
    void release()
    {
        for (void *q : owned) {
            hipFree(q);
        }
        owned.clear();
    }
    template <typename T> hipError_t alloc(size_t bytes, T **out)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes > 0 ? bytes : 1);
        if (e == hipSuccess) {
            owned.push_back(q);
            *out = static_cast<T *>(q);
        }
        return e;
    }
    // a device copy of `bytes` host bytes
    template <typename T> hipError_t upload(const T *host, size_t bytes, const T **out)
    {
        T *copy = nullptr;
        hipError_t e = alloc(bytes, &copy);
        if (e == hipSuccess) {
            *out = copy;
            e = bytes > 0 ? hipMemcpy(copy, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
        }
        return e;
    }
    void keep(void *q) { owned.erase(std::find(owned.begin(), owned.end(), q)); }
};

// ExportPointCloud's header (APD.cpp:214-254) for `count` vertices, with or without nx ny nz
void write_ply_header(FILE *f, long long count, bool normals);

}  // namespace apd_points_host

namespace apd_fusion {

// The arrays of an apd_points_t: host memory (malloc) or device memory
struct PointArrays {
    float *xyz = nullptr, *normal = nullptr;
    uint8_t *bgr = nullptr, *support = nullptr;
    int32_t *view = nullptr, *pixel = nullptr;
    uint32_t *sources = nullptr;  // bit j: source j of the point's view is one of the votes counted in support
};

// a set of the arrays: one bit each
enum : unsigned { kXyz = 1, kNormal = 2, kBgr = 4, kSupport = 8, kView = 16, kPixel = 32, kSources = 64, kAllArrays = 127 };

// The table: which arrays a points object has and how many bytes each takes per point.  f(member, bytes per point, bit)
template <typename F> void for_each_array(F &&f)
{
    f(&PointArrays::xyz, (size_t)12, kXyz);
    f(&PointArrays::normal, (size_t)12, kNormal);
    f(&PointArrays::bgr, (size_t)3, kBgr);
    f(&PointArrays::support, (size_t)1, kSupport);
    f(&PointArrays::view, (size_t)4, kView);
    f(&PointArrays::pixel, (size_t)4, kPixel);
    f(&PointArrays::sources, (size_t)4, kSources);
}

// The operations on the table (apd_points.hip); `which`: the arrays they touch, the others stay as they are.
// Device arrays for n points, owned by `scratch` until keep_arrays
hipError_t alloc_arrays(apd_points_host::Scratch &scratch, PointArrays &p, size_t n, unsigned which = kAllArrays);
// the arrays of p are the caller's from here on
void keep_arrays(apd_points_host::Scratch &scratch, const PointArrays &p);
// Host arrays for n points; false: out of memory, and p holds what there was room for
bool alloc_host_arrays(PointArrays &p, size_t n);
void free_arrays(PointArrays &p, bool on_device);  // hipFree (on the current device) or free of each array
// n points of `from`, from point `first` on, to the start of `to`; hipMemcpyHostToHost is a memcpy
hipError_t copy_arrays(const PointArrays &to, const PointArrays &from, size_t n, hipMemcpyKind kind, unsigned which = kAllArrays, size_t first = 0);

}  // namespace apd_fusion

// One fusion's points (apd_points_t): the arrays are host memory (malloc) or device memory on `device`.
struct apd_points {
    int device = 0, on_device = 0;
    long long count = 0;
    apd_fusion::PointArrays arrays;
    std::vector<int> pair_offsets, pair_indices;  // the call's source lists: what bit j of sources[k] means
    std::vector<int> rows, cols;                  // the call's view sizes: what pixel[k] and a projection into a source mean
    // apd_points_visibility: built on the first call, where the arrays live (host: malloc; device: hipMalloc)
    long long *vis_offsets = nullptr;
    int32_t *vis_views = nullptr;
    // a result of apd_points_merge_voxels: made with its lists (the union of its members'), view / pixel / sources are its
    // representative's and say nothing about the lists
    int merged = 0;
};

namespace apd_points_host {

// A new object without points: where it lives, and the source lists and view sizes of a call or of another object
apd_points *new_points(int device, int on_device, int num_views, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices);
inline apd_points *new_points_like(const apd_points *p)
{
    return new_points(p->device, p->on_device, (int)p->rows.size(), p->rows.data(), p->cols.data(), p->pair_offsets.data(), p->pair_indices.data());
}

// The points k of p (count > 0, fewer than 2^31) with keep[k] != 0 -- `keep`: count flags of 0 or 1 in device memory on p's device,
// which is the current one; `in`: p's arrays on that device, its own or the caller's upload of them -- in p's order into `result`
// (of new_points_like(p), without arrays so far): a scan of the flags and one gather per array of the table, on the null stream.
// The result of host-resident points comes down.  A merged p hands the kept points' lists on (new offsets by a 64-bit scan of the
// kept lengths) and result->merged = 1; any other result builds its lists from its sources like p.  Messages start with `who`;
// on failure the caller destroys `result`.
int compact_points(const char *who, const apd_points *p, const apd_fusion::PointArrays &in, const uint32_t *keep, apd_points *result);

}  // namespace apd_points_host
