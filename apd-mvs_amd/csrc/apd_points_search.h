// apd_points_search.h -- what every search of the 27 cells around a point shares (apd_points_radius.hip: contract C11,
// apd_points_knn.hip: C12, apd_points_clusters.hip: C13, apd_points_normals.hip: C14, apd_points_smooth.hip: C16,
// apd_points_nearest.hip: C17).
// Device: the positions gathered into cell order (k_gather_xyz), the binary search for a (dz, dy) row's run (lower_bound), THE walk
// over the 27 cells (for_each_candidate_around: the one place where the x range is clamped and a row outside the grid skipped, around
// a cell given as integers; for_each_candidate: around the cell of a member, the one place where a key is decoded), a typed fill, the
// flags "v[k] >= bound" of the removals and the binary64 chunk sums of contract C12 (k_chunk_sums).
// Host, as methods of Search, one call of an entry point: what such a call refuses before any device is touched (check); the points
// inside the grid of cell size `radius` brought into cell order -- keys, scan, compaction (apd_points_grid.h), the stable sort of
// (key, input index), the gather -- ready for a kernel with one lane per point in sorted order (sort_into_cells); where a query
// reads the points and writes its answer when they are host-resident (positions, readable, stage, download); the seven arrays a
// removal compacts (device_arrays); the totals of the chunk sums (chunk_totals); and the tail of an entry point that hands a new object back (into_new_points).  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_knn_math.h"
#include "apd_points_grid.h"
#include "apd_points_host.h"
#include "apd_radius_math.h"
#include "apd_sort.h"

namespace apd_points_search {
namespace {

using apd_points_grid::Grid;
using apd_points_grid::grid_of;
using apd_points_grid::k_voxel_compact;
using apd_points_grid::k_voxel_keys;
using apd_points_host::Scratch;

template <typename T> __global__ __launch_bounds__(256) void k_fill(T *__restrict__ out, size_t n, T value)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        out[k] = value;
    }
}

// keep[k] = 1 where v[k] reaches `bound`: a count capped at min_neighbours, the size of a component
__global__ __launch_bounds__(256) void k_keep_flags(const uint32_t *__restrict__ v, size_t n, uint32_t bound, uint32_t *__restrict__ keep)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        keep[k] = v[k] >= bound ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_gather_xyz(const float *__restrict__ xyz, const uint32_t *__restrict__ member, size_t m,
                                                     float *__restrict__ sorted_xyz)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        const size_t k = member[i];
        sorted_xyz[3 * i] = xyz[3 * k];
        sorted_xyz[3 * i + 1] = xyz[3 * k + 1];
        sorted_xyz[3 * i + 2] = xyz[3 * k + 2];
    }
}

// Chunk c < chunks of kKnnChunk consecutive input indices: its sums by contract C12.  One lane per chunk: the order of a
// binary64 sum is the contract
__global__ __launch_bounds__(64) void k_chunk_sums(const float *__restrict__ mean, size_t n, size_t chunks, double *__restrict__ s1,
                                                    double *__restrict__ s2, uint32_t *__restrict__ full)
{
    const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= chunks) {
        return;
    }
    const size_t first = c * apd_fusion::kKnnChunk;
    const size_t count = n - first < (size_t)apd_fusion::kKnnChunk ? n - first : (size_t)apd_fusion::kKnnChunk;
    double a = 0.0, b = 0.0;
    unsigned f = 0;
    apd_fusion::knn_chunk_sums(mean + first, count, a, b, f);
    s1[c] = a;
    s2[c] = b;
    full[c] = f;
}

// the first position in [from, m) whose key is not below `want`
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *__restrict__ keys, uint32_t from, uint32_t m, uint64_t want)
{
    uint32_t lo = from, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// The walk.  Sorted element i (keys: ascending; xyz: in the same order): f(at, Q) for every sorted position at < end in the 27
// cells around i's, Q its position, i itself included when i < end; f returns true to end the walk.  The positions are visited in
// ASCENDING order, each once -- contract C14 adds its binary64 sums in this order, and the link of C13 relies on everything
// after the first position >= end being above it too: the 9 (dz, dy) rows are taken in ascending key order -- x is the fastest field
// of a key, so the three x-adjacent cells of a row are one run of the sorted keys, found by one binary search that starts where
// the row before ended.  The x range is clamped and a row whose y or z cell leaves the grid is skipped: a search bound never
// borrows into the next field of the key.  Every candidate lies in a cell adjacent to i's by construction; what is left of the
// relation of apd_radius_math.h is the index and the distance, which are f's.  No read of keys or xyz reaches position `end` but
// that of keys[i]: end = m walks all 27 cells, end = i the part of them below i.
//
// for_each_candidate_around is that walk around a cell given as three integers (each in [-2^20, 2^20)), which need not hold a
// member of the cloud walked: keys / xyz may be another cloud's than the one the cell was taken from (apd_points_nearest.hip,
// contract C17), and then no read reaches position `end` at all.  for_each_candidate is the walk around the cell of member i.
//
// for_each_position_around is the walk itself: f(at) for every such position, whatever stands there -- a point's xyz for
// for_each_candidate_around, the face of a (cell, face) pair for apd_mesh_nearest.hip (contract C27).
template <typename F> __device__ __forceinline__ void for_each_position_around(const uint64_t *__restrict__ keys, const int cell[3], uint32_t end, F &&f)
{
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    const int x0 = cell[0] > lo ? cell[0] - 1 : lo, x1 = cell[0] < hi ? cell[0] + 1 : hi;
    uint32_t at = 0;
    for (int dz = -1; dz <= 1 && at < end; ++dz) {
        const int cz = cell[2] + dz;
        if (cz < lo || cz > hi) {
            continue;
        }
        for (int dy = -1; dy <= 1 && at < end; ++dy) {
            const int cy = cell[1] + dy;
            if (cy < lo || cy > hi) {
                continue;
            }
            const uint64_t last = apd_fusion::radius_key(x1, cy, cz);
            at = lower_bound(keys, at, end, apd_fusion::radius_key(x0, cy, cz));
            for (; at < end && keys[at] <= last; ++at) {
                if (f(at)) {
                    return;
                }
            }
        }
    }
}

template <typename F>
__device__ __forceinline__ void for_each_candidate_around(const uint64_t *__restrict__ keys, const float *__restrict__ xyz, const int cell[3], uint32_t end,
                                                          F &&f)
{
    for_each_position_around(keys, cell, end, [&](uint32_t at) {
        const float Q[3] = {xyz[3 * (size_t)at], xyz[3 * (size_t)at + 1], xyz[3 * (size_t)at + 2]};
        return f(at, Q);
    });
}

template <typename F>
__device__ __forceinline__ void for_each_candidate(const uint64_t *__restrict__ keys, const float *__restrict__ xyz, uint32_t i, uint32_t end, F &&f)
{
    int cell[3];
    apd_fusion::radius_cells_of_key(keys[i], cell);
    for_each_candidate_around(keys, xyz, cell, end, static_cast<F &&>(f));
}

std::string &err() { return apd_fusion::g_fusion_error; }

// The m points inside the grid in cell order: device memory of the call's Scratch
struct Sorted {
    size_t m = 0;
    const uint64_t *keys = nullptr;    // ascending
    const uint32_t *member = nullptr;  // the input index of sorted element i
    const float *xyz = nullptr;        // its position
};

// An output of a query on p, where the kernels write it and where the caller wants it
template <typename T> struct Staged {
    T *device = nullptr;  // the caller's own pointer when p is device-resident, scratch otherwise; null: the caller wants none, and what
                          // the call needs all the same (the sizes of apd_points_components) it allocates itself
    T *host = nullptr;    // where download() brings it: null when `device` is the caller's
    size_t bytes = 0;
};

// One call of an entry point: its name, which starts every message, and the steps the searches share
struct Search {
    const char *const who;
    Grid grid = {{0.0f, 0.0f, 0.0f}, 0.0f};

    int hip_failed(const char *expr, hipError_t e, const char *, int) const  // what HIP_TRY returns
    {
        return apd::set_error(err(), APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
    }

    // What every call refuses before any device is touched; fills `grid`
    int check(apd_points_t p, const void *output, float radius, const float *origin3)
    {
        err().clear();
        if (!p || !output) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: null argument", who);
        }
        if (!(isfinite(radius) && radius > 0.0f)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a radius of %g, not a positive finite number", who, (double)radius);
        }
        const float r2 = radius * radius;
        if (!(isfinite(r2) && r2 > 0.0f)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a radius of %g, whose square %g is not a positive finite number", who, (double)radius,
                                  (double)r2);
        }
        grid.size = radius;
        for (int a = 0; origin3 && a < 3; ++a) {
            if (!isfinite(origin3[a])) {
                return apd::set_error(err(), APD_ERR_INVALID, "%s: origin component %d is %g", who, a, (double)origin3[a]);
            }
            grid.origin[a] = origin3[a];
        }
        if (p->count >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld points, 2^31 or more (the sort carries a 32-bit index)", who, p->count);
        }
        return APD_OK;
    }

    // The n > 0 points at xyz (device memory on the current device) that lie inside the grid, in cell order, on the null stream;
    // s.m == 0: none, and nothing else of s is set.  The memory is `scratch`'s
    int sort_into_cells(Scratch &scratch, const float *xyz, size_t n, Sorted &s) const
    {
        uint64_t *key = nullptr, *at = nullptr, *keys[2] = {nullptr, nullptr};
        uint32_t *keep = nullptr, *index[2] = {nullptr, nullptr};
        HIP_TRY(scratch.alloc(n * 8, &key));
        HIP_TRY(scratch.alloc(n * 4, &keep));
        HIP_TRY(scratch.alloc((n + 1) * 8, &at));
        hipLaunchKernelGGL(k_voxel_keys, grid_of(n), dim3(256), 0, 0, xyz, n, grid, key, keep);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(keep, at, n));
        uint64_t inside = 0;
        HIP_TRY(hipMemcpy(&inside, at + n, 8, hipMemcpyDeviceToHost));
        s.m = (size_t)inside;
        if (s.m == 0) {
            return APD_OK;
        }
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(scratch.alloc(s.m * 8, &keys[b]));
            HIP_TRY(scratch.alloc(s.m * 4, &index[b]));
        }
        hipLaunchKernelGGL(k_voxel_compact, grid_of(n), dim3(256), 0, 0, (const uint64_t *)key, (const uint32_t *)keep, (const uint64_t *)at, n, keys[0],
                           index[0]);
        HIP_TRY(hipGetLastError());
        int side = 0;
        HIP_TRY(apd_sort::sort_pairs(keys[0], keys[1], index[0], index[1], s.m, &side, nullptr));
        float *sorted_xyz = nullptr;
        HIP_TRY(scratch.alloc(s.m * 12, &sorted_xyz));
        hipLaunchKernelGGL(k_gather_xyz, grid_of(s.m), dim3(256), 0, 0, xyz, (const uint32_t *)index[side], s.m, sorted_xyz);
        HIP_TRY(hipGetLastError());
        s.keys = keys[side];
        s.member = index[side];
        s.xyz = sorted_xyz;
        return APD_OK;
    }

    // *out = `own`, one of p's arrays of `bytes` bytes, where a kernel can read it: itself if p is device-resident, an upload owned by
    // `scratch` otherwise.  p's device is the current one
    template <typename T> int readable(Scratch &scratch, apd_points_t p, const T *own, size_t bytes, const T **out) const
    {
        *out = own;
        if (!p->on_device) {
            HIP_TRY(scratch.upload(own, bytes, out));
        }
        return APD_OK;
    }

    // A query's first step: selects p's device; *xyz = p's positions, readable
    int positions(Scratch &scratch, apd_points_t p, const float **xyz) const
    {
        HIP_TRY(hipSetDevice(p->device));
        return readable(scratch, p, (const float *)p->arrays.xyz, (size_t)p->count * 12, xyz);
    }

    // A removal's first step: selects p's device; in = p's seven arrays, readable: host-resident points send every array up once,
    // for the search and for the compaction
    int device_arrays(Scratch &scratch, apd_points_t p, apd_fusion::PointArrays &in) const
    {
        const size_t n = (size_t)p->count;
        HIP_TRY(hipSetDevice(p->device));
        in = p->arrays;
        if (!p->on_device) {
            HIP_TRY(alloc_arrays(scratch, in, n));
            HIP_TRY(copy_arrays(in, p->arrays, n, hipMemcpyHostToDevice));
        }
        return APD_OK;
    }

    // The caller's output `out` of `bytes` bytes (null: not wanted, and s.device stays null) as a query on p writes it
    template <typename T> int stage(Scratch &scratch, apd_points_t p, T *out, size_t bytes, Staged<T> &s) const
    {
        s.device = out;
        s.bytes = bytes;
        s.host = out && !p->on_device ? out : nullptr;
        if (s.host) {
            HIP_TRY(scratch.alloc(bytes, &s.device));
        }
        return APD_OK;
    }

    template <typename T> int download(const Staged<T> &s) const
    {
        if (s.host) {
            HIP_TRY(hipMemcpy(s.host, s.device, s.bytes, hipMemcpyDeviceToHost));
        }
        return APD_OK;
    }

    // The totals of contract C12 over the n > 0 values at v (device memory on the current device): k_chunk_sums, the chunk sums --
    // n / 256 triples, never the n values -- come down and the host adds them in ascending order.  *S2 may be null
    int chunk_totals(const float *v, size_t n, double *S1, double *S2, unsigned long long *n_f) const
    {
        const size_t chunks = (n + apd_fusion::kKnnChunk - 1) / apd_fusion::kKnnChunk;
        Scratch scratch;
        double *s1 = nullptr, *s2 = nullptr;
        uint32_t *full = nullptr;
        HIP_TRY(scratch.alloc(chunks * 8, &s1));
        HIP_TRY(scratch.alloc(chunks * 8, &s2));
        HIP_TRY(scratch.alloc(chunks * 4, &full));
        hipLaunchKernelGGL(k_chunk_sums, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, 0, v, n, chunks, s1, s2, full);
        HIP_TRY(hipGetLastError());
        std::vector<double> h1(chunks), h2(chunks);
        std::vector<uint32_t> hf(chunks);
        HIP_TRY(hipMemcpy(h1.data(), s1, chunks * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h2.data(), s2, chunks * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hf.data(), full, chunks * 4, hipMemcpyDeviceToHost));
        double t1 = 0.0, t2 = 0.0;
        unsigned long long count = 0;
        for (size_t c = 0; c < chunks; ++c) {
            t1 = t1 + h1[c];
            t2 = t2 + h2[c];
            count += hf[c];
        }
        *S1 = t1;
        if (S2) {
            *S2 = t2;
        }
        *n_f = count;
        return APD_OK;
    }

    // The tail of an entry point that answers with a new object like p: body(result) fills it from p (count > 0) with p's device
    // current or fails with its message set, which stays the last error; an empty p gives an empty object and touches no device.
    // *removed (may be null): how many points fewer the result has
    template <typename Body> int into_new_points(apd_points_t p, apd_points_t *out, long long *removed, Body &&body) const
    {
        apd_points *result = apd_points_host::new_points_like(p);
        result->merged = p->merged;
        if (p->count > 0) {
            apd_points_host::DeviceScope scope(true);
            if (const int rc = body(result); rc != APD_OK) {
                const std::string why = err();
                apd_points_destroy(result);  // its arrays are host memory, or none yet
                err() = why;
                return rc;
            }
        }
        *out = result;
        if (removed) {
            *removed = p->count - result->count;
        }
        return APD_OK;
    }
};

}  // namespace
}  // namespace apd_points_search
