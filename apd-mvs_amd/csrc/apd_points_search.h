// apd_points_search.h -- what every search of the 27 cells around a point shares (apd_points_radius.hip: contract C11,
// apd_points_knn.hip: contract C12): what such a call refuses before any device is touched, and the points inside the grid of
// cell size `radius` brought into cell order -- keys, scan, compaction (apd_points_grid.h), the stable sort of (key, input index)
// and the positions gathered into sorted order -- ready for a kernel with one lane per point in sorted order; and the binary
// search such a kernel finds a (dz, dy) row's run with.  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_grid.h"
#include "apd_points_host.h"
#include "apd_sort.h"

namespace apd_points_search {
namespace {

using apd_points_grid::Grid;
using apd_points_grid::grid_of;
using apd_points_grid::k_voxel_compact;
using apd_points_grid::k_voxel_keys;
using apd_points_host::Scratch;

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

std::string &err() { return apd_fusion::g_fusion_error; }

// The m points inside the grid in cell order: device memory of the call's Scratch
struct Sorted {
    size_t m = 0;
    const uint64_t *keys = nullptr;    // ascending
    const uint32_t *member = nullptr;  // the input index of sorted element i
    const float *xyz = nullptr;        // its position
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
};

}  // namespace
}  // namespace apd_points_search
