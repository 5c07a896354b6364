// apd_points_grid.h -- the first steps of everything that puts a cloud on a cubic grid (apd_points_merge.hip: contract C10,
// apd_points_radius.hip: contract C11): the key of every point and whether it has one (k_voxel_keys), and the (key, input index)
// pairs of the points that have, in input order (k_voxel_compact), ready for apd_sort::sort_pairs.  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "apd_voxel_math.h"

namespace apd_points_grid {
namespace {

struct Grid {
    float origin[3];
    float size;
};

__global__ __launch_bounds__(256) void k_voxel_keys(const float *__restrict__ xyz, size_t n, Grid grid, uint64_t *__restrict__ key,
                                                     uint32_t *__restrict__ keep)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    const float P[3] = {xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]};
    uint64_t code = 0;
    const bool kept = apd_fusion::voxel_key(P, grid.origin, grid.size, code);
    key[k] = code;
    keep[k] = kept ? 1u : 0u;
}

// at[k]: kept points before point k
__global__ __launch_bounds__(256) void k_voxel_compact(const uint64_t *__restrict__ key, const uint32_t *__restrict__ keep,
                                                        const uint64_t *__restrict__ at, size_t n, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ index)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n && keep[k]) {
        keys[at[k]] = key[k];
        index[at[k]] = (uint32_t)k;
    }
}

inline dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }  // n < 2^32: fits

}  // namespace
}  // namespace apd_points_grid
