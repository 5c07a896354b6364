// apd_render_device.h -- what the two renderers share on the device (apd_points_render.hip: a cloud's splats; apd_mesh_render.hip: a
// mesh's faces): the image of 64-bit keys of one camera, cleared to the empty key, offered keys with an atomic min and resolved into
// the depth and the index map.  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include "apd_lab.h"
#include "apd_render_math.h"

namespace apd_render_device {
namespace {

__global__ __launch_bounds__(256) void k_render_clear(uint64_t *__restrict__ keys, size_t px)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < px) {
        keys[i] = apd_fusion::kRenderEmptyKey;
    }
}

// `key` to one pixel: a 64-bit unsigned atomic min, relaxed, agent scope.  The min of integers does not depend on the order of
// arrival.  Before it a relaxed load of the pixel skips the atomic when the key held there is already smaller: keys only ever
// decrease, so a value read early can only be too large and a skip decided on it stays right.  The load is an agent-scope one,
// served by the L2 where the atomics execute: a plain load may be served by a line of the CU's L1 that no atomic ever updates.
__device__ __forceinline__ void render_offer(uint64_t *pixel, uint64_t key)
{
#if APD_RENDER_LOAD_BEFORE_MIN
    if (__hip_atomic_load(pixel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) {
        return;
    }
#endif
    __hip_atomic_fetch_min(pixel, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// depth and index (either may be null) of the px pixels of a key image
__global__ __launch_bounds__(256) void k_render_resolve(const uint64_t *__restrict__ keys, size_t px, float *__restrict__ depth,
                                                         uint32_t *__restrict__ index)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) {
        return;
    }
    const uint64_t key = keys[i];
    if (depth) {
        depth[i] = apd_fusion::render_depth(key);
    }
    if (index) {
        index[i] = apd_fusion::render_index(key);
    }
}

}  // namespace
}  // namespace apd_render_device
