// apd_points_nearest.h -- the search of contract C17 (the relation: apd_nearest_math.h) as the entry points that relate
// two clouds share it: the kernel k_nearest_in and, as methods of NearestSearch on the host frame of apd_points_search.h, what
// such a call refuses about the other cloud, the sorts of both clouds on one grid and the launch that answers the queries of one
// sorted cloud among the targets of another.  Used by apd_points_nearest.hip (apd_points_nearest, apd_points_score) and
// apd_points_align.hip (apd_points_align).  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_nearest_math.h"
#include "apd_points_host.h"
#include "apd_points_search.h"

namespace apd_nearest_search {
namespace {

using apd_points_grid::grid_of;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::for_each_candidate_around;
using apd_points_search::k_fill;
using apd_points_search::Search;
using apd_points_search::Sorted;

// Sorted query i < m with a candidate among the targets: distance[member[i]] and index[member[i]] by contract C17 (either may be
// null); the others keep what they have.  keys / xyz / member: the queries in cell order; target_*: the m_target > 0 targets in
// cell order, on the same grid.
__global__ __launch_bounds__(256) void k_nearest_in(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                     const uint32_t *__restrict__ member, uint32_t m, const uint64_t *__restrict__ target_keys,
                                                     const float *__restrict__ target_xyz, const uint32_t *__restrict__ target_member,
                                                     uint32_t m_target, float r2, float *__restrict__ distance, int32_t *__restrict__ index)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    int cell[3];
    apd_fusion::radius_cells_of_key(keys[i], cell);
    bool have = false;
    float best = 0.0f;
    uint32_t best_j = 0;
    for_each_candidate_around(target_keys, target_xyz, cell, m_target, [&](uint32_t at, const float Q[3]) {
        const float d2 = apd_fusion::radius_d2(P, Q);
        if (d2 <= r2 && (!have || d2 <= best)) {
            const uint32_t j = target_member[at];
            if (apd_fusion::nearest_takes(d2, j, have, best, best_j)) {
                have = true;
                best = d2;
                best_j = j;
            }
        }
        return false;
    });
    if (!have) {
        return;  // the fill
    }
    const size_t k = member[i];
    if (distance) {
        distance[k] = apd_fusion::nearest_distance(best);
    }
    if (index) {
        index[k] = (int32_t)best_j;  // fewer than 2^31 targets
    }
}

// One call of an entry point that searches one cloud in another
struct NearestSearch : Search {
    // What both calls refuse on top of Search::check of p: that of q, and a q that lives on another device than the one p computes on
    int check_other(apd_points_t p, apd_points_t q, const void *output, float radius, const float *origin3)
    {
        if (const int rc = check(q, output, radius, origin3); rc != APD_OK) {
            return rc;
        }
        if (q->on_device && q->device != p->device) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: the other points live on device %d, the computation runs on device %d", who, q->device,
                                  p->device);
        }
        return APD_OK;
    }

    // The n points at xyz (device memory on the current device) in cell order; n == 0: none
    int sorted(Scratch &scratch, const float *xyz, size_t n, Sorted &s) const
    {
        return n > 0 ? sort_into_cells(scratch, xyz, n, s) : (int)APD_OK;
    }

    // The answers for the n > 0 queries `from` against the targets `in`; distance and index (either may be null): n entries each
    // in device memory on the current device
    int search(const Sorted &from, size_t n, const Sorted &in, float *distance, int32_t *index) const
    {
        if (distance) {
            hipLaunchKernelGGL(k_fill<float>, grid_of(n), dim3(256), 0, 0, distance, n, apd_fusion::nearest_no_distance());
            HIP_TRY(hipGetLastError());
        }
        if (index) {
            hipLaunchKernelGGL(k_fill<int32_t>, grid_of(n), dim3(256), 0, 0, index, n, apd_fusion::kNearestNoIndex);
            HIP_TRY(hipGetLastError());
        }
        if (from.m > 0 && in.m > 0) {
            hipLaunchKernelGGL(k_nearest_in, grid_of(from.m), dim3(256), 0, 0, from.keys, from.xyz, from.member, (uint32_t)from.m, in.keys, in.xyz,
                               in.member, (uint32_t)in.m, grid.size * grid.size, distance, index);
            HIP_TRY(hipGetLastError());
        }
        return APD_OK;
    }

    // Selects p's device; both clouds' positions readable there and in cell order.  The same object is sorted once
    int both_sorted(Scratch &scratch, apd_points_t p, apd_points_t q, Sorted &sp, Sorted &sq) const
    {
        const float *xyz = nullptr, *other = nullptr;
        if (const int rc = positions(scratch, p, &xyz); rc != APD_OK) {
            return rc;
        }
        if (const int rc = sorted(scratch, xyz, (size_t)p->count, sp); rc != APD_OK) {
            return rc;
        }
        if (q == p) {
            sq = sp;
            return APD_OK;
        }
        if (const int rc = readable(scratch, q, (const float *)q->arrays.xyz, (size_t)q->count * 12, &other); rc != APD_OK) {
            return rc;
        }
        return sorted(scratch, other, (size_t)q->count, sq);
    }
};

}  // namespace
}  // namespace apd_nearest_search
