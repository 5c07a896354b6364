// apd_points_radius.hip -- apd_points_neighbour_counts and apd_points_remove_sparse of include/apd_mi355x.h: how many other points
// every point has within a radius, and the object without the points that have too few (arithmetic contract C11; the
// relation: apd_radius_math.h).
//
// On the points' device, on its null stream, on top of the sort and the scan of apd_sort.h (the refusals, steps 1 to 3, the walk
// of step 4, the flags of step 5 and the host frame of both entry points: apd_points_search.h, shared with the statistical filter,
// the clusters and the normals):
//   1. k_voxel_keys, scan, k_voxel_compact (apd_points_grid.h): (key, input index) of the points inside the grid of cell size
//      `radius`, in input order.
//   2. sort_pairs: the points of a cell together, the cells in key order -- x fastest, so the three x-adjacent cells of a (y, z)
//      row are one contiguous run of the sorted keys.
//   3. k_gather_xyz: the positions in sorted order.
//   4. k_neighbour_count: one lane per point in sorted order; for_each_candidate: for each of the 9 (dz, dy) rows around its cell
//      a binary search for the start of the run and a walk to its end.  Lanes of a wave stand next to each other in sorted order: they mostly share
//      their cell, so their searches take the same branches and their candidate loads go to the same address.  A lane leaves the
//      walk at `cap`.  No LDS, no atomics; the count goes to the point's input index, a point outside the grid keeps 0.
//   5. removal: k_keep_flags, compact_points (apd_points.hip).
// The work is the number of (point, candidate in the 27 cells) pairs: with cap == 0 a cell of m members costs m * m distance
// tests, each lane of the cell walking all m; the removal runs with cap = min_neighbours and is bounded by that early exit in
// dense regions.  There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_radius_math.h"

namespace {

using apd_fusion::PointArrays;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::for_each_candidate;
using apd_points_search::k_keep_flags;
using apd_points_search::Search;
using apd_points_search::Sorted;
using apd_points_search::Staged;

// Sorted element i < m: counts[member[i]] = min(neighbours, cap) by contract C11.  keys: ascending; xyz: in the same order.
// The walk (apd_points_search.h) hands over every point of the 27 cells around the lane's; what is left of the relation is the
// index and the distance.  The walk ends where the count reaches `cap`.
__global__ __launch_bounds__(256) void k_neighbour_count(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                          const uint32_t *__restrict__ member, uint32_t m, float r2, uint32_t cap,
                                                          uint32_t *__restrict__ counts)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    uint32_t count = 0;
    for_each_candidate(keys, xyz, i, m, [&](uint32_t at, const float Q[3]) {
        if (at != i && apd_fusion::radius_within(P, Q, r2)) {
            ++count;
            return count == cap;  // cap == 0: never
        }
        return false;
    });
    counts[member[i]] = count;
}

// One call of either entry point: the refusals, the cell order and the host frame of apd_points_search.h, and the step the two share
struct Call : Search {
    // counts[k] for the n > 0 points at xyz; both in device memory on the current device
    int count_neighbours(const float *xyz, size_t n, uint32_t cap, uint32_t *counts) const
    {
        Scratch scratch;
        HIP_TRY(hipMemsetAsync(counts, 0, n * 4, 0));  // the points outside the grid
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK || s.m == 0) {
            return rc;
        }
        hipLaunchKernelGGL(k_neighbour_count, grid_of(s.m), dim3(256), 0, 0, s.keys, s.xyz, s.member, (uint32_t)s.m, grid.size * grid.size, cap, counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_points_neighbour_counts of p (count > 0)
    int counts_of(apd_points_t p, uint32_t cap, uint32_t *counts) const
    {
        Scratch scratch;
        const float *xyz = nullptr;
        Staged<uint32_t> out;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : stage(scratch, p, counts, (size_t)p->count * 4, out);
        rc = rc != APD_OK ? rc : count_neighbours(xyz, (size_t)p->count, cap, out.device);
        return rc != APD_OK ? rc : download(out);
    }

    // apd_points_remove_sparse of p (count > 0) into `result`
    int remove_sparse(apd_points_t p, uint32_t min_neighbours, apd_points *result) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        uint32_t *counts = nullptr, *keep = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &counts));
        HIP_TRY(scratch.alloc(n * 4, &keep));
        if (min_neighbours == 0) {  // every point stays, those outside the grid too: nothing to count
            HIP_TRY(hipMemsetAsync(counts, 0, n * 4, 0));
        } else if (const int rc = count_neighbours(in.xyz, n, min_neighbours, counts); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_keep_flags, grid_of(n), dim3(256), 0, 0, (const uint32_t *)counts, n, min_neighbours, keep);
        HIP_TRY(hipGetLastError());
        return apd_points_host::compact_points(who, p, in, keep, result);
    }
};

}  // namespace

extern "C" int apd_points_neighbour_counts(apd_points_t p, float radius, const float *origin3, unsigned cap, uint32_t *counts)
{
    Call call{{"apd_points_neighbour_counts"}};
    if (const int rc = call.check(p, counts, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.counts_of(p, cap, counts);
}

extern "C" int apd_points_remove_sparse(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, apd_points_t *out,
                                        long long *removed)
{
    Call call{{"apd_points_remove_sparse"}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    const auto body = [&](apd_points *result) { return call.remove_sparse(p, min_neighbours, result); };
    return call.into_new_points(p, out, removed, body);
}
