// apd_points_smooth.hip -- apd_points_smoothed_positions and apd_points_with_smoothed_positions of include/apd_mi355x.h: every
// point's position projected on the weighted least-squares plane of its neighbourhood within a radius, once or iterated, and the
// object with those positions in place of the stored ones (arithmetic contract C16; the relation: apd_smooth_math.h).
// The fifth search on the walk and the host frame of apd_points_search.h.
//
// On the points' device, on its null stream, per iteration:
//   1. k_smooth_fill: the position copied and +inf for every point -- what a point outside the grid and a point with fewer than
//      min_neighbours neighbours keep.
//   2. the points inside the grid in cell order (Search::sort_into_cells), from the positions of this iteration.
//   3. k_point_smooth: one lane per point in sorted order, the walk over the 27 cells (for_each_candidate with end = m), which
//      never ends early, and for each candidate within the radius the weight and the ten weighted binary64 sums; then, in the same
//      lane, the solve of contract C14 on those sums and the projection.  The result goes to the point's input index.  No LDS, no
//      atomics, no array indexed by a runtime value: sums, matrix and vectors stay in registers.
// with_smoothed_positions: the iterations run between two position buffers on the device, each with a Scratch of its own for the
// sort, released before the next; a flag per point collects "had an estimate in some iteration" by plain stores; then
// compact_points (apd_points.hip) with every flag set and the new positions in the place of the stored ones.
// There is no host path: host-resident points go up once, the result comes down once.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_smooth_math.h"
#include "apd_sort.h"

namespace {

using apd_fusion::PointArrays;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::for_each_candidate;
using apd_points_search::k_fill;
using apd_points_search::Search;
using apd_points_search::Sorted;
using apd_points_search::Staged;

// "No estimate" for every point: the position copied and +inf; either output may be null
__global__ __launch_bounds__(256) void k_smooth_fill(const float *__restrict__ xyz, size_t n, float *__restrict__ smoothed, float *__restrict__ offset)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    if (smoothed) {
        smoothed[3 * k] = xyz[3 * k];
        smoothed[3 * k + 1] = xyz[3 * k + 1];
        smoothed[3 * k + 2] = xyz[3 * k + 2];
    }
    if (offset) {
        offset[k] = apd_fusion::smooth_none();
    }
}

// Sorted element i < m with at least min_neighbours neighbours: smoothed[member[i]] and offset[member[i]] by contract C16 (either
// may be null), estimated[member[i]] = 1 (may be null); the others keep what they have.  keys: ascending; xyz: in the same
// order; stored: the stored normals by input index.  The lane's own position is one of the walk's candidates and its term, d = 0
// and w = 1, is added where the walk meets it.
__global__ __launch_bounds__(256) void k_point_smooth(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                       const uint32_t *__restrict__ member, uint32_t m, float r2, uint32_t min_neighbours,
                                                       const float *__restrict__ stored, float *__restrict__ smoothed,
                                                       float *__restrict__ offset, uint32_t *__restrict__ estimated)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    uint32_t count = 0;
    apd_fusion::NormalSums sums;
    for_each_candidate(keys, xyz, i, m, [&](uint32_t at, const float Q[3]) {
        if (apd_fusion::radius_within(P, Q, r2)) {  // the lane's own position passes: d2 = 0
            count += at != i ? 1u : 0u;
            apd_fusion::smooth_add(sums, P, Q, r2);
        }
        return false;
    });
    if (count < min_neighbours) {
        return;  // the fill
    }
    const size_t k = member[i];
    const float N[3] = {stored[3 * k], stored[3 * k + 1], stored[3 * k + 2]};
    float X[3], plane[3], h = 0.0f;
    unsigned sweeps = 0;
    bool capped = false;
    apd_fusion::smooth_project(sums, N, P, X, h, plane, sweeps, capped);
    if (smoothed) {
        smoothed[3 * k] = X[0];
        smoothed[3 * k + 1] = X[1];
        smoothed[3 * k + 2] = X[2];
    }
    if (offset) {
        offset[k] = h;
    }
    if (estimated) {
        estimated[k] = 1u;
    }
}

// One call of either entry point
struct Call : Search {
    unsigned min_neighbours = 0;

    // What both calls refuse on top of Search::check
    int check_min(unsigned want)
    {
        if (want < apd_fusion::kNormalMinNeighbours || want > apd_fusion::kNormalMaxNeighbours) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: min_neighbours = %u, not in %u .. %u", who, want, apd_fusion::kNormalMinNeighbours,
                                  apd_fusion::kNormalMaxNeighbours);
        }
        min_neighbours = want;
        return APD_OK;
    }

    int check_iterations(unsigned want) const
    {
        if (want < 1 || want > apd_fusion::kSmoothMaxIterations) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: iterations = %u, not in 1 .. %u", who, want, apd_fusion::kSmoothMaxIterations);
        }
        return APD_OK;
    }

    // One iteration on the n > 0 points at xyz with the stored normals at `stored` into smoothed and offset, each of which may be
    // null; estimated (may be null): set to 1 where a point has an estimate, left as it is elsewhere.  All in device memory on
    // the current device; smoothed is not xyz.  The sort's memory is released on return
    int iterate(const float *xyz, const float *stored, size_t n, float *smoothed, float *offset, uint32_t *estimated) const
    {
        Scratch scratch;
        hipLaunchKernelGGL(k_smooth_fill, grid_of(n), dim3(256), 0, 0, xyz, n, smoothed, offset);
        HIP_TRY(hipGetLastError());
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK) {
            return rc;
        }
        if (s.m > 0) {
            hipLaunchKernelGGL(k_point_smooth, grid_of(s.m), dim3(256), 0, 0, s.keys, s.xyz, s.member, (uint32_t)s.m, grid.size * grid.size,
                               (uint32_t)min_neighbours, stored, smoothed, offset, estimated);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());  // before the sort's memory goes
        return APD_OK;
    }

    // apd_points_smoothed_positions of p (count > 0): host-resident points send positions and normals up
    int smoothed_of(apd_points_t p, float *xyz3, float *offset) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        const float *xyz = nullptr, *stored = nullptr;
        Staged<float> out_xyz, out_offset;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : readable(scratch, p, (const float *)p->arrays.normal, n * 12, &stored);
        rc = rc != APD_OK ? rc : stage(scratch, p, xyz3, n * 12, out_xyz);
        rc = rc != APD_OK ? rc : stage(scratch, p, offset, n * 4, out_offset);
        rc = rc != APD_OK ? rc : iterate(xyz, stored, n, out_xyz.device, out_offset.device, nullptr);
        rc = rc != APD_OK ? rc : download(out_xyz);
        return rc != APD_OK ? rc : download(out_offset);
    }

    // apd_points_with_smoothed_positions of p (count > 0) into `result`
    int with_positions(apd_points_t p, unsigned iterations, apd_points *result, long long *moved) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        float *buffer[2] = {nullptr, nullptr};
        uint32_t *flags = nullptr;
        uint64_t *before = nullptr;
        HIP_TRY(scratch.alloc(n * 12, &buffer[0]));
        HIP_TRY(scratch.alloc(iterations > 1 ? n * 12 : 0, &buffer[1]));
        HIP_TRY(scratch.alloc(n * 4, &flags));
        HIP_TRY(scratch.alloc((n + 1) * 8, &before));
        HIP_TRY(hipMemsetAsync(flags, 0, n * 4, 0));
        const float *from = in.xyz;
        for (unsigned k = 0; k < iterations; ++k) {
            float *to = buffer[k & 1];
            if (const int rc = iterate(from, in.normal, n, to, nullptr, flags); rc != APD_OK) {
                return rc;
            }
            from = to;
        }
        HIP_TRY(apd_sort::exclusive_scan(flags, before, n));
        uint64_t total = 0;
        HIP_TRY(hipMemcpy(&total, before + n, 8, hipMemcpyDeviceToHost));
        *moved = (long long)total;
        hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(n), dim3(256), 0, 0, flags, n, 1u);  // every point stays
        HIP_TRY(hipGetLastError());
        in.xyz = const_cast<float *>(from);
        return apd_points_host::compact_points(who, p, in, flags, result);
    }
};

}  // namespace

extern "C" int apd_points_smoothed_positions(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *xyz3, float *offset)
{
    Call call{{"apd_points_smoothed_positions"}};
    if (const int rc = call.check(p, xyz3 ? (const void *)xyz3 : (const void *)offset, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_min(min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.smoothed_of(p, xyz3, offset);
}

extern "C" int apd_points_with_smoothed_positions(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, unsigned iterations,
                                                  apd_points_t *out, long long *moved)
{
    Call call{{"apd_points_with_smoothed_positions"}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_min(min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_iterations(iterations); rc != APD_OK) {
        return rc;
    }
    long long count = 0;
    const auto body = [&](apd_points *result) { return call.with_positions(p, iterations, result, &count); };
    const int rc = call.into_new_points(p, out, nullptr, body);
    if (rc == APD_OK && moved) {
        *moved = count;
    }
    return rc;
}
