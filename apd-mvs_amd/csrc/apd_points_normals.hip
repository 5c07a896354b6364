// apd_points_normals.hip -- apd_points_estimate_normals and apd_points_with_estimated_normals of include/apd_mi355x.h: every point's
// normal as the direction of least variance of its neighbourhood within a radius, with the surface variation that the same
// eigenvalues give, and the object with those normals in place of the stored ones (arithmetic contract C14; the relation:
// apd_normal_math.h).
//
// On the points' device, on its null stream:
//   1. k_normal_fill: the stored normal and +inf for every point -- what a point outside the grid and a point with fewer than
//      min_neighbours neighbours keep.
//   2. the points inside the grid in cell order (apd_points_search.h, shared with the radius, the statistical and the cluster filter,
//      like step 3's walk, step 4's fill and the host frame of both entry points).
//   3. k_point_normals: one lane per point in sorted order, the walk over the 27 cells (for_each_candidate), which never ends early,
//      and for each of its candidates the ten binary64 sums of the lane's neighbourhood; then, in the same lane, the covariance
//      and the cyclic Jacobi solve of apd_normal_math.h, its three rotations written out on named scalars, so that no array is
//      indexed by a runtime value and the matrix, the vectors and the sums stay in registers.  The result goes to the point's
//      input index.  No LDS, no atomics.
//   4. with_estimated_normals: k_estimated_flags, a scan for their number, and compact_points (apd_points.hip) with every flag set
//      and the new normals in the place of the stored ones: the copy of the other six arrays and of a merged object's lists is
//      the one every filter makes.
// There is no host path: host-resident points go up, the result comes down.
//
// One kernel, not a walk kernel and a solve kernel.  The solve is a few hundred binary64 operations per point with an estimate,
// once; the walk is ten binary64 additions and six multiplications per neighbour.  Split, the ten sums and the count would go
// through memory (88 bytes a point, written and read) to save registers the walk does not lack: the walk's own state is a dozen
// registers, the sums twenty, and the solve reuses them.  The lanes of a wave take different numbers of sweeps, and the wave pays
// for its slowest lane; with a cap of kNormalSweepCap sweeps that is bounded.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_normal_math.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
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

// "No estimate" for every point: the stored normal and +inf; either output may be null
__global__ __launch_bounds__(256) void k_normal_fill(const float *__restrict__ stored, size_t n, float *__restrict__ normal,
                                                      float *__restrict__ variation)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    if (normal) {
        normal[3 * k] = stored[3 * k];
        normal[3 * k + 1] = stored[3 * k + 1];
        normal[3 * k + 2] = stored[3 * k + 2];
    }
    if (variation) {
        variation[k] = apd_fusion::normal_none();
    }
}

// Sorted element i < m with at least min_neighbours neighbours: normal[member[i]] and variation[member[i]] by contract C14 (either
// may be null), estimated[member[i]] = 1 (may be null); the others keep what they have.  keys: ascending; xyz: in the same
// order; stored: the stored normals by input index.  The lane's own position is one of the walk's candidates and its term, d = 0, is
// added where the walk meets it: the sums run in the walk's order, ascending (cell key, input index), over the point and its
// neighbours.
__global__ __launch_bounds__(256) void k_point_normals(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                        const uint32_t *__restrict__ member, uint32_t m, float r2, uint32_t min_neighbours,
                                                        const float *__restrict__ stored, float *__restrict__ normal,
                                                        float *__restrict__ variation, uint32_t *__restrict__ estimated)
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
            apd_fusion::normal_add(sums, P, Q);
        }
        return false;
    });
    if (count < min_neighbours) {
        return;  // the fill
    }
    const size_t k = member[i];
    const float N[3] = {stored[3 * k], stored[3 * k + 1], stored[3 * k + 2]};
    float result[3], v = 0.0f;
    unsigned sweeps = 0;
    bool capped = false;
    apd_fusion::normal_solve(sums, N, result, v, sweeps, capped);
    if (normal) {
        normal[3 * k] = result[0];
        normal[3 * k + 1] = result[1];
        normal[3 * k + 2] = result[2];
    }
    if (variation) {
        variation[k] = v;
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

    // The estimates of the n > 0 points at xyz with the stored normals at `stored` into normal, variation and estimated (flags of
    // 0 or 1), each of which may be null; all in device memory on the current device
    int estimate(const float *xyz, const float *stored, size_t n, float *normal, float *variation, uint32_t *estimated) const
    {
        Scratch scratch;
        hipLaunchKernelGGL(k_normal_fill, grid_of(n), dim3(256), 0, 0, stored, n, normal, variation);
        HIP_TRY(hipGetLastError());
        if (estimated) {
            HIP_TRY(hipMemsetAsync(estimated, 0, n * 4, 0));
        }
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK || s.m == 0) {
            return rc;
        }
        hipLaunchKernelGGL(k_point_normals, grid_of(s.m), dim3(256), 0, 0, s.keys, s.xyz, s.member, (uint32_t)s.m, grid.size * grid.size,
                           (uint32_t)min_neighbours, stored, normal, variation, estimated);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_points_estimate_normals of p (count > 0): host-resident points send positions and normals up
    int estimate_of(apd_points_t p, float *normal, float *variation) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        const float *xyz = nullptr, *stored = nullptr;
        Staged<float> out_normal, out_variation;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : readable(scratch, p, (const float *)p->arrays.normal, n * 12, &stored);
        rc = rc != APD_OK ? rc : stage(scratch, p, normal, n * 12, out_normal);
        rc = rc != APD_OK ? rc : stage(scratch, p, variation, n * 4, out_variation);
        rc = rc != APD_OK ? rc : estimate(xyz, stored, n, out_normal.device, out_variation.device, nullptr);
        rc = rc != APD_OK ? rc : download(out_normal);
        return rc != APD_OK ? rc : download(out_variation);
    }

    // apd_points_with_estimated_normals of p (count > 0) into `result`
    int with_normals(apd_points_t p, apd_points *result, long long *estimated) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        float *normal = nullptr;
        uint32_t *flags = nullptr;
        uint64_t *before = nullptr;
        HIP_TRY(scratch.alloc(n * 12, &normal));
        HIP_TRY(scratch.alloc(n * 4, &flags));
        HIP_TRY(scratch.alloc((n + 1) * 8, &before));
        if (const int rc = estimate(in.xyz, in.normal, n, normal, nullptr, flags); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(apd_sort::exclusive_scan(flags, before, n));
        uint64_t total = 0;
        HIP_TRY(hipMemcpy(&total, before + n, 8, hipMemcpyDeviceToHost));
        *estimated = (long long)total;
        hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(n), dim3(256), 0, 0, flags, n, 1u);  // every point stays
        HIP_TRY(hipGetLastError());
        in.normal = normal;
        return apd_points_host::compact_points(who, p, in, flags, result);
    }
};

}  // namespace

extern "C" int apd_points_estimate_normals(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *normal3,
                                           float *variation)
{
    Call call{{"apd_points_estimate_normals"}};
    if (const int rc = call.check(p, normal3 ? (const void *)normal3 : (const void *)variation, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_min(min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.estimate_of(p, normal3, variation);
}

extern "C" int apd_points_with_estimated_normals(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, apd_points_t *out,
                                                 long long *estimated)
{
    Call call{{"apd_points_with_estimated_normals"}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_min(min_neighbours); rc != APD_OK) {
        return rc;
    }
    long long count = 0;
    const auto body = [&](apd_points *result) { return call.with_normals(p, result, &count); };
    const int rc = call.into_new_points(p, out, nullptr, body);
    if (rc == APD_OK && estimated) {
        *estimated = count;
    }
    return rc;
}
