// apd_points_knn.hip -- apd_points_knn_mean_distances and apd_points_remove_statistical of include/apd_mi355x.h: every point's mean
// distance to its k nearest neighbours within a radius, and the object without the points whose value lies above mu + ratio * sigma
// of the cloud's own distribution of it -- the statistical outlier filter (arithmetic contract C12; the relation:
// apd_knn_math.h).
//
// On the points' device, on its null stream:
//   1. k_fill (apd_points_search.h, like steps 2 and 3's walk and the host frame of both entry points): +inf for every point --
//      what a point outside the grid and a point with fewer than k neighbours keep.
//   2. the points inside the grid in cell order.
//   3. k_knn_mean: one lane per point in sorted order, the walk over the 27 cells (for_each_candidate), and for each of its
//      candidates the selection of the k smallest d2 the lane has seen.
//   4. removal: k_chunk_sums (apd_points_search.h: one lane per chunk of 256 input indices, binary64, sequential: the order is the contract), the
//      chunk sums -- n / 256 triples, never the n scores -- come down and the host adds them in order and forms T;
//      k_keep_flags; compact_points (apd_points.hip).
// There is no host path: host-resident points go up, the result comes down.
//
// The selection.  k is a runtime argument, 1 .. 64, and a per-lane array indexed by a runtime value would live in scratch memory;
// the lane's k slots live in LDS instead, laid out [slot][lane]: slot s of lane l is word 64 * s + l, so all slots of a lane sit
// in bank l % 32 and the lanes of a 32-lane half, the group a ds_read_b32 / ds_write_b32 is served in, are on 32 different
// banks whatever slots they touch: no access of the selection conflicts, however the lanes diverge.  A workgroup is one wave
// of 64 lanes with 256 * k bytes of dynamic LDS -- 16 KiB at k = 64, ten workgroups on a CU's 160 KiB, and at k <= 20 the LDS no
// longer bounds residency -- and needs no barrier: a lane touches its own column only.
// Replacement policy: a running maximum with a rescan on replacement.  While a lane holds fewer than k values a neighbour is
// stored in the next slot (1 LDS write; the maximum and its slot are kept in registers).  Once it holds k, a neighbour is
// accepted when its d2 is below the maximum (equal: the multiset would not change); it overwrites the maximum's slot and the
// lane reads its k slots once to find the new maximum: 1 write + k reads per accepted candidate, none per rejected one, and
// the trip count of the rescan is the same k in every lane, where a sorted insert would shift a lane-dependent number of slots
// (k / 2 reads and k / 2 writes on average, the wave paying for its longest lane).  The lanes of a wave mostly share a cell and
// see the candidates in the same order, at the same time, but each against its own maximum: the rescan is a divergent branch
// that the wave runs whenever ANY of its lanes accepts.  A lane accepts about k * ln(c / k) of c candidates in random order,
// the wave up to 64 times as often until that saturates at every candidate, so in a crowded cell (c >> 64 k) the wave runs
// about 64 k * (1 + ln(c / (64 k))) rescans of k reads, and in a sparse one (c < k) none.  Measured against the bare walk:
// DESIGN.md section 6.
// The end: an insertion sort of the lane's k slots in LDS (once per point, at most k * k / 2 reads and writes, about half of that
// on average), knn_score over them in ascending order, and the result goes to the point's input index.  No atomics.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_knn_math.h"
#include "apd_points_host.h"
#include "apd_points_search.h"

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

constexpr int kLanes = 64;  // of a workgroup of k_knn_mean: one wave

// Sorted element i < m with at least k neighbours: mean[member[i]] = its score by contract C12; the others keep what they have.
// keys: ascending; xyz: in the same order; dynamic LDS: k * kLanes floats.
__global__ __launch_bounds__(kLanes) void k_knn_mean(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                      const uint32_t *__restrict__ member, uint32_t m, float r2, uint32_t k,
                                                      float *__restrict__ mean)
{
    extern __shared__ __attribute__((aligned(16))) float slots[];  // [slot][lane]
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;           // m < 2^31
    if (i >= m) {
        return;
    }
    float *const mine = slots + threadIdx.x;  // slot s: mine[kLanes * s]
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    uint32_t have = 0, worst_at = 0;
    float worst = 0.0f;  // the largest of the values held, in slot worst_at
    for_each_candidate(keys, xyz, i, m, [&](uint32_t at, const float Q[3]) {
        const float d2 = apd_fusion::radius_d2(P, Q);
        if (at == i || !(d2 <= r2)) {
            return false;
        }
        if (have < k) {
            mine[kLanes * have] = d2;
            if (have == 0 || d2 >= worst) {
                worst = d2;
                worst_at = have;
            }
            ++have;
        } else if (d2 < worst) {
            mine[kLanes * worst_at] = d2;
            worst = mine[0];
            worst_at = 0;
            for (uint32_t s = 1; s < k; ++s) {
                const float v = mine[kLanes * s];
                if (v > worst) {
                    worst = v;
                    worst_at = s;
                }
            }
        }
        return false;
    });
    if (have < k) {
        return;  // +inf from k_fill
    }
    for (uint32_t a = 1; a < k; ++a) {  // ascending
        const float v = mine[kLanes * a];
        uint32_t b = a;
        for (; b > 0; --b) {
            const float before = mine[kLanes * (b - 1)];
            if (!(before > v)) {
                break;
            }
            mine[kLanes * b] = before;
        }
        mine[kLanes * b] = v;
    }
    mean[member[i]] = apd_fusion::knn_score([mine](unsigned s) { return mine[kLanes * s]; }, k);
}

// keep[k] = 1 where the score is finite and at most T
__global__ __launch_bounds__(256) void k_keep_flags(const float *__restrict__ mean, size_t n, double T, uint32_t *__restrict__ keep)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        keep[k] = apd_fusion::knn_kept(mean[k], T) ? 1u : 0u;
    }
}

// One call of either entry point
struct Call : Search {
    unsigned k = 0;

    // What both calls refuse on top of Search::check
    int check_k(unsigned want)
    {
        if (want < 1 || want > apd_fusion::kKnnMaxK) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: k = %u, not in 1 .. %u", who, want, apd_fusion::kKnnMaxK);
        }
        k = want;
        return APD_OK;
    }

    // mean[j] for the n > 0 points at xyz; both in device memory on the current device
    int scores(const float *xyz, size_t n, float *mean) const
    {
        Scratch scratch;
        hipLaunchKernelGGL(k_fill<float>, grid_of(n), dim3(256), 0, 0, mean, n, apd_fusion::knn_none());
        HIP_TRY(hipGetLastError());
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK || s.m == 0) {
            return rc;
        }
        const unsigned blocks = (unsigned)((s.m + kLanes - 1) / kLanes);
        hipLaunchKernelGGL(k_knn_mean, dim3(blocks), dim3(kLanes), (size_t)k * kLanes * 4, 0, s.keys, s.xyz, s.member, (uint32_t)s.m,
                           grid.size * grid.size, (uint32_t)k, mean);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_points_knn_mean_distances of p (count > 0)
    int scores_of(apd_points_t p, float *mean) const
    {
        Scratch scratch;
        const float *xyz = nullptr;
        Staged<float> out;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : stage(scratch, p, mean, (size_t)p->count * 4, out);
        rc = rc != APD_OK ? rc : scores(xyz, (size_t)p->count, out.device);
        return rc != APD_OK ? rc : download(out);
    }

    // T of the n scores at `mean` (device memory): the chunk sums on the device, their totals and the threshold on the host
    int threshold_of(const float *mean, size_t n, float std_ratio, double *T) const
    {
        double S1 = 0.0, S2 = 0.0;
        unsigned long long n_f = 0;
        if (const int rc = chunk_totals(mean, n, &S1, &S2, &n_f); rc != APD_OK) {
            return rc;
        }
        *T = apd_fusion::knn_threshold(n_f, S1, S2, std_ratio);
        return APD_OK;
    }

    // apd_points_remove_statistical of p (count > 0) into `result`
    int remove_statistical(apd_points_t p, float std_ratio, apd_points *result, double *T) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        float *mean = nullptr;
        uint32_t *keep = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &mean));
        HIP_TRY(scratch.alloc(n * 4, &keep));
        if (const int rc = scores(in.xyz, n, mean); rc != APD_OK) {
            return rc;
        }
        if (const int rc = threshold_of(mean, n, std_ratio, T); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_keep_flags, grid_of(n), dim3(256), 0, 0, (const float *)mean, n, *T, keep);
        HIP_TRY(hipGetLastError());
        return apd_points_host::compact_points(who, p, in, keep, result);
    }
};

}  // namespace

extern "C" int apd_points_knn_mean_distances(apd_points_t p, float radius, const float *origin3, unsigned k, float *mean)
{
    Call call{{"apd_points_knn_mean_distances"}};
    if (const int rc = call.check(p, mean, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_k(k); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.scores_of(p, mean);
}

extern "C" int apd_points_remove_statistical(apd_points_t p, float radius, const float *origin3, unsigned k, float std_ratio, apd_points_t *out,
                                             long long *removed, double *threshold)
{
    Call call{{"apd_points_remove_statistical"}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_k(k); rc != APD_OK) {
        return rc;
    }
    if (!isfinite(std_ratio)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a ratio of %g, not a finite number", call.who, (double)std_ratio);
    }
    double T = 0.0;  // no points: no full points
    const auto body = [&](apd_points *result) { return call.remove_statistical(p, std_ratio, result, &T); };
    const int rc = call.into_new_points(p, out, removed, body);
    if (rc == APD_OK && threshold) {
        *threshold = T;
    }
    return rc;
}
