// apd_points_nearest.hip -- apd_points_nearest and apd_points_score of include/apd_mi355x.h: for every point of one points object
// the nearest point of another within a radius, and from two such searches the precision, recall and F-score of a cloud against
// another at a threshold (arithmetic contract C17; the relation: apd_nearest_math.h).  The sixth search on the walk
// and the host frame of apd_points_search.h, and the first that relates two clouds.
//
// On the query points' device, on its null stream:
//   1. k_fill (apd_points_search.h): +inf and -1 for every query -- what a query outside the grid and one without a candidate keep.
//   2. both clouds inside the grid in cell order (Search::sort_into_cells), on ONE grid: the same cell size and origin, so that a
//      cell of the queries is the same three integers in the targets' keys.  The same object on both sides is sorted once.
//   3. k_nearest_in: one lane per query in the QUERIES' sorted order, so that the lanes of a wave mostly share their cell and
//      with it the nine rows of the targets they search; the lane's cell comes from its own key, the walk
//      (for_each_candidate_around) goes over the targets' keys and positions and never ends early -- a candidate of equal d2 and
//      smaller index may stand in a later cell; (best d2, best index) stay in registers; the targets' input index is read only for
//      a candidate that is within the radius and not farther than the best so far.  The result goes to the query's input index.
//      No atomics, no LDS, no array indexed by a runtime value.
// apd_points_score: both directions from the one pair of sorts, the distances into scratch memory, and of them only the chunk sums
// of contract C12 (Search::chunk_totals) come down.
// There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_nearest_math.h"
#include "apd_points_host.h"
#include "apd_points_search.h"

namespace {

using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::for_each_candidate_around;
using apd_points_search::k_fill;
using apd_points_search::Search;
using apd_points_search::Sorted;
using apd_points_search::Staged;

static_assert(sizeof(apd_points_score_t) == sizeof(apd_fusion::NearestScore), "apd_points_score_t is NearestScore");

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

// One call of either entry point
struct Call : Search {
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

    // apd_points_nearest of p (count > 0) in q
    int nearest_of(apd_points_t p, apd_points_t q, float *distance, int32_t *index) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        Sorted sp, sq;
        Staged<float> out_distance;
        Staged<int32_t> out_index;
        int rc = both_sorted(scratch, p, q, sp, sq);
        rc = rc != APD_OK ? rc : stage(scratch, p, distance, n * 4, out_distance);
        rc = rc != APD_OK ? rc : stage(scratch, p, index, n * 4, out_index);
        rc = rc != APD_OK ? rc : search(sp, n, sq, out_distance.device, out_index.device);
        if (rc != APD_OK) {
            return rc;
        }
        HIP_TRY(hipDeviceSynchronize());  // before the sorts' memory goes
        rc = download(out_distance);
        return rc != APD_OK ? rc : download(out_index);
    }

    // The finite distances of the n > 0 queries `from` against `in`: their number and their binary64 sum in contract C12's order
    int within(const Sorted &from, size_t n, const Sorted &in, unsigned long long *count, double *sum) const
    {
        Scratch scratch;
        float *distance = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &distance));
        if (const int rc = search(from, n, in, distance, nullptr); rc != APD_OK) {
            return rc;
        }
        return chunk_totals(distance, n, sum, nullptr, count);
    }

    // apd_points_score of p against truth, both with points
    int score_of(apd_points_t p, apd_points_t truth, apd_points_score_t *out) const
    {
        Scratch scratch;
        Sorted sp, st;
        unsigned long long a = 0, b = 0;
        double sum_p = 0.0, sum_q = 0.0;
        int rc = both_sorted(scratch, p, truth, sp, st);
        rc = rc != APD_OK ? rc : within(sp, (size_t)p->count, st, &a, &sum_p);
        rc = rc != APD_OK ? rc : within(st, (size_t)truth->count, sp, &b, &sum_q);
        if (rc != APD_OK) {
            return rc;
        }
        set(out, apd_fusion::nearest_score((unsigned long long)p->count, (unsigned long long)truth->count, a, b, sum_p, sum_q));
        return APD_OK;
    }

    static void set(apd_points_score_t *out, const apd_fusion::NearestScore &s)
    {
        *out = {s.n_p, s.n_q, s.p_within, s.q_within, s.precision, s.recall, s.fscore, s.mean_p, s.mean_q};
    }
};

}  // namespace

extern "C" int apd_points_nearest(apd_points_t p, apd_points_t q, float radius, const float *origin3, float *distance, int32_t *index)
{
    Call call{{"apd_points_nearest"}};
    const void *output = distance ? (const void *)distance : (const void *)index;
    if (const int rc = call.check(p, output, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, q, output, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.nearest_of(p, q, distance, index);
}

extern "C" int apd_points_score(apd_points_t p, apd_points_t truth, float threshold, const float *origin3, apd_points_score_t *out)
{
    Call call{{"apd_points_score"}};
    if (const int rc = call.check(p, out, threshold, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, truth, out, threshold, origin3); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0 || truth->count == 0) {  // no distance is finite: the counts, and zeros
        Call::set(out, apd_fusion::nearest_score((unsigned long long)p->count, (unsigned long long)truth->count, 0, 0, 0.0, 0.0));
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.score_of(p, truth, out);
}
