// apd_points_nearest.hip -- apd_points_nearest and apd_points_score of include/apd_mi355x.h: for every point of one points object
// the nearest point of another within a radius, and from two such searches the precision, recall and F-score of a cloud against
// another at a threshold (arithmetic contract C17; the relation: apd_nearest_math.h).  The sixth search on the walk
// and the host frame of apd_points_search.h, and the first that relates two clouds.
//
// On the query points' device, on its null stream:
//   1. k_fill (apd_points_search.h): +inf and -1 for every query -- what a query outside the grid and one without a candidate keep.
//   2. both clouds inside the grid in cell order (Search::sort_into_cells), on ONE grid: the same cell size and origin, so that a
//      cell of the queries is the same three integers in the targets' keys.  The same object on both sides is sorted once.
//   3. k_nearest_in (apd_points_nearest.h, with the sorts and the launch: apd_points_align.hip searches the same way): one lane
//      per query in the QUERIES' sorted order, so that the lanes of a wave mostly share their cell and with it the nine rows
//      of the targets they search; the lane's cell comes from its own key, the walk
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
#include "apd_points_nearest.h"
#include "apd_points_search.h"

namespace {

using apd_nearest_search::NearestSearch;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::Sorted;
using apd_points_search::Staged;

static_assert(sizeof(apd_points_score_t) == sizeof(apd_fusion::NearestScore), "apd_points_score_t is NearestScore");

// One call of either entry point
struct Call : NearestSearch {
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
