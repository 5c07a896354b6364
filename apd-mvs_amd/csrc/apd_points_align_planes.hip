// apd_points_align_planes.hip -- apd_points_align_planes of include/apd_mi355x.h: the rigid transform that brings one points
// object onto another by point-to-plane ICP within a radius, onto the tangent planes that the other object's stored normals give
// (arithmetic contract C20; the relation, the solve and the iteration: apd_align_plane_math.h).  The search is that of
// contract C17 as apd_points_nearest.h gives it, asked for the index alone; pass 1, the move and the totals of the chunk sums are
// those of apd_points_align_sums.h, which apd_points_align.hip and apd_points_register.hip share.
//
// On p's device, on its null stream.  Once per call: q's positions readable and in cell order, q's normals readable.  Per step k:
//   1. k_align_move for k > 0: X_k from p's own positions and the total so far.
//   2. X_k in cell order (in a Scratch of the step's own) and NearestSearch::search for index[].
//   3. k_align_sums1: the eight sums of pass 1; the chunk sums come down and the host adds them ascending.
//   4. k_align_plane_sums: one 256-lane workgroup per chunk of 256 consecutive input indices, one lane per slot.  The lane reads
//      its position, its index and -- two gathers -- its match's position and normal from q's input-order arrays, forms its thirty
//      terms about the centre, which goes down as three doubles (+0.0 each when unmatched, unusable or past the end), and the tree
//      of contract C18 runs as align_reduce<30>: a wave64 __shfl_down ladder on doubles, four partial sums per sum in LDS.  Thirty
//      doubles per lane are sixty registers, kept as named elements of one array that only unrolled loops index: no atomics, no
//      scratch, no array indexed by a runtime value.
//   5. the 6 x 6 solve, the stopping rule and the composition on the host (apd_fusion::align_plane_run); no position leaves the
//      device.
// There is no host path: host-resident points go up.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>

#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_align_math.h"
#include "apd_align_plane_math.h"
#include "apd_fusion_device.h"
#include "apd_points_align_sums.h"
#include "apd_points_host.h"
#include "apd_points_nearest.h"
#include "apd_points_search.h"

namespace {

using apd_fusion::AlignTransform;
using apd_fusion::kAlignPlaneSums;
using apd_fusion::kAlignSums1;
using apd_fusion::kKnnChunk;
using apd_fusion::PlaneAlignment;
using apd_align_sums::align_pair;
using apd_align_sums::align_reduce;
using apd_align_sums::AlignSums;
using apd_align_sums::k_align_sums1;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::Sorted;

static_assert(sizeof(apd_points_plane_alignment_t) == sizeof(PlaneAlignment) && sizeof(apd_points_alignment_t) == sizeof(apd_fusion::Alignment) &&
                  offsetof(apd_points_plane_alignment_t, planes_before) == offsetof(PlaneAlignment, planes_before) &&
                  offsetof(apd_points_plane_alignment_t, planes_before) == sizeof(apd_points_alignment_t) &&
                  offsetof(apd_points_plane_alignment_t, stopped) == offsetof(apd_points_alignment_t, stopped),
              "apd_points_plane_alignment_t is PlaneAlignment and begins as apd_points_alignment_t");
static_assert(APD_ALIGN_DEGENERATE == apd_fusion::kAlignDegenerate, "APD_ALIGN_DEGENERATE is kAlignDegenerate");

// The centre of pass 2: qm, as pass 1 gave it
struct AlignCentre {
    double c[3];
};

// Chunk blockIdx.x of the n points at xyz: sums[30 * chunk ..] by pass 2 of contract C20.  index: n matches; target, normal: q's
// positions and stored normals, in input order
__global__ __launch_bounds__(256) void k_align_plane_sums(const float *__restrict__ xyz, const int32_t *__restrict__ index, const float *__restrict__ target,
                                                           const float *__restrict__ normal, size_t n, AlignCentre about, double *__restrict__ sums)
{
    float P[3], Q[3];
    double v[kAlignPlaneSums];
#pragma unroll
    for (int j = 0; j < kAlignPlaneSums; ++j) {
        v[j] = 0.0;
    }
    if (align_pair(xyz, index, target, n, P, Q)) {
        const size_t at = (size_t)index[(size_t)blockIdx.x * kKnnChunk + threadIdx.x];  // matched: 0 <= index < n_q
        const float N[3] = {normal[3 * at], normal[3 * at + 1], normal[3 * at + 2]};
        apd_fusion::align_plane_terms(P, Q, N, about.c, v);
    }
    align_reduce(v, sums + (size_t)blockIdx.x * kAlignPlaneSums);
}

// One call of apd_points_align_planes
struct Call : AlignSums {
    int check_options(const apd_points_align_planes_options &o) const
    {
        if (o.iterations < 1 || o.iterations > apd_fusion::kAlignMaxIterations) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: iterations = %u, not in 1 .. %u", who, o.iterations, apd_fusion::kAlignMaxIterations);
        }
        if (!(isfinite(o.tolerance) && o.tolerance >= 0.0)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a tolerance of %g, not a finite number >= 0", who, o.tolerance);
        }
        return APD_OK;
    }

    // p onto the planes of q, both with points
    int align_of(apd_points_t p, apd_points_t q, const apd_points_align_planes_options &o, PlaneAlignment &out) const
    {
        const size_t n = (size_t)p->count, chunks = (n + kKnnChunk - 1) / kKnnChunk;
        Scratch scratch;
        const float *own = nullptr, *target = nullptr, *normal = nullptr;
        Sorted sq;
        float *moved = nullptr;
        int32_t *index = nullptr;
        double *sums = nullptr;
        int rc = positions(scratch, p, &own);
        rc = rc != APD_OK || q == p ? rc : readable(scratch, q, (const float *)q->arrays.xyz, (size_t)q->count * 12, &target);
        rc = rc != APD_OK ? rc : readable(scratch, q, (const float *)q->arrays.normal, (size_t)q->count * 12, &normal);
        if (rc != APD_OK) {
            return rc;
        }
        target = q == p ? own : target;
        if (rc = sorted(scratch, target, (size_t)q->count, sq); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(scratch.alloc(n * 12, &moved));
        HIP_TRY(scratch.alloc(n * 4, &index));
        HIP_TRY(scratch.alloc(chunks * (size_t)kAlignPlaneSums * 8, &sums));
        std::vector<double> host(chunks * (size_t)kAlignPlaneSums);
        const float *current = own;
        const auto pass1 = [&](unsigned k, const AlignTransform &total, double *s) -> int {
            if (k > 0) {
                if (const int moved_rc = move(own, n, apd_fusion::align_move_of(total, true), moved); moved_rc != APD_OK) {
                    return moved_rc;
                }
                current = moved;
            }
            {
                Scratch of_step;
                Sorted sp;
                if (const int sort_rc = sorted(of_step, current, n, sp); sort_rc != APD_OK) {
                    return sort_rc;
                }
                if (const int search_rc = search(sp, n, sq, nullptr, index); search_rc != APD_OK) {
                    return search_rc;
                }
                HIP_TRY(hipDeviceSynchronize());  // before the sort's memory goes
            }
            hipLaunchKernelGGL(k_align_sums1, dim3((unsigned)chunks), dim3(256), 0, 0, current, (const int32_t *)index, target, n, sums);
            HIP_TRY(hipGetLastError());
            return totals(sums, chunks, kAlignSums1, host, s);
        };
        const auto pass2 = [&](const double centre[3], double *s) -> int {
            const AlignCentre about = {{centre[0], centre[1], centre[2]}};
            hipLaunchKernelGGL(k_align_plane_sums, dim3((unsigned)chunks), dim3(256), 0, 0, current, (const int32_t *)index, target, normal, n, about, sums);
            HIP_TRY(hipGetLastError());
            return totals(sums, chunks, kAlignPlaneSums, host, s);
        };
        return apd_fusion::align_plane_run(o.iterations, o.tolerance, pass1, pass2, out);
    }
};

}  // namespace

extern "C" int apd_points_align_planes(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_align_planes_options *opt,
                                       apd_points_plane_alignment_t *out)
{
    Call call{{{{"apd_points_align_planes"}}}};
    const apd_points_align_planes_options options = opt ? *opt : apd_points_align_planes_options{16, 1e-6};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, q, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_options(options); rc != APD_OK) {
        return rc;
    }
    PlaneAlignment result = apd_fusion::align_plane_identity();
    if (p->count > 0 && q->count > 0) {
        DeviceScope scope(true);
        if (const int rc = call.align_of(p, q, options, result); rc != APD_OK) {
            return rc;
        }
    }
    const apd_fusion::Alignment &a = result.points;
    *out = {a.scale, {}, {}, a.matched_before, a.matched_after, a.rms_before, a.rms_after, a.steps, a.stopped,
            result.planes_before, result.planes_after, result.plane_rms_before, result.plane_rms_after};
    for (int e = 0; e < 9; ++e) {
        out->rotation[e] = a.rotation[e];
    }
    for (int a3 = 0; a3 < 3; ++a3) {
        out->translation[a3] = a.translation[a3];
    }
    return APD_OK;
}
