// apd_points_align.hip -- apd_points_align and apd_points_transformed of include/apd_mi355x.h: the rigid or similarity transform
// that brings one points object onto another by point-to-point ICP within a radius, and the object moved by such a transform
// (arithmetic contract C18; the relation, the solve and the iteration: apd_align_math.h).  The search is that of
// contract C17 as apd_points_nearest.h gives it, asked for the index alone; the kernels of steps 1, 3 and 4 and the totals of
// their sums stand in apd_points_align_sums.h, which apd_points_register.hip shares.
//
// apd_points_align, on p's device, on its null stream.  Once per call: q's positions readable and in cell order.  Per step k:
//   1. k_align_move for k > 0: X_k from p's own positions and the total so far, one lane per point.
//   2. X_k in cell order (sort_into_cells, in a Scratch of the step's own: memory does not grow with the steps) and
//      NearestSearch::search for index[]: the input index in q of every point's match, -1 without one.
//   3. k_align_sums1: one 256-lane workgroup per chunk of 256 consecutive input indices, one lane per slot.  The lane reads its
//      position, its index and -- a gather -- its match's position from q's input-order xyz, forms its eight terms (+0.0 each when
//      unmatched or past the end) and the tree of contract C18 runs as a wave64 __shfl_down ladder on doubles, offsets 32 .. 1;
//      lane 0 of each of the four waves leaves its sums in LDS and lane 0 of the workgroup adds them as (g0 + g1) + (g2 + g3).
//      No atomics, no scratch, no array indexed by a runtime value.  The chunk sums come down and the host adds them ascending.
//   4. k_align_sums2, likewise, for the ten moments about the means, which go down as six doubles.
//   5. the solve, the stopping rule and the composition on the host (apd_fusion::align_run); no position leaves the device.
// apd_points_transformed: k_align_move on the positions (m = scale * R, t) and on the normals (m = R, t = +0.0), then
// compact_points (apd_points.hip) with every flag set and the two new arrays in the place of the stored ones.
// There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_align_math.h"
#include "apd_fusion_device.h"
#include "apd_points_align_sums.h"
#include "apd_points_host.h"
#include "apd_points_nearest.h"
#include "apd_points_search.h"

namespace {

using apd_fusion::AlignMove;
using apd_fusion::AlignTransform;
using apd_fusion::kAlignSums1;
using apd_fusion::kAlignSums2;
using apd_fusion::kKnnChunk;
using apd_fusion::PointArrays;
using apd_align_sums::AlignMeans;
using apd_align_sums::AlignSums;
using apd_align_sums::k_align_move;
using apd_align_sums::k_align_sums1;
using apd_align_sums::k_align_sums2;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::k_fill;
using apd_points_search::Search;
using apd_points_search::Sorted;

static_assert(sizeof(apd_points_alignment_t) == sizeof(apd_fusion::Alignment), "apd_points_alignment_t is Alignment");
static_assert(APD_ALIGN_ITERATIONS == apd_fusion::kAlignIterations && APD_ALIGN_CONVERGED == apd_fusion::kAlignConverged &&
                  APD_ALIGN_TOO_FEW == apd_fusion::kAlignTooFew,
              "APD_ALIGN_* are kAlign*");

// One call of apd_points_align
struct Call : AlignSums {
    int check_options(const apd_points_align_options &o) const
    {
        if (o.iterations < 1 || o.iterations > apd_fusion::kAlignMaxIterations) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: iterations = %u, not in 1 .. %u", who, o.iterations, apd_fusion::kAlignMaxIterations);
        }
        if (!(isfinite(o.tolerance) && o.tolerance >= 0.0)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a tolerance of %g, not a finite number >= 0", who, o.tolerance);
        }
        return APD_OK;
    }

    // p onto q, both with points
    int align_of(apd_points_t p, apd_points_t q, const apd_points_align_options &o, apd_fusion::Alignment &out) const
    {
        const size_t n = (size_t)p->count, chunks = (n + kKnnChunk - 1) / kKnnChunk;
        Scratch scratch;
        const float *own = nullptr, *target = nullptr;
        Sorted sq;
        float *moved = nullptr;
        int32_t *index = nullptr;
        double *sums = nullptr;
        int rc = positions(scratch, p, &own);
        rc = rc != APD_OK || q == p ? rc : readable(scratch, q, (const float *)q->arrays.xyz, (size_t)q->count * 12, &target);
        if (rc != APD_OK) {
            return rc;
        }
        target = q == p ? own : target;
        if (rc = sorted(scratch, target, (size_t)q->count, sq); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(scratch.alloc(n * 12, &moved));
        HIP_TRY(scratch.alloc(n * 4, &index));
        HIP_TRY(scratch.alloc(chunks * (size_t)kAlignSums2 * 8, &sums));
        std::vector<double> host(chunks * (size_t)kAlignSums2);
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
        const auto pass2 = [&](const double mean[6], double *s) -> int {
            AlignMeans about;
            for (int a = 0; a < 6; ++a) {
                about.mean[a] = mean[a];
            }
            hipLaunchKernelGGL(k_align_sums2, dim3((unsigned)chunks), dim3(256), 0, 0, current, (const int32_t *)index, target, n, about, sums);
            HIP_TRY(hipGetLastError());
            return totals(sums, chunks, kAlignSums2, host, s);
        };
        return apd_fusion::align_run(o.iterations, o.tolerance, o.with_scale != 0, pass1, pass2, out);
    }
};

// One call of apd_points_transformed
struct Transform : Search {
    // What the call refuses, before any device is touched
    int check_transform(apd_points_t p, double scale, const double *rotation9, const double *translation3, apd_points_t *out, AlignTransform &by) const
    {
        err().clear();
        if (!p || !rotation9 || !translation3 || !out) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: null argument", who);
        }
        if (!(isfinite(scale) && scale > 0.0)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: a scale of %g, not a positive finite number", who, scale);
        }
        for (int e = 0; e < 12; ++e) {
            const double v = e < 9 ? rotation9[e] : translation3[e - 9];
            if (!isfinite(v)) {
                return apd::set_error(err(), APD_ERR_INVALID, "%s: %s component %d is %g", who, e < 9 ? "rotation" : "translation", e < 9 ? e : e - 9, v);
            }
        }
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) {
                const double x = rotation9[a] * rotation9[b], y = rotation9[3 + a] * rotation9[3 + b], z = rotation9[6 + a] * rotation9[6 + b];
                const double dot = (x + y) + z, off = dot - (a == b ? 1.0 : 0.0);
                if (!(fabs(off) <= 1e-6)) {
                    return apd::set_error(err(), APD_ERR_INVALID, "%s: not a rotation: entry (%d, %d) of R^T R is %.17g", who, a, b, dot);
                }
            }
        }
        if (p->count >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld points, 2^31 or more (the gather carries a 32-bit index)", who, p->count);
        }
        by.scale = scale;
        for (int e = 0; e < 9; ++e) {
            by.R[e] = rotation9[e];
        }
        for (int a = 0; a < 3; ++a) {
            by.t[a] = translation3[a];
        }
        return APD_OK;
    }

    // p (count > 0) moved by `by` into `result`
    int moved_into(apd_points_t p, const AlignTransform &by, apd_points *result) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        float *xyz = nullptr, *normal = nullptr;
        uint32_t *flags = nullptr;
        HIP_TRY(scratch.alloc(n * 12, &xyz));
        HIP_TRY(scratch.alloc(n * 12, &normal));
        HIP_TRY(scratch.alloc(n * 4, &flags));
        hipLaunchKernelGGL(k_align_move, grid_of(n), dim3(256), 0, 0, (const float *)in.xyz, n, apd_fusion::align_move_of(by, true), xyz);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_align_move, grid_of(n), dim3(256), 0, 0, (const float *)in.normal, n, apd_fusion::align_move_of(by, false), normal);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(n), dim3(256), 0, 0, flags, n, 1u);  // every point stays
        HIP_TRY(hipGetLastError());
        in.xyz = xyz;
        in.normal = normal;
        return apd_points_host::compact_points(who, p, in, flags, result);
    }
};

}  // namespace

extern "C" int apd_points_align(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_align_options *opt,
                                apd_points_alignment_t *out)
{
    Call call{{{{"apd_points_align"}}}};
    const apd_points_align_options options = opt ? *opt : apd_points_align_options{16, 1e-6, 0};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, q, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_options(options); rc != APD_OK) {
        return rc;
    }
    apd_fusion::Alignment result = apd_fusion::align_identity();
    if (p->count > 0 && q->count > 0) {
        DeviceScope scope(true);
        if (const int rc = call.align_of(p, q, options, result); rc != APD_OK) {
            return rc;
        }
    }
    *out = {result.scale, {}, {}, result.matched_before, result.matched_after, result.rms_before, result.rms_after, result.steps, result.stopped};
    for (int e = 0; e < 9; ++e) {
        out->rotation[e] = result.rotation[e];
    }
    for (int a = 0; a < 3; ++a) {
        out->translation[a] = result.translation[a];
    }
    return APD_OK;
}

extern "C" int apd_points_transformed(apd_points_t p, double scale, const double *rotation9, const double *translation3, apd_points_t *out)
{
    Transform call{{"apd_points_transformed"}};
    AlignTransform by;
    if (const int rc = call.check_transform(p, scale, rotation9, translation3, out, by); rc != APD_OK) {
        return rc;
    }
    return call.into_new_points(p, out, nullptr, [&](apd_points *result) { return call.moved_into(p, by, result); });
}
