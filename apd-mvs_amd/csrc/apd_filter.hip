// apd_filter.hip -- the geometric filter: apd_filter_views of include/apd_mi355x.h.  Per view a filtered depth map, the number of
// agreeing sources and the consistency score of every pixel: the vote test of RunFusion (APD.cpp:896-951) without its consumption
// of source pixels (`masks`, APD.cpp:928, :959).
//
// The ETH loop judges a pixel against what earlier points have left of its sources, so what a view's own pixels look like after
// the check depends on the views fused before it.  Here every view is judged against the unfiltered maps of its sources: the
// result of a pixel depends on nothing but the inputs, there is no order between pixels or views, and so no vote table, no
// claim / decide rounds, no atomics and no compaction -- one kernel, one launch per view, every launch queued on one stream and
// one wait at the end.
//
// The arithmetic is apd_fusion_math.h's (lift, vote_target, vote_check, accept_point; contract C9), the host side is
// apd_fusion::Call's (argument checks, the device memory of the call, geometry and maps of a view).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_fusion_math.h"

namespace {

using apd_fusion::View;

struct FilterView {
    View geo;
    const float *depth;    // <= 0: no estimate
    const float *normal;   // 3 per pixel, world frame
    const uint8_t *weak;   // PixelState
    const uint8_t *block;  // optional: pixels < 128 are not judged
};

struct FilterTask {
    int ref;  // index of the reference view
    int num_src;
    int src[APD_MAX_IMAGES];
    // the acceptance rule (apd_fusion_options; apd_fusion_math.h)
    float max_reproj_error, max_relative_depth, max_angle, depth_weight, angle_weight;
    int min_consistent;
    float factor_strong, factor_weak;
    // of the reference view; each may be null
    float *depth_out;
    uint8_t *votes_out;
    float *consistency_out;
};

// One lane per reference pixel.  The source index j is the same for every lane, so views[task.src[j]] is read with scalar loads
// and a source's K, R, t, centre and size live in scalar registers for the length of its iteration; the lanes keep the reference
// pixel, its point and the two sums.  Neighbouring pixels land on neighbouring source pixels: the depth (4 bytes) and, only
// behind a valid depth, the normal (12 bytes) are the gathers.  The sums run in source order from 0.0f, as in k_fusion_decide.
__global__ __launch_bounds__(256) void k_filter_view(const FilterView *__restrict__ views, FilterTask task)
{
    const FilterView &rv = views[task.ref];
    const int n = rv.geo.rows * rv.geo.cols;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) {
        return;
    }
    int votes = 0;
    float consistency = 0.0f;
    const float ref_depth = rv.depth[p];
    if (!(rv.block && rv.block[p] < 128) && !(ref_depth <= 0.0f)) {
        const int r = p / rv.geo.cols, c = p - r * rv.geo.cols;
        const float ref_n[3] = {rv.normal[3 * (size_t)p], rv.normal[3 * (size_t)p + 1], rv.normal[3 * (size_t)p + 2]};
        float P[3];
        apd_fusion::lift(rv.geo, c, r, ref_depth, P);
#pragma unroll 1
        for (int j = 0; j < task.num_src; ++j) {
            const FilterView &sv = views[task.src[j]];
            int sc, sr;
            if (!apd_fusion::vote_target(sv.geo, P, sc, sr)) {
                continue;
            }
            const int s = sr * sv.geo.cols + sc;
            const float src_depth = sv.depth[s];
            if (src_depth <= 0.0f) {
                continue;
            }
            const float src_n[3] = {sv.normal[3 * (size_t)s], sv.normal[3 * (size_t)s + 1], sv.normal[3 * (size_t)s + 2]};
            float w;
            if (apd_fusion::vote_check(rv.geo, sv.geo, c, r, ref_depth, ref_n, sc, sr, src_depth, src_n, task.max_reproj_error,
                                       task.max_relative_depth, task.max_angle, task.depth_weight, task.angle_weight, w)) {
                votes++;
                consistency += w;
            }
        }
    }
    if (task.votes_out) {
        task.votes_out[p] = (uint8_t)votes;
    }
    if (task.consistency_out) {
        task.consistency_out[p] = consistency;
    }
    if (task.depth_out) {
        // a pixel that was not judged has no vote, and min_consistent >= 1
        const bool ok = apd_fusion::accept_point(votes, consistency, (int)rv.weak[p], task.min_consistent, task.factor_strong, task.factor_weak);
        task.depth_out[p] = ok ? ref_depth : 0.0f;
    }
}

struct Outputs {
    float *const *depth;
    uint8_t *const *votes;
    float *const *consistency;
    int on_device;
};

struct Filter : apd_fusion::Call {
    Filter(const char *who_, const apd_fusion::Args &args, const Outputs &outputs) : Call(who_, args), out(outputs) {}
    int run();

private:
    const Outputs out;
    template <typename T> static T *entry(T *const *table, int i) { return table ? table[i] : nullptr; }
};

int Filter::run()
{
    using apd_fusion::g_fusion_error;
    using apd_fusion::g_fusion_ms;
    auto invalid = [this](const char *what) { return apd::set_error(g_fusion_error, APD_ERR_INVALID, "%s: %s", who, what); };
    g_fusion_error.clear();
    if (a.num_views <= 0 || !a.depths || !a.normals || !a.weaks) {
        return invalid("null argument");
    }
    // an output must not be a map the sources of another view still read
    bool any = false;
    for (int i = 0; i < a.num_views; ++i) {
        const void *outs[3] = {entry(out.depth, i), entry(out.votes, i), entry(out.consistency, i)};
        for (const void *o : outs) {
            if (!o) {
                continue;
            }
            any = true;
            for (int k = 0; k < a.num_views; ++k) {
                if (o == a.depths[k] || o == a.normals[k] || o == a.weaks[k] || (a.blocks && o == a.blocks[k])) {
                    return invalid("an output is one of the input maps (the sources read the unfiltered maps)");
                }
            }
        }
    }
    if (!any) {
        return invalid("no output is asked for");
    }
    if (const int rc = begin(true, false); rc != APD_OK) {
        return rc;
    }
    std::vector<FilterView> hv(a.num_views);
    for (int i = 0; i < a.num_views; ++i) {
        FilterView &v = hv[i];
        if (const int rc = fill_maps(i, v); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(device_map(a.weaks[i], (size_t)pixels(i), &v.weak));
        if (const int rc = fill_block(i, v); rc != APD_OK) {
            return rc;
        }
    }
    FilterView *dviews = nullptr;
    if (const int rc = upload_views(hv, &dviews); rc != APD_OK) {
        return rc;
    }
    // host outputs: one device buffer per output of every view, brought down after the one wait
    std::vector<FilterTask> tasks(a.num_views);
    for (int i = 0; i < a.num_views; ++i) {
        FilterTask &t = tasks[i];
        const size_t n = (size_t)pixels(i);
        t.depth_out = entry(out.depth, i);
        t.votes_out = entry(out.votes, i);
        t.consistency_out = entry(out.consistency, i);
        if (!out.on_device && n > 0) {
            if (t.depth_out) {
                HIP_TRY(alloc(n * 4, &t.depth_out));
            }
            if (t.votes_out) {
                HIP_TRY(alloc(n, &t.votes_out));
            }
            if (t.consistency_out) {
                HIP_TRY(alloc(n * 4, &t.consistency_out));
            }
        }
    }
    g_fusion_ms[0] = lap();
    for (int i = 0; i < a.num_views; ++i) {
        FilterTask &t = tasks[i];
        const int n = pixels(i);
        if (n == 0 || !(t.depth_out || t.votes_out || t.consistency_out)) {
            continue;
        }
        t.ref = i;
        t.num_src = sources(i);
        for (int j = 0; j < t.num_src; ++j) {
            t.src[j] = a.pair_indices[a.pair_offsets[i] + j];
        }
        t.max_reproj_error = a.opt.max_reproj_error;
        t.max_relative_depth = a.opt.max_relative_depth;
        t.max_angle = a.opt.max_angle;
        t.depth_weight = a.opt.depth_weight;
        t.angle_weight = a.opt.angle_weight;
        t.min_consistent = a.opt.min_consistent;
        t.factor_strong = a.opt.factor_strong;
        t.factor_weak = a.opt.factor_weak;
        hipLaunchKernelGGL(k_filter_view, dim3((n + 255) / 256), dim3(256), 0, 0, dviews, t);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(0));
    if (!out.on_device) {
        for (int i = 0; i < a.num_views; ++i) {
            const FilterTask &t = tasks[i];
            const size_t n = (size_t)pixels(i);
            if (n == 0) {
                continue;
            }
            if (t.depth_out) {
                HIP_TRY(hipMemcpy(out.depth[i], t.depth_out, n * 4, hipMemcpyDeviceToHost));
            }
            if (t.votes_out) {
                HIP_TRY(hipMemcpy(out.votes[i], t.votes_out, n, hipMemcpyDeviceToHost));
            }
            if (t.consistency_out) {
                HIP_TRY(hipMemcpy(out.consistency[i], t.consistency_out, n * 4, hipMemcpyDeviceToHost));
            }
        }
    }
    g_fusion_ms[1] = lap();
    g_fusion_ms[2] = 0.0;
    return APD_OK;
}

}  // namespace

extern "C" int apd_filter_views(const apd_fusion_options *options, int device, int num_views, const apd_camera *cameras,
                                const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                                const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets,
                                const int *pair_indices, int maps_on_device, float *const *depth_out, uint8_t *const *votes_out,
                                float *const *consistency_out, int outputs_on_device)
{
    const char *who = "apd_filter_views";
    bool preset = false;
    if (const int rc = apd_fusion::check_options(who, options, &preset); rc != APD_OK) {
        return rc;
    }
    if (options->variant != APD_FUSION_ETH) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_INVALID, "%s: the filter is the ETH loop's vote test: variant must be APD_FUSION_ETH",
                              who);
    }
    apd_fusion::Args a = {device, num_views, cameras, nullptr, 0, depths, normals, weaks, blocks, rows, cols, pair_offsets, pair_indices,
                          maps_on_device, nullptr, nullptr};
    a.opt = *options;
    return Filter(who, a, Outputs{depth_out, votes_out, consistency_out, outputs_on_device}).run();
}
