// apd_fusion.hip -- depth-map fusion (RunFusion, APD.cpp:826-977) on the device: apd_fuse_views of include/apd_mi355x.h.
//
// The reference fuses on the host: views in problem order, pixels in raster order, and a source pixel that supported an
// accepted point is consumed (`masks`), so later pixels of the same view can no longer use it -- pixel order is part of
// the result.  Views stay sequential here.  Within one view the per-pixel geometry (one thread per reference pixel: lift,
// project into every source view, back-project, thresholds -- apd_fusion_math.h, shared with the host build) has no
// order at all; only the consumption has, and it is resolved exactly by a fixed-point iteration:
//
//   * every pixel that is still undecided or accepted "claims" the source pixels of its (still possible) votes with
//     atomicMin(epoch-stamped raster index): claim(s) = first such pixel in raster order;
//   * an undecided pixel p looks at each of its votes: claim == p  -> nobody earlier can take it: the vote counts;
//     claim == q < p, q accepted -> consumed by q: the vote is lost for good; q undecided -> wait for the next round;
//   * when no vote is waiting, p is decided exactly as the sequential loop would decide it (sum in source order).
//
// The first undecided pixel of a round always decides (everything before it is decided), so the iteration ends, and a
// pixel's decision only ever depends on decisions of earlier pixels: same result as the raster-order loop, bit for bit.
// Accepted pixels then consume their supports, and a block scan compacts the points in raster order.
//
// The acceptance rule's eight values (apd_fusion_options) reach the kernels in RefTask, as kernel arguments.  A pixel is decided
// when no vote is waiting, whatever min_consistent is; no pixel is rejected early because its possible votes fell below
// min_consistent (the only early rejection is the one there always was: a pixel without any vote has nothing to claim).
//
// The host side of a call (argument checks, memory, the compaction of a view's points, the file, the points in memory) is the
// driver every device fusion shares: apd_fusion::Call, apd_fusion_device.h, apd_fusion_call.hip.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_fusion_math.h"

namespace {

using apd_fusion::View;

constexpr int kMaxSrc = APD_MAX_IMAGES;  // sources of one reference view (main.h: MAX_IMAGES 32 includes the reference)

struct DevView {
    View geo;
    const float *image;   // rows*cols*channels, 0..255; channels 1 (grey) or 3 (blue, green, red)
    const float *depth;   // <= 0: no estimate
    const float *normal;  // 3 per pixel, world frame
    const uint8_t *weak;  // PixelState
    const uint8_t *block; // optional `blocks/mask_<id>.jpg` (APD.cpp:849-853): pixels < 128 are not fused as reference pixels
    uint8_t *consumed;    // the reference's `masks`
    unsigned long long *claim;  // epoch-stamped first claimant of this pixel in the view being fused
};

struct RefTask {
    int ref;                 // index of the reference view
    int num_src;
    int src[kMaxSrc];
    int *vote_idx;           // [pixel][num_src]: source pixel index, -1 = no (more) vote
    float *vote_w;           // exp(-score) of that vote
    uint8_t *state;          // 0 inactive, 1 undecided, 2 accepted, 3 rejected
    int *flags;              // [0] undecided pixels left after this round
    int channels;            // of the images
    uint8_t *support;        // [pixel]: num_consistent of an accepted pixel
    uint32_t *agreeing;      // [pixel]: bit j = source j is one of them; null: not asked for
    // the acceptance rule (apd_fusion_options; apd_fusion_math.h)
    float max_reproj_error, max_relative_depth, max_angle, depth_weight, angle_weight;
    int min_consistent;
    float factor_strong, factor_weak;
};

enum : uint8_t { kInactive = 0, kUndecided = 1, kAccepted = 2, kRejected = 3 };

__device__ __forceinline__ unsigned long long stamp(unsigned epoch, unsigned p) { return ((unsigned long long)(0xFFFFFFFFu - epoch) << 32) | p; }

// Votes of every reference pixel, ignoring consumption inside this view (APD.cpp:882-926).
__global__ __launch_bounds__(256) void k_fusion_votes(const DevView *__restrict__ views, RefTask task)
{
    const DevView &rv = views[task.ref];
    const int n = rv.geo.rows * rv.geo.cols;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) {
        return;
    }
    uint8_t st = kInactive;
    const float ref_depth = rv.depth[p];
    if (!(rv.block && rv.block[p] < 128) && rv.consumed[p] != 1 && !(ref_depth <= 0.0f)) {
        const int r = p / rv.geo.cols, c = p - r * rv.geo.cols;
        const float ref_n[3] = {rv.normal[3 * (size_t)p], rv.normal[3 * (size_t)p + 1], rv.normal[3 * (size_t)p + 2]};
        float P[3];
        apd_fusion::lift(rv.geo, c, r, ref_depth, P);
        int votes = 0;
        for (int j = 0; j < task.num_src; ++j) {
            const DevView &sv = views[task.src[j]];
            int idx = -1;
            float w = 0.0f;
            int sc, sr;
            if (apd_fusion::vote_target(sv.geo, P, sc, sr)) {
                const int s = sr * sv.geo.cols + sc;
                const float src_depth = sv.depth[s];
                if (sv.consumed[s] != 1 && !(src_depth <= 0.0f)) {
                    const float src_n[3] = {sv.normal[3 * (size_t)s], sv.normal[3 * (size_t)s + 1], sv.normal[3 * (size_t)s + 2]};
                    if (apd_fusion::vote_check(rv.geo, sv.geo, c, r, ref_depth, ref_n, sc, sr, src_depth, src_n, task.max_reproj_error,
                                                   task.max_relative_depth, task.max_angle, task.depth_weight, task.angle_weight, w)) {
                        idx = s;
                        votes++;
                    }
                }
            }
            task.vote_idx[(size_t)p * task.num_src + j] = idx;
            task.vote_w[(size_t)p * task.num_src + j] = w;
        }
        st = votes > 0 ? kUndecided : kRejected;  // no vote: num_consistent == 0, never a point
    }
    task.state[p] = st;
}

__global__ __launch_bounds__(256) void k_fusion_claim(const DevView *__restrict__ views, RefTask task, unsigned epoch)
{
    const DevView &rv = views[task.ref];
    const int n = rv.geo.rows * rv.geo.cols;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) {
        return;
    }
    const uint8_t st = task.state[p];
    if (st != kUndecided && st != kAccepted) {
        return;
    }
    for (int j = 0; j < task.num_src; ++j) {
        const int s = task.vote_idx[(size_t)p * task.num_src + j];
        if (s >= 0) {
            atomicMin(&views[task.src[j]].claim[s], stamp(epoch, (unsigned)p));
        }
    }
}

__global__ __launch_bounds__(256) void k_fusion_decide(const DevView *__restrict__ views, RefTask task, unsigned epoch)
{
    const DevView &rv = views[task.ref];
    const int n = rv.geo.rows * rv.geo.cols;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n || task.state[p] != kUndecided) {
        return;
    }
    bool waiting = false;
    for (int j = 0; j < task.num_src; ++j) {
        const int s = task.vote_idx[(size_t)p * task.num_src + j];
        if (s < 0) {
            continue;
        }
        const unsigned first = (unsigned)(views[task.src[j]].claim[s] & 0xFFFFFFFFull);  // stamped this round: p itself claimed
        if (first == (unsigned)p) {
            continue;  // every earlier claimant is rejected or lost this vote: it counts
        }
        // first < p.  Its state may change while this kernel runs; a stale "undecided" only costs a round.
        const uint8_t fs = reinterpret_cast<volatile uint8_t *>(task.state)[first];
        if (fs == kAccepted) {
            task.vote_idx[(size_t)p * task.num_src + j] = -1;  // consumed by an earlier point of this view
        } else {
            waiting = true;  // undecided, or rejected a moment ago (then the next claim round names its successor)
        }
    }
    if (waiting) {
        atomicAdd(&task.flags[0], 1);
        return;
    }
    int agreeing = 0;
    float consistency = 0.0f;
    for (int j = 0; j < task.num_src; ++j) {
        if (task.vote_idx[(size_t)p * task.num_src + j] >= 0) {
            consistency += task.vote_w[(size_t)p * task.num_src + j];
            agreeing++;
        }
    }
    const bool ok = apd_fusion::accept_point(agreeing, consistency, (int)rv.weak[p], task.min_consistent, task.factor_strong, task.factor_weak);
    __threadfence();
    reinterpret_cast<volatile uint8_t *>(task.state)[p] = ok ? kAccepted : kRejected;
}

// Accepted pixels consume their supports and produce their point (APD.cpp:939-960); per-block counts for the scan.
__global__ __launch_bounds__(256) void k_fusion_emit(const DevView *__restrict__ views, RefTask task, float *__restrict__ xyz_sparse,
                                                      uint8_t *__restrict__ bgr_sparse, int *__restrict__ block_counts)
{
    const DevView &rv = views[task.ref];
    const int n = rv.geo.rows * rv.geo.cols;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool acc = p < n && task.state[p] == kAccepted;
    if (acc) {
        const int r = p / rv.geo.cols, c = p - r * rv.geo.cols;
        float P[3];
        apd_fusion::lift(rv.geo, c, r, rv.depth[p], P);
        const int nc = task.channels;
        float colour[3];
        for (int k = 0; k < 3; ++k) {
            colour[k] = rv.image[(size_t)p * nc + (nc == 3 ? k : 0)];
        }
        int agreeing = 0;
        uint32_t used = 0;
        for (int j = 0; j < task.num_src; ++j) {
            const int s = task.vote_idx[(size_t)p * task.num_src + j];
            if (s >= 0) {
                const DevView &sv = views[task.src[j]];
                sv.consumed[s] = 1;
                used |= 1u << j;
                for (int k = 0; k < 3; ++k) {
                    colour[k] += sv.image[(size_t)s * nc + (nc == 3 ? k : 0)];
                }
                agreeing++;
            }
        }
        xyz_sparse[3 * (size_t)p + 0] = P[0];
        xyz_sparse[3 * (size_t)p + 1] = P[1];
        xyz_sparse[3 * (size_t)p + 2] = P[2];
        for (int k = 0; k < 3; ++k) {
            bgr_sparse[3 * (size_t)p + k] = static_cast<uint8_t>(colour[k] / (agreeing + 1));
        }
        task.support[p] = (uint8_t)agreeing;
        if (task.agreeing) {
            task.agreeing[p] = used;
        }
    }
    const unsigned long long m = __ballot(acc);
    __shared__ int wave_counts[4];
    if ((threadIdx.x & 63) == 0) {
        wave_counts[threadIdx.x >> 6] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
    }
}


struct EthFusion : apd_fusion::Call {
    using Call::Call;
    int run();
};

int EthFusion::run()
{
    if (const int rc = begin(true); rc != APD_OK) {
        return rc;
    }
    std::vector<DevView> hv(a.num_views);
    for (int i = 0; i < a.num_views; ++i) {
        DevView &v = hv[i];
        const size_t n = (size_t)pixels(i);
        if (const int rc = fill_view(i, v); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(device_map(a.weaks[i], n, &v.weak));
        if (const int rc = fill_block(i, v); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(alloc(n, &v.consumed));
        HIP_TRY(alloc(n * 8, &v.claim));
        HIP_TRY(hipMemset(v.consumed, 0, n));
        HIP_TRY(hipMemset(v.claim, 0xFF, n * 8));
    }
    DevView *dviews = nullptr;
    if (const int rc = upload_views(hv, &dviews); rc != APD_OK) {
        return rc;
    }
    RefTask task;
    task.channels = a.image_channels;
    HIP_TRY(alloc(max_px * max_src * 4, &task.vote_idx));
    HIP_TRY(alloc(max_px * max_src * 4, &task.vote_w));
    HIP_TRY(alloc(max_px, &task.state));
    HIP_TRY(alloc(sizeof(int), &task.flags));
    if (const int rc = alloc_common(); rc != APD_OK) {
        return rc;
    }
    task.support = support;
    task.agreeing = agreeing;
    task.max_reproj_error = a.opt.max_reproj_error;
    task.max_relative_depth = a.opt.max_relative_depth;
    task.max_angle = a.opt.max_angle;
    task.depth_weight = a.opt.depth_weight;
    task.angle_weight = a.opt.angle_weight;
    task.min_consistent = a.opt.min_consistent;
    task.factor_strong = a.opt.factor_strong;
    task.factor_weak = a.opt.factor_weak;
    unsigned epoch = 0;
    for (int i = 0; i < a.num_views; ++i) {
        const int n = pixels(i);
        const int blocks = (n + 255) / 256;
        if (n == 0) {
            continue;
        }
        task.ref = i;
        task.num_src = sources(i);
        for (int j = 0; j < task.num_src; ++j) {
            task.src[j] = a.pair_indices[a.pair_offsets[i] + j];
        }
        hipLaunchKernelGGL(k_fusion_votes, dim3(blocks), dim3(256), 0, 0, dviews, task);
        HIP_TRY(hipGetLastError());
        int rounds = 0;
        for (;;) {
            ++epoch;
            ++rounds;
            HIP_TRY(hipMemsetAsync(task.flags, 0, sizeof(int), 0));
            hipLaunchKernelGGL(k_fusion_claim, dim3(blocks), dim3(256), 0, 0, dviews, task, epoch);
            hipLaunchKernelGGL(k_fusion_decide, dim3(blocks), dim3(256), 0, 0, dviews, task, epoch);
            HIP_TRY(hipGetLastError());
            int undecided = 0;
            HIP_TRY(hipMemcpy(&undecided, task.flags, sizeof(int), hipMemcpyDeviceToHost));
            if (undecided == 0) {
                break;
            }
            if (rounds > n) {  // cannot happen: the first undecided pixel decides in every round
                return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_STATE, "%s: consumption rounds did not converge", who);
            }
        }
        hipLaunchKernelGGL(k_fusion_emit, dim3(blocks), dim3(256), 0, 0, dviews, task, xyz, bgr, block_counts);
        if (const int rc = collect(i, task.state, kAccepted, hv[i].normal); rc != APD_OK) {
            return rc;
        }
    }
    return finish();
}

}  // namespace

namespace apd_fusion {

int run_eth(const char *who, const Args &args) { return EthFusion(who, args).run(); }

}  // namespace apd_fusion

extern "C" int apd_fuse_views(int device, int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                              const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                              const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, int maps_on_device,
                              const char *ply_path, long long *num_points)
{
    const apd_fusion::Args a = {device, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                                pair_indices, maps_on_device, ply_path, num_points};
    return apd_fusion::run_eth("apd_fuse_views", a);
}
