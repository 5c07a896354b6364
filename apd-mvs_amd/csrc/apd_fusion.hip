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
// The second half of the file is the host driver of every device fusion (apd_fusion_device.h), the T&T ones included.  Points in
// memory (apd_points_t): the total is not known before the last view, so the arrays grow geometrically on the device
// (reserve_points: twice the capacity, one device-to-device copy of what is there) and k_fusion_compact_soa appends each view's
// points at the running count; a host result is one download at the end.  Nothing is sized by pixels x views.  Among the arrays
// is `sources`, per point the sources whose votes it was accepted with as a bit mask (k_fusion_emit / k_tat_decide write it per
// pixel, only when the points are asked for); apd_points_visibility turns the masks into lists of views, on the device for
// device-resident points (k_vis_count, k_vis_scan, k_vis_scatter below).
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_fusion_math.h"

namespace {

// exclusive scan of the block counts (one workgroup; a view has at most a few hundred thousand blocks)
__global__ __launch_bounds__(1024) void k_fusion_scan(int *__restrict__ counts, int nblocks, int *__restrict__ total)
{
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, nblocks);
    int sum = 0;
    for (int b = b0; b < b1; ++b) {
        sum += counts[b];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int b = b0; b < b1; ++b) {
        const int c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (t == 1023) {
        *total = part[1023];
    }
}

// Packs the points of a view (pixels p < n with state[p] == accepted) in raster order as the 15-byte records of the PLY body
// (x y z float, diffuse_blue / green / red uchar, APD.cpp:214-254): one download per view straight into the file image, no
// per-point loop on the host.  block_offsets: k_fusion_scan of the per-256-pixel point counts.  kNormals: the 27-byte records
// x y z nx ny nz + colour, the normal read from the view's normal map at the pixel.
template <bool kNormals>
__global__ __launch_bounds__(256) void k_fusion_compact(const uint8_t *__restrict__ state, uint8_t accepted, int n,
                                                         const float *__restrict__ xyz_sparse, const uint8_t *__restrict__ bgr_sparse,
                                                         const float *__restrict__ normal_map, const int *__restrict__ block_offsets,
                                                         uint8_t *__restrict__ records)
{
    constexpr int kFloats = kNormals ? 6 : 3, kRecord = 4 * kFloats + 3;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool acc = p < n && state[p] == accepted;
    const unsigned long long m = __ballot(acc);
    __shared__ int wave_counts[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        wave_counts[wave] = __popcll(m);
    }
    __syncthreads();
    if (acc) {
        int pos = block_offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) {
            pos += wave_counts[w];
        }
        uint8_t *rec = records + (size_t)pos * kRecord;
        for (int k = 0; k < kFloats; ++k) {
            // little endian, as the host's memcpy wrote them
            const uint32_t bits = __float_as_uint(k < 3 ? xyz_sparse[3 * (size_t)p + k] : normal_map[3 * (size_t)p + (k - 3)]);
            rec[4 * k + 0] = (uint8_t)(bits & 0xFFu);
            rec[4 * k + 1] = (uint8_t)((bits >> 8) & 0xFFu);
            rec[4 * k + 2] = (uint8_t)((bits >> 16) & 0xFFu);
            rec[4 * k + 3] = (uint8_t)(bits >> 24);
        }
        rec[4 * kFloats + 0] = bgr_sparse[3 * (size_t)p + 0];
        rec[4 * kFloats + 1] = bgr_sparse[3 * (size_t)p + 1];
        rec[4 * kFloats + 2] = bgr_sparse[3 * (size_t)p + 2];
    }
}

// The same points as a structure of arrays, appended at `base`: point base + block offset + rank in the block gets xyz, the
// normal of the view's normal map at the pixel, colour, support, the agreeing sources, the view and the raster index.  One lane per
// pixel; the rank inside a wave from the ballot and mbcnt, across the four waves of the block through LDS.  Every offset is a size_t.
__global__ __launch_bounds__(256) void k_fusion_compact_soa(const uint8_t *__restrict__ state, uint8_t accepted, int n, int view,
                                                             const float *__restrict__ xyz_sparse, const uint8_t *__restrict__ bgr_sparse,
                                                             const uint8_t *__restrict__ support_sparse,
                                                             const uint32_t *__restrict__ agreeing_sparse,
                                                             const float *__restrict__ normal_map, const int *__restrict__ block_offsets,
                                                             size_t base, apd_fusion::PointArrays out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool acc = p < n && state[p] == accepted;
    const unsigned long long m = __ballot(acc);
    __shared__ int wave_counts[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        wave_counts[wave] = __popcll(m);
    }
    __syncthreads();
    if (acc) {
        int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        for (int w = 0; w < wave; ++w) {
            rank += wave_counts[w];
        }
        const size_t pos = base + (size_t)block_offsets[blockIdx.x] + (size_t)rank;
        for (int k = 0; k < 3; ++k) {
            out.xyz[3 * pos + k] = xyz_sparse[3 * (size_t)p + k];
            out.normal[3 * pos + k] = normal_map[3 * (size_t)p + k];
            out.bgr[3 * pos + k] = bgr_sparse[3 * (size_t)p + k];
        }
        out.support[pos] = support_sparse[p];
        out.sources[pos] = agreeing_sparse[p];
        out.view[pos] = view;
        out.pixel[pos] = p;
    }
}

// ---- visibility lists of device-resident points (apd_points_visibility) ----
// Point k has 1 + popcount(sources[k]) entries: its own view, then the views behind the set bits in ascending bit order.  Three
// kernels: per block of 256 points the number of entries (k_vis_count), an exclusive 64-bit scan of those block sums by one
// workgroup (k_vis_scan: a full ETH3D or 152-view run has more than 10^8 points, so the entries can pass 2^31 and every offset
// is 64-bit; 1024 lanes, each over a run of consecutive blocks, so up to kVisScanSpan points every lane has one block), and the
// scatter, which repeats the block's own scan in LDS (k_vis_scatter).

constexpr long long kVisScanSpan = 1024LL * 256;  // points up to which every lane of k_vis_scan scans at most one block sum

// the bits of sources[k] that name a source of the point's view: all of them, by construction of the mask
__device__ __forceinline__ uint32_t vis_mask(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                             const int *__restrict__ pair_offsets, size_t k, int &first)
{
    const int v = view[k];
    first = pair_offsets[v];
    const int ns = pair_offsets[v + 1] - first;
    return sources[k] & (ns >= 32 ? 0xFFFFFFFFu : ((1u << ns) - 1u));
}

// exclusive scan of one value per lane over the 256 lanes of the block; *block_total: the sum
__device__ __forceinline__ int vis_block_scan(int value, int *block_total)
{
    __shared__ int part[256];
    const int t = threadIdx.x;
    part[t] = value;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    *block_total = part[255];
    return part[t] - value;
}

__global__ __launch_bounds__(256) void k_vis_count(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                                    const int *__restrict__ pair_offsets, size_t n, long long *__restrict__ block_sums)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int first;
    const int entries = k < n ? 1 + __popc(vis_mask(sources, view, pair_offsets, k, first)) : 0;
    int total;
    vis_block_scan(entries, &total);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = total;
    }
}

// block_sums[b] becomes the number of entries before block b; *total: all entries
__global__ __launch_bounds__(1024) void k_vis_scan(long long *__restrict__ block_sums, size_t nblocks, long long *__restrict__ total)
{
    __shared__ long long part[1024];
    const size_t t = threadIdx.x;
    const size_t per = (nblocks + 1023) / 1024;
    const size_t b0 = t * per < nblocks ? t * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    long long sum = 0;
    for (size_t b = b0; b < b1; ++b) {
        sum += block_sums[b];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long v = ((int)t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (size_t b = b0; b < b1; ++b) {
        const long long c = block_sums[b];
        block_sums[b] = run;
        run += c;
    }
    if (t == 1023) {
        *total = part[1023];
    }
}

// offsets[k] = entries before point k (offsets[n] = all of them); views[offsets[k] ..]: the point's view, then its agreeing sources
__global__ __launch_bounds__(256) void k_vis_scatter(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                                      const int *__restrict__ pair_offsets, const int *__restrict__ pair_indices, size_t n,
                                                      const long long *__restrict__ block_prefix, const long long *__restrict__ total,
                                                      long long *__restrict__ offsets, int32_t *__restrict__ views)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int first = 0;
    uint32_t m = 0;
    int entries = 0;
    if (k < n) {
        m = vis_mask(sources, view, pair_offsets, k, first);
        entries = 1 + __popc(m);
    }
    int block_total;
    const long long at = block_prefix[blockIdx.x] + vis_block_scan(entries, &block_total);
    if (k < n) {
        offsets[k] = at;
        int32_t *list = views + at;
        *list++ = view[k];
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            *list++ = pair_indices[first + j];
        }
    }
    if (k == 0) {
        offsets[n] = *total;
    }
}

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

thread_local std::string g_fusion_error;
thread_local double g_fusion_ms[3] = {0.0, 0.0, 0.0};

namespace {

double ms_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// ExportPointCloud (APD.cpp:214-254): header + the views' records in order.  APD_OK, or APD_ERR_IO with g_fusion_error set
int write_ply(const char *who, const char *ply_path, long long count, const std::vector<std::vector<uint8_t>> &body, bool normals)
{
    FILE *f = fopen(ply_path, "wb");
    if (!f) {
        g_fusion_error = std::string(who) + ": cannot write " + ply_path;  // no length limit: not through set_error
        return APD_ERR_IO;
    }
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
               "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n", (int)count,
            normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "");
    bool ok = true;
    for (const std::vector<uint8_t> &part : body) {
        ok = ok && (part.empty() || fwrite(part.data(), 1, part.size(), f) == part.size());
    }
    if (fclose(f) != 0 || !ok) {
        g_fusion_error = std::string(who) + ": short write to " + ply_path;
        return APD_ERR_IO;
    }
    return APD_OK;
}

}  // namespace

void free_device_arrays(PointArrays &p)
{
    hipFree(p.xyz);
    hipFree(p.normal);
    hipFree(p.bgr);
    hipFree(p.support);
    hipFree(p.view);
    hipFree(p.pixel);
    hipFree(p.sources);
    p = PointArrays();
}

void free_host_arrays(PointArrays &p)
{
    free(p.xyz);
    free(p.normal);
    free(p.bgr);
    free(p.support);
    free(p.view);
    free(p.pixel);
    free(p.sources);
    p = PointArrays();
}

int check_options(const char *who, const apd_fusion_options *options, bool *preset_out)
{
    std::string &err = g_fusion_error;
    if (!options) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: null options", who);
    }
    if (options->struct_size != sizeof(apd_fusion_options)) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: struct_size %zu is not sizeof(apd_fusion_options) = %zu", who, options->struct_size,
                              sizeof(apd_fusion_options));
    }
    const apd_fusion_options o = *options, d = default_options();
    if (o.variant != APD_FUSION_ETH && o.variant != APD_FUSION_TAT_INTERMEDIATE && o.variant != APD_FUSION_TAT_ADVANCED) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: unknown variant %d", who, o.variant);
    }
    const struct {
        const char *name;
        float value, preset;
    } values[] = {{"max_reproj_error", o.max_reproj_error, d.max_reproj_error}, {"max_relative_depth", o.max_relative_depth, d.max_relative_depth},
                  {"max_angle", o.max_angle, d.max_angle},                      {"depth_weight", o.depth_weight, d.depth_weight},
                  {"angle_weight", o.angle_weight, d.angle_weight},             {"factor_strong", o.factor_strong, d.factor_strong},
                  {"factor_weak", o.factor_weak, d.factor_weak}};
    bool preset = o.min_consistent == d.min_consistent;
    for (const auto &v : values) {
        if (!(v.value >= 0.0f) || v.value > FLT_MAX) {
            return apd::set_error(err, APD_ERR_INVALID, "%s: %s is negative or not finite", who, v.name);
        }
        preset = preset && v.value == v.preset;
    }
    if (o.min_consistent < 1 || o.min_consistent > APD_MAX_IMAGES) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: min_consistent %d is outside 1 .. %d", who, o.min_consistent, APD_MAX_IMAGES);
    }
    *preset_out = preset;
    return APD_OK;
}

int Call::begin(bool eth, bool points)
{
    g_fusion_error.clear();
    auto invalid = [this](const char *what) { return apd::set_error(g_fusion_error, APD_ERR_INVALID, "%s: %s", who, what); };
    if (a.num_views <= 0 || !a.cameras || (points && !a.images) || !a.depths || !a.normals || (eth && !a.weaks) || !a.rows || !a.cols ||
        !a.pair_offsets || !a.pair_indices || (points && ((!a.ply_path && !a.points) || !a.num_points))) {
        return invalid("null argument");
    }
    if (points && a.image_channels != 1 && a.image_channels != 3) {
        return invalid("images have 1 (grey) or 3 (blue, green, red) channels");
    }
    for (int i = 0; i < a.num_views; ++i) {
        const int ns = a.pair_offsets[i + 1] - a.pair_offsets[i];
        if (ns < 0 || ns > APD_MAX_IMAGES) {
            return invalid("a view has more than APD_MAX_IMAGES sources");
        }
        if (a.rows[i] < 0 || a.cols[i] < 0 || (long long)a.rows[i] * a.cols[i] > 0x7fffff00LL) {  // pixel indices are ints
            return invalid("view size out of range");
        }
        for (int k = a.pair_offsets[i]; k < a.pair_offsets[i + 1]; ++k) {
            if (a.pair_indices[k] < 0 || a.pair_indices[k] >= a.num_views) {
                return invalid("source index out of range");
            }
            // ETH: the consumption of a view's own pixels would be order dependent inside the vote kernel; T&T: the view would read the
            // masks it writes
            if (a.pair_indices[k] == i) {
                return invalid(eth ? "a view lists itself as a source (use the host fusion)" : "a view lists itself as a source");
            }
        }
    }
    for (int i = 0; i < a.num_views; ++i) {
        max_px = std::max(max_px, (size_t)pixels(i));
        max_src = std::max(max_src, sources(i));
    }
    body_.resize((size_t)a.num_views);
    HIP_TRY(hipSetDevice(a.device));
    return APD_OK;
}

Call::Call(const char *who_, const Args &args) : who(who_), a(args), t_lap_(std::chrono::steady_clock::now()) {}

void Call::release()
{
    for (void *p : owned_) {
        hipFree(p);
    }
    owned_.clear();
    if (staging_) {
        hipHostFree(staging_);
        staging_ = nullptr;
    }
}

int Call::hip_failed(const char *expr, hipError_t e, const char *, int) const
{
    return apd::set_error(g_fusion_error, APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
}

int Call::alloc_common()
{
    HIP_TRY(alloc(max_px * 12, &xyz));
    HIP_TRY(alloc(max_px * 3, &bgr));
    HIP_TRY(alloc(max_px, &support));
    if (a.points) {  // the PLY-only call has no such buffer and its emit kernels no such store
        HIP_TRY(alloc(max_px * 4, &agreeing));
    }
    HIP_TRY(alloc(max_blocks() * 4, &block_counts));
    HIP_TRY(alloc(sizeof(int), &total_));
    if (a.ply_path) {  // without a file no record is packed or downloaded
        const size_t bytes = max_px * (size_t)record_bytes();
        HIP_TRY(alloc(bytes, &records_));
        if (hipHostMalloc(&staging_, bytes > 0 ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
            staging_ = nullptr;  // pageable downloads then
        }
    }
    g_fusion_ms[0] = lap();
    return APD_OK;
}

double Call::lap()
{
    const double ms = ms_since(t_lap_);
    t_lap_ = std::chrono::steady_clock::now();
    return ms;
}

int Call::collect(int i, const uint8_t *state, uint8_t accepted, const float *normal)
{
    const int n = pixels(i);
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_fusion_scan, dim3(1), dim3(1024), 0, 0, block_counts, blocks, total_);
    if (a.ply_path && a.opt.ply_normals) {
        hipLaunchKernelGGL(k_fusion_compact<true>, dim3(blocks), dim3(256), 0, 0, state, accepted, n, (const float *)xyz, (const uint8_t *)bgr,
                           normal, (const int *)block_counts, records_);
    } else if (a.ply_path) {
        hipLaunchKernelGGL(k_fusion_compact<false>, dim3(blocks), dim3(256), 0, 0, state, accepted, n, (const float *)xyz, (const uint8_t *)bgr,
                           normal, (const int *)block_counts, records_);
    }
    HIP_TRY(hipGetLastError());
    int npts = 0;
    HIP_TRY(hipMemcpy(&npts, total_, sizeof(int), hipMemcpyDeviceToHost));
    if (npts <= 0) {
        return APD_OK;
    }
    if (a.ply_path) {
        std::vector<uint8_t> &part = body_[i];
        part.resize((size_t)npts * record_bytes());
        if (staging_) {
            HIP_TRY(hipMemcpy(staging_, records_, part.size(), hipMemcpyDeviceToHost));
            memcpy(part.data(), staging_, part.size());
        } else {
            HIP_TRY(hipMemcpy(part.data(), records_, part.size(), hipMemcpyDeviceToHost));
        }
    }
    if (a.points) {
        if (const int rc = reserve_points(count_ + npts); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_fusion_compact_soa, dim3(blocks), dim3(256), 0, 0, state, accepted, n, i, (const float *)xyz, (const uint8_t *)bgr,
                           (const uint8_t *)support, (const uint32_t *)agreeing, normal, (const int *)block_counts, (size_t)count_, soa_);
        HIP_TRY(hipGetLastError());
    }
    count_ += npts;
    return APD_OK;
}

int Call::reserve_points(long long need)
{
    if (need <= soa_capacity_) {
        return APD_OK;
    }
    const long long capacity = std::max({need, 2 * soa_capacity_, 4096LL});
    const size_t c = (size_t)capacity, have = (size_t)count_;
    PointArrays grown;
    struct Guard {
        PointArrays &p;
        ~Guard() { free_device_arrays(p); }  // whatever `grown` still holds when this function returns
    } guard{grown};
    HIP_TRY(hipMalloc((void **)&grown.xyz, c * 12));
    HIP_TRY(hipMalloc((void **)&grown.normal, c * 12));
    HIP_TRY(hipMalloc((void **)&grown.bgr, c * 3));
    HIP_TRY(hipMalloc((void **)&grown.support, c));
    HIP_TRY(hipMalloc((void **)&grown.view, c * 4));
    HIP_TRY(hipMalloc((void **)&grown.pixel, c * 4));
    HIP_TRY(hipMalloc((void **)&grown.sources, c * 4));
    if (have > 0) {
        HIP_TRY(hipMemcpy(grown.xyz, soa_.xyz, have * 12, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.normal, soa_.normal, have * 12, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.bgr, soa_.bgr, have * 3, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.support, soa_.support, have, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.view, soa_.view, have * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.pixel, soa_.pixel, have * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(grown.sources, soa_.sources, have * 4, hipMemcpyDeviceToDevice));
    }
    std::swap(soa_, grown);  // the guard frees the old arrays
    soa_capacity_ = capacity;
    return APD_OK;
}

void Call::release_points()
{
    free_device_arrays(soa_);
    soa_capacity_ = 0;
}

int Call::finish()
{
    g_fusion_ms[1] = lap();
    apd_points *pts = nullptr;
    if (a.points) {
        HIP_TRY(hipDeviceSynchronize());  // the last view's compaction
        pts = new apd_points();
        pts->device = a.device;
        pts->on_device = a.opt.result_on_device ? 1 : 0;
        pts->count = count_;
        pts->pair_offsets.assign(a.pair_offsets, a.pair_offsets + a.num_views + 1);
        pts->pair_indices.assign(a.pair_indices, a.pair_indices + a.pair_offsets[a.num_views]);
        pts->rows.assign(a.rows, a.rows + a.num_views);
        pts->cols.assign(a.cols, a.cols + a.num_views);
        if (pts->on_device) {
            std::swap(pts->arrays, soa_);
            soa_capacity_ = 0;
        } else if (count_ > 0) {
            const size_t c = (size_t)count_;
            PointArrays &h = pts->arrays;
            h.xyz = (float *)malloc(c * 12);
            h.normal = (float *)malloc(c * 12);
            h.bgr = (uint8_t *)malloc(c * 3);
            h.support = (uint8_t *)malloc(c);
            h.view = (int32_t *)malloc(c * 4);
            h.pixel = (int32_t *)malloc(c * 4);
            h.sources = (uint32_t *)malloc(c * 4);
            hipError_t e = (h.xyz && h.normal && h.bgr && h.support && h.view && h.pixel && h.sources) ? hipSuccess : hipErrorOutOfMemory;
            e = e != hipSuccess ? e : hipMemcpy(h.xyz, soa_.xyz, c * 12, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.normal, soa_.normal, c * 12, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.bgr, soa_.bgr, c * 3, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.support, soa_.support, c, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.view, soa_.view, c * 4, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.pixel, soa_.pixel, c * 4, hipMemcpyDeviceToHost);
            e = e != hipSuccess ? e : hipMemcpy(h.sources, soa_.sources, c * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                apd_points_destroy(pts);
                return hip_failed("download of the points", e, __FILE__, __LINE__);
            }
        }
        release_points();
    }
    release();
    if (a.ply_path) {
        const int written = write_ply(who, a.ply_path, count_, body_, a.opt.ply_normals != 0);
        if (written != APD_OK) {
            apd_points_destroy(pts);
            return written;
        }
    }
    *a.num_points = count_;
    if (a.points) {
        *a.points = pts;
    }
    g_fusion_ms[2] = ms_since(t_lap_);
    return APD_OK;
}

}  // namespace apd_fusion

extern "C" const char *apd_fusion_last_error(void) { return apd_fusion::g_fusion_error.c_str(); }

extern "C" int apd_fusion_last_timing(double *setup_ms, double *views_ms, double *file_ms)
{
    if (setup_ms) {
        *setup_ms = apd_fusion::g_fusion_ms[0];
    }
    if (views_ms) {
        *views_ms = apd_fusion::g_fusion_ms[1];
    }
    if (file_ms) {
        *file_ms = apd_fusion::g_fusion_ms[2];
    }
    return APD_OK;
}

extern "C" int apd_fuse_views(int device, int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                              const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                              const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, int maps_on_device,
                              const char *ply_path, long long *num_points)
{
    const apd_fusion::Args a = {device, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                                pair_indices, maps_on_device, ply_path, num_points};
    return apd_fusion::run_eth("apd_fuse_views", a);
}

extern "C" void apd_fusion_default_options(apd_fusion_options *o)
{
    if (o) {
        *o = apd_fusion::default_options();
    }
}

extern "C" long long apd_points_count(apd_points_t p) { return p ? p->count : 0; }
extern "C" int apd_points_on_device(apd_points_t p) { return p ? p->on_device : 0; }
extern "C" const float *apd_points_xyz(apd_points_t p) { return p ? p->arrays.xyz : nullptr; }
extern "C" const float *apd_points_normal(apd_points_t p) { return p ? p->arrays.normal : nullptr; }
extern "C" const uint8_t *apd_points_bgr(apd_points_t p) { return p ? p->arrays.bgr : nullptr; }
extern "C" const uint8_t *apd_points_support(apd_points_t p) { return p ? p->arrays.support : nullptr; }
extern "C" const int32_t *apd_points_view(apd_points_t p) { return p ? p->arrays.view : nullptr; }
extern "C" const int32_t *apd_points_pixel(apd_points_t p) { return p ? p->arrays.pixel : nullptr; }
extern "C" const uint32_t *apd_points_sources(apd_points_t p) { return p ? p->arrays.sources : nullptr; }

namespace {

// Selects the device of device-resident points for one call and puts the caller's back
struct PointsDevice {
    int previous = -1;
    explicit PointsDevice(const apd_points *p)
    {
        if (p->on_device && hipGetDevice(&previous) != hipSuccess) {
            previous = -1;
        }
    }
    ~PointsDevice()
    {
        if (previous >= 0) {
            hipSetDevice(previous);
        }
    }
};

int vis_hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: %s: %s", expr, hipGetErrorString(e));
}

// The lists of host-resident points: the plain loop
int build_visibility_host(apd_points *p)
{
    const size_t n = (size_t)p->count;
    long long *offsets = (long long *)malloc((n + 1) * sizeof(long long));
    if (!offsets) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: out of host memory");
    }
    const apd_fusion::PointArrays &a = p->arrays;
    long long total = 0;
    for (size_t k = 0; k < n; ++k) {
        offsets[k] = total;
        total += 1 + __builtin_popcount(a.sources[k]);
    }
    offsets[n] = total;
    int32_t *views = (int32_t *)malloc(total > 0 ? (size_t)total * sizeof(int32_t) : sizeof(int32_t));
    if (!views) {
        free(offsets);
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: out of host memory");
    }
    for (size_t k = 0; k < n; ++k) {
        int32_t *list = views + offsets[k];
        *list++ = a.view[k];
        const int first = p->pair_offsets[(size_t)a.view[k]];
        for (int j = 0; j < 32; ++j) {
            if ((a.sources[k] >> j) & 1u) {
                *list++ = p->pair_indices[(size_t)(first + j)];
            }
        }
    }
    p->vis_offsets = offsets;
    p->vis_views = views;
    return APD_OK;
}

// The lists of device-resident points, on their device: k_vis_count, k_vis_scan, k_vis_scatter
int build_visibility_device(apd_points *p)
{
    const auto hip_failed = vis_hip_failed;  // what HIP_TRY returns here
    const size_t n = (size_t)p->count;
    const size_t nblocks = (n + 255) / 256;
    struct Scratch {
        std::vector<void *> owned;
        ~Scratch()
        {
            for (void *q : owned) {
                hipFree(q);
            }
        }
        hipError_t alloc(size_t bytes, void **out)
        {
            const hipError_t e = hipMalloc(out, bytes > 0 ? bytes : 1);
            if (e == hipSuccess) {
                owned.push_back(*out);
            }
            return e;
        }
        void keep(void *q) { owned.erase(std::find(owned.begin(), owned.end(), q)); }
    } scratch;
    long long *offsets = nullptr, *block_sums = nullptr, *dtotal = nullptr;
    int32_t *views = nullptr;
    int *pair_offsets = nullptr, *pair_indices = nullptr;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(scratch.alloc((n + 1) * sizeof(long long), (void **)&offsets));
    long long total = 0;
    if (n == 0) {
        HIP_TRY(hipMemset(offsets, 0, sizeof(long long)));
    } else {
        HIP_TRY(scratch.alloc(nblocks * sizeof(long long), (void **)&block_sums));
        HIP_TRY(scratch.alloc(sizeof(long long), (void **)&dtotal));
        HIP_TRY(scratch.alloc(p->pair_offsets.size() * sizeof(int), (void **)&pair_offsets));
        HIP_TRY(scratch.alloc(p->pair_indices.size() * sizeof(int), (void **)&pair_indices));
        HIP_TRY(hipMemcpy(pair_offsets, p->pair_offsets.data(), p->pair_offsets.size() * sizeof(int), hipMemcpyHostToDevice));
        if (!p->pair_indices.empty()) {
            HIP_TRY(hipMemcpy(pair_indices, p->pair_indices.data(), p->pair_indices.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        const apd_fusion::PointArrays &a = p->arrays;
        hipLaunchKernelGGL(k_vis_count, dim3((unsigned)nblocks), dim3(256), 0, 0, (const uint32_t *)a.sources, (const int32_t *)a.view,
                           (const int *)pair_offsets, n, block_sums);
        hipLaunchKernelGGL(k_vis_scan, dim3(1), dim3(1024), 0, 0, block_sums, nblocks, dtotal);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&total, dtotal, sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIP_TRY(scratch.alloc(total > 0 ? (size_t)total * sizeof(int32_t) : sizeof(int32_t), (void **)&views));
    if (n > 0) {
        const apd_fusion::PointArrays &a = p->arrays;
        hipLaunchKernelGGL(k_vis_scatter, dim3((unsigned)nblocks), dim3(256), 0, 0, (const uint32_t *)a.sources, (const int32_t *)a.view,
                           (const int *)pair_offsets, (const int *)pair_indices, n, (const long long *)block_sums, (const long long *)dtotal,
                           offsets, views);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    scratch.keep(offsets);
    scratch.keep(views);
    p->vis_offsets = offsets;
    p->vis_views = views;
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_visibility(apd_points_t p, const long long **offsets, const int32_t **views)
{
    apd_fusion::g_fusion_error.clear();
    if (!p || !offsets || !views) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_INVALID, "apd_points_visibility: null argument");
    }
    if (!p->vis_offsets) {
        PointsDevice device(p);
        if (const int rc = p->on_device ? build_visibility_device(p) : build_visibility_host(p); rc != APD_OK) {
            return rc;
        }
    }
    *offsets = p->vis_offsets;
    *views = p->vis_views;
    return APD_OK;
}

extern "C" int apd_points_write_vis(apd_points_t p, const char *path)
{
    std::string &err = apd_fusion::g_fusion_error;
    err.clear();
    if (!p || !path) {
        return apd::set_error(err, APD_ERR_INVALID, "apd_points_write_vis: null argument");
    }
    const long long *offsets = nullptr;
    const int32_t *views = nullptr;
    if (const int rc = apd_points_visibility(p, &offsets, &views); rc != APD_OK) {
        return rc;
    }
    const size_t n = (size_t)p->count;
    std::vector<long long> host_offsets;
    std::vector<int32_t> host_views;
    if (p->on_device) {  // one download of each array
        PointsDevice device(p);
        host_offsets.resize(n + 1);
        hipError_t e = hipSetDevice(p->device);
        e = e != hipSuccess ? e : hipMemcpy(host_offsets.data(), offsets, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost);
        if (e == hipSuccess && host_offsets[n] > 0) {
            host_views.resize((size_t)host_offsets[n]);
            e = hipMemcpy(host_views.data(), views, host_views.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        if (e != hipSuccess) {
            return apd::set_error(err, APD_ERR_HIP, "apd_points_write_vis: download of the lists: %s", hipGetErrorString(e));
        }
        offsets = host_offsets.data();
        views = host_views.data();
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        err = std::string("apd_points_write_vis: cannot write ") + path;
        return APD_ERR_IO;
    }
    // uint64 number of points, then per point uint32 n and n x uint32 view index, little endian like every file of the project
    const uint64_t count = (uint64_t)n;
    bool ok = fwrite(&count, 8, 1, f) == 1;
    std::vector<uint32_t> chunk;
    const size_t kChunk = 1u << 16;  // points per fwrite
    for (size_t k0 = 0; k0 < n && ok; k0 += kChunk) {
        const size_t k1 = std::min(n, k0 + kChunk);
        chunk.clear();
        for (size_t k = k0; k < k1; ++k) {
            chunk.push_back((uint32_t)(offsets[k + 1] - offsets[k]));
            for (long long e = offsets[k]; e < offsets[k + 1]; ++e) {
                chunk.push_back((uint32_t)views[e]);
            }
        }
        ok = fwrite(chunk.data(), 4, chunk.size(), f) == chunk.size();
    }
    if (fclose(f) != 0 || !ok) {
        err = std::string("apd_points_write_vis: short write to ") + path;
        return APD_ERR_IO;
    }
    return APD_OK;
}

extern "C" int apd_points_destroy(apd_points_t p)
{
    if (!p) {
        return APD_OK;
    }
    if (p->on_device) {
        int current = 0;
        const bool known = hipGetDevice(&current) == hipSuccess;
        hipSetDevice(p->device);
        apd_fusion::free_device_arrays(p->arrays);
        hipFree(p->vis_offsets);
        hipFree(p->vis_views);
        if (known) {
            hipSetDevice(current);
        }
    } else {
        apd_fusion::free_host_arrays(p->arrays);
        free(p->vis_offsets);
        free(p->vis_views);
    }
    delete p;
    return APD_OK;
}
