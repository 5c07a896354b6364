// apd_fusion_tat.hip -- the Tanks and Temples fusions (RunFusion_TAT_Intermediate, APD.cpp:979-1147, and RunFusion_TAT_advanced,
// APD.cpp:1149-1296) on the device: apd_fuse_views_variant of include/apd_mi355x.h.
//
// Both loops walk the views in order and the pixels of a view in raster order, like the ETH loop (apd_fusion.hip), but they
// depend on that order in another way.  They never consume source pixels: they read `masks` of the sources only and set
// `masks` of the reference pixels they emit, so a view depends on earlier views through the masks and the pixels of one view
// do not depend on each other's decisions.  What they do depend on is `diff`, one entry per source that is declared once per
// view (APD.cpp:1069, :1233) and overwritten only where the source is valid (in bounds, not masked, depth > 0): a pixel at
// which source j is not valid sees the values of the last earlier pixel of the view, in raster order, at which j was.  That
// pixel is an inclusive max-scan over raster order of `valid_j(p) ? p : -1`, exact under any association.  Per view:
//
//   k_tat_valid   one lane per pixel: valid_j for every source (bit j of a 32-bit word per pixel), and per 256-pixel block
//                 and source the last valid pixel (wave ballots);
//   k_tat_scan    one workgroup per source: exclusive max-scan of the block values over the blocks of the view;
//   k_tat_decide  one lane per pixel: the last valid pixel q_j <= p of every source (own wave's ballot, the earlier waves of
//                 the block, then the block prefix), the costs recomputed at q_j (apd_fusion_math.h: the very arithmetic of the
//                 scan's pixel, so the same bits the reference stored in diff[j]), the k loop, and the point;
//   Call::collect (apd_fusion_device.h; k_fusion_scan + k_fusion_compact of apd_fusion_call.hip): the points in raster order as PLY
//                 records.
//
// Memory per view of n pixels and S sources: 4 n (validity words) + 8 S n / 256 (block values) + 1 n (emitted) + 30 n (the
// points before and after compaction, as in the ETH fusion) bytes, about 36 bytes per pixel (4 n more for the agreeing sources
// when the points in memory are asked for), plus one mask byte per pixel of every view for the whole run.  No (pixel, source) record is stored: at 6200 x 4130 with 10 sources the records would be
// ~4 GB, this layout is ~0.9 GB.
#include <hip/hip_runtime.h>

#include <float.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_fusion_math.h"

namespace {

using apd_fusion::View;

constexpr int kMaxSrc = APD_MAX_IMAGES;

struct TatView {
    View geo;
    const float *image;   // rows*cols*channels, 0..255; channels 1 (grey) or 3 (blue, green, red)
    const float *depth;   // <= 0: no estimate
    const float *normal;  // 3 per pixel, world frame
    const uint8_t *block; // optional `blocks/mask_<id>.jpg`: pixels < 128 are not fused as reference pixels
    uint8_t *mask;        // the reference's `masks`: 1 = emitted as a reference pixel
};

struct TatTask {
    int ref;                 // index of the reference view
    int num_src;
    int n;                   // pixels of the reference view
    int channels;            // of the images
    int intermediate;        // 1: RunFusion_TAT_Intermediate (angle test, averaged colour), 0: RunFusion_TAT_advanced
    int src[kMaxSrc];
    // thresholds of round k (index k = 2 .. num_src), computed on the host in float like the reference's `k * dist_base`,
    // `k * depth_base`, `k * angle_grad + angle_base`
    float max_dist[kMaxSrc + 1], max_depth[kMaxSrc + 1], max_angle[kMaxSrc + 1];
    uint32_t *valid;         // [pixel]: bit j = source j valid at the pixel
    int *block_last;         // [block][num_src]: last valid pixel of the block (-1: none); after k_tat_scan, of the blocks before it
    uint8_t *emitted;        // [pixel]: 1 = the pixel is a point
    float *xyz;              // [pixel][3]
    uint8_t *bgr;            // [pixel][3]
    uint8_t *support;        // [pixel]: `count` of the round that emitted the point
    uint32_t *agreeing;      // [pixel]: bit j = source j is counted in it; null: not asked for
    int *block_counts;       // points per block
};

__device__ __forceinline__ bool is_reference_pixel(const TatView &rv, int p)
{
    return !(rv.block && rv.block[p] < 128) && !(rv.depth[p] <= 0.0f);  // APD.cpp:1072-1078 (:1236-1242)
}

// valid(j) of APD.cpp:1086-1096 (:1252-1262): the pixel that world point P projects to in source sv, if any and usable
__device__ __forceinline__ bool source_pixel(const TatView &sv, const float P[3], int &sc, int &sr)
{
    if (!apd_fusion::vote_target(sv.geo, P, sc, sr)) {
        return false;
    }
    const int s = sr * sv.geo.cols + sc;
    return sv.mask[s] != 1 && !(sv.depth[s] <= 0.0f);
}

__global__ __launch_bounds__(256) void k_tat_valid(const TatView *__restrict__ views, TatTask task)
{
    const TatView &rv = views[task.ref];
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint32_t bits = 0;
    if (p < task.n) {
        if (is_reference_pixel(rv, p)) {
            const int r = p / rv.geo.cols, c = p - r * rv.geo.cols;
            float P[3];
            apd_fusion::lift(rv.geo, c, r, rv.depth[p], P);
            for (int j = 0; j < task.num_src; ++j) {
                int sc, sr;
                if (source_pixel(views[task.src[j]], P, sc, sr)) {
                    bits |= 1u << j;
                }
            }
        }
        task.valid[p] = bits;
    }
    __shared__ int wave_last[4][kMaxSrc];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < task.num_src; ++j) {
        const unsigned long long m = __ballot((bits >> j) & 1u);
        if (lane == 0) {
            wave_last[wave][j] = m ? (int)(blockIdx.x * 256 + wave * 64 + 63 - __clzll(m)) : -1;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < task.num_src) {
        const int j = threadIdx.x;
        const int last = max(max(wave_last[0][j], wave_last[1][j]), max(wave_last[2][j], wave_last[3][j]));
        task.block_last[(size_t)blockIdx.x * task.num_src + j] = last;
    }
}

// exclusive max-scan of block_last over the blocks of the view, for source j = blockIdx.x
__global__ __launch_bounds__(1024) void k_tat_scan(TatTask task, int nblocks)
{
    __shared__ int part[1024];
    const int j = blockIdx.x, t = threadIdx.x, S = task.num_src;
    const int per = (nblocks + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, nblocks);
    int m = -1;
    for (int b = b0; b < b1; ++b) {
        m = max(m, task.block_last[(size_t)b * S + j]);
    }
    part[t] = m;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (t >= off) ? part[t - off] : -1;
        __syncthreads();
        part[t] = max(part[t], v);
        __syncthreads();
    }
    int run = t > 0 ? part[t - 1] : -1;
    for (int b = b0; b < b1; ++b) {
        const int v = task.block_last[(size_t)b * S + j];
        task.block_last[(size_t)b * S + j] = run;
        run = max(run, v);
    }
}

// Last pixel <= this lane's of the view at which source j was valid, -1 if none: this wave's ballot up to the lane, else the
// last one of an earlier wave of the block, else the scanned prefix of the earlier blocks.
__device__ __forceinline__ int last_valid(const unsigned long long (*wave_mask)[kMaxSrc], const TatTask &task, int j, int wave,
                                          unsigned long long lanes_le)
{
    const unsigned long long mine = wave_mask[wave][j] & lanes_le;
    if (mine) {
        return (int)(blockIdx.x * 256 + wave * 64 + 63 - __clzll(mine));
    }
    for (int w = wave - 1; w >= 0; --w) {
        const unsigned long long m = wave_mask[w][j];
        if (m) {
            return (int)(blockIdx.x * 256 + w * 64 + 63 - __clzll(m));
        }
    }
    return task.block_last[(size_t)blockIdx.x * task.num_src + j];
}

// dynamic LDS: num_src * 256 bytes (first round each source passes at, per lane)
__global__ __launch_bounds__(256) void k_tat_decide(const TatView *__restrict__ views, TatTask task)
{
    extern __shared__ uint8_t first_round[];  // [j][lane of the block]
    __shared__ unsigned long long wave_mask[4][kMaxSrc];
    const TatView &rv = views[task.ref];
    const int S = task.num_src;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t bits = p < task.n ? task.valid[p] : 0u;
    for (int j = 0; j < S; ++j) {
        const unsigned long long m = __ballot((bits >> j) & 1u);
        if (lane == 0) {
            wave_mask[wave][j] = m;
        }
    }
    __syncthreads();
    const unsigned long long lanes_le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    bool emit = false;
    if (p < task.n && is_reference_pixel(rv, p)) {
        // diff[j] (APD.cpp:1097-1107): the costs at the last pixel q <= p where j was valid; FLT_MAX (never passes) if none
        for (int j = 0; j < S; ++j) {
            const TatView &sv = views[task.src[j]];
            const int q = last_valid(wave_mask, task, j, wave, lanes_le);
            int first = S + 1;
            int sc, sr;
            if (q >= 0) {
                const int rq = q / rv.geo.cols, cq = q - rq * rv.geo.cols;
                const float depth_q = rv.depth[q];
                float P[3];
                apd_fusion::lift(rv.geo, cq, rq, depth_q, P);
                if (apd_fusion::vote_target(sv.geo, P, sc, sr)) {  // always true: j was valid at q
                    const int s = sr * sv.geo.cols + sc;
                    const float ref_n[3] = {rv.normal[3 * (size_t)q], rv.normal[3 * (size_t)q + 1], rv.normal[3 * (size_t)q + 2]};
                    const float src_n[3] = {sv.normal[3 * (size_t)s], sv.normal[3 * (size_t)s + 1], sv.normal[3 * (size_t)s + 2]};
                    float dist, depth, angle;
                    apd_fusion::measure(rv.geo, sv.geo, cq, rq, depth_q, ref_n, sc, sr, sv.depth[s], src_n, dist, depth, angle);
                    // the thresholds grow with k, so "j is used in round k" is "k >= first round j passes"
                    for (int k = 2; k <= S; ++k) {
                        if (dist < task.max_dist[k] && depth < task.max_depth[k] && (!task.intermediate || angle < task.max_angle[k])) {
                            first = k;
                            break;
                        }
                    }
                }
            }
            first_round[j * 256 + threadIdx.x] = (uint8_t)first;
        }
        // the k loop (APD.cpp:1111-1144, :1277-1293): the first k with at least k sources used emits
        int count = 0, round = 0;
        for (int k = 2; k <= S && round == 0; ++k) {
            count = 0;
            for (int j = 0; j < S; ++j) {
                count += first_round[j * 256 + threadIdx.x] <= k;
            }
            if (count >= k) {
                round = k;
            }
        }
        if (round > 0) {
            emit = true;
            const int r = p / rv.geo.cols, c = p - r * rv.geo.cols;
            float P[3];
            apd_fusion::lift(rv.geo, c, r, rv.depth[p], P);
            const int nc = task.channels;
            float colour[3];
            for (int k = 0; k < 3; ++k) {
                colour[k] = rv.image[(size_t)p * nc + (nc == 3 ? k : 0)];
            }
            if (task.intermediate) {  // + the colours at diff[j].src_r / src_c of the used sources, in source order
                for (int j = 0; j < S; ++j) {
                    if (first_round[j * 256 + threadIdx.x] > round) {
                        continue;
                    }
                    const TatView &sv = views[task.src[j]];
                    const int q = last_valid(wave_mask, task, j, wave, lanes_le);
                    const int rq = q / rv.geo.cols, cq = q - rq * rv.geo.cols;
                    float Q[3];
                    int sc, sr;
                    apd_fusion::lift(rv.geo, cq, rq, rv.depth[q], Q);
                    if (!apd_fusion::vote_target(sv.geo, Q, sc, sr)) {  // never: the pixel k_tat_valid found at q
                        continue;
                    }
                    const size_t s = (size_t)sr * sv.geo.cols + sc;
                    for (int k = 0; k < 3; ++k) {
                        colour[k] += sv.image[s * nc + (nc == 3 ? k : 0)];
                    }
                }
                for (int k = 0; k < 3; ++k) {
                    colour[k] /= (count + 1.0f);
                }
            }
            task.xyz[3 * (size_t)p + 0] = P[0];
            task.xyz[3 * (size_t)p + 1] = P[1];
            task.xyz[3 * (size_t)p + 2] = P[2];
            for (int k = 0; k < 3; ++k) {
                task.bgr[3 * (size_t)p + k] = static_cast<uint8_t>(colour[k]);
            }
            task.support[p] = (uint8_t)count;
            if (task.agreeing) {
                uint32_t used = 0;
                for (int j = 0; j < S; ++j) {
                    used |= (uint32_t)(first_round[j * 256 + threadIdx.x] <= round) << j;
                }
                task.agreeing[p] = used;
            }
            rv.mask[p] = 1;
        }
    }
    if (p < task.n) {
        task.emitted[p] = emit ? 1 : 0;
    }
    const unsigned long long m = __ballot(emit);
    __shared__ int wave_counts[4];
    if (lane == 0) {
        wave_counts[wave] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        task.block_counts[blockIdx.x] = wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
    }
}

struct TatFusion : apd_fusion::Call {
    using Call::Call;
    int run(bool intermediate);
};

int TatFusion::run(bool intermediate)
{
    if (const int rc = begin(false); rc != APD_OK) {
        return rc;
    }
    std::vector<TatView> hv(a.num_views);
    for (int i = 0; i < a.num_views; ++i) {
        TatView &v = hv[i];
        const size_t n = (size_t)pixels(i);
        if (const int rc = fill_view(i, v); rc != APD_OK) {
            return rc;
        }
        if (const int rc = fill_block(i, v); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(alloc(n, &v.mask));
        HIP_TRY(hipMemset(v.mask, 0, n));  // APD.cpp:1038, :1205: one zeroed mask per view
    }
    TatView *dviews = nullptr;
    if (const int rc = upload_views(hv, &dviews); rc != APD_OK) {
        return rc;
    }
    uint32_t *valid;
    int *block_last;
    uint8_t *emitted;
    HIP_TRY(alloc(max_px * 4, &valid));
    HIP_TRY(alloc(max_blocks() * max_src * 4, &block_last));
    HIP_TRY(alloc(max_px, &emitted));
    if (const int rc = alloc_common(); rc != APD_OK) {
        return rc;
    }
    // APD.cpp:984-989, :1154-1155
    const float dist_base = 0.25f;
    const float depth_base = intermediate ? 1.0f / 3500.0f : 1.0f / 3000.0f;
    const float angle_base = 0.06981317007977318f;  // 4 degrees
    const float angle_grad = 0.05235987755982988f;  // 3 degrees
    for (int i = 0; i < a.num_views; ++i) {
        const int n = pixels(i);
        const int S = sources(i);
        if (n == 0 || S < 2) {
            continue;  // the k loop runs from 2 to the number of sources: nothing to emit
        }
        const int nblocks = (n + 255) / 256;
        TatTask task;
        memset(&task, 0, sizeof(task));
        task.ref = i;
        task.num_src = S;
        task.n = n;
        task.channels = a.image_channels;
        task.intermediate = intermediate ? 1 : 0;
        for (int j = 0; j < S; ++j) {
            task.src[j] = a.pair_indices[a.pair_offsets[i] + j];
        }
        for (int k = 2; k <= S; ++k) {
            task.max_dist[k] = k * dist_base;
            task.max_depth[k] = k * depth_base;
            task.max_angle[k] = k * angle_grad + angle_base;  // two roundings: the library is built without contraction
        }
        task.valid = valid;
        task.block_last = block_last;
        task.emitted = emitted;
        task.xyz = xyz;
        task.bgr = bgr;
        task.support = support;
        task.agreeing = agreeing;
        task.block_counts = block_counts;
        hipLaunchKernelGGL(k_tat_valid, dim3(nblocks), dim3(256), 0, 0, dviews, task);
        hipLaunchKernelGGL(k_tat_scan, dim3(S), dim3(1024), 0, 0, task, nblocks);
        hipLaunchKernelGGL(k_tat_decide, dim3(nblocks), dim3(256), (size_t)S * 256, 0, dviews, task);
        if (const int rc = collect(i, emitted, 1, hv[i].normal); rc != APD_OK) {
            return rc;
        }
    }
    return finish();
}

}  // namespace

extern "C" int apd_fuse_views_variant(int variant, int device, int num_views, const apd_camera *cameras, const float *const *images,
                                      int image_channels, const float *const *depths, const float *const *normals,
                                      const uint8_t *const *weaks, const uint8_t *const *blocks, const int *rows, const int *cols,
                                      const int *pair_offsets, const int *pair_indices, int maps_on_device, const char *ply_path,
                                      long long *num_points)
{
    if (variant == APD_FUSION_ETH) {
        return apd_fuse_views(device, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                              pair_indices, maps_on_device, ply_path, num_points);
    }
    const char *who = "apd_fuse_views_variant";
    if (variant != APD_FUSION_TAT_INTERMEDIATE && variant != APD_FUSION_TAT_ADVANCED) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_INVALID, "%s: unknown variant %d", who, variant);
    }
    const apd_fusion::Args a = {device, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                                pair_indices, maps_on_device, ply_path, num_points};
    return TatFusion(who, a).run(variant == APD_FUSION_TAT_INTERMEDIATE);
}

extern "C" int apd_fuse_views_opt(const apd_fusion_options *options, int device, int num_views, const apd_camera *cameras,
                                  const float *const *images, int image_channels, const float *const *depths, const float *const *normals,
                                  const uint8_t *const *weaks, const uint8_t *const *blocks, const int *rows, const int *cols,
                                  const int *pair_offsets, const int *pair_indices, int maps_on_device, const char *ply_path,
                                  long long *num_points, apd_points_t *points)
{
    const char *who = "apd_fuse_views_opt";
    std::string &err = apd_fusion::g_fusion_error;
    bool preset = false;
    if (const int rc = apd_fusion::check_options(who, options, &preset); rc != APD_OK) {
        return rc;
    }
    const apd_fusion_options o = *options;
    if (!ply_path && !points) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: ply_path and points are both NULL", who);
    }
    if (o.variant != APD_FUSION_ETH && !preset) {
        return apd::set_error(err, APD_ERR_UNSUPPORTED, "%s: the thresholds apply to APD_FUSION_ETH only; the T&T loops keep their own", who);
    }
    apd_fusion::Args a = {device, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                          pair_indices, maps_on_device, ply_path, num_points};
    a.opt = o;
    a.points = points;
    if (o.variant == APD_FUSION_ETH) {
        return apd_fusion::run_eth(who, a);
    }
    return TatFusion(who, a).run(o.variant == APD_FUSION_TAT_INTERMEDIATE);
}
