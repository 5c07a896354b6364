// apd_kernels.hip -- hand-written gfx950 kernels of the PatchMatch path (K1..K15 of SURVEY.md 2.1).
//
// Thread mapping: one lane per pixel.  Checkerboard kernels give a wave64 the 64 same-colour pixels
// of a 16x8 footprint (not the reference's 32x2 strip, APD.cu:1512-1519) and a 256-thread workgroup
// a 32x16 tile whose reference-image patch halo is staged in LDS.  Workgroups are dealt to XCDs in
// contiguous bands of tiles so every XCD's L2 holds one band of each image.
#include "apd_device.h"
#include "apd_sweep.h"

#include <float.h>
#include <stdlib.h>
#include <rocrand/rocrand_xorwow.h>

namespace apd {

// ------------------------------------------------------------------------------------------------
// K1  InitRandomStates (APD.cu:791-804): state(y, x) = xorwow(seed, subsequence = y, offset = x)
// ------------------------------------------------------------------------------------------------

// rocRAND keeps its state protected; this only exposes the six words after rocrand_init.
struct XorwowPeek : public rocrand_device::xorwow_engine {
    __device__ XorwowPeek(unsigned long long seed, unsigned long long subsequence, unsigned long long offset)
        : rocrand_device::xorwow_engine(seed, subsequence, offset)
    {
    }
    __device__ Rng words() const { return Rng{m_state.x[0], m_state.x[1], m_state.x[2], m_state.x[3], m_state.x[4], m_state.d}; }
};

constexpr int kRngSegment = 64;  // pixels stepped sequentially after one skip-ahead

// One lane jumps to (row y, column x0) with rocRAND's skip-ahead matrices, then walks kRngSegment
// columns with plain xorwow steps: identical to rocrand_init(seed, y, x) per pixel, ~64x cheaper.
__global__ __launch_bounds__(64) void k1_init_random_states(FrameArgs fa)
{
    const int segs_per_row = (fa.W + kRngSegment - 1) / kRngSegment;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= segs_per_row * fa.H) {
        return;
    }
    const int y = gid / segs_per_row;
    const int x0 = (gid - y * segs_per_row) * kRngSegment;
    XorwowPeek eng(fa.seed, (unsigned long long)y, (unsigned long long)x0);
    Rng r = eng.words();
    const int x1 = min(x0 + kRngSegment, fa.W);
    for (int x = x0; x < x1; ++x) {
        rng_store(fa.rng, y * fa.W + x, r);
        rng_next(r);
    }
}

// ------------------------------------------------------------------------------------------------
// K5  RandomInitialization (APD.cu:806-835) with the initial costs of :616-693
// ------------------------------------------------------------------------------------------------

// The full-frame tiling (full_frame_pixel, stage_full_frame_ref) is in apd_sweep.h; the window-less kernels pad the tile
// rows to an odd pitch.
constexpr int kFullPitch = kFullLdsW | 1;

// kTiled: the NCCs of the random planes (FIRST_INIT) gather from the tiled copy of the quad image
template <bool kQuad, bool kTiled>
__global__ __launch_bounds__(256) void k5_random_initialization(FrameArgs fa)
{
    __shared__ float tile[kFullLdsH * kFullPitch];
    int px, py;
    full_frame_pixel(px, py);
    const RefPatchLds<kFullPitch> rp = stage_full_frame_ref<kFullPitch>(fa, tile, px, py);
    if (px >= fa.W || py >= fa.H) {
        return;
    }
    const int center = py * fa.W + px;
    if (fa.state == APD_FIRST_INIT) {
        Rng rng = rng_load(fa.rng, center);
        const float4 pl = random_plane(fa, px, py, rng);
        rng_store(fa.rng, center, rng);
        fa.planes[center] = pl;
        // ComputeMultiViewInitialCostandSelectedViews, :616-662
        float qx, qy, qz;
        plane_q(pl, qx, qy, qz);
        float sorted[32], orig[32];
        int valid = 0;
#pragma unroll 1
        for (int v = 0; v < fa.num_src; ++v) {
            const float c = ncc_fixed<kQuad, RefPatchLds<kFullPitch>, kTiled>(fa, view_const(fa, v), rp, px, py, qx, qy, qz);
            sorted[v] = c;
            orig[v] = c;
            if (c < 2.0f) {
                valid++;
            }
        }
        sort_ascending(sorted, fa.num_src);
        uint32_t sel = 0;
        float cost = 2.0f;
        const int top_k = min(valid, fa.top_k);
        if (top_k > 0) {
            float acc = 0.0f;
            for (int i = 0; i < top_k; ++i) {
                acc += sorted[i];
            }
            const float thr = sorted[top_k - 1];
            for (int i = 0; i < fa.num_src; ++i) {
                if (orig[i] <= thr) {
                    sel |= 1u << i;
                }
            }
            cost = acc / (float)top_k;
        }
        fa.selected_views[center] = sel;
        fa.costs[center] = cost;
    } else {
        // loaded (world normal, depth) -> (camera normal, distance), :827-832
        float4 pl = normal_world_to_cam(fa, fa.planes[center]);
        const float depth = pl.w;
        pl.w = distance_to_origin(fa, px, py, depth, pl.x, pl.y, pl.z);
        fa.planes[center] = pl;
        // ComputeMultiViewInitialCost, :664-693
        float qx, qy, qz;
        plane_q(pl, qx, qy, qz);
        uint32_t sel = fa.selected_views[center];
        int count = 0;
        float cost = 0.0f;
#pragma unroll 1
        for (int v = 0; v < fa.num_src; ++v) {
            if (bit_test(sel, (unsigned)v)) {
                const float c = ncc_fixed<kQuad>(fa, view_const(fa, v), rp, px, py, qx, qy, qz);
                if (c < 2.0f) {
                    count++;
                    cost += c;
                } else {
                    sel = bit_unset_quirk(sel, (unsigned)v);
                }
            }
        }
        fa.selected_views[center] = sel;
        fa.costs[center] = (count == 0) ? 2.0f : cost / (float)count;
    }
}

// ------------------------------------------------------------------------------------------------
// K6/K7  Black/RedPixelUpdateStrong -> CheckerboardPropagationStrong (APD.cu:982-1321, 837-890)
// ------------------------------------------------------------------------------------------------

// minimum waves per SIMD the register allocator must leave room for (ms per launch at 4096x3072 N=8 -- ref patch in registers:
// 2: 32.0, 3: 28.3; ref patch in LDS: 3: 28.2, 4: 27.4)
constexpr int kK67Waves = 4;

// One launch = one colour.  Hypotheses 0..7 are the propagation arms, 8 the current plane,
// 9..13 the refinement set; a single loop keeps one inlined copy of the 36-sample NCC.
template <int NMAX, bool kQuad>
__global__ __launch_bounds__(256, kK67Waves) void k67_update_strong(FrameArgs fa, int colour, int iter)
{
    __shared__ float tile[kLdsH * kLdsPitch];
    const TilePixel t = checkerboard_pixel(fa, colour);
    // stage the reference tile + 5 px halo (clamp-to-edge, as the texture unit would)
    for (int idx = threadIdx.x; idx < kLdsW * kLdsH; idx += 256) {
        const int r = idx / kLdsW, c = idx - r * kLdsW;
        tile[r * kLdsPitch + c] = fetch_texel(fa.ref_img, fa.W, fa.H, t.tx0 + c - kHalo, t.ty0 + r - kHalo);
    }
    __syncthreads();
    if (!checkerboard_active(fa, t)) {
        return;
    }
    const int px = t.px, py = t.py;
    const int center = py * fa.W + px;
    if (fa.weak_info[center] == APD_WEAK || masked_out(fa, center)) {
        return;
    }
    // ref_patch_from_lds (apd_sweep.h), written out: through the helper this kernel's generated code changes
    RefPatchLds<kLdsPitch> rp;
    rp.base = &tile[t.ly * kLdsPitch + t.lx];
    {
        RefPatch tmp;
#pragma unroll
        for (int i = 0; i < kPatchN; ++i) {
#pragma unroll
            for (int j = 0; j < kPatchN; ++j) {
                tmp.v[i * kPatchN + j] = rp.at(i, j);
            }
        }
        ref_patch_finish(tmp);
        rp.mean = tmp.mean;
        rp.var = tmp.var;
    }

    const int nsrc = fa.num_src;
    Rng rng = rng_load(fa.rng, center);
    float cost_array[9][NMAX];  // [8] = current plane
    for (int h = 0; h < 9; ++h) {
        for (int v = 0; v < NMAX; ++v) {
            cost_array[h][v] = 0.0f;
        }
    }
    cost_array[0][0] = 2.0f;  // "= { 2.0f }" sets only the first element (APD.cu:1004)
    int positions[8];
    unsigned flags = 0;
    ViewWeights<NMAX> vw;
    vw.clear();
    float weight_norm = 0.0f;
    uint32_t sel = 0;
    float4 plane_now = fa.planes[center];
    float depth_now = 0.0f, cost_now = 0.0f, cost_committed = 0.0f;
    float ref_depths[5];
    float4 ref_normals[5];

#pragma unroll 1
    for (int h = 0; h < 14; ++h) {
        if (h == 9) {
            // ---- joint view selection (:1203-1271) ----
            float priors[NMAX];
            for (int j = 0; j < NMAX; ++j) {
                priors[j] = 0.0f;
            }
            const int nb_pos[4] = {center - fa.W, center + fa.W, center - 1, center + 1};
            for (int i = 0; i < 4; ++i) {
                if (flags & (1u << (2 * i))) {
                    const uint32_t sv = fa.selected_views[nb_pos[i]];
                    for (int j = 0; j < nsrc; ++j) {
                        priors[j] += bit_test(sv, (unsigned)j) == 1 ? 0.9f : 0.1f;
                    }
                }
            }
            select_views<NMAX>(fa, iter, cost_array, priors, rng, vw, sel, weight_norm);
            vw.store(fa, center);
            float final_costs[8];
            for (int i = 0; i < 8; ++i) {
                float f = 0.0f;
                for (int j = 0; j < nsrc; ++j) {
                    const uint32_t wj = vw.get(j);
                    if (wj > 0) {
                        f += (float)wj * cost_array[i][j];
                    }
                }
                final_costs[i] = f / weight_norm;
            }
            int best = 0;  // FindMinCostIndex: "<=" -> last minimum wins (:29-40)
            float best_c = final_costs[0];
            for (int i = 1; i < 8; ++i) {
                if (final_costs[i] <= best_c) {
                    best_c = final_costs[i];
                    best = i;
                }
            }
            cost_now = 0.0f;
            for (int i = 0; i < nsrc; ++i) {
                cost_now += (float)vw.get(i) * cost_array[8][i];
            }
            cost_now /= weight_norm;
            cost_committed = cost_now;  // costs[center] = cost_now (:1295)
            depth_now = depth_from_plane(fa, plane_now, px, py);
            if (flags & (1u << best)) {
                const float4 cand = fa.planes[positions[best]];
                const float d = depth_from_plane(fa, cand, px, py);
                if (d >= fa.depth_min && d <= fa.depth_max && final_costs[best] < cost_now) {
                    depth_now = d;
                    plane_now = cand;
                    cost_now = final_costs[best];
                    fa.selected_views[center] = sel;
                }
            }
            make_refinement_set(fa, px, py, rng, plane_now, depth_now, ref_depths, ref_normals);
        }
        float4 pl;
        if (h < 8) {
            int pos;
            if (!arm_candidate(fa, px, py, h, pos)) {
                continue;
            }
            positions[h] = pos;
            flags |= 1u << h;
            pl = fa.planes[pos];
        } else if (h == 8) {
            pl = plane_now;
        } else {
            pl = ref_normals[h - 9];
            pl.w = distance_to_origin(fa, px, py, ref_depths[h - 9], pl.x, pl.y, pl.z);
        }
        float qx, qy, qz;
        plane_q(pl, qx, qy, qz);
        float tc = 0.0f;
#pragma unroll 1
        for (int v = 0; v < nsrc; ++v) {
            const uint32_t wv = vw.get(v);
            if (h >= 9 && wv == 0) {
                continue;  // a refinement hypothesis only ever uses the costs of the selected views (:876-880)
            }
            const float c = ncc_fixed<kQuad>(fa, view_const(fa, v), rp, px, py, qx, qy, qz);
            if (h < 9) {
                cost_array[h][v] = c;
            } else {
                tc += (float)wv * c;
            }
        }
        if (h >= 9) {  // PlaneHypothesisRefinementStrong accept test (:881-888)
            tc /= weight_norm;
            const float d = depth_from_plane(fa, pl, px, py);
            if (d >= fa.depth_min && d <= fa.depth_max && tc < cost_now) {
                depth_now = d;
                plane_now = pl;
                cost_now = tc;
            }
        }
    }
    rng_store(fa.rng, center, rng);
    if (fa.state == APD_REFINE_INIT) {  // :1311-1316, double comparison
        if ((double)cost_now < (double)cost_committed - 0.1) {
            fa.costs[center] = cost_now;
            fa.planes[center] = plane_now;
        } else {
            fa.costs[center] = cost_committed;
        }
    } else {
        fa.costs[center] = cost_now;
        fa.planes[center] = plane_now;
    }
}

// ------------------------------------------------------------------------------------------------
// K11  GetDepthandNormal (APD.cu:1587-1602)
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k11_depth_and_normal(FrameArgs fa)
{
    const int center = blockIdx.x * 256 + threadIdx.x;
    if (center >= fa.W * fa.H || masked_out(fa, center)) {
        return;
    }
    const int py = center / fa.W, px = center - py * fa.W;
    float4 pl = fa.planes[center];
    pl.w = depth_from_plane(fa, pl, px, py);
    fa.planes[center] = normal_cam_to_world(fa, pl);
}

// ------------------------------------------------------------------------------------------------
// K12/K13  Black/RedPixelFilterStrong (APD.cu:1604-1748)
// ------------------------------------------------------------------------------------------------

// {dx, dy, extra top margin}: every reference condition is "tap inside the image" except the two
// (+-1,-2) taps, which additionally need p.y > 2 (:1691, :1695).
__constant__ int8_t k_filter_taps[20][3] = {
    {0, -1, 0}, {0, -3, 0}, {0, -5, 0},  {0, 1, 0},  {0, 3, 0},   {0, 5, 0},   {-1, 0, 0},
    {-3, 0, 0}, {-5, 0, 0}, {1, 0, 0},   {3, 0, 0},  {5, 0, 0},   {2, -1, 0},  {2, 1, 0},
    {-2, -1, 0}, {-2, 1, 0}, {-1, -2, 1}, {1, -2, 1}, {-1, 2, 0}, {1, 2, 0}};

__global__ __launch_bounds__(256) void k1213_filter_strong(FrameArgs fa, int colour)
{
    const TilePixel t = checkerboard_pixel(fa, colour);
    if (!checkerboard_active(fa, t)) {
        return;
    }
    const int px = t.px, py = t.py, W = fa.W;
    const int center = py * W + px;
    if (fa.weak_info[center] == APD_WEAK || masked_out(fa, center)) {
        return;
    }
    if (fa.costs[center] < 0.001f) {
        return;
    }
    float f[21];
    int n = 0;
    f[n++] = fa.planes[center].w;
    for (int k = 0; k < 20; ++k) {
        const int qx = px + k_filter_taps[k][0], qy = py + k_filter_taps[k][1];
        if (inside(fa, qx, qy - k_filter_taps[k][2]) && fa.weak_info[qx + qy * W] == APD_STRONG) {
            f[n++] = fa.planes[qx + qy * W].w;
        }
    }
    sort_ascending(f, n);
    const int m = n / 2;
    fa.planes[center].w = (n % 2 == 0) ? (f[m - 1] + f[m]) / 2 : f[m];
}

// ------------------------------------------------------------------------------------------------
// K14 DepthToWeak (APD.cu:1990-2144) and K15 LocalRefine (:2146-2232)
// ------------------------------------------------------------------------------------------------

// Weighted cost of one depth sample along the pixel's ray over the selected views.
//   kLocalRefine == false: sum_sel (ncc + gf*geom) * w           (:2070-2080, :2031-2035)
//   kLocalRefine == true : sum_sel ncc*w (+ gf*geom*w)            (:2217-2220)
template <bool kLocalRefine, bool kQuad, typename Ref>
__device__ __forceinline__ float disparity_sample_cost(const FrameArgs &fa, const Ref &rp, int px, int py, const float4 origin,
                                                       float depth, uint32_t sel, const ViewWeights<32> &vw)
{
    float4 pl = origin;
    pl.w = distance_to_origin(fa, px, py, depth, pl.x, pl.y, pl.z);
    float qx, qy, qz;
    plane_q(pl, qx, qy, qz);
    float acc = 0.0f;
#pragma unroll 1
    for (int v = 0; v < fa.num_src; ++v) {
        if (bit_test(sel, (unsigned)v)) {
            const float c = ncc_fixed<kQuad>(fa, view_const(fa, v), rp, px, py, qx, qy, qz);
            if (kLocalRefine) {
                const float wv = (float)vw.get(v);
                acc += c * wv;
                if (fa.geom_consistency) {
                    acc += fa.geom_factor * geom_cost(fa, view_const(fa, v), px, py, pl) * wv;
                }
            } else {
                float tc = 0.0f;
                tc += c;
                if (fa.geom_consistency) {
                    tc += fa.geom_factor * geom_cost(fa, view_const(fa, v), px, py, pl);
                }
                acc += tc * (float)vw.get(v);
            }
        }
    }
    return acc;
}

template <bool kQuad>
__global__ __launch_bounds__(256) void k14_depth_to_weak(FrameArgs fa)
{
    __shared__ float tile[kFullLdsH * kFullPitch];
    int px, py;
    full_frame_pixel(px, py);
    const RefPatchLds<kFullPitch> rp = stage_full_frame_ref<kFullPitch>(fa, tile, px, py);
    if (px >= fa.W || py >= fa.H) {
        return;
    }
    const int W = fa.W, H = fa.H;
    const int min_margin = 6;
    const int center = px + py * W;
    if (masked_out(fa, center)) {
        return;
    }
    if (px < min_margin || py < min_margin || px >= W - min_margin || py >= H - min_margin) {
        fa.weak_info[center] = APD_UNKNOWN;
        return;
    }
    const float4 origin = normal_world_to_cam(fa, fa.planes[center]);
    const float origin_depth = origin.w;
    if (origin_depth == 0) {
        fa.weak_info[center] = APD_UNKNOWN;
        return;
    }
    const uint32_t sel = fa.selected_views[center];
    ViewWeights<32> vw;
    vw.load(fa, center);
    float base_line, weight_normal;
    const int valid = baseline_and_weight(fa, sel, vw, base_line, weight_normal);
    if (valid == 0) {
        fa.weak_info[center] = APD_UNKNOWN;
        return;
    }
    // cost_now of :2022-2051 is computed by the reference but never used by K14's classification
    base_line /= (float)valid;
    const float disp = fa.K[0] * base_line / origin_depth;
    constexpr int RADIUS = 30, NP = 2 * RADIUS + 1;
    float pc[NP];
#pragma unroll 1
    for (int pd = -RADIUS; pd <= RADIUS; ++pd) {
        const float p_depth = fa.K[0] * base_line / (disp + (float)pd);
        if (p_depth < fa.depth_min || p_depth > fa.depth_max) {
            pc[pd + RADIUS] = 2.0f;
            continue;
        }
        float p_cost = disparity_sample_cost<false, kQuad>(fa, rp, px, py, origin, p_depth, sel, vw);
        p_cost /= weight_normal;
        pc[pd + RADIUS] = (2.0f > p_cost) ? p_cost : 2.0f;  // MIN(2.0f, p_cost): NaN -> 2
    }
    uint64_t peaks = 0;
    int peak_count = 0, min_peak = 0;
    float min_cost = 2.0f;
    for (int i = 2; i < NP - 2; ++i) {
        if (pc[i - 1] > pc[i] && pc[i + 1] > pc[i]) {
            peaks |= 1ull << i;
            peak_count++;
            if (pc[i] < min_cost) {
                min_peak = i;
                min_cost = pc[i];
            }
        }
    }
    if (abs(min_peak - RADIUS) > fa.weak_peak_radius || pc[min_peak] > 0.5f) {
        fa.weak_info[center] = APD_WEAK;
        return;
    }
    if (peak_count == 1) {
        fa.weak_info[center] = (pc[min_peak] <= 0.15f) ? APD_STRONG : APD_WEAK;
        return;
    }
    float var = 0.0f;
    for (int i = 2; i < NP - 2; ++i) {
        if (((peaks >> i) & 1ull) && i != min_peak) {
            const float dist = pc[i] - min_cost;
            var += dist * dist;
        }
    }
    var = sqrtf(var);
    var /= (float)(peak_count - 1);
    fa.weak_info[center] = (var > 0.2f) ? APD_STRONG : APD_WEAK;
}

template <bool kQuad>
__global__ __launch_bounds__(256) void k15_local_refine(FrameArgs fa)
{
    __shared__ float tile[kFullLdsH * kFullPitch];
    int px, py;
    full_frame_pixel(px, py);
    const RefPatchLds<kFullPitch> rp = stage_full_frame_ref<kFullPitch>(fa, tile, px, py);
    if (px >= fa.W || py >= fa.H) {
        return;
    }
    const int W = fa.W;
    const int center = px + py * W;
    if (masked_out(fa, center)) {
        return;
    }
    const float4 origin = normal_world_to_cam(fa, fa.planes[center]);
    const float origin_depth = origin.w;
    if (origin_depth == 0) {
        return;
    }
    const uint32_t sel = fa.selected_views[center];
    ViewWeights<32> vw;
    vw.load(fa, center);
    float base_line, weight_normal;
    const int valid = baseline_and_weight(fa, sel, vw, base_line, weight_normal);
    if (weight_normal == 0 || valid == 0) {
        return;
    }
    base_line /= (float)valid;
    const float disp = fa.K[0] * base_line / origin_depth;
    const int radius = 5;
    float cost_now = 0.0f;
    float min_cost = 2.0f;
    float best_depth = origin_depth;
    // pd == -radius-1 evaluates the current depth with K14's cost form (:2173-2183)
#pragma unroll 1
    for (int pd = -radius - 1; pd <= radius; ++pd) {
        if (pd == -radius - 1) {
            cost_now = disparity_sample_cost<false, kQuad>(fa, rp, px, py, origin, origin_depth, sel, vw) / weight_normal;
            continue;
        }
        const float p_depth = fa.K[0] * base_line / (disp + (float)pd);
        if (p_depth < fa.depth_min || p_depth > fa.depth_max) {
            continue;
        }
        const float tc = disparity_sample_cost<true, kQuad>(fa, rp, px, py, origin, p_depth, sel, vw) / weight_normal;
        if (tc < min_cost) {
            min_cost = tc;
            best_depth = p_depth;
        }
    }
    if ((double)(cost_now - min_cost) > 0.1) {
        fa.planes[center].w = best_depth;
    }
}

// ------------------------------------------------------------------------------------------------
// texel-quad images (built once per upload)
// ------------------------------------------------------------------------------------------------

// *flag stays 1 only if every pixel is an integer in [0, 255] (8-bit input at scale 1; -0.0f counts as 0: every sum of an NCC
// starts at +0.0f, so the sign of a zero texel never shows).  *outside is set to 1 by a pixel outside the domain the NCC tail is
// exact in (kPixelLimit, apd_device.h): NaN, +-inf or |v| > 2^20.
__global__ __launch_bounds__(256) void k_check_u8(const float *__restrict__ img, int n, int *flag, int *outside)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = img[i];
        if (!(v >= 0.0f && v <= 255.0f && v == floorf(v))) {
            *flag = 0;
        }
        if (!(fabsf(v) <= kPixelLimit)) {
            *outside = 1;
        }
    }
}

// 2-byte column pairs (the row-major copy, apd_device.h): entry (t, u), t in [0, W + 1], u in [0, H], =
// {I(t - 1, u - 1), I(t - 1, u)} with clamped coordinates
__global__ __launch_bounds__(256) void k_pack_pairs(const float *__restrict__ img, int W, int H, uint16_t *__restrict__ pairs)
{
    const int t = blockIdx.x * 32 + (threadIdx.x & 31);
    const int u = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (t > W + 1 || u > H) {
        return;
    }
    const uint32_t top = (uint32_t)fetch_texel(img, W, H, t - 1, u - 1), bot = (uint32_t)fetch_texel(img, W, H, t - 1, u);
    pairs[(size_t)u * (W + 2) + t] = (uint16_t)(top | (bot << 8));
}

// the tiled copy (apd_device.h: quad_tiled_offset_tu).  One thread per (tile row, slot): slots 0..6 are the tile's own
// columns, slot 7 repeats the first column of the next tile so that every dword of the tile holds two consecutive pairs
__global__ __launch_bounds__(256) void k_pack_quads_tiled(const float *__restrict__ img, int W, int H, quad_t *__restrict__ quad)
{
    const unsigned tiles_x = quad_tiles_x(W), tiles_y = quad_tiles_y(H);
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;  // (tile, row in tile, slot)
    const unsigned slot = gid & 7u, iy = (gid >> 3) & 7u, tile = gid >> 6;
    if (tile >= tiles_x * tiles_y) {
        return;
    }
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int t = (int)(tx * 7u + slot), u = (int)(ty * 8u + iy);
    const uint32_t top = (uint32_t)fetch_texel(img, W, H, t - 1, u - 1), bot = (uint32_t)fetch_texel(img, W, H, t - 1, u);
    reinterpret_cast<uint16_t *>(quad)[(size_t)tile * 64u + iy * 8u + slot] = (uint16_t)(top | (bot << 8));
}

// float texel quads of a float image: entry (qx, qy), qx in [-1, W-1], qy in [-1, H-1] (clamped coordinates)
__global__ __launch_bounds__(256) void k_pack_fquads(const float *__restrict__ img, int W, int H, fquad_t *__restrict__ fq)
{
    const int qx = blockIdx.x * 32 + (threadIdx.x & 31);  // 0..W  <-> image x = qx - 1
    const int qy = blockIdx.y * 8 + (threadIdx.x >> 5);   // 0..H  <-> image y = qy - 1
    if (qx > W || qy > H) {
        return;
    }
    const float t00 = fetch_texel(img, W, H, qx - 1, qy - 1), t10 = fetch_texel(img, W, H, qx, qy - 1);
    const float t01 = fetch_texel(img, W, H, qx - 1, qy), t11 = fetch_texel(img, W, H, qx, qy);
    fq[(size_t)qy * (W + 1) + qx] = fquad_t{t00, t10 - t00, t01, t11 - t01};
}

hipError_t launch_pack_fquads(const float *img, int W, int H, fquad_t *fq, hipStream_t s)
{
    hipLaunchKernelGGL(k_pack_fquads, dim3((W + 1 + 31) / 32, (H + 1 + 7) / 8), dim3(256), 0, s, img, W, H, fq);
    return hipGetLastError();
}

hipError_t launch_check_u8(const float *img, int n, int *flag, int *outside, hipStream_t s)
{
    hipLaunchKernelGGL(k_check_u8, dim3((n + 255) / 256), dim3(256), 0, s, img, n, flag, outside);
    return hipGetLastError();
}

hipError_t launch_pack_pairs(const float *img, int W, int H, quad_t *quad, hipStream_t s)
{
    hipLaunchKernelGGL(k_pack_pairs, dim3((W + 2 + 31) / 32, (H + 1 + 7) / 8), dim3(256), 0, s, img, W, H, reinterpret_cast<uint16_t *>(quad));
    return hipGetLastError();
}

hipError_t launch_pack_quads_tiled(const float *img, int W, int H, quad_t *quad, hipStream_t s)
{
    const size_t threads = (size_t)quad_tiles_x(W) * quad_tiles_y(H) * 64u;
    hipLaunchKernelGGL(k_pack_quads_tiled, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, img, W, H, quad);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------

static inline dim3 grid_full_frame(const FrameArgs &fa) { return dim3((fa.W + kFullTileW - 1) / kFullTileW, (fa.H + kFullTileH - 1) / kFullTileH); }
static inline int checkerboard_tiles(const FrameArgs &fa) { return ((fa.W + kTileW - 1) / kTileW) * ((fa.H + kTileH - 1) / kTileH); }

hipError_t launch_k67_windowed(const FrameArgs &fa, int colour, int iter, hipStream_t s);  // apd_kernels_k67w.hip

// APD_OPT_K67_WINDOWS = 0 selects the kernel without the LDS source windows (A/B timing and the window-vs-global parity
// test; same results)

hipError_t launch_k14_windowed(const FrameArgs &fa, hipStream_t s);  // apd_kernels_k1415w.hip
hipError_t launch_k15_windowed(const FrameArgs &fa, hipStream_t s);

// APD_OPT_K1415_WINDOWS = 0: K14/K15 without LDS source windows (same results)

template <int NMAX>
static void launch_k67(const FrameArgs &fa, int colour, int iter, hipStream_t s)
{
    if (fa.use_quads) {
        hipLaunchKernelGGL((k67_update_strong<NMAX, true>), dim3(checkerboard_tiles(fa)), dim3(256), 0, s, fa, colour, iter);
    } else {
        hipLaunchKernelGGL((k67_update_strong<NMAX, false>), dim3(checkerboard_tiles(fa)), dim3(256), 0, s, fa, colour, iter);
    }
}

hipError_t launch_kernel(const FrameArgs &fa, int kernel_id, int iter, hipStream_t s)
{
    switch (kernel_id) {
    case APD_K1_INIT_RANDOM_STATES: {
        const int segs = ((fa.W + kRngSegment - 1) / kRngSegment) * fa.H;
        hipLaunchKernelGGL(k1_init_random_states, dim3((segs + 63) / 64), dim3(64), 0, s, fa);
        break;
    }
    case APD_K5_RANDOM_INITIALIZATION:
        if (fa.use_quads) {
            if (fa.have_tiled && fa.state == APD_FIRST_INIT) {
                hipLaunchKernelGGL((k5_random_initialization<true, true>), grid_full_frame(fa), dim3(256), 0, s, fa);
            } else {
                hipLaunchKernelGGL((k5_random_initialization<true, false>), grid_full_frame(fa), dim3(256), 0, s, fa);
            }
        } else {
            hipLaunchKernelGGL((k5_random_initialization<false, false>), grid_full_frame(fa), dim3(256), 0, s, fa);
        }
        break;
    case APD_K6_BLACK_UPDATE_STRONG:
    case APD_K7_RED_UPDATE_STRONG: {
        const int colour = (kernel_id == APD_K6_BLACK_UPDATE_STRONG) ? 0 : 1;
        if (fa.k67_windows) {
            return launch_k67_windowed(fa, colour, iter, s);
        }
        with_view_capacity(fa.num_src, [&](auto nmax) { launch_k67<decltype(nmax)::value>(fa, colour, iter, s); });
        break;
    }
    case APD_K11_GET_DEPTH_NORMAL:
        hipLaunchKernelGGL(k11_depth_and_normal, dim3((fa.W * fa.H + 255) / 256), dim3(256), 0, s, fa);
        break;
    case APD_K12_BLACK_FILTER:
    case APD_K13_RED_FILTER:
        hipLaunchKernelGGL(k1213_filter_strong, dim3(checkerboard_tiles(fa)), dim3(256), 0, s, fa,
                           (kernel_id == APD_K12_BLACK_FILTER) ? 0 : 1);
        break;
    case APD_K14_DEPTH_TO_WEAK:
        if (fa.k1415_windows) {
            return launch_k14_windowed(fa, s);
        }
        if (fa.use_quads) {
            hipLaunchKernelGGL(k14_depth_to_weak<true>, grid_full_frame(fa), dim3(256), 0, s, fa);
        } else {
            hipLaunchKernelGGL(k14_depth_to_weak<false>, grid_full_frame(fa), dim3(256), 0, s, fa);
        }
        break;
    case APD_K15_LOCAL_REFINE:
        if (fa.k1415_windows) {
            return launch_k15_windowed(fa, s);
        }
        if (fa.use_quads) {
            hipLaunchKernelGGL(k15_local_refine<true>, grid_full_frame(fa), dim3(256), 0, s, fa);
        } else {
            hipLaunchKernelGGL(k15_local_refine<false>, grid_full_frame(fa), dim3(256), 0, s, fa);
        }
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace apd
