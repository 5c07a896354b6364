// apd_sweep.h -- pieces shared by the strong and weak checkerboard kernels, by the two forms of K6/K7 (with LDS source
// windows, apd_kernels_k67w.hip; without, apd_kernels.hip) and by the full-frame kernels K5, K14, K15 in both forms.
#pragma once

#include <float.h>

#include <type_traits>

#include "apd_device.h"

namespace apd {

__device__ __forceinline__ void sort_ascending(float *d, int n)  // APD.cu:3-12
{
    for (int i = 1; i < n; ++i) {
        const float v = d[i];
        int j = i;
        while (j >= 1 && v < d[j - 1]) {
            d[j] = d[j - 1];
            --j;
        }
        d[j] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// checkerboard tiling shared by K6/K7, K9/K10, K12/K13
// ------------------------------------------------------------------------------------------------

// A wave64 owns the 64 same-colour pixels of a (128 / APD_CB_ROWS) x APD_CB_ROWS footprint; four waves make the
// workgroup tile.  The footprint shape trades two things: a wide, flat footprint makes one wave-level gather touch
// fewer 128-B lines of the row-major source image (the L1 looks lines up one per cycle), a square one keeps the
// patch halo, i.e. the L1 working set, small.
constexpr int kWaveH = APD_CB_ROWS, kWaveLanesX = 64 / kWaveH, kWaveW = 2 * kWaveLanesX;
constexpr int kWavesX = (kWaveH == 8) ? 2 : 1, kWavesY = 4 / kWavesX;
constexpr int kTileW = kWaveW * kWavesX, kTileH = kWaveH * kWavesY, kHalo = kPatchRadius;  // 32x16 (rows 8, 4) or 64x8 (rows 2)
constexpr int kLdsW = kTileW + 2 * kHalo;
constexpr int kLdsH = kTileH + 2 * kHalo;
constexpr int kLdsPitch = kLdsW | 1;           // odd pitch spreads the column reads over banks

struct TilePixel {
    int tx0, ty0;  // tile origin
    int lx, ly;    // pixel inside the tile
    int px, py;
};

// colour 0 = black ((x + y) even), 1 = red; wave w covers sub-tile (w % kWavesX, w / kWavesX).
__device__ __forceinline__ TilePixel checkerboard_pixel(const FrameArgs &fa, int colour)
{
    const int tiles_x = (fa.W + kTileW - 1) / kTileW;
    const int tiles_y = (fa.H + kTileH - 1) / kTileH;
    const int tile = xcd_band_tile(blockIdx.x, tiles_x * tiles_y);
    TilePixel t;
    t.ty0 = (tile / tiles_x) * kTileH;
    t.tx0 = (tile - (tile / tiles_x) * tiles_x) * kTileW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    t.ly = (wave / kWavesX) * kWaveH + lane / kWaveLanesX;
    t.lx = (wave % kWavesX) * kWaveW + 2 * (lane % kWaveLanesX) + ((t.ly + colour) & 1);
    t.px = t.tx0 + t.lx;
    t.py = t.ty0 + t.ly;
    return t;
}

__device__ __forceinline__ bool checkerboard_active(const FrameArgs &fa, const TilePixel &t)
{
    // rows beyond half_rows are never visited by the reference's HALF launch (APD.cu:2402)
    return t.px < fa.W && t.py < fa.H && t.py < fa.half_rows;
}

// The 36 reference texels stay in the LDS tile (one ds_read per sample); only their moments live in registers.
// `base` is the texel at offset (-radius, -radius) of the lane's pixel.
template <int kPitch>
__device__ __forceinline__ RefPatchLds<kPitch> ref_patch_from_lds(const float *base)
{
    RefPatchLds<kPitch> rp;
    rp.base = base;
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
    return rp;
}

// ------------------------------------------------------------------------------------------------
// view weights: counts 0..15 (15 draws, APD.cu:1249) kept as nibbles in registers; the reference's
// uchar[32] per pixel (view_weight_cuda) is still what is stored in HBM.
// ------------------------------------------------------------------------------------------------

template <int NMAX>
struct ViewWeights {
    static constexpr int kWords = (NMAX + 7) / 8;
    uint32_t w[kWords];

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < kWords; ++i) {
            w[i] = 0;
        }
    }
    __device__ __forceinline__ uint32_t word(int v) const
    {
        uint32_t x = w[0];
#pragma unroll
        for (int i = 1; i < kWords; ++i) {
            x = ((v >> 3) == i) ? w[i] : x;
        }
        return x;
    }
    __device__ __forceinline__ uint32_t get(int v) const { return (word(v) >> ((v & 7) * 4)) & 15u; }
    __device__ __forceinline__ void inc(int v)
    {
        const uint32_t one = 1u << ((v & 7) * 4);
#pragma unroll
        for (int i = 0; i < kWords; ++i) {
            w[i] += ((v >> 3) == i) ? one : 0u;
        }
    }
    // view_weight_cuda layout: one byte per view, 32 bytes per pixel
    __device__ __forceinline__ void store(const FrameArgs &fa, int center) const
    {
        uint32_t b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t nib = (i / 2 < kWords) ? (w[i / 2 < kWords ? i / 2 : 0] >> ((i & 1) * 16)) & 0xFFFFu : 0u;
            b[i] = (nib & 15u) | (((nib >> 4) & 15u) << 8) | (((nib >> 8) & 15u) << 16) | (((nib >> 12) & 15u) << 24);
        }
        uint4 *dst = reinterpret_cast<uint4 *>(fa.view_weight + (size_t)center * APD_MAX_IMAGES);
        dst[0] = make_uint4(b[0], b[1], b[2], b[3]);
        dst[1] = make_uint4(b[4], b[5], b[6], b[7]);
    }
    __device__ __forceinline__ void load(const FrameArgs &fa, int center)
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(fa.view_weight + (size_t)center * APD_MAX_IMAGES);
        const uint4 a = src[0], c = src[1];
        const uint32_t b[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int i = 0; i < kWords; ++i) {
            uint32_t x = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t d = b[2 * i + k];
                const uint32_t nib = (d & 15u) | (((d >> 8) & 15u) << 4) | (((d >> 16) & 15u) << 8) | (((d >> 24) & 15u) << 12);
                x |= nib << (16 * k);
            }
            w[i] = x;
        }
    }
};

// ------------------------------------------------------------------------------------------------
// view selection shared by strong (:1203-1271) and weak (:1365-1434) propagation
// ------------------------------------------------------------------------------------------------

template <int NMAX>
__device__ __forceinline__ void select_views(const FrameArgs &fa, int iter, const float (*cost_array)[NMAX], const float *priors,
                                             Rng &rng, ViewWeights<NMAX> &vw, uint32_t &sel_out, float &weight_norm_out)
{
    const int nsrc = fa.num_src;
    float probs[NMAX];
    const float thr = (float)(0.8 * (double)exp_poly((float)(iter * iter) / (-90.0f)));
    for (int i = 0; i < nsrc; ++i) {
        float count = 0;
        int count_false = 0;
        float tmpw = 0;
        for (int j = 0; j < 8; ++j) {
            const float c = cost_array[j][i];
            if (c < thr) {
                tmpw += exp_poly(c * c / (-0.18f));
                count++;
            }
            if (c > 1.2f) {
                count_false++;
            }
        }
        float p = 0.0f;
        if (count > 2 && count_false < 3) {
            p = tmpw / count;
        } else if (count_false < 3) {
            p = exp_poly(thr * thr / (-0.32f));
        }
        probs[i] = p * priors[i];
    }
    // TransformPDFToCDF, APD.cu:143-157
    float sum = 0.0f;
    for (int i = 0; i < nsrc; ++i) {
        sum += probs[i];
    }
    const float inv = 1.0f / sum;
    float acc = 0.0f;
    for (int i = 0; i < nsrc; ++i) {
        acc += probs[i] * inv;
        probs[i] = acc;
    }
    for (int sample = 0; sample < 15; ++sample) {
        const float rp = rng_uniform(rng) - FLT_EPSILON;
        for (int v = 0; v < nsrc; ++v) {
            if (probs[v] > rp) {
                vw.inc(v);
                break;
            }
        }
    }
    uint32_t sel = 0;
    float wn = 0;
    for (int i = 0; i < nsrc; ++i) {
        const uint32_t wi = vw.get(i);
        if (wi > 0) {
            sel |= 1u << i;
            wn += (float)wi;
        }
    }
    sel_out = sel;
    weight_norm_out = wn;
}

// Early-out bound of the refinement loops (K6/K7, K9/K10).  A refinement hypothesis is accepted iff
// fl(sum / weight_norm) < cost (APD.cu:884, :932, :974) with sum = the weighted costs added view by view.  Every term is
// >= 0, so the partial sums and their quotients never decrease; if a partial sum has reached a value t with
// t / weight_norm >= cost in real arithmetic, the final quotient is >= cost as well and the hypothesis is rejected
// whatever the remaining views cost.  Returns such a t: fl(cost * weight_norm) is within 2^-24 (relative) of the
// product, two roundings and the factor 1 + 2^-22 put the result strictly above it.  Tiny, zero-weight and non-finite
// inputs return +inf or NaN (never "lost": the loops then score every view, as the reference does).
__device__ __forceinline__ float refinement_lost_bound(const FrameArgs &fa, float cost, float weight_norm)
{
    const float p = cost * weight_norm;
    if (!fa.early_out || !(p >= 0x1p-100f) || !(weight_norm > 0.0f)) {
        return __builtin_inff();
    }
    return p * (1.0f + 0x1p-22f);
}

// The five refinement hypotheses of APD.cu:855-867 / :939-951 (RNG order: depth, normal, depth, 3 angles).
__device__ __forceinline__ void make_refinement_set(const FrameArgs &fa, int px, int py, Rng &rng, const float4 plane, float depth,
                                                    float *depths, float4 *normals)
{
    const float depth_perturbation = 0.02f, normal_perturbation = 0.02f;
    const float depth_rand = rng_uniform(rng) * (fa.depth_max - fa.depth_min) + fa.depth_min;
    const float4 n_rand = random_normal(fa, px, py, rng, depth);
    const float lo = (1 - depth_perturbation) * depth;
    const float hi = (1 + depth_perturbation) * depth;
    const float depth_pert = rng_uniform(rng) * (hi - lo) + lo;  // the reference's do-while never loops
    const float4 n_pert = perturbed_normal(fa, px, py, plane, rng, (float)((double)normal_perturbation * 3.14159265358979323846));
    depths[0] = depth_rand;
    depths[1] = depth;
    depths[2] = depth_rand;
    depths[3] = depth;
    depths[4] = depth_pert;
    normals[0] = plane;
    normals[1] = n_rand;
    normals[2] = n_rand;
    normals[3] = n_pert;
    normals[4] = plane;
}

// ------------------------------------------------------------------------------------------------
// K6/K7  Black/RedPixelUpdateStrong (APD.cu:982-1321): shared by the kernel with LDS source windows and the one without.
// Their tile staging, decision block and commit are written out in each kernel: as a shared inlined function every form
// tried changed the generated code of one of the two (profiles/shared_sweep/isa_identity.txt).
// ------------------------------------------------------------------------------------------------

// Cheapest candidate of propagation arm `arm` (order of APD.cu:1020: near/far x up,down,left,right).
__device__ __forceinline__ bool arm_candidate(const FrameArgs &fa, int px, int py, int arm, int &pos)
{
    const int d = arm >> 1;
    const int dx = (d == 2) ? -1 : (d == 3 ? 1 : 0);
    const int dy = (d == 0) ? -1 : (d == 1 ? 1 : 0);
    const float *__restrict__ costs = fa.costs;
    const int W = fa.W;
    if (arm & 1) {  // far: +-3, then ten more at stride 2 (:1021-1095)
        if (!inside(fa, px + 3 * dx, py + 3 * dy)) {
            return false;
        }
        int best = (px + 3 * dx) + (py + 3 * dy) * W;
        float cmin = costs[best];
        for (int i = 1; i < 11; ++i) {
            const int qx = px + (3 + 2 * i) * dx, qy = py + (3 + 2 * i) * dy;
            if (inside(fa, qx, qy)) {
                const int q = qx + qy * W;
                const float c = costs[q];
                if (c < cmin) {
                    cmin = c;
                    best = q;
                }
            }
        }
        pos = best;
        return true;
    }
    // near: +-1, then three V-shaped pairs, negative side first (:1097-1199)
    if (!inside(fa, px + dx, py + dy)) {
        return false;
    }
    const int ex = dy != 0 ? 1 : 0, ey = dx != 0 ? 1 : 0;
    int best = (px + dx) + (py + dy) * W;
    float cmin = costs[best];
    for (int i = 0; i < 3; ++i) {
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            const int qx = px + (2 + i) * dx + sgn * (1 + i) * ex;
            const int qy = py + (2 + i) * dy + sgn * (1 + i) * ey;
            if (inside(fa, qx, qy)) {
                const int q = qx + qy * W;
                const float c = costs[q];
                if (c < cmin) {
                    cmin = c;
                    best = q;
                }
            }
        }
    }
    pos = best;
    return true;
}

// The kernels that keep a per-pixel table over the views are compiled for NMAX = 8, 12, 16 and 32 columns: calls
// f(std::integral_constant<int, NMAX>) with the smallest that holds num_src.  Ten sources is the common MVS count: it
// does not pay scratch for sixteen columns.
template <typename F>
static inline void with_view_capacity(int num_src, F &&f)
{
    if (num_src <= 8) {
        f(std::integral_constant<int, 8>());
    } else if (num_src <= 12) {
        f(std::integral_constant<int, 12>());
    } else if (num_src <= 16) {
        f(std::integral_constant<int, 16>());
    } else {
        f(std::integral_constant<int, 32>());
    }
}

// ------------------------------------------------------------------------------------------------
// full-frame kernels (K5, K14, K15; K14 and K15 with and without LDS source windows)
// ------------------------------------------------------------------------------------------------

// A wave64 covers a (64 / APD_FF_ROWS) x APD_FF_ROWS block of pixels, four waves a workgroup tile (same trade-off as
// APD_CB_ROWS above).
constexpr int kFfWaveH = APD_FF_ROWS, kFfWaveW = 64 / kFfWaveH;
constexpr int kFfWavesX = (kFfWaveH == 8) ? 2 : 1, kFfWavesY = 4 / kFfWavesX;
constexpr int kFullTileW = kFfWaveW * kFfWavesX, kFullTileH = kFfWaveH * kFfWavesY;  // 16x16 (rows 8, 4) or 32x8 (rows 2)
constexpr int kFullLdsW = kFullTileW + 2 * kPatchRadius, kFullLdsH = kFullTileH + 2 * kPatchRadius;

__device__ __forceinline__ void full_frame_pixel(int &px, int &py)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    px = blockIdx.x * kFullTileW + (wave % kFfWavesX) * kFfWaveW + lane % kFfWaveW;
    py = blockIdx.y * kFullTileH + (wave / kFfWavesX) * kFfWaveH + lane / kFfWaveW;
}

// Stages the workgroup's reference tile + 5 px halo (clamp-to-edge) at kPitch floats per row and returns this lane's patch
// accessor.  Every thread of the block must call it.
template <int kPitch>
__device__ __forceinline__ RefPatchLds<kPitch> stage_full_frame_ref(const FrameArgs &fa, float *tile, int px, int py)
{
    const int x0 = blockIdx.x * kFullTileW - kPatchRadius, y0 = blockIdx.y * kFullTileH - kPatchRadius;
    for (int idx = threadIdx.x; idx < kFullLdsW * kFullLdsH; idx += 256) {
        const int r = idx / kFullLdsW, c = idx - r * kFullLdsW;
        tile[r * kPitch + c] = fetch_texel(fa.ref_img, fa.W, fa.H, x0 + c, y0 + r);
    }
    __syncthreads();
    return ref_patch_from_lds<kPitch>(&tile[(py - y0 - kPatchRadius) * kPitch + (px - x0 - kPatchRadius)]);
}

// baseline + weight sum over the selected views (:2036-2044); no image access
__device__ __forceinline__ int baseline_and_weight(const FrameArgs &fa, uint32_t sel, const ViewWeights<32> &vw, float &base_line, float &weight_normal)
{
    float bl = 0, wn = 0.0f;
    int valid = 0;
    for (int v = 0; v < fa.num_src; ++v) {
        if (bit_test(sel, (unsigned)v)) {
            const ViewConst &vc = view_const(fa, v);
            wn += (float)vw.get(v);
            const float d0 = fa.c[0] - vc.c[0];
            const float d1 = fa.c[1] - vc.c[1];
            const float d2 = fa.c[2] - vc.c[2];
            const double tv = (double)(d0 * d0 + d1 * d1 + d2 * d2);
            bl += sqrtf((float)tv);
            valid++;
        }
    }
    base_line = bl;
    weight_normal = wn;
    return valid;
}

}  // namespace apd
