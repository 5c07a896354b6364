// apd_render_math.h -- the per-point arithmetic of the z-buffered rendering of a cloud into a camera (arithmetic contract C15,
// DESIGN.md): the relation under apd_points_render and apd_points_rendered_visibility, written once and compiled twice: by hipcc
// into the kernels (apd_points_render.hip) and by g++ into the sequential checker (tests/helpers/points_render_ref.cpp), both with
// -ffp-contract=off and no fast-math.  The projection and the rounding to a pixel are the fusion's (drop, nearest_pixel:
// apd_fusion_math.h), so a point lands in the pixel the fusion would have voted in.
#pragma once

#include "apd_fusion_math.h"

namespace apd_fusion {

constexpr int kRenderMaxSplat = 8;            // the footprint is at most 17 x 17 pixels
constexpr uint64_t kRenderEmptyKey = ~0ull;   // of a pixel no footprint covers: above every key of a drawn point
constexpr uint32_t kRenderNoIndex = 0xFFFFFFFFu;

// Whether the point at P is drawn into `view` (K, R, t, rows = height, cols = width), and then its centre pixel (c, r) and depth d:
// d > 0 and finite, both pixel coordinates convertible, and the centre pixel inside the image.  A point whose centre pixel is
// outside is not drawn at all, whatever its footprint would cover.
APD_HD bool render_draw(const View &view, const float P[3], int &c, int &r, float &d)
{
    float u, w;
    drop(view, P, u, w, d);
    if (!(d > 0.0f) || f32_bits(d) >= 0x7f800000u) {
        return false;
    }
    if (!nearest_pixel(u, c) || !nearest_pixel(w, r)) {
        return false;
    }
    return c >= 0 && c < view.cols && r >= 0 && r < view.rows;
}

// The footprint of a point drawn at centre coordinate x along an axis of `size` pixels: [lo, hi], clipped.  Written so that no
// sum leaves the ints: x + splat is formed only where it stays below size.
APD_HD void render_span(int x, int splat, int size, int &lo, int &hi)
{
    lo = x > splat ? x - splat : 0;
    hi = x < size - splat ? x + splat : size - 1;
}

// Positive finite binary32 values order like their bits: the smallest key of a pixel is its nearest point, and among equal
// depths the lowest index
APD_HD uint64_t render_key(float d, uint32_t k) { return ((uint64_t)f32_bits(d) << 32) | (uint64_t)k; }

APD_HD float render_depth(uint64_t key)
{
    if (key == kRenderEmptyKey) {
        return 0.0f;
    }
    const uint32_t bits = (uint32_t)(key >> 32);
    float d;
    memcpy(&d, &bits, 4);
    return d;
}

APD_HD uint32_t render_index(uint64_t key) { return (uint32_t)key; }  // of the empty key: kRenderNoIndex

// A drawn point of depth d is seen when the map holds z at its centre pixel and d - z <= rel_tolerance * z: one subtraction, one
// multiplication, one comparison.  z <= d, since the point itself competed for that pixel.
APD_HD bool render_seen(float d, float z, float rel_tolerance)
{
    const float behind = d - z;
    const float allowed = rel_tolerance * z;
    return behind <= allowed;
}

}  // namespace apd_fusion
