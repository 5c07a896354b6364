// apd_mesh_colour_math.h -- the rules by which the vertices of a mesh take their colour from the images of the cameras that see them
// (arithmetic contract C26): the relation under apd_mesh_colour_from_views, written once and compiled twice: by hipcc into
// the kernels (apd_mesh_colour.hip) and by g++ into the sequential checker (tests/helpers/mesh_colour_ref.cpp), both with
// -ffp-contract=off and no fast-math.  The projection is the fusion's (drop: apd_fusion_math.h), the seen test the points'
// (render_seen: apd_render_math.h), the depth map the mesh's own (contract C25, apd_mesh_render_math.h, both sides drawn), the normal
// the mesh's (contract C22, apd_mesh_math.h).
//
// Per view, in the call's order, Z = the C25 depth map of the mesh in that camera with kRenderCullNone.
//
// Sample.  The vertex at P with normal n takes a sample from a view when
//   1. n is not (0, 0, 0): some face names the vertex;
//   2. drop() gives d > 0 and finite;
//   3. the footprint is inside: with c0 = (int)floorf(u), r0 = (int)floorf(w): 0 <= c0, c0 + 1 <= cols - 1, 0 <= r0, r0 + 1 <= rows - 1,
//      evaluated on floorf(.) as a float before the conversion (colour_tap), so that a huge, infinite or NaN coordinate fails;
//   4. it is not occluded at any tap: for each of the pixels (c0 | c0 + 1, r0 | r0 + 1), z = Z[r][c] has z > 0 and
//      render_seen(d, z, rel_tolerance): the points' test on the whole bilinear footprint, which keeps the colour of a nearer surface
//      from bleeding into a vertex just behind its silhouette;
//   5. it faces the camera: e = centre - P per component, both widened to binary64 first; ne = (n.x e.x + n.y e.y) + n.z e.z,
//      ee = (e.x e.x + e.y e.y) + e.z e.z, c = ne / sqrt(ee), every product, sum, the root and the quotient one binary64 operation;
//      c > (double)min_cos.  A NaN fails.  The weight of the sample is c.
//
// Colour of a sample, binary32, one operation per step: fu = u - floorf(u), fw = w - floorf(w); per channel, with a, b the pixels
// (c0, r0), (c0 + 1, r0) and a', b' those of row r0 + 1: top = a + fu * (b - a), bot = a' + fu * (b' - a'),
// value = top + fw * (bot - top).  An image of one channel gives the three channels that value.
//
// Sums, binary64, in view order from +0.0: S_k = S_k + c * (double)value_k per channel (blue, green, red), W = W + c, count + 1.
//
// Result.  count > 0: per channel x = (float)(S_k / W), clamped to 0 .. 255 (a NaN is 0), (int)(x + 0.5f): the conversion of the
// volume's vertex colours (apd_volume_math.h).  count == 0: the vertex keeps its input colour, (0, 0, 0) without one.
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_render_math.h"

namespace apd_fusion {

// -R^T t in binary32, the term order of view_geometry (apd_fusion_device.h): what View::centre holds
APD_HD void colour_view_centre(const float R[9], const float t[3], float centre[3])
{
    centre[0] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
    centre[1] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
    centre[2] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
}

// Rule 3 along one axis of `size` pixels: lo = (int)floorf(v) when 0 <= lo and lo + 1 <= size - 1.  The comparison that guards the
// conversion is made on the float, as nearest_pixel makes its own: a NaN fails it
APD_HD bool colour_tap(float v, int size, int &lo)
{
    const float f = floorf(v);
    if (!(f >= 0.0f && f < 2147483648.0f)) {
        lo = -1;
        return false;
    }
    lo = (int)f;
    return lo <= size - 2;
}

// Rule 5: whether the vertex at P with normal n faces the camera of `view` by more than min_cos, and then the cosine c
APD_HD bool colour_facing(const View &view, const float P[3], const float n[3], float min_cos, double &c)
{
    const double ex = (double)view.centre[0] - (double)P[0];
    const double ey = (double)view.centre[1] - (double)P[1];
    const double ez = (double)view.centre[2] - (double)P[2];
    const double nx = (double)n[0] * ex, ny = (double)n[1] * ey, nz = (double)n[2] * ez;
    const double nxy = nx + ny;
    const double ne = nxy + nz;
    const double xx = ex * ex, yy = ey * ey, zz = ez * ez;
    const double xy = xx + yy;
    const double ee = xy + zz;
    const double len = sqrt(ee);
    c = ne / len;
    return c > (double)min_cos;
}

// What a vertex reads of a view that it takes a sample from: the upper left pixel of its footprint, the two fractions and its weight
struct ColourSample {
    int c0, r0;
    float fu, fw;
    double c;
};

// Rules 1 to 5 for the vertex at P with normal n; `depth_at(c, r)` is Z of an inside pixel
template <typename DepthAt>
APD_HD bool colour_sample(const View &view, const float P[3], const float n[3], float rel_tolerance, float min_cos, DepthAt &&depth_at, ColourSample &s)
{
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) {
        return false;
    }
    float u, w, d;
    drop(view, P, u, w, d);
    if (!(d > 0.0f) || f32_bits(d) >= 0x7f800000u) {
        return false;
    }
    if (!colour_tap(u, view.cols, s.c0) || !colour_tap(w, view.rows, s.r0)) {
        return false;
    }
    for (int k = 0; k < 4; ++k) {
        const float z = depth_at(s.c0 + (k & 1), s.r0 + (k >> 1));
        if (!(z > 0.0f) || !render_seen(d, z, rel_tolerance)) {
            return false;
        }
    }
    if (!colour_facing(view, P, n, min_cos, s.c)) {
        return false;
    }
    s.fu = u - floorf(u);
    s.fw = w - floorf(w);
    return true;
}

// One channel of a sample: a, b of row r0, a2, b2 of row r0 + 1
APD_HD float colour_bilinear(float a, float b, float a2, float b2, float fu, float fw)
{
    const float dt = b - a;
    const float pt = fu * dt;
    const float top = a + pt;
    const float db = b2 - a2;
    const float pb = fu * db;
    const float bot = a2 + pb;
    const float dv = bot - top;
    const float pv = fw * dv;
    return top + pv;
}

// S = S + c * (double)value
APD_HD double colour_add(double S, double c, float value)
{
    const double term = c * (double)value;
    return S + term;
}

// The byte of a channel with the sums S and W > 0
APD_HD uint8_t colour_byte(double S, double W)
{
    float x = (float)(S / W);
    x = !(x > 0.0f) ? 0.0f : (x > 255.0f ? 255.0f : x);  // a NaN is 0
    return (uint8_t)(int)(x + 0.5f);
}

}  // namespace apd_fusion
