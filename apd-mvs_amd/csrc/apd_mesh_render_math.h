// apd_mesh_render_math.h -- the rules of the z-buffered rasterisation of a mesh into a camera and of the face visibility that
// follows from it (arithmetic contract C25): the relation under apd_mesh_render, apd_mesh_face_visibility and
// apd_mesh_remove_unseen, written once and compiled twice: by hipcc into the kernels (apd_mesh_render.hip) and by g++ into the
// sequential checker (tests/helpers/mesh_render_ref.cpp), both with -ffp-contract=off and no fast-math.  The projection is the
// fusion's (drop: apd_fusion_math.h); the key, the empty pixel and the seen test are the points' (apd_render_math.h).
//
// Vertex.  drop() gives u, w, d in binary32.  The vertex is usable when d > 0 and finite and su = u * 256.0f + 0.5f and
// sw = w * 256.0f + 0.5f (a multiplication, then an addition) are finite with |floorf(.)| <= 2^27: the guard band, 2^19 pixels
// either side of the origin.  Its fixed-point position is X = (int)floorf(su), Y = (int)floorf(sw), in 1/256 pixel; pixel (c, r)
// has its centre at (256 c, 256 r), the convention of nearest_pixel: integer coordinates are pixel centres.
//
// Face.  Drawn when its three vertices are usable and A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) (int64) is not 0.  Two stated
// limits: there is no near-plane clipping, so a face with a corner behind the camera (or at a non-finite position) is not drawn at
// all, and neither is a face with a corner beyond the guard band.
// Facing.  With camera coordinates p_i (x right, y down, z forward) p0 . ((p1 - p0) x (p2 - p0)) = det(p0, p1, p2) = z0 z1 z2 times
// the projected doubled area, and for a K with K[0] K[4] - K[1] K[3] > 0 (every usual camera) that area has the sign of A2.  The
// right-hand normal n = (p1 - p0) x (p2 - p0), the one apd_mesh_with_vertex_normals sums, points towards the camera when
// n . (0 - p0) > 0, that is p0 . n < 0: a face is FRONT-facing when A2 < 0 and back-facing when A2 > 0.  kRenderCullBack draws
// front faces only, kRenderCullNone both sides.
// If A2 < 0 corners 1 and 2 are exchanged for everything below, so that A2 > 0.
//
// Coverage, integers only, top-left rule.  For edge a -> b: dx = Xb - Xa, dy = Yb - Ya, E(p) = dx * (py - Ya) - dy * (px - Xa) in
// int64.  Only the pixels of the face's bounding box clipped to the image are candidates, so |px - Xa|, |dx| <= 2^28 and every
// product is below 2^57.  A pixel centre is covered when for all three edges (0 -> 1, 1 -> 2, 2 -> 0) E > 0, or E == 0 with dy < 0,
// or E == 0 with dy == 0 and dx > 0.  Two faces that share an edge walk it in opposite directions, so a centre on it belongs to one.
//
// Depth, perspective-correct, binary64, one IEEE operation per step.  w_i = the edge function opposite corner i at the pixel
// (w0 = E of 1 -> 2, w1 = E of 2 -> 0, w2 = E of 0 -> 1), S = w0 + w1 + w2 in int64,
// q = ((double)w0 / (double)d0 + (double)w1 / (double)d1) + (double)w2 / (double)d2, z = (float)((double)S / q).  The pixel takes
// the face only when z > 0 and z is finite.
//
// Maps.  Per pixel the smallest render_key(z, f) over the faces that cover it: the nearest face, and among equal depth bits the
// lowest face index.  depth = that z or 0.0f, face = that f or 0xFFFFFFFF.
//
// Seen.  Face f is seen by a camera when it is drawn (and not culled) and (a) it owns at least min_pixels pixels of the camera's
// face map, or (b) each of its three corners passes the points' test: nearest_pixel of (u, w) is inside the image, the map depth z
// there is > 0 and render_seen(d_i, z, rel_tolerance) holds.
#pragma once

#include "apd_render_math.h"

namespace apd_fusion {

constexpr int kRenderCullNone = 0, kRenderCullBack = 1;
constexpr float kMeshRenderGuard = 134217728.0f;  // 2^27 units of 1/256 pixel

// A projected vertex: 16 bytes, one load
struct RenderVertex {
    int X, Y;
    float d;
    int usable;
};

// floorf(s) as a fixed-point coordinate within the guard band
APD_HD bool mesh_render_fixed(float s, int &out)
{
    const float f = floorf(s);
    if (!(f >= -kMeshRenderGuard && f <= kMeshRenderGuard)) {  // NaN and the infinities fail both
        out = 0;
        return false;
    }
    out = (int)f;
    return true;
}

APD_HD RenderVertex mesh_render_vertex(const View &view, const float P[3])
{
    float u, w, d;
    drop(view, P, u, w, d);
    RenderVertex v;
    const float su = u * 256.0f + 0.5f;
    const float sw = w * 256.0f + 0.5f;
    const bool deep = d > 0.0f && f32_bits(d) < 0x7f800000u;
    const bool hx = mesh_render_fixed(su, v.X);
    const bool hy = mesh_render_fixed(sw, v.Y);
    v.d = d;
    v.usable = deep && hx && hy ? 1 : 0;
    return v;
}

// A drawn face after the exchange: A2 > 0.  [c0, c1] x [r0, r1]: the pixels of its bounding box inside the image, empty when
// c0 > c1 or r0 > r1
struct RenderFace {
    int X[3], Y[3];
    float d[3];
    int c0, c1, r0, r1;
};

APD_HD int render_min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
APD_HD int render_max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// floor(x / 256) and ceil(x / 256) of |x| <= 2^27, without a shift of a negative number
APD_HD int render_floor256(int x) { return x >= 0 ? x / 256 : -((255 - x) / 256); }
APD_HD int render_ceil256(int x) { return x >= 0 ? (x + 255) / 256 : -((-x) / 256); }

// Whether the face with corners v0, v1, v2 is drawn into an image of cols x rows pixels under `cull`, and then the face
APD_HD bool mesh_render_face(const RenderVertex &v0, const RenderVertex &v1, const RenderVertex &v2, int cull, int cols, int rows, RenderFace &f)
{
    if (!(v0.usable && v1.usable && v2.usable)) {
        return false;
    }
    const int64_t A2 = (int64_t)(v1.X - v0.X) * (int64_t)(v2.Y - v0.Y) - (int64_t)(v1.Y - v0.Y) * (int64_t)(v2.X - v0.X);
    if (A2 == 0 || (cull == kRenderCullBack && A2 > 0)) {
        return false;
    }
    const RenderVertex &a = A2 < 0 ? v2 : v1, &b = A2 < 0 ? v1 : v2;
    f.X[0] = v0.X, f.Y[0] = v0.Y, f.d[0] = v0.d;
    f.X[1] = a.X, f.Y[1] = a.Y, f.d[1] = a.d;
    f.X[2] = b.X, f.Y[2] = b.Y, f.d[2] = b.d;
    const int c0 = render_ceil256(render_min3(f.X[0], f.X[1], f.X[2])), c1 = render_floor256(render_max3(f.X[0], f.X[1], f.X[2]));
    const int r0 = render_ceil256(render_min3(f.Y[0], f.Y[1], f.Y[2])), r1 = render_floor256(render_max3(f.Y[0], f.Y[1], f.Y[2]));
    f.c0 = c0 > 0 ? c0 : 0;
    f.c1 = c1 < cols - 1 ? c1 : cols - 1;
    f.r0 = r0 > 0 ? r0 : 0;
    f.r1 = r1 < rows - 1 ? r1 : rows - 1;
    return true;
}

// The pixels of the clipped box: 0 for an empty one
APD_HD int64_t mesh_render_box_pixels(const RenderFace &f)
{
    return f.c0 > f.c1 || f.r0 > f.r1 ? 0 : (int64_t)(f.c1 - f.c0 + 1) * (int64_t)(f.r1 - f.r0 + 1);
}

// E of edge a -> b at the fixed-point position (px, py)
APD_HD int64_t mesh_render_edge(const RenderFace &f, int a, int b, int px, int py)
{
    const int64_t dx = f.X[b] - f.X[a], dy = f.Y[b] - f.Y[a];
    return dx * (int64_t)(py - f.Y[a]) - dy * (int64_t)(px - f.X[a]);
}

// The top-left rule for edge a -> b with the edge function E
APD_HD bool mesh_render_inside(const RenderFace &f, int a, int b, int64_t E)
{
    const int dx = f.X[b] - f.X[a], dy = f.Y[b] - f.Y[a];
    return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// Whether the centre of pixel (c, r) of the face's box is covered and the face has a depth there; then z
APD_HD bool mesh_render_pixel(const RenderFace &f, int c, int r, float &z)
{
    const int px = 256 * c, py = 256 * r;
    const int64_t w2 = mesh_render_edge(f, 0, 1, px, py), w0 = mesh_render_edge(f, 1, 2, px, py), w1 = mesh_render_edge(f, 2, 0, px, py);
    if (!(mesh_render_inside(f, 0, 1, w2) && mesh_render_inside(f, 1, 2, w0) && mesh_render_inside(f, 2, 0, w1))) {
        return false;
    }
    const int64_t S = w0 + w1 + w2;
    const double q0 = (double)w0 / (double)f.d[0];
    const double q1 = (double)w1 / (double)f.d[1];
    const double q2 = (double)w2 / (double)f.d[2];
    const double q = (q0 + q1) + q2;
    z = (float)((double)S / q);
    return z > 0.0f && f32_bits(z) < 0x7f800000u;
}

// Rule (b) for one corner at world position P: `depth_at(c, r)` is the map depth of an inside pixel
template <typename DepthAt> APD_HD bool mesh_render_corner_seen(const View &view, const float P[3], float rel_tolerance, DepthAt &&depth_at)
{
    float u, w, d;
    drop(view, P, u, w, d);
    int c, r;
    if (!nearest_pixel(u, c) || !nearest_pixel(w, r) || c < 0 || c >= view.cols || r < 0 || r >= view.rows) {
        return false;
    }
    const float z = depth_at(c, r);
    return z > 0.0f && render_seen(d, z, rel_tolerance);
}

}  // namespace apd_fusion
