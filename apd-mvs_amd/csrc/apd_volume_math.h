// apd_volume_math.h -- the per-sample arithmetic of the truncated signed distance volume and of the marching-tetrahedra mesh taken
// from it (arithmetic contract C21): the relation under apd_volume_integrate and apd_volume_extract_mesh, written once
// and compiled twice: by hipcc into the kernels (apd_volume.hip) and by g++ into the sequential checker
// (tests/helpers/volume_ref.cpp), both with -ffp-contract=off and no fast-math.  The projection, the rounding to a pixel and the
// draw rule are the fusion's and the rendering's (drop, nearest_pixel: apd_fusion_math.h; render_draw: apd_render_math.h), so a
// sample reads the pixel the fusion would have voted in.  Every operation is a binary32 IEEE operation in the order written.
#pragma once

#include "apd_render_math.h"

namespace apd_fusion {

// nx, ny, nz samples (each >= 2, product < 2^31); sample (i, j, k) has the linear index i + nx * (j + ny * k)
struct VolumeGrid {
    int nx, ny, nz;
    float origin[3];
    float voxel, trunc, max_weight;
};

// One view of an integrate call: the geometry at the size of its maps, the depth map, the image (may be null) with 1 or 3
// interleaved float channels (blue, green, red, as the fusion's images), and the weight of the view
struct VolumeView {
    View geo;
    const float *depth;
    const float *image;
    int channels;
    float weight;
};

// What extraction keeps per sample: bits 0 .. 6 the edges that carry a vertex, by direction; then known and inside
constexpr uint32_t kVolumeKnown = 1u << 7;
constexpr uint32_t kVolumeInside = 1u << 8;

APD_HD size_t volume_index(const VolumeGrid &g, int i, int j, int k) { return (size_t)i + (size_t)g.nx * ((size_t)j + (size_t)g.ny * (size_t)k); }

// origin + (float)index * voxel: one multiply, one add
APD_HD float volume_coord(float origin, int index, float voxel)
{
    const float s = (float)index * voxel;
    return origin + s;
}

APD_HD void volume_position(const VolumeGrid &g, int i, int j, int k, float P[3])
{
    P[0] = volume_coord(g.origin[0], i, g.voxel);
    P[1] = volume_coord(g.origin[1], j, g.voxel);
    P[2] = volume_coord(g.origin[2], k, g.voxel);
}

// W + w, saturated
APD_HD float volume_weight(float W, float w, float max_weight)
{
    const float s = W + w;
    return s > max_weight ? max_weight : s;
}

// (X * W + x * w) / (W + w)
APD_HD float volume_mean(float X, float W, float x, float w)
{
    const float a = X * W;
    const float b = x * w;
    const float s = W + w;
    return (a + b) / s;
}

// One view applied to the sample at P.  D, W: the sample's distance and weight; C: its blue, green, red and colour weight, read and
// written only in a volume with colour.  The sample is observed when it is drawn into the view (render_draw: depth d > 0 and finite, both
// pixel conversions defined, the pixel inside the map), the map holds z > 0 and finite there, and sdf = z - d >= -trunc.
APD_HD void volume_integrate(const VolumeView &v, const float P[3], float trunc, float max_weight, float &D, float &W, bool colour, float C[4])
{
    int c, r;
    float d;
    if (!render_draw(v.geo, P, c, r, d)) {
        return;
    }
    const size_t px = (size_t)r * (size_t)v.geo.cols + (size_t)c;
    const float z = v.depth[px];
    if (!(z > 0.0f) || f32_bits(z) >= 0x7f800000u) {
        return;
    }
    const float sdf = z - d;
    if (!(sdf >= -trunc)) {
        return;
    }
    float val = sdf / trunc;
    if (val > 1.0f) {
        val = 1.0f;
    }
    D = volume_mean(D, W, val, v.weight);
    W = volume_weight(W, v.weight, max_weight);
    if (colour && v.image && sdf <= trunc) {
        for (int ch = 0; ch < 3; ++ch) {
            const float col = v.image[px * (size_t)v.channels + (size_t)(v.channels == 3 ? ch : 0)];
            C[ch] = volume_mean(C[ch], C[3], col, v.weight);
        }
        C[3] = volume_weight(C[3], v.weight, max_weight);
    }
}

// The seven edge directions from a sample, numbered 0 .. 6: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), as three bits
// (bit 0: x, bit 1: y, bit 2: z), and back
APD_HD constexpr int volume_dir_bits(int dir) { return (int)((0x7653421u >> (4 * dir)) & 7u); }
APD_HD constexpr int volume_bits_dir(int bits) { return (int)((0x65423100u >> (4 * bits)) & 7u); }

APD_HD bool volume_known(float W) { return W > 0.0f; }
APD_HD bool volume_inside(float D, float W) { return W > 0.0f && D < 0.0f; }  // zero and -0 are outside

// The code of sample (i, j, k): known, inside, and per direction whether the edge to the upper end, where that exists in the grid,
// carries a vertex: both ends known and exactly one inside
APD_HD uint32_t volume_code(const VolumeGrid &g, const float *D, const float *W, int i, int j, int k)
{
    const size_t at = volume_index(g, i, j, k);
    const float fa = D[at], wa = W[at];
    if (!volume_known(wa)) {
        return 0;
    }
    const bool in_a = volume_inside(fa, wa);
    uint32_t code = kVolumeKnown | (in_a ? kVolumeInside : 0u);
    for (int dir = 0; dir < 7; ++dir) {
        const int b = volume_dir_bits(dir);
        const int iu = i + (b & 1), ju = j + ((b >> 1) & 1), ku = k + (b >> 2);
        if (iu >= g.nx || ju >= g.ny || ku >= g.nz) {
            continue;
        }
        const size_t up = volume_index(g, iu, ju, ku);
        const float wb = W[up];
        if (volume_known(wb) && volume_inside(D[up], wb) != in_a) {
            code |= 1u << dir;
        }
    }
    return code;
}

APD_HD int volume_popcount(uint32_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(m);
#else
    return __builtin_popcount(m);
#endif
}

// The vertices a code carries, and the rank of direction dir among them: the id of (sample, dir) is the sample's offset -- the
// exclusive scan of the counts in linear order -- plus that rank
APD_HD int volume_carried(uint32_t code) { return volume_popcount(code & 0x7fu); }
APD_HD int volume_rank(uint32_t code, int dir) { return volume_popcount(code & ((1u << dir) - 1u)); }

// One colour channel of a vertex at t between ends with values ca, cb and colour weights wa, wb, as a byte
APD_HD uint8_t volume_colour(float ca, float wa, float cb, float wb, float t)
{
    float x = 0.0f;
    if (wa > 0.0f && wb > 0.0f) {
        const float e = cb - ca;
        const float m = t * e;
        x = ca + m;
    } else if (wa > 0.0f) {
        x = ca;
    } else if (wb > 0.0f) {
        x = cb;
    }
    x = !(x > 0.0f) ? 0.0f : (x > 255.0f ? 255.0f : x);  // a NaN is 0
    return (uint8_t)(int)(x + 0.5f);
}

// The vertex of the edge from sample (i, j, k) in direction dir, which carries one: t = fa / (fa - fb) with fa at the lower end,
// and per component pa + t * (pb - pa).  C: 4 floats per sample (blue, green, red, colour weight) or null; bgr is then not written.
APD_HD void volume_vertex(const VolumeGrid &g, const float *D, const float *C, int i, int j, int k, int dir, float xyz[3], uint8_t bgr[3])
{
    const int b = volume_dir_bits(dir);
    const int iu = i + (b & 1), ju = j + ((b >> 1) & 1), ku = k + (b >> 2);
    const size_t lo = volume_index(g, i, j, k), up = volume_index(g, iu, ju, ku);
    const float fa = D[lo], fb = D[up];
    const float t = fa / (fa - fb);
    float Pa[3], Pb[3];
    volume_position(g, i, j, k, Pa);
    volume_position(g, iu, ju, ku, Pb);
    for (int a = 0; a < 3; ++a) {
        const float e = Pb[a] - Pa[a];
        const float m = t * e;
        xyz[a] = Pa[a] + m;
    }
    if (C) {
        for (int ch = 0; ch < 3; ++ch) {
            bgr[ch] = volume_colour(C[4 * lo + ch], C[4 * lo + 3], C[4 * up + ch], C[4 * up + 3], t);
        }
    }
}

// Corner c = 0 .. 3 of tetrahedron q = 0 .. 5 of a cell, as three bits: the Kuhn split along the axis permutations xyz, xzy, yxz,
// yzx, zxy, zyx -- v0 = (0,0,0), v1 = v0 + e_p1, v2 = v1 + e_p2, v3 = (1,1,1).  Corner bits only grow along a tetrahedron, so
// each of its edges runs in one of the seven directions from its lower corner: volume_bits_dir(upper ^ lower).
APD_HD constexpr int volume_tet_corner(int q, int c)
{
    const int p1 = q >> 1;
    const int p2 = (q & 1) ? (p1 == 2 ? 1 : 2) : (p1 == 0 ? 1 : 0);
    return c == 0 ? 0 : (c == 1 ? (1 << p1) : (c == 2 ? ((1 << p1) | (1 << p2)) : 7));
}

// The faces of a tetrahedron whose corners are all known, by mask (bit c: corner c is inside): at most two triangles, each three
// edges, an edge as (lower corner << 2) | upper corner, in the order that faces outward.
struct VolumeCase {
    uint8_t count;
    uint8_t edge[6];
};
struct VolumeCases {
    VolumeCase c[6][16];
    bool decided;  // every orientation product was non-zero
};

// The rule.  One corner a apart from b < c < d: (ab, ac, ad).  Two inside a < b and two outside c < d: (ac, ad, bd) and
// (ac, bd, bc).  A triangle is turned -- (first, third, second) -- unless, with its vertices at the edge midpoints of the unit cell,
// its right-hand normal has a positive product with (sum of outside corners * number of inside corners - sum of inside corners *
// number of outside corners).  Exact in integers: midpoints are taken twice.
constexpr VolumeCases make_volume_cases()
{
    VolumeCases t{};
    t.decided = true;
    for (int q = 0; q < 6; ++q) {
        for (int m = 1; m < 15; ++m) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int c = 0; c < 4; ++c) {
                if ((m >> c) & 1) {
                    in[ni++] = c;
                } else {
                    out[no++] = c;
                }
            }
            int tri[2][3][2] = {};
            int nt = 0;
            if (ni == 1 || no == 1) {
                const int a = ni == 1 ? in[0] : out[0];
                for (int e = 0; e < 3; ++e) {
                    tri[0][e][0] = a;
                    tri[0][e][1] = ni == 1 ? out[e] : in[e];
                }
                nt = 1;
            } else {
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                const int two[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
                for (int k = 0; k < 2; ++k) {
                    for (int e = 0; e < 3; ++e) {
                        tri[k][e][0] = two[k][e][0];
                        tri[k][e][1] = two[k][e][1];
                    }
                }
                nt = 2;
            }
            int g[3] = {0, 0, 0};
            for (int axis = 0; axis < 3; ++axis) {
                int sum_in = 0, sum_out = 0;
                for (int c = 0; c < ni; ++c) {
                    sum_in += (volume_tet_corner(q, in[c]) >> axis) & 1;
                }
                for (int c = 0; c < no; ++c) {
                    sum_out += (volume_tet_corner(q, out[c]) >> axis) & 1;
                }
                g[axis] = sum_out * ni - sum_in * no;
            }
            t.c[q][m].count = (uint8_t)nt;
            for (int k = 0; k < nt; ++k) {
                int V[3][3] = {};
                for (int e = 0; e < 3; ++e) {
                    for (int axis = 0; axis < 3; ++axis) {
                        V[e][axis] = ((volume_tet_corner(q, tri[k][e][0]) >> axis) & 1) + ((volume_tet_corner(q, tri[k][e][1]) >> axis) & 1);
                    }
                }
                const int u[3] = {V[1][0] - V[0][0], V[1][1] - V[0][1], V[1][2] - V[0][2]};
                const int w[3] = {V[2][0] - V[0][0], V[2][1] - V[0][1], V[2][2] - V[0][2]};
                const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                const int dot = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
                if (dot == 0) {
                    t.decided = false;
                }
                const int order[3] = {0, dot > 0 ? 1 : 2, dot > 0 ? 2 : 1};
                for (int e = 0; e < 3; ++e) {
                    const int x = tri[k][order[e]][0], y = tri[k][order[e]][1];
                    t.c[q][m].edge[3 * k + e] = (uint8_t)(((x < y ? x : y) << 2) | (x < y ? y : x));
                }
            }
        }
    }
    return t;
}

static_assert(make_volume_cases().decided, "an orientation of the marching-tetrahedra table is undecided");

APD_HD const VolumeCase &volume_case(int q, int mask)
{
    static constexpr VolumeCases kCases = make_volume_cases();
    return kCases.c[q][mask];
}

// The mask of tetrahedron q of the cell whose corner codes are gathered in known8 / inside8 (bit b: the corner at offset bits b),
// or -1 when a corner is unknown: such a tetrahedron has no faces
APD_HD int volume_tet_mask(uint32_t known8, uint32_t inside8, int q)
{
    int m = 0;
    for (int c = 0; c < 4; ++c) {
        const int b = volume_tet_corner(q, c);
        if (!((known8 >> b) & 1u)) {
            return -1;
        }
        m |= (int)((inside8 >> b) & 1u) << c;
    }
    return m;
}

// The faces of a tetrahedron with that mask: 0 for a mask of -1, 0 or 15; 2 for two inside; 1 otherwise
APD_HD int volume_tet_faces(int mask)
{
    if (mask <= 0 || mask == 15) {
        return 0;
    }
    return volume_popcount((uint32_t)mask) == 2 ? 2 : 1;
}

// known8 and inside8 of the cell with lower sample (i, j, k), i < nx - 1 and so on, from the codes of its eight corners
template <typename Code> APD_HD void volume_cell_corners(const VolumeGrid &g, const Code *code, int i, int j, int k, uint32_t &known8, uint32_t &inside8)
{
    known8 = inside8 = 0;
    for (int b = 0; b < 8; ++b) {
        const uint32_t c = code[volume_index(g, i + (b & 1), j + ((b >> 1) & 1), k + (b >> 2))];
        known8 |= ((c & kVolumeKnown) ? 1u : 0u) << b;
        inside8 |= ((c & kVolumeInside) ? 1u : 0u) << b;
    }
}

APD_HD int volume_cell_faces(uint32_t known8, uint32_t inside8)
{
    int n = 0;
    for (int q = 0; q < 6; ++q) {
        n += volume_tet_faces(volume_tet_mask(known8, inside8, q));
    }
    return n;
}

// The faces of that cell, in the order of q and then of the table, as vertex ids, three per face, to `faces`; offset[s]: the id of
// the first vertex of sample s.  Returns their number.
template <typename Code, typename Offset>
APD_HD int volume_emit_faces(const VolumeGrid &g, const Code *code, const Offset *offset, int i, int j, int k, uint32_t known8, uint32_t inside8,
                             int32_t *faces)
{
    int n = 0;
    for (int q = 0; q < 6; ++q) {
        const int mask = volume_tet_mask(known8, inside8, q);
        if (volume_tet_faces(mask) == 0) {
            continue;
        }
        const VolumeCase &vc = volume_case(q, mask);
        for (int e = 0; e < 3 * (int)vc.count; ++e) {
            const int lo = volume_tet_corner(q, vc.edge[e] >> 2), up = volume_tet_corner(q, vc.edge[e] & 3);
            const size_t s = volume_index(g, i + (lo & 1), j + ((lo >> 1) & 1), k + (lo >> 2));
            faces[3 * n + e] = (int32_t)((long long)offset[s] + volume_rank((uint32_t)code[s], volume_bits_dir(lo ^ up)));
        }
        n += (int)vc.count;
    }
    return n;
}

}  // namespace apd_fusion
