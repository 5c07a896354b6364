// mesh_render_ref.cpp -- the z-buffered rasterisation of a mesh into a camera, the face visibility that follows from it and the
// removal of unseen faces, as a sequential restatement of arithmetic contract C25: a loop over the faces in index order
// and over the pixels of each clipped bounding box that keeps the smaller key in a plain array, then the resolve; for the visibility
// a loop over the cameras, then over the pixels and the faces.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_mesh_render, apd_mesh_face_visibility and apd_mesh_remove_unseen
// (apd-mvs_amd/csrc/apd_mesh_render.hip), compiled by tests/mesh_render_checker.py with -ffp-contract=off.  It shares the contract's
// header with the product and nothing else: no threads, no atomics, no split by size, no tiles.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_mesh_render_math.h"

namespace {

using apd_fusion::RenderFace;
using apd_fusion::RenderVertex;
using apd_fusion::View;

// camera: K (9), R (9), t (3); the centre is not read by the projection
View view_of(const float *camera, int width, int height)
{
    View v;
    memset(&v, 0, sizeof(v));
    memcpy(v.K, camera, sizeof(v.K));
    memcpy(v.R, camera + 9, sizeof(v.R));
    memcpy(v.t, camera + 18, sizeof(v.t));
    v.rows = height;
    v.cols = width;
    return v;
}

struct Drawn {
    std::vector<RenderVertex> verts;
    std::vector<uint64_t> keys;
};

bool face_of(const Drawn &d, const int32_t *index, long long f, int cull, const View &view, RenderFace &face)
{
    return apd_fusion::mesh_render_face(d.verts[index[3 * f]], d.verts[index[3 * f + 1]], d.verts[index[3 * f + 2]], cull, view.cols, view.rows, face);
}

Drawn draw(long long nv, const float *xyz, long long nf, const int32_t *index, const View &view, int cull)
{
    Drawn d;
    d.verts.resize((size_t)nv);
    for (long long v = 0; v < nv; ++v) {
        d.verts[v] = apd_fusion::mesh_render_vertex(view, xyz + 3 * v);
    }
    d.keys.assign((size_t)view.rows * (size_t)view.cols, apd_fusion::kRenderEmptyKey);
    for (long long f = 0; f < nf; ++f) {
        RenderFace face;
        if (!face_of(d, index, f, cull, view, face)) {
            continue;
        }
        for (int r = face.r0; r <= face.r1; ++r) {
            for (int c = face.c0; c <= face.c1; ++c) {
                float z;
                if (!apd_fusion::mesh_render_pixel(face, c, r, z)) {
                    continue;
                }
                const uint64_t key = apd_fusion::render_key(z, (uint32_t)f);
                uint64_t &held = d.keys[(size_t)r * (size_t)view.cols + (size_t)c];
                if (key < held) {
                    held = key;
                }
            }
        }
    }
    return d;
}

}  // namespace

extern "C" {

// depth and face: width * height entries each
void mesh_render(long long nv, const float *xyz, long long nf, const int32_t *index, const float *camera, int width, int height, int cull, float *depth,
                 uint32_t *face)
{
    const Drawn d = draw(nv, xyz, nf, index, view_of(camera, width, height), cull);
    for (size_t i = 0; i < d.keys.size(); ++i) {
        depth[i] = apd_fusion::render_depth(d.keys[i]);
        face[i] = apd_fusion::render_index(d.keys[i]);
    }
}

// What the projection makes of every vertex: X, Y, the bits of d, usable: 4 ints a vertex (for the numpy restatement)
void mesh_render_vertices(long long nv, const float *xyz, const float *camera, int width, int height, int32_t *out)
{
    const View view = view_of(camera, width, height);
    for (long long v = 0; v < nv; ++v) {
        const RenderVertex p = apd_fusion::mesh_render_vertex(view, xyz + 3 * v);
        out[4 * v] = p.X;
        out[4 * v + 1] = p.Y;
        memcpy(out + 4 * v + 2, &p.d, 4);
        out[4 * v + 3] = p.usable;
    }
}

// cameras: 21 floats each; sizes: width, height each.  views, pixels: nf entries.  Returns the faces no camera sees
long long mesh_face_visibility(long long nv, const float *xyz, long long nf, const int32_t *index, int num_views, const float *cameras, const int *sizes,
                               int cull, unsigned min_pixels, float rel_tolerance, uint32_t *views, uint64_t *pixels)
{
    for (long long f = 0; f < nf; ++f) {
        views[f] = 0;
        pixels[f] = 0;
    }
    for (int s = 0; s < num_views; ++s) {
        const View view = view_of(cameras + 21 * s, sizes[2 * s], sizes[2 * s + 1]);
        const Drawn d = draw(nv, xyz, nf, index, view, cull);
        std::vector<uint64_t> owned((size_t)nf, 0);
        for (const uint64_t key : d.keys) {
            if (key != apd_fusion::kRenderEmptyKey) {
                ++owned[apd_fusion::render_index(key)];
            }
        }
        for (long long f = 0; f < nf; ++f) {
            RenderFace face;
            if (!face_of(d, index, f, cull, view, face)) {
                continue;
            }
            bool seen = owned[f] >= min_pixels;
            if (!seen) {
                seen = true;
                for (int c = 0; c < 3; ++c) {
                    seen = apd_fusion::mesh_render_corner_seen(view, xyz + 3 * (long long)index[3 * f + c], rel_tolerance, [&](int x, int y) {
                               return apd_fusion::render_depth(d.keys[(size_t)y * (size_t)view.cols + (size_t)x]);
                           }) && seen;
                }
            }
            views[f] += seen ? 1u : 0u;
            pixels[f] += owned[f];
        }
    }
    long long unseen = 0;
    for (long long f = 0; f < nf; ++f) {
        unseen += views[f] == 0 ? 1 : 0;
    }
    return unseen;
}

}  // extern "C"
