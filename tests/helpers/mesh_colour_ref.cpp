// mesh_colour_ref.cpp -- the colouring of a mesh's vertices from the images of the cameras that see them, as a sequential restatement
// of arithmetic contract C26: the normals by contract C22 in a loop over the corners in ascending order, per view the
// depth map of contract C25 in a loop over the faces and the pixels of each clipped bounding box, then a loop over the vertices
// that adds to plain arrays of sums, and one more that divides.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_mesh_colour_from_views (apd-mvs_amd/csrc/apd_mesh_colour.hip), compiled by
// tests/mesh_colour_checker.py with -ffp-contract=off.  It shares the contracts' headers with the product and nothing else: no
// threads, no atomics, no split by size, no tiles, no sort.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_mesh_colour_math.h"
#include "../../apd-mvs_amd/csrc/apd_mesh_math.h"
#include "../../apd-mvs_amd/csrc/apd_mesh_render_math.h"

namespace {

using apd_fusion::RenderFace;
using apd_fusion::RenderVertex;
using apd_fusion::View;

// camera: K (9), R (9), t (3)
View view_of(const float *camera, int width, int height)
{
    View v;
    memset(&v, 0, sizeof(v));
    memcpy(v.K, camera, sizeof(v.K));
    memcpy(v.R, camera + 9, sizeof(v.R));
    memcpy(v.t, camera + 18, sizeof(v.t));
    apd_fusion::colour_view_centre(v.R, v.t, v.centre);
    v.rows = height;
    v.cols = width;
    return v;
}

// The C25 depth map with both sides drawn
std::vector<float> depth_map(long long nv, const float *xyz, long long nf, const int32_t *index, const View &view)
{
    std::vector<RenderVertex> verts((size_t)nv);
    for (long long v = 0; v < nv; ++v) {
        verts[v] = apd_fusion::mesh_render_vertex(view, xyz + 3 * v);
    }
    std::vector<uint64_t> keys((size_t)view.rows * (size_t)view.cols, apd_fusion::kRenderEmptyKey);
    for (long long f = 0; f < nf; ++f) {
        RenderFace face;
        if (!apd_fusion::mesh_render_face(verts[index[3 * f]], verts[index[3 * f + 1]], verts[index[3 * f + 2]], apd_fusion::kRenderCullNone, view.cols,
                                          view.rows, face)) {
            continue;
        }
        for (int r = face.r0; r <= face.r1; ++r) {
            for (int c = face.c0; c <= face.c1; ++c) {
                float z;
                if (!apd_fusion::mesh_render_pixel(face, c, r, z)) {
                    continue;
                }
                const uint64_t key = apd_fusion::render_key(z, (uint32_t)f);
                uint64_t &held = keys[(size_t)r * (size_t)view.cols + (size_t)c];
                if (key < held) {
                    held = key;
                }
            }
        }
    }
    std::vector<float> depth(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
        depth[i] = apd_fusion::render_depth(keys[i]);
    }
    return depth;
}

}  // namespace

extern "C" {

// normal: 3 floats a vertex or null (then contract C22's); bgr: 3 bytes a vertex or null; cameras: 21 floats each; sizes: width, height
// each; images: per view height x width x channels floats.  out_bgr: 3 bytes a vertex, views: one entry a vertex.  Returns the
// vertices without a sample
long long mesh_colour_from_views(long long nv, const float *xyz, const float *normal, const uint8_t *bgr, long long nf, const int32_t *index, int num_views,
                                 const float *cameras, const int *sizes, const float *const *images, int channels, float rel_tolerance, float min_cos,
                                 uint8_t *out_bgr, uint32_t *views)
{
    std::vector<float> own;
    if (!normal) {
        std::vector<double> s(3 * (size_t)nv, 0.0);
        for (long long k = 0; k < 3 * nf; ++k) {  // ascending 3 f + c
            const long long f = k / 3;
            double g[3];
            apd_fusion::mesh_face_normal(xyz + 3 * (long long)index[3 * f], xyz + 3 * (long long)index[3 * f + 1], xyz + 3 * (long long)index[3 * f + 2], g);
            apd_fusion::mesh_add(s.data() + 3 * (long long)index[k], g);
        }
        own.resize(3 * (size_t)nv);
        for (long long v = 0; v < nv; ++v) {
            apd_fusion::mesh_vertex_normal(s.data() + 3 * v, own.data() + 3 * v);
        }
        normal = own.data();
    }
    std::vector<double> S(4 * (size_t)nv, 0.0);
    for (long long v = 0; v < nv; ++v) {
        views[v] = 0;
    }
    for (int s = 0; s < num_views && nf > 0; ++s) {
        const View view = view_of(cameras + 21 * s, sizes[2 * s], sizes[2 * s + 1]);
        const std::vector<float> depth = depth_map(nv, xyz, nf, index, view);
        const float *image = images[s];
        const size_t cols = (size_t)view.cols;
        for (long long v = 0; v < nv; ++v) {
            apd_fusion::ColourSample at;
            if (!apd_fusion::colour_sample(view, xyz + 3 * v, normal + 3 * v, rel_tolerance, min_cos,
                                           [&](int c, int r) { return depth[(size_t)r * cols + (size_t)c]; }, at)) {
                continue;
            }
            for (int k = 0; k < 3; ++k) {
                const int ch = channels == 3 ? k : 0;
                const float *top = image + ((size_t)at.r0 * cols + (size_t)at.c0) * channels + ch;
                const float *bot = top + cols * channels;
                const float value = apd_fusion::colour_bilinear(top[0], top[channels], bot[0], bot[channels], at.fu, at.fw);
                S[4 * v + k] = apd_fusion::colour_add(S[4 * v + k], at.c, value);
            }
            S[4 * v + 3] = S[4 * v + 3] + at.c;
            views[v] += 1;
        }
    }
    long long uncoloured = 0;
    for (long long v = 0; v < nv; ++v) {
        for (int k = 0; k < 3; ++k) {
            out_bgr[3 * v + k] = views[v] > 0 ? apd_fusion::colour_byte(S[4 * v + k], S[4 * v + 3]) : bgr ? bgr[3 * v + k] : (uint8_t)0;
        }
        uncoloured += views[v] == 0 ? 1 : 0;
    }
    return uncoloured;
}

// u, w, d of the projection and the cosine of rule 5 for every vertex in one camera: 4 doubles a vertex, for the tests that plant a
// vertex at a known place
void mesh_colour_geometry(long long nv, const float *xyz, const float *normal, const float *camera, int width, int height, double *out)
{
    const View view = view_of(camera, width, height);
    for (long long v = 0; v < nv; ++v) {
        float u, w, d;
        apd_fusion::drop(view, xyz + 3 * v, u, w, d);
        double c = 0.0;
        apd_fusion::colour_facing(view, xyz + 3 * v, normal + 3 * v, 0.0f, c);
        out[4 * v] = u;
        out[4 * v + 1] = w;
        out[4 * v + 2] = d;
        out[4 * v + 3] = c;
    }
}

}  // extern "C"
