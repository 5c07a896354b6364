// volume_ref.cpp -- the truncated signed distance volume and the marching-tetrahedra mesh taken from it, as a sequential
// restatement of arithmetic contract C21: for the integration a loop over the samples in linear order and over the
// views in the call's order; for the extraction a loop over (sample, direction) that numbers the vertices as it meets them into a
// plain table of seven ids per sample, then a loop over the cells and their six tetrahedra that looks the ids up.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_volume_integrate and apd_volume_extract_mesh (apd-mvs_amd/csrc/apd_volume.hip),
// compiled by tests/volume_checker.py with -ffp-contract=off.  It shares the contract's header with the product (the update, the
// codes, the vertex, the table of cases) and nothing else: no scan, no ranks in masks, no threads.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_volume_math.h"

namespace {

apd_fusion::VolumeGrid grid_of(const int *dims, const float *origin, float voxel, float trunc, float max_weight)
{
    apd_fusion::VolumeGrid g;
    g.nx = dims[0];
    g.ny = dims[1];
    g.nz = dims[2];
    memcpy(g.origin, origin, sizeof(g.origin));
    g.voxel = voxel;
    g.trunc = trunc;
    g.max_weight = max_weight;
    return g;
}

}  // namespace

extern "C" {

// cameras: K (9), R (9), t (3) per view; sizes: width, height per view; images and weights may be null; C: 4 floats per sample or null
void volume_integrate(const int *dims, const float *origin, float voxel, float trunc, float max_weight, int num_views, const float *cameras,
                      const int *sizes, const float *const *depths, const float *const *images, int channels, const float *weights, float *D,
                      float *W, float *C)
{
    const apd_fusion::VolumeGrid g = grid_of(dims, origin, voxel, trunc, max_weight);
    std::vector<apd_fusion::VolumeView> views((size_t)num_views);
    for (int s = 0; s < num_views; ++s) {
        apd_fusion::VolumeView &v = views[(size_t)s];
        memset(&v, 0, sizeof(v));
        memcpy(v.geo.K, cameras + 21 * s, sizeof(v.geo.K));
        memcpy(v.geo.R, cameras + 21 * s + 9, sizeof(v.geo.R));
        memcpy(v.geo.t, cameras + 21 * s + 18, sizeof(v.geo.t));
        v.geo.cols = sizes[2 * s];
        v.geo.rows = sizes[2 * s + 1];
        v.depth = depths[s];
        v.image = images ? images[s] : nullptr;
        v.channels = channels;
        v.weight = weights ? weights[s] : 1.0f;
    }
    for (int k = 0; k < g.nz; ++k) {
        for (int j = 0; j < g.ny; ++j) {
            for (int i = 0; i < g.nx; ++i) {
                const size_t at = apd_fusion::volume_index(g, i, j, k);
                float P[3], none[4] = {0, 0, 0, 0};
                apd_fusion::volume_position(g, i, j, k, P);
                for (int s = 0; s < num_views; ++s) {
                    apd_fusion::volume_integrate(views[(size_t)s], P, g.trunc, g.max_weight, D[at], W[at], C != nullptr, C ? C + 4 * at : none);
                }
            }
        }
    }
}

// The mesh of the field D, W (and C: 4 floats per sample, or null).  *vertices and *faces are always set; xyz (3 per vertex), bgr
// (3 per vertex, written only with C) and faces (3 per face) are written where they are not null.
void volume_extract(const int *dims, const float *origin, float voxel, const float *D, const float *W, const float *C, long long *vertices,
                    long long *faces, float *xyz, uint8_t *bgr, int32_t *index)
{
    const apd_fusion::VolumeGrid g = grid_of(dims, origin, voxel, 1.0f, 1.0f);
    const size_t n = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    std::vector<uint32_t> code(n);
    std::vector<int32_t> id(7 * n, -1);
    long long nv = 0;
    for (int k = 0; k < g.nz; ++k) {
        for (int j = 0; j < g.ny; ++j) {
            for (int i = 0; i < g.nx; ++i) {
                const size_t at = apd_fusion::volume_index(g, i, j, k);
                code[at] = apd_fusion::volume_code(g, D, W, i, j, k);
                for (int dir = 0; dir < 7; ++dir) {
                    if (!((code[at] >> dir) & 1u)) {
                        continue;
                    }
                    float P[3];
                    uint8_t col[3] = {0, 0, 0};
                    apd_fusion::volume_vertex(g, D, C, i, j, k, dir, P, col);
                    if (xyz) {
                        memcpy(xyz + 3 * nv, P, sizeof(P));
                    }
                    if (bgr && C) {
                        memcpy(bgr + 3 * nv, col, sizeof(col));
                    }
                    id[7 * at + (size_t)dir] = (int32_t)nv++;
                }
            }
        }
    }
    long long nf = 0;
    for (int k = 0; k + 1 < g.nz; ++k) {
        for (int j = 0; j + 1 < g.ny; ++j) {
            for (int i = 0; i + 1 < g.nx; ++i) {
                for (int q = 0; q < 6; ++q) {
                    size_t corner[4];
                    int mask = 0;
                    bool known = true;
                    for (int c = 0; c < 4; ++c) {
                        const int b = apd_fusion::volume_tet_corner(q, c);
                        corner[c] = apd_fusion::volume_index(g, i + (b & 1), j + ((b >> 1) & 1), k + (b >> 2));
                        known = known && (code[corner[c]] & apd_fusion::kVolumeKnown);
                        mask |= ((code[corner[c]] & apd_fusion::kVolumeInside) ? 1 : 0) << c;
                    }
                    if (!known || mask == 0 || mask == 15) {
                        continue;
                    }
                    const apd_fusion::VolumeCase &vc = apd_fusion::volume_case(q, mask);
                    for (int e = 0; e < 3 * (int)vc.count; ++e) {
                        const int lo = vc.edge[e] >> 2, up = vc.edge[e] & 3;
                        const int dir = apd_fusion::volume_bits_dir(apd_fusion::volume_tet_corner(q, lo) ^ apd_fusion::volume_tet_corner(q, up));
                        if (index) {
                            index[3 * nf + e] = id[7 * corner[lo] + (size_t)dir];
                        }
                    }
                    nf += vc.count;
                }
            }
        }
    }
    *vertices = nv;
    *faces = nf;
}

// The table itself, for the tests that restate the rule: count and six edges per (q, mask), 7 bytes each
void volume_cases(uint8_t *out)
{
    for (int q = 0; q < 6; ++q) {
        for (int m = 0; m < 16; ++m) {
            const apd_fusion::VolumeCase &vc = apd_fusion::volume_case(q, m);
            *out++ = vc.count;
            memcpy(out, vc.edge, 6);
            out += 6;
        }
    }
}

}  // extern "C"
