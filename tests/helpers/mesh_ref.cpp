// mesh_ref.cpp -- welding, face components, removal of small components and vertex normals of an indexed triangle mesh, as a
// sequential restatement of contract C22:
//   weld:        the double loop over all pairs of vertices, the relation of apd_radius_math.h applied to each, a sequential
//                union-find (union by index, path compression) over the pairs it holds for; then the rule on faces and vertices;
//   components:  the same union-find over the vertex indices, the three of every face united, faces grouped by the root of their
//                first index;
//   normals:     one loop over the faces in order and over their corners in order, each adding the face's binary64 cross product
//                to its vertex's sum -- which is ascending 3 f + c for every vertex.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_mesh_weld, apd_mesh_components, apd_mesh_remove_small_components and
// apd_mesh_with_vertex_normals (apd-mvs_amd/csrc/apd_mesh.hip), compiled by tests/mesh_checker.py with -ffp-contract=off.  It
// shares the contract's headers with the product (the cell, the squared distance, the cross product, the normalisation) and nothing
// else: no sort, no scan, no kernel, no atomic.
#include <cstdint>
#include <map>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_mesh_math.h"

namespace {

long long find(std::vector<long long> &parent, long long v)
{
    long long r = v;
    while (parent[(size_t)r] != r) {
        r = parent[(size_t)r];
    }
    while (parent[(size_t)v] != r) {
        const long long next = parent[(size_t)v];
        parent[(size_t)v] = r;
        v = next;
    }
    return r;
}

void unite(std::vector<long long> &parent, long long i, long long j)
{
    const long long a = find(parent, i), b = find(parent, j);
    if (a != b) {
        parent[(size_t)(a > b ? a : b)] = a > b ? b : a;  // the root is the smallest index of its tree
    }
}

// The faces with keep[f], their indices taken from `index`, and the vertices they name, in order and renumbered
void compact(long long nv, const float *xyz, const uint8_t *bgr, const float *normal, long long nf, const std::vector<int32_t> &index,
             const std::vector<char> &keep, long long *out_nv, long long *out_nf, float *out_xyz, uint8_t *out_bgr, float *out_normal, int32_t *out_index)
{
    std::vector<char> used((size_t)nv, 0);
    for (long long f = 0; f < nf; ++f) {
        for (int c = 0; c < 3 && keep[(size_t)f]; ++c) {
            used[(size_t)index[(size_t)(3 * f + c)]] = 1;
        }
    }
    std::vector<int32_t> renumbered((size_t)nv, -1);
    long long kept = 0;
    for (long long v = 0; v < nv; ++v) {
        if (!used[(size_t)v]) {
            continue;
        }
        renumbered[(size_t)v] = (int32_t)kept;
        for (int a = 0; a < 3; ++a) {
            out_xyz[3 * kept + a] = xyz[3 * v + a];
            if (bgr) {
                out_bgr[3 * kept + a] = bgr[3 * v + a];
            }
            if (normal) {
                out_normal[3 * kept + a] = normal[3 * v + a];
            }
        }
        ++kept;
    }
    *out_nv = kept;
    kept = 0;
    for (long long f = 0; f < nf; ++f) {
        if (!keep[(size_t)f]) {
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            out_index[3 * kept + c] = renumbered[(size_t)index[(size_t)(3 * f + c)]];
        }
        ++kept;
    }
    *out_nf = kept;
}

// label[f], size[f]; returns the number of components
long long label_faces(long long nv, long long nf, const int32_t *index, uint32_t *label, uint32_t *size)
{
    std::vector<long long> parent((size_t)nv);
    for (long long v = 0; v < nv; ++v) {
        parent[(size_t)v] = v;
    }
    for (long long f = 0; f < nf; ++f) {
        unite(parent, index[3 * f], index[3 * f + 1]);
        unite(parent, index[3 * f], index[3 * f + 2]);
    }
    std::map<long long, std::pair<long long, long long>> seen;  // root -> (first face, faces)
    for (long long f = 0; f < nf; ++f) {
        const long long r = find(parent, index[3 * f]);
        auto at = seen.find(r);
        if (at == seen.end()) {
            seen[r] = {f, 1};
        } else {
            ++at->second.second;
        }
    }
    for (long long f = 0; f < nf; ++f) {
        const auto &g = seen[find(parent, index[3 * f])];
        label[f] = (uint32_t)g.first;
        size[f] = (uint32_t)g.second;
    }
    return (long long)seen.size();
}

}  // namespace

extern "C" {

// bgr and normal may be null (then out_bgr / out_normal are not written).  The out arrays have room for nv vertices and nf faces.
void mesh_weld(long long nv, const float *xyz, const uint8_t *bgr, const float *normal, long long nf, const int32_t *index, float tolerance,
               const float *origin, long long *out_nv, long long *out_nf, float *out_xyz, uint8_t *out_bgr, float *out_normal, int32_t *out_index)
{
    std::vector<char> inside((size_t)nv);
    std::vector<int> cell((size_t)(3 * nv));
    std::vector<long long> parent((size_t)nv);
    for (long long v = 0; v < nv; ++v) {
        inside[(size_t)v] = apd_fusion::radius_cells(xyz + 3 * v, origin, tolerance, cell.data() + 3 * v) ? 1 : 0;
        parent[(size_t)v] = v;
    }
    const float r2 = tolerance * tolerance;
    for (long long i = 0; i < nv; ++i) {
        for (long long j = 0; j < i && inside[(size_t)i]; ++j) {
            if (inside[(size_t)j] && apd_fusion::radius_neighbour(xyz + 3 * i, cell.data() + 3 * i, xyz + 3 * j, cell.data() + 3 * j, r2)) {
                unite(parent, i, j);
            }
        }
    }
    std::vector<int32_t> mapped((size_t)(3 * nf));
    std::vector<char> keep((size_t)nf);
    for (long long f = 0; f < nf; ++f) {
        for (int c = 0; c < 3; ++c) {
            mapped[(size_t)(3 * f + c)] = (int32_t)find(parent, index[3 * f + c]);
        }
        keep[(size_t)f] = apd_fusion::mesh_face_degenerate(mapped[(size_t)(3 * f)], mapped[(size_t)(3 * f + 1)], mapped[(size_t)(3 * f + 2)]) ? 0 : 1;
    }
    compact(nv, xyz, bgr, normal, nf, mapped, keep, out_nv, out_nf, out_xyz, out_bgr, out_normal, out_index);
}

long long mesh_components(long long nv, long long nf, const int32_t *index, uint32_t *label, uint32_t *size)
{
    return label_faces(nv, nf, index, label, size);
}

void mesh_remove_small(long long nv, const float *xyz, const uint8_t *bgr, const float *normal, long long nf, const int32_t *index, uint32_t min_faces,
                       long long *out_nv, long long *out_nf, float *out_xyz, uint8_t *out_bgr, float *out_normal, int32_t *out_index)
{
    std::vector<uint32_t> label((size_t)nf), size((size_t)nf);
    label_faces(nv, nf, index, label.data(), size.data());
    std::vector<char> keep((size_t)nf);
    for (long long f = 0; f < nf; ++f) {
        keep[(size_t)f] = size[(size_t)f] >= min_faces ? 1 : 0;
    }
    compact(nv, xyz, bgr, normal, nf, std::vector<int32_t>(index, index + 3 * nf), keep, out_nv, out_nf, out_xyz, out_bgr, out_normal, out_index);
}

void mesh_normals(long long nv, const float *xyz, long long nf, const int32_t *index, float *normal)
{
    std::vector<double> s((size_t)(3 * nv), 0.0);
    for (long long f = 0; f < nf; ++f) {
        double g[3];
        apd_fusion::mesh_face_normal(xyz + 3 * (long long)index[3 * f], xyz + 3 * (long long)index[3 * f + 1], xyz + 3 * (long long)index[3 * f + 2], g);
        for (int c = 0; c < 3; ++c) {
            apd_fusion::mesh_add(s.data() + 3 * (long long)index[3 * f + c], g);
        }
    }
    for (long long v = 0; v < nv; ++v) {
        apd_fusion::mesh_vertex_normal(s.data() + 3 * v, normal + 3 * v);
    }
}

}  // extern "C"
