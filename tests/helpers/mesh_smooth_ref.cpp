// mesh_smooth_ref.cpp -- the vertex adjacency of an indexed triangle mesh and Laplacian / Taubin smoothing over it, as a sequential
// restatement of contract C24:
//   adjacency:   one loop over the faces in order, the six keys of each; the kept keys sorted with std::sort; one loop over the
//                sorted keys that counts each run (the multiplicity) and appends the neighbour to its vertex's list;
//   a step:      one loop over the vertices, for each one loop over its list in order, the sums and the new position by the
//                functions of apd_mesh_smooth_math.h; two arrays of positions that swap after every step.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_mesh_adjacency and apd_mesh_smooth (apd-mvs_amd/csrc/apd_mesh_smooth.hip), compiled by
// tests/mesh_smooth_checker.py with -ffp-contract=off.  It shares the contract's header with the product (the keys, the entry of a
// list, the modes, the finite test, the step's arithmetic) and nothing else: no radix sort, no scan, no kernel.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_mesh_smooth_math.h"

namespace {

struct Lists {
    std::vector<std::vector<uint32_t>> of;  // per vertex: the entries of its neighbours, ascending
    std::vector<char> boundary;             // per vertex
    long long edges = 0, boundary_edges = 0, nonmanifold_edges = 0;
};

Lists lists_of(long long nv, long long nf, const int32_t *index)
{
    std::vector<uint64_t> keys;
    for (long long f = 0; f < nf; ++f) {
        uint64_t k[6];
        apd_fusion::smooth_face_keys(index[3 * f], index[3 * f + 1], index[3 * f + 2], k);
        for (int i = 0; i < 6; ++i) {
            if (k[i] != apd_fusion::kSmoothNoPair) {
                keys.push_back(k[i]);
            }
        }
    }
    std::sort(keys.begin(), keys.end());
    Lists l;
    l.of.resize((size_t)nv);
    l.boundary.assign((size_t)nv, 0);
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j] == keys[i]) {
            ++j;
        }
        const uint32_t v = (uint32_t)(keys[i] >> 32), w = (uint32_t)keys[i], multiplicity = (uint32_t)(j - i);
        l.of[v].push_back(apd_fusion::smooth_entry(w, multiplicity));
        if (multiplicity == 1) {
            l.boundary[v] = 1;
        }
        if (v < w) {
            l.edges += 1;
            l.boundary_edges += multiplicity == 1 ? 1 : 0;
            l.nonmanifold_edges += apd_fusion::smooth_nonmanifold(multiplicity) ? 1 : 0;
        }
        i = j;
    }
    return l;
}

// One step from p to q; returns the vertices that move
long long step(const Lists &l, long long nv, const float *p, int mode, double k, float *q)
{
    long long moved = 0;
    for (long long v = 0; v < nv; ++v) {
        const float *P = p + 3 * v;
        float *Q = q + 3 * v;
        Q[0] = P[0], Q[1] = P[1], Q[2] = P[2];
        const bool open = l.boundary[(size_t)v] != 0;
        if (apd_fusion::smooth_held(mode, open) || !apd_fusion::smooth_finite(P[0], P[1], P[2])) {
            continue;
        }
        double s[3] = {0.0, 0.0, 0.0};
        uint32_t count = 0;
        for (uint32_t entry : l.of[(size_t)v]) {
            if (!apd_fusion::smooth_takes(mode, open, entry)) {
                continue;
            }
            const float *W = p + 3 * (size_t)apd_fusion::smooth_entry_vertex(entry);
            if (apd_fusion::smooth_finite(W[0], W[1], W[2])) {
                apd_fusion::smooth_add(s, W[0], W[1], W[2]);
                ++count;
            }
        }
        if (count == 0) {
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            Q[a] = apd_fusion::smooth_place(P[a], s[a], count, k);
        }
        ++moved;
    }
    return moved;
}

}  // namespace

extern "C" {

// valence: nv entries, boundary: nv bytes, counts: edges, boundary edges, non-manifold edges
void mesh_adjacency(long long nv, long long nf, const int32_t *index, uint32_t *valence, uint8_t *boundary, long long *counts)
{
    const Lists l = lists_of(nv, nf, index);
    for (long long v = 0; v < nv; ++v) {
        valence[v] = (uint32_t)l.of[(size_t)v].size();
        boundary[v] = l.boundary[(size_t)v] ? 1 : 0;
    }
    counts[0] = l.edges;
    counts[1] = l.boundary_edges;
    counts[2] = l.nonmanifold_edges;
}

// out_xyz: nv positions; returns the vertices that move in the first step.  mode: 0 fixed, 1 along, 2 free
long long mesh_smooth(long long nv, const float *xyz, long long nf, const int32_t *index, int iterations, float lambda, float mu, int mode, float *out_xyz)
{
    const Lists l = lists_of(nv, nf, index);
    std::vector<float> a(xyz, xyz + 3 * nv), b((size_t)(3 * nv));
    long long moved = 0;
    for (int it = 0; it < iterations; ++it) {
        const long long first = step(l, nv, a.data(), mode, (double)lambda, b.data());
        moved = it == 0 ? first : moved;
        a.swap(b);
        if (mu != 0.0f) {
            step(l, nv, a.data(), mode, (double)mu, b.data());
            a.swap(b);
        }
    }
    std::copy(a.begin(), a.end(), out_xyz);
    return moved;
}

}  // extern "C"
