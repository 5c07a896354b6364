// mesh_simplify_ref.cpp -- simplification of an indexed triangle mesh by vertex clustering, as a sequential restatement of contract
// C23:
//   clusters:    one loop over the vertices in index order, the key of apd_voxel_math.h for each, the members of every key collected
//                in an ordered map -- ascending key, and within a key ascending vertex index;
//   faces:       one loop over the faces in order; the rotated triples of the faces kept so far in an ordered set, so that the first
//                face of a set of duplicates is the one that stays;
//   placement:   per cluster one loop over its members, and for QUADRIC one loop over ALL faces in order and over their corners in
//                order, which is ascending 3 f + k for every cluster; then the solve of apd_simplify_math.h;
//   numbering:   one loop over the clusters in key order.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_mesh_simplify (apd-mvs_amd/csrc/apd_mesh_simplify.hip), compiled by
// tests/mesh_simplify_checker.py with -ffp-contract=off.  It shares the contract's headers with the product (the key, the cross
// product, the terms of the sums, the solve) and nothing else: no sort, no scan, no kernel, no atomic.
#include <array>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_simplify_math.h"

extern "C" {

// bgr may be null (then out_bgr is not written).  The out arrays have room for nv vertices and nf faces.  placement: 0 mean, 1 quadric
void mesh_simplify(long long nv, const float *xyz, const uint8_t *bgr, long long nf, const int32_t *index, float cell, const float *origin,
                   int placement, long long *out_nv, long long *out_nf, float *out_xyz, uint8_t *out_bgr, int32_t *out_index)
{
    std::map<uint64_t, std::vector<long long>> members;
    std::vector<uint64_t> key_of((size_t)nv);
    std::vector<char> inside((size_t)nv);
    for (long long v = 0; v < nv; ++v) {
        inside[(size_t)v] = apd_fusion::voxel_key(xyz + 3 * v, origin, cell, key_of[(size_t)v]) ? 1 : 0;
        if (inside[(size_t)v]) {
            members[key_of[(size_t)v]].push_back(v);
        }
    }
    std::vector<int32_t> cluster_of((size_t)nv, -1);
    std::vector<uint64_t> keys;
    for (const auto &entry : members) {
        for (long long v : entry.second) {
            cluster_of[(size_t)v] = (int32_t)keys.size();
        }
        keys.push_back(entry.first);
    }
    const size_t clusters = keys.size();
    // faces
    std::vector<char> whole((size_t)nf), keep((size_t)nf, 0);
    std::vector<int32_t> mapped((size_t)(3 * nf), 0);
    std::set<std::array<int32_t, 3>> seen;
    std::vector<char> used(clusters, 0);
    for (long long f = 0; f < nf; ++f) {
        whole[(size_t)f] = inside[(size_t)index[3 * f]] && inside[(size_t)index[3 * f + 1]] && inside[(size_t)index[3 * f + 2]];
        if (!whole[(size_t)f]) {
            continue;
        }
        int32_t *t = mapped.data() + 3 * f;
        for (int k = 0; k < 3; ++k) {
            t[k] = cluster_of[(size_t)index[3 * f + k]];
        }
        if (apd_fusion::mesh_face_degenerate(t[0], t[1], t[2])) {
            continue;
        }
        int32_t r[3];
        apd_fusion::simplify_rotated(t[0], t[1], t[2], r);
        if (!seen.insert({r[0], r[1], r[2]}).second) {
            continue;
        }
        keep[(size_t)f] = 1;
        used[(size_t)t[0]] = used[(size_t)t[1]] = used[(size_t)t[2]] = 1;
    }
    // the sums of every cluster: all faces in order, their corners in order
    std::vector<apd_fusion::SimplifySums> sums(placement == 1 ? clusters : 0);
    std::vector<double> centre(3 * clusters);
    for (size_t c = 0; c < clusters; ++c) {
        int i[3];
        apd_fusion::simplify_cell(keys[c], i);
        for (int a = 0; a < 3; ++a) {
            centre[3 * c + a] = apd_fusion::simplify_centre(origin[a], i[a], cell);
        }
    }
    for (long long f = 0; f < nf && placement == 1; ++f) {
        for (int k = 0; k < 3 && whole[(size_t)f]; ++k) {
            const size_t c = (size_t)mapped[(size_t)(3 * f + k)];
            apd_fusion::simplify_add(sums[c], xyz + 3 * (long long)index[3 * f], xyz + 3 * (long long)index[3 * f + 1], xyz + 3 * (long long)index[3 * f + 2],
                                     centre[3 * c], centre[3 * c + 1], centre[3 * c + 2]);
        }
    }
    // placement and numbering
    std::vector<int32_t> renumbered(clusters, -1);
    long long kept = 0;
    size_t c = 0;
    for (const auto &entry : members) {
        const std::vector<long long> &vs = entry.second;
        if (used[c]) {
            renumbered[c] = (int32_t)kept;
            const uint64_t m = vs.size();
            if (bgr) {
                for (int a = 0; a < 3; ++a) {
                    uint64_t sum = 0;
                    for (long long v : vs) {
                        sum += bgr[3 * v + a];
                    }
                    out_bgr[3 * kept + a] = apd_fusion::simplify_colour(sum, m);
                }
            }
            if (placement == 0) {
                for (int a = 0; a < 3; ++a) {
                    float sum = xyz[3 * vs[0] + a];
                    for (size_t j = 1; j < vs.size(); ++j) {
                        sum += xyz[3 * vs[j] + a];
                    }
                    out_xyz[3 * kept + a] = sum / (float)m;
                }
            } else {
                double mu[3];
                for (int a = 0; a < 3; ++a) {
                    double sum = 0.0;
                    for (long long v : vs) {
                        const double d = (double)xyz[3 * v + a] - centre[3 * c + a];
                        sum = sum + d;
                    }
                    mu[a] = sum / (double)m;
                }
                double x[3];
                apd_fusion::simplify_place(sums[c], mu[0], mu[1], mu[2], cell, x[0], x[1], x[2]);
                for (int a = 0; a < 3; ++a) {
                    out_xyz[3 * kept + a] = (float)(centre[3 * c + a] + x[a]);
                }
            }
            ++kept;
        }
        ++c;
    }
    *out_nv = kept;
    kept = 0;
    for (long long f = 0; f < nf; ++f) {
        if (!keep[(size_t)f]) {
            continue;
        }
        for (int k = 0; k < 3; ++k) {
            out_index[3 * kept + k] = renumbered[(size_t)mapped[(size_t)(3 * f + k)]];
        }
        ++kept;
    }
    *out_nf = kept;
}

// What a test needs of one cluster's solve: the offset x from the centre for given sums (s00 s01 s02 s11 s12 s22 t0 t1 t2) and mean
void mesh_simplify_place(const double *sums9, const double *mu, float cell, double *x)
{
    apd_fusion::SimplifySums m;
    m.s00 = sums9[0], m.s01 = sums9[1], m.s02 = sums9[2], m.s11 = sums9[3], m.s12 = sums9[4], m.s22 = sums9[5];
    m.t0 = sums9[6], m.t1 = sums9[7], m.t2 = sums9[8];
    apd_fusion::simplify_place(m, mu[0], mu[1], mu[2], cell, x[0], x[1], x[2]);
}

double mesh_simplify_rank_cut() { return apd_fusion::kSimplifyRankCut; }

}  // extern "C"
