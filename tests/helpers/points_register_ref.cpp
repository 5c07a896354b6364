// points_register_ref.cpp -- FPFH descriptors, their matches and the registration of one cloud to another, as a sequential
// restatement of arithmetic contract C19, with the neighbourhoods of contract C11 under it in two ways:
//   mode 0, brute: every point's neighbours by the loop over all points, the cell condition and the distance of the relation
//                  applied to each, then put into the walk's order (ascending cell key, equal keys by ascending index);
//   mode 1, grid:  a std::map from cell key to the indices of the cell, built once, the 27 cells of a point looked up in
//                  ascending key order.
// The two must agree in every bit.  The matches are the double loop over all pairs of descriptors; the sums of the refit are
// taken as contract C18 words them: an array of 256 slots per chunk and per sum and the tree over it.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_features, apd_points_match_features and apd_points_register
// (apd-mvs_amd/csrc/apd_points_register.hip), compiled by tests/points_register_checker.py with -ffp-contract=off.  It shares the
// contract's headers with the product (the pair features, the bins, the descriptor, the distance, the generator, the trial, the
// driver of the trials and the refit; the cell, the key, the distance of the neighbourhood; the terms, the tree and the solve of
// contract C18) and nothing else: no sort of cells, no kernel, no LDS.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_register_math.h"

namespace {

using apd_fusion::kRegisterBins;
using apd_fusion::kRegisterWidth;

struct Cloud {
    long long n = 0;
    const float *xyz = nullptr;
    std::vector<char> frame;              // inside the grid, with a unit normal
    std::vector<uint64_t> key;            // of a point inside the grid
    std::vector<int> cell;                // 3 per point
    std::vector<double> unit;             // 3 per point
    std::map<uint64_t, std::vector<long long>> cells;  // every point inside the grid
    std::vector<std::vector<long long>> near;          // the neighbours by contract C11 in the walk's order
    std::vector<unsigned> admitted;       // k when it reaches min_neighbours, else 0
    std::vector<double> spfh;             // 33 per point
    std::vector<float> features;          // 33 per point
    std::vector<unsigned char> has;
};

void neighbourhoods(int mode, Cloud &c, const std::vector<char> &inside, float radius)
{
    const float r2 = radius * radius;
    c.near.assign((size_t)c.n, {});
    for (long long i = 0; i < c.n; ++i) {
        if (!inside[(size_t)i]) {
            continue;
        }
        std::vector<long long> &out = c.near[(size_t)i];
        const int *ci = &c.cell[3 * (size_t)i];
        if (mode == 0) {
            for (long long j = 0; j < c.n; ++j) {
                if (j != i && inside[(size_t)j] && apd_fusion::radius_neighbour(c.xyz + 3 * i, ci, c.xyz + 3 * j, &c.cell[3 * (size_t)j], r2)) {
                    out.push_back(j);
                }
            }
            std::sort(out.begin(), out.end(), [&](long long a, long long b) {
                return c.key[(size_t)a] != c.key[(size_t)b] ? c.key[(size_t)a] < c.key[(size_t)b] : a < b;
            });
        } else {
            const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
            std::vector<uint64_t> around;
            for (int d = 0; d < 27; ++d) {
                const int x = ci[0] + d % 3 - 1, y = ci[1] + d / 3 % 3 - 1, z = ci[2] + d / 9 - 1;
                if (x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi) {
                    around.push_back(apd_fusion::radius_key(x, y, z));
                }
            }
            std::sort(around.begin(), around.end());
            for (uint64_t k : around) {
                const auto found = c.cells.find(k);
                if (found == c.cells.end()) {
                    continue;
                }
                for (long long j : found->second) {
                    if (j != i && apd_fusion::radius_within(c.xyz + 3 * i, c.xyz + 3 * j, r2)) {
                        out.push_back(j);
                    }
                }
            }
        }
    }
}

void describe(int mode, Cloud &c, long long n, const float *xyz, const float *normal, float radius, const float *origin, unsigned min_neighbours)
{
    c.n = n;
    c.xyz = xyz;
    c.frame.assign((size_t)n, 0);
    c.key.assign((size_t)n, 0);
    c.cell.assign(3 * (size_t)n, 0);
    c.unit.assign(3 * (size_t)n, 0.0);
    c.admitted.assign((size_t)n, 0);
    c.spfh.assign((size_t)n * kRegisterWidth, 0.0);
    c.features.assign((size_t)n * kRegisterWidth, 0.0f);
    c.has.assign((size_t)n, 0);
    std::vector<char> inside((size_t)n, 0);
    for (long long i = 0; i < n; ++i) {
        int *cell = &c.cell[3 * (size_t)i];
        inside[(size_t)i] = apd_fusion::radius_cells(xyz + 3 * i, origin, radius, cell) ? 1 : 0;
        if (inside[(size_t)i]) {
            c.key[(size_t)i] = apd_fusion::radius_key(cell[0], cell[1], cell[2]);
            c.cells[c.key[(size_t)i]].push_back(i);
            c.frame[(size_t)i] = apd_fusion::register_unit_normal(normal + 3 * i, &c.unit[3 * (size_t)i]) ? 1 : 0;
        }
    }
    neighbourhoods(mode, c, inside, radius);
    for (long long i = 0; i < n; ++i) {
        if (!c.frame[(size_t)i]) {
            continue;
        }
        unsigned counts[kRegisterWidth] = {}, k = 0;
        for (long long j : c.near[(size_t)i]) {
            double d2;
            int bins[3];
            if (c.frame[(size_t)j] && apd_fusion::register_pair(xyz + 3 * i, &c.unit[3 * (size_t)i], xyz + 3 * j, &c.unit[3 * (size_t)j], d2, bins)) {
                counts[bins[0]] += 1;
                counts[kRegisterBins + bins[1]] += 1;
                counts[2 * kRegisterBins + bins[2]] += 1;
                ++k;
            }
        }
        if (k >= min_neighbours) {
            c.admitted[(size_t)i] = k;
            for (int b = 0; b < kRegisterWidth; ++b) {
                c.spfh[(size_t)i * kRegisterWidth + b] = (double)counts[b] / (double)k;
            }
        }
    }
    for (long long i = 0; i < n; ++i) {
        if (c.admitted[(size_t)i] == 0) {
            continue;
        }
        double acc[kRegisterWidth];
        for (int b = 0; b < kRegisterWidth; ++b) {
            acc[b] = 0.0;
        }
        for (long long j : c.near[(size_t)i]) {
            double d2;
            int bins[3];
            if (c.admitted[(size_t)j] != 0 &&
                apd_fusion::register_pair(xyz + 3 * i, &c.unit[3 * (size_t)i], xyz + 3 * j, &c.unit[3 * (size_t)j], d2, bins)) {
                for (int b = 0; b < kRegisterWidth; ++b) {
                    acc[b] = acc[b] + c.spfh[(size_t)j * kRegisterWidth + b] / d2;
                }
            }
        }
        apd_fusion::register_fpfh(&c.spfh[(size_t)i * kRegisterWidth], acc, c.admitted[(size_t)i], &c.features[(size_t)i * kRegisterWidth]);
        c.has[(size_t)i] = 1;
    }
}

// best[i] = the match of point i of `from` in `in`, -1 without one, and d2[i] its squared distance
void nearest_descriptors(const Cloud &from, const Cloud &in, std::vector<int32_t> &best, std::vector<float> &d2)
{
    best.assign((size_t)from.n, -1);
    d2.assign((size_t)from.n, 0.0f);
    for (long long i = 0; i < from.n; ++i) {
        if (!from.has[(size_t)i]) {
            continue;
        }
        for (long long j = 0; j < in.n; ++j) {
            if (!in.has[(size_t)j]) {
                continue;
            }
            const float d = apd_fusion::register_distance2(&from.features[(size_t)i * kRegisterWidth], &in.features[(size_t)j * kRegisterWidth]);
            if (best[(size_t)i] < 0 || d < d2[(size_t)i]) {
                best[(size_t)i] = (int32_t)j;
                d2[(size_t)i] = d;
            }
        }
    }
}

void match(const Cloud &p, const Cloud &q, bool mutual, int32_t *index, float *distance)
{
    std::vector<int32_t> best, back;
    std::vector<float> d2, back_d2;
    nearest_descriptors(p, q, best, d2);
    if (mutual) {
        nearest_descriptors(q, p, back, back_d2);
    }
    for (long long i = 0; i < p.n; ++i) {
        const int32_t j = best[(size_t)i];
        const bool stands = j >= 0 && (!mutual || back[(size_t)j] == (int32_t)i);
        index[i] = stands ? j : apd_fusion::kNearestNoIndex;
        distance[i] = stands ? apd_fusion::nearest_distance(d2[(size_t)i]) : apd_fusion::nearest_no_distance();
    }
}

// The totals of `width` sums over the points at x with the matches `index`; terms(P, Q, v) gives a matched point's
template <typename Terms> void totals(const float *x, const std::vector<int32_t> &index, const float *q, int width, Terms &&terms, double *total)
{
    const size_t n = index.size();
    for (int j = 0; j < width; ++j) {
        total[j] = 0.0;
    }
    for (size_t first = 0; first < n; first += apd_fusion::kKnnChunk) {
        double slots[apd_fusion::kAlignSums2][apd_fusion::kKnnChunk];
        for (int s = 0; s < apd_fusion::kKnnChunk; ++s) {
            double v[apd_fusion::kAlignSums2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const size_t k = first + (size_t)s;
            if (k < n && index[k] >= 0) {
                terms(x + 3 * k, q + 3 * (size_t)index[k], v);
            }
            for (int j = 0; j < width; ++j) {
                slots[j][s] = v[j];
            }
        }
        for (int j = 0; j < width; ++j) {
            total[j] = total[j] + apd_fusion::align_tree(slots[j]);
        }
    }
}

}  // namespace

extern "C" {

// features: 33 per point; has: one byte per point
void points_features(int mode, long long n, const float *xyz, const float *normal, float radius, const float *origin, unsigned min_neighbours,
                     float *features, unsigned char *has)
{
    Cloud c;
    describe(mode, c, n, xyz, normal, radius, origin, min_neighbours);
    std::copy(c.features.begin(), c.features.end(), features);
    std::copy(c.has.begin(), c.has.end(), has);
}

void points_match_features(int mode, long long n_p, const float *p, const float *p_normal, long long n_q, const float *q, const float *q_normal,
                           float radius, const float *origin, unsigned min_neighbours, int mutual, int32_t *index, float *distance)
{
    Cloud cp, cq;
    describe(mode, cp, n_p, p, p_normal, radius, origin, min_neighbours);
    describe(mode, cq, n_q, q, q_normal, radius, origin, min_neighbours);
    match(cp, cq, mutual != 0, index, distance);
}

// The matches given as two index arrays of M entries (from ascending): the trials, the best one and the refit alone
void points_register_matches(long long n_p, const float *p, const float *q, long long M, const int32_t *from, const int32_t *to,
                             const apd_fusion::RegisterOptions *o, apd_fusion::Registration *out)
{
    std::vector<float> mp, mq;
    for (long long e = 0; e < M; ++e) {
        mp.insert(mp.end(), p + 3 * (size_t)from[e], p + 3 * (size_t)from[e] + 3);
        mq.insert(mq.end(), q + 3 * (size_t)to[e], q + 3 * (size_t)to[e] + 3);
    }
    const float r2 = o->inlier_distance * o->inlier_distance;
    std::vector<int32_t> index((size_t)n_p, apd_fusion::kNearestNoIndex);
    std::vector<float> moved(3 * (size_t)n_p);
    const auto count = [&](const std::vector<apd_fusion::AlignMove> &moves, std::vector<uint32_t> &counts) {
        for (size_t a = 0; a < moves.size(); ++a) {
            for (long long e = 0; e < M; ++e) {
                counts[a] += apd_fusion::register_inlier(moves[a], &mp[3 * (size_t)e], &mq[3 * (size_t)e], r2) ? 1u : 0u;
            }
        }
        return 0;
    };
    const auto mark = [&](const apd_fusion::AlignMove &by) {
        std::fill(index.begin(), index.end(), apd_fusion::kNearestNoIndex);
        for (long long e = 0; e < M; ++e) {
            if (apd_fusion::register_inlier(by, &mp[3 * (size_t)e], &mq[3 * (size_t)e], r2)) {
                index[(size_t)from[e]] = to[e];
            }
        }
        return 0;
    };
    const auto pass1 = [&](const apd_fusion::AlignMove *by, double *s) {
        const float *x = p;
        if (by) {
            for (long long i = 0; i < n_p; ++i) {
                apd_fusion::align_moved(*by, p + 3 * i, &moved[3 * (size_t)i]);
            }
            x = moved.data();
        }
        totals(x, index, q, apd_fusion::kAlignSums1, [](const float *P, const float *Q, double *v) { apd_fusion::align_terms1(P, Q, v); }, s);
        return 0;
    };
    const auto pass2 = [&](const double mean[6], double *s) {
        totals(p, index, q, apd_fusion::kAlignSums2, [&](const float *P, const float *Q, double *v) { apd_fusion::align_terms2(P, Q, mean, v); }, s);
        return 0;
    };
    apd_fusion::register_run(*o, (size_t)M, mp.data(), mq.data(), count, mark, pass1, pass2, *out);
}

void points_register(int mode, long long n_p, const float *p, const float *p_normal, long long n_q, const float *q, const float *q_normal, float radius,
                     const float *origin, const apd_fusion::RegisterOptions *o, apd_fusion::Registration *out)
{
    *out = apd_fusion::register_identity(apd_fusion::kRegisterTooFewMatches);
    if (n_p == 0 || n_q == 0) {
        return;
    }
    Cloud cp, cq;
    describe(mode, cp, n_p, p, p_normal, radius, origin, o->min_neighbours);
    describe(mode, cq, n_q, q, q_normal, radius, origin, o->min_neighbours);
    std::vector<int32_t> index((size_t)n_p), from, to;
    std::vector<float> distance((size_t)n_p);
    match(cp, cq, o->mutual != 0, index.data(), distance.data());
    for (long long i = 0; i < n_p; ++i) {
        if (index[(size_t)i] >= 0) {
            from.push_back((int32_t)i);
            to.push_back(index[(size_t)i]);
        }
    }
    out->features_p = std::count(cp.has.begin(), cp.has.end(), 1);
    out->features_q = std::count(cq.has.begin(), cq.has.end(), 1);
    points_register_matches(n_p, p, q, (long long)from.size(), from.data(), to.data(), o, out);
}

// The pieces, for the tests of the contract itself
int points_register_theta_bin(double y, double x) { return apd_fusion::register_theta_bin(y, x); }
int points_register_linear_bin(double value) { return apd_fusion::register_linear_bin(value); }
void points_register_three(unsigned long long seed, unsigned t, unsigned M, unsigned *at) { apd_fusion::register_three(seed, t, M, at); }
unsigned points_register_draw(unsigned long long seed, unsigned t, unsigned c, unsigned M) { return apd_fusion::register_draw(seed, t, c, M); }
int points_register_pair(const float *C, const float *nc, const float *Q, const float *nq, double *d2, int *bins)
{
    double uc[3], uq[3];
    if (!apd_fusion::register_unit_normal(nc, uc) || !apd_fusion::register_unit_normal(nq, uq)) {
        return -1;
    }
    return apd_fusion::register_pair(C, uc, Q, uq, *d2, bins) ? 1 : 0;
}

}  // extern "C"
