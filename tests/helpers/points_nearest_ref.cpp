// points_nearest_ref.cpp -- the nearest point of another cloud within a radius and the score built on it, as a sequential
// restatement of arithmetic contract C17 in two ways:
//   mode 0, brute: the double loop over all (query, target) pairs, the cell condition and the distance of the relation applied to
//                  each, the targets taken in input order;
//   mode 1, grid:  a std::map from cell key to the target indices of the cell in input order, the 27 cells of a query looked up
//                  in ascending key order;
//                  a query's result depends on no other's, so both modes share the queries out to threads.
// The two must agree bit for bit: the cell condition of the relation makes the 27-cell search the definition, and the rule for
// equal distances (the smallest target index) does not depend on the order in which candidates are met.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_nearest and apd_points_score (apd-mvs_amd/csrc/apd_points_nearest.hip),
// compiled by tests/points_nearest_checker.py with -ffp-contract=off.  It shares the contract's headers with the product (the cell,
// the key, the squared distance, the rule for ties, the square root, the chunk sums, the score) and nothing else: no sort of
// cells, no scan, no kernel.
#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <thread>
#include <vector>

#include "../../apd-mvs_amd/csrc/apd_nearest_math.h"

namespace {

struct Located {
    bool inside;
    int cell[3];
    uint64_t key;
};

std::vector<Located> locate(long long n, const float *xyz, float radius, const float *origin)
{
    std::vector<Located> where((size_t)n);
    for (long long k = 0; k < n; ++k) {
        Located &w = where[(size_t)k];
        w.inside = apd_fusion::radius_cells(xyz + 3 * k, origin, radius, w.cell);
        w.key = w.inside ? apd_fusion::radius_key(w.cell[0], w.cell[1], w.cell[2]) : 0;
    }
    return where;
}

// The best candidate of one query so far
struct Best {
    bool have = false;
    float d2 = 0.0f;
    uint32_t j = 0;
    void offer(const float *P, const float *Q, uint32_t index, float r2)
    {
        const float d = apd_fusion::radius_d2(P, Q);
        if (d <= r2 && apd_fusion::nearest_takes(d, index, have, d2, j)) {
            have = true;
            d2 = d;
            j = index;
        }
    }
    void write(long long i, float *distance, int32_t *index) const
    {
        distance[i] = have ? apd_fusion::nearest_distance(d2) : apd_fusion::nearest_no_distance();
        index[i] = have ? (int32_t)j : apd_fusion::kNearestNoIndex;
    }
};

struct Clouds {
    long long n_p, n_q;
    const float *p, *q;
    std::vector<Located> where_p, where_q;
};

using Cells = std::map<uint64_t, std::vector<long long>>;

// Queries i of [first, n_p) in steps of `step`
void brute_part(long long first, long long step, const Clouds &c, float r2, float *distance, int32_t *index)
{
    for (long long i = first; i < c.n_p; i += step) {
        Best best;
        const Located &wi = c.where_p[(size_t)i];
        for (long long j = 0; j < c.n_q && wi.inside; ++j) {
            const Located &wj = c.where_q[(size_t)j];
            if (wj.inside && apd_fusion::radius_cells_adjacent(wi.cell, wj.cell)) {
                best.offer(c.p + 3 * i, c.q + 3 * j, (uint32_t)j, r2);
            }
        }
        best.write(i, distance, index);
    }
}

void grid_part(long long first, long long step, const Clouds &c, const Cells &cells, float r2, float *distance, int32_t *index)
{
    const int lo = -apd_fusion::kVoxelHalf, hi = apd_fusion::kVoxelHalf - 1;
    for (long long i = first; i < c.n_p; i += step) {
        Best best;
        const Located &wi = c.where_p[(size_t)i];
        for (int d = 0; d < 27 && wi.inside; ++d) {  // x fastest, then y, then z: ascending keys
            const int x = wi.cell[0] + d % 3 - 1, y = wi.cell[1] + d / 3 % 3 - 1, z = wi.cell[2] + d / 9 - 1;
            if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) {
                continue;
            }
            const auto found = cells.find(apd_fusion::radius_key(x, y, z));
            if (found == cells.end()) {
                continue;
            }
            for (long long j : found->second) {
                best.offer(c.p + 3 * i, c.q + 3 * j, (uint32_t)j, r2);
            }
        }
        best.write(i, distance, index);
    }
}

// distance and index (n_p each) of the queries p among the targets q
void nearest(int mode, long long n_p, const float *p, long long n_q, const float *q, float radius, const float *origin, float *distance, int32_t *index)
{
    const float r2 = radius * radius;
    const Clouds c = {n_p, n_q, p, q, locate(n_p, p, radius, origin), locate(n_q, q, radius, origin)};
    Cells cells;
    for (long long j = 0; j < n_q && mode != 0; ++j) {
        if (c.where_q[(size_t)j].inside) {
            cells[c.where_q[(size_t)j].key].push_back(j);
        }
    }
    const long long threads = n_p < 4096 ? 1 : std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 8);
    const auto part = [&](long long first) {
        if (mode == 0) {
            brute_part(first, threads, c, r2, distance, index);
        } else {
            grid_part(first, threads, c, cells, r2, distance, index);
        }
    };
    std::vector<std::thread> pool;
    for (long long t = 1; t < threads; ++t) {
        pool.emplace_back(part, t);
    }
    part(0);
    for (std::thread &t : pool) {
        t.join();
    }
}

// The finite values of d[0 .. n): their number and their sum in contract C12's order
void totals(const std::vector<float> &d, unsigned long long &count, double &sum)
{
    count = 0;
    sum = 0.0;
    for (size_t first = 0; first < d.size(); first += apd_fusion::kKnnChunk) {
        double s1 = 0.0, s2 = 0.0;
        unsigned full = 0;
        apd_fusion::knn_chunk_sums(d.data() + first, std::min(d.size() - first, (size_t)apd_fusion::kKnnChunk), s1, s2, full);
        sum = sum + s1;
        count += full;
    }
}

}  // namespace

extern "C" {

void points_nearest(int mode, long long n_p, const float *p, long long n_q, const float *q, float radius, const float *origin, float *distance,
                    int32_t *index)
{
    nearest(mode, n_p, p, n_q, q, radius, origin, distance, index);
}

// integers: n_p, n_q, p_within, q_within; reals: precision, recall, fscore, mean_p, mean_q
void points_score(int mode, long long n_p, const float *p, long long n_q, const float *q, float threshold, const float *origin, long long *integers,
                  double *reals)
{
    std::vector<float> dp((size_t)n_p), dq((size_t)n_q);
    std::vector<int32_t> ip((size_t)n_p), iq((size_t)n_q);
    nearest(mode, n_p, p, n_q, q, threshold, origin, dp.data(), ip.data());
    nearest(mode, n_q, q, n_p, p, threshold, origin, dq.data(), iq.data());
    unsigned long long a = 0, b = 0;
    double sum_p = 0.0, sum_q = 0.0;
    totals(dp, a, sum_p);
    totals(dq, b, sum_q);
    const apd_fusion::NearestScore s = apd_fusion::nearest_score((unsigned long long)n_p, (unsigned long long)n_q, a, b, sum_p, sum_q);
    integers[0] = s.n_p;
    integers[1] = s.n_q;
    integers[2] = s.p_within;
    integers[3] = s.q_within;
    reals[0] = s.precision;
    reals[1] = s.recall;
    reals[2] = s.fscore;
    reals[3] = s.mean_p;
    reals[4] = s.mean_q;
}

}  // extern "C"
