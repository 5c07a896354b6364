// apd_points_register.hip -- apd_points_features, apd_points_match_features and apd_points_register of include/apd_mi355x.h: FPFH
// descriptors from the stored normals, the nearest descriptor of another points object, and the rigid or similarity transform
// that brings one object onto another from any start, by RANSAC over those matches and a refit on the inliers (arithmetic
// contract C19; the relation, the generator, the trials and the driver: apd_register_math.h).
//
// On the points' device, on its null stream.  Descriptors of one cloud (Call::describe):
//   1. the points inside the grid in cell order (Search::sort_into_cells) and k_register_frames: the unit normals, binary64,
//      gathered into that order beside the positions; zeros for a point without a frame.
//   2. k_register_spfh: one lane per sorted point on the walk (for_each_candidate).  A bin is a runtime value and a per-lane
//      array indexed by one would live in scratch memory, so the lane's 33 counters live in LDS laid out [slot][lane] as the
//      slots of apd_points_knn.hip are: slot s of lane l is word 64 * s + l, every slot of a lane in bank l % 32, so no access
//      conflicts however the lanes diverge.  One wave per workgroup, 8448 bytes of LDS, no barrier: a lane touches its own column
//      only.  The row goes out as 33 doubles in SORTED order, so that the rows of a cell run are contiguous for step 3, with
//      the number of admitted neighbours (0: no SPFH).
//   3. k_register_fpfh: the second walk; the lane's 33 binary64 sums are registers (every index is a constant after unrolling)
//      and take the neighbours' rows in the walk's ascending order; the descriptor goes to the point's input index.
// Matches (Call::nearest_rows): the descriptors of the points that have one are compacted in input order (apd_sort's scan), so
// that ascending position is ascending input index.  k_register_match: one lane per query, its 33 floats in registers; the
// candidates pass through LDS in tiles of kMatchTile rows and every lane reads the same row at the same time, a broadcast; the
// running (distance, position) minimum is replaced only by a strictly smaller distance, and the candidates come in ascending
// order, so ties go to the smaller index.  The minimum lives in device memory between launches: the host splits the work into
// launches of at most `pair_bound` (query, candidate) pairs (kMatchLaunchPairs; profiles/points_register/timing.txt), so that no
// launch runs long on a shared machine.
// Registration: the index array and the matches' positions (k_register_gather) come to the host, which draws the trials, tests them and solves the
// admitted ones (apd_fusion::register_run); only the admitted trials' moves go up and only their counts come down.
// k_register_count: one lane per admitted trial, its twelve doubles in registers, the matches' six floats staged through LDS in
// tiles and read as broadcasts; an integer per trial written by an ordinary store.  k_register_mark writes the index array of the
// refit -- the match for an inlier, -1 otherwise -- and the sums are those of apd_points_align_sums.h.
// No atomics, no scratch memory.  There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_align_math.h"
#include "apd_fusion_device.h"
#include "apd_points_align_sums.h"
#include "apd_points_host.h"
#include "apd_points_nearest.h"
#include "apd_points_search.h"
#include "apd_register_math.h"
#include "apd_sort.h"

namespace {

using apd_align_sums::AlignMeans;
using apd_align_sums::AlignSums;
using apd_align_sums::k_align_sums1;
using apd_align_sums::k_align_sums2;
using apd_fusion::AlignMove;
using apd_fusion::kAlignSums1;
using apd_fusion::kAlignSums2;
using apd_fusion::kKnnChunk;
using apd_fusion::kRegisterWidth;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::for_each_candidate;
using apd_points_search::k_fill;
using apd_points_search::Sorted;
using apd_points_search::Staged;

static_assert(sizeof(apd_points_registration_t) == sizeof(apd_fusion::Registration), "apd_points_registration_t is Registration");
static_assert(sizeof(apd_points_register_options) == sizeof(apd_fusion::RegisterOptions), "apd_points_register_options is RegisterOptions");
static_assert(APD_REGISTER_OK == apd_fusion::kRegisterOk && APD_REGISTER_TOO_FEW_MATCHES == apd_fusion::kRegisterTooFewMatches &&
                  APD_REGISTER_NO_TRIAL == apd_fusion::kRegisterNoTrial,
              "APD_REGISTER_* are kRegister*");

constexpr int kLanes = 64;         // of a workgroup of the two walks and of the count: one wave
constexpr int kMatchLanes = 256;   // of a workgroup of k_register_match
constexpr int kMatchTile = 128;    // candidate rows in LDS at a time: 16896 bytes
constexpr int kCountTile = 256;    // matches in LDS at a time: 6144 bytes
// (query, candidate) pairs of one launch of k_register_match at most: about 25 ms at the measured 4 * 10^10 pairs per second
// (profiles/points_register/timing.txt), so that the largest match allowed, 2^36 pairs, is 64 launches and none runs long
constexpr unsigned long long kMatchLaunchPairs = 1ull << 30;

// Where a call's time goes, for tools/points_register_time.py alone: off unless apd_points_register_time_phases(1) was called, and
// then every phase ends in a device synchronise, which the product path does not pay
enum : int { kPhaseSort = 0, kPhaseSpfh, kPhaseFpfh, kPhaseMatch, kPhaseTrials, kPhaseCount, kPhaseRefit, kPhases };
bool g_time_phases = false;
double g_phase_ms[kPhases] = {};
std::chrono::steady_clock::time_point g_phase_start;

// The time since the last call, on the device and the host, goes to phase `to`
void phase(int to)
{
    if (g_time_phases) {
        (void)hipDeviceSynchronize();
        g_phase_ms[to] += apd_points_host::ms_since(g_phase_start);
        g_phase_start = std::chrono::steady_clock::now();
    }
}

// Sorted element i < m: unit[3 i ..] = the unit normal of its stored normal, zeros without one
__global__ __launch_bounds__(256) void k_register_frames(const float *__restrict__ normal, const uint32_t *__restrict__ member, size_t m,
                                                          double *__restrict__ unit)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) {
        return;
    }
    const size_t k = member[i];
    const float N[3] = {normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]};
    double u[3];
    apd_fusion::register_unit_normal(N, u);
    unit[3 * i] = u[0];
    unit[3 * i + 1] = u[1];
    unit[3 * i + 2] = u[2];
}

// Sorted element i < m: admitted[i] = the number of its admitted neighbours when that reaches min_neighbours and 0 otherwise, and
// then spfh[33 i ..] = its SPFH by contract C19.  keys: ascending; xyz, unit: in the same order
__global__ __launch_bounds__(kLanes) void k_register_spfh(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                           const double *__restrict__ unit, uint32_t m, float r2, uint32_t min_neighbours,
                                                           double *__restrict__ spfh, uint32_t *__restrict__ admitted)
{
    __shared__ uint32_t counters[kRegisterWidth * kLanes];  // [slot][lane]
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;   // m < 2^31
    if (i >= m) {
        return;
    }
    uint32_t *const mine = counters + threadIdx.x;  // slot s: mine[kLanes * s]
    for (int s = 0; s < kRegisterWidth; ++s) {
        mine[kLanes * s] = 0;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    const double np[3] = {unit[3 * (size_t)i], unit[3 * (size_t)i + 1], unit[3 * (size_t)i + 2]};
    uint32_t k = 0;
    if (apd_fusion::register_has_frame(np)) {
        for_each_candidate(keys, xyz, i, m, [&](uint32_t at, const float Q[3]) {
            if (at == i || !(apd_fusion::radius_d2(P, Q) <= r2)) {
                return false;
            }
            const double nq[3] = {unit[3 * (size_t)at], unit[3 * (size_t)at + 1], unit[3 * (size_t)at + 2]};
            double d2;
            int bins[3];
            if (apd_fusion::register_has_frame(nq) && apd_fusion::register_pair(P, np, Q, nq, d2, bins)) {
                mine[kLanes * bins[0]] += 1;
                mine[kLanes * (apd_fusion::kRegisterBins + bins[1])] += 1;
                mine[kLanes * (2 * apd_fusion::kRegisterBins + bins[2])] += 1;
                ++k;
            }
            return false;
        });
    }
    const bool has = k >= min_neighbours;
    admitted[i] = has ? k : 0u;
    if (has) {
        const double count = (double)k;
        for (int s = 0; s < kRegisterWidth; ++s) {
            spfh[(size_t)i * kRegisterWidth + s] = (double)mine[kLanes * s] / count;
        }
    }
}

// Sorted element i < m with an SPFH: features[33 member[i] ..] = its descriptor and has[member[i]] = 1; the others keep what
// they have
__global__ __launch_bounds__(kLanes) void k_register_fpfh(const uint64_t *__restrict__ keys, const float *__restrict__ xyz,
                                                           const double *__restrict__ unit, const uint32_t *__restrict__ member, uint32_t m, float r2,
                                                           const double *__restrict__ spfh, const uint32_t *__restrict__ admitted,
                                                           float *__restrict__ features, uint8_t *__restrict__ has)
{
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= m || admitted[i] == 0) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    const double np[3] = {unit[3 * (size_t)i], unit[3 * (size_t)i + 1], unit[3 * (size_t)i + 2]};
    double acc[kRegisterWidth];
#pragma unroll
    for (int b = 0; b < kRegisterWidth; ++b) {
        acc[b] = 0.0;
    }
    for_each_candidate(keys, xyz, i, m, [&](uint32_t at, const float Q[3]) {
        if (at == i || admitted[at] == 0 || !(apd_fusion::radius_d2(P, Q) <= r2)) {
            return false;  // a point with an SPFH has a frame
        }
        const double nq[3] = {unit[3 * (size_t)at], unit[3 * (size_t)at + 1], unit[3 * (size_t)at + 2]};
        double d2;
        int bins[3];
        if (apd_fusion::register_pair(P, np, Q, nq, d2, bins)) {
            const double *const row = spfh + (size_t)at * kRegisterWidth;
#pragma unroll
            for (int b = 0; b < kRegisterWidth; ++b) {
                acc[b] = acc[b] + row[b] / d2;
            }
        }
        return false;
    });
    float out[kRegisterWidth];
    apd_fusion::register_fpfh(spfh + (size_t)i * kRegisterWidth, acc, admitted[i], out);
    const size_t k = member[i];
#pragma unroll
    for (int b = 0; b < kRegisterWidth; ++b) {
        features[k * kRegisterWidth + b] = out[b];
    }
    has[k] = 1;
}

__global__ __launch_bounds__(256) void k_register_flags(const uint8_t *__restrict__ has, size_t n, uint32_t *__restrict__ keep)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        keep[k] = has[k] ? 1u : 0u;
    }
}

// The descriptors of the points with one, in input order: row at[k] is point k's, origin[at[k]] = k
__global__ __launch_bounds__(256) void k_register_compact(const float *__restrict__ features, const uint32_t *__restrict__ keep,
                                                           const uint64_t *__restrict__ at, size_t n, float *__restrict__ rows, int32_t *__restrict__ origin)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || keep[k] == 0) {
        return;
    }
    const size_t c = (size_t)at[k];
    for (int b = 0; b < kRegisterWidth; ++b) {
        rows[c * kRegisterWidth + b] = features[k * kRegisterWidth + b];
    }
    origin[c] = (int32_t)k;  // fewer than 2^31 points
}

// Queries first .. first + count of `rows` against the candidates c0 .. c1 of `cand` (rows of 33 floats each): (best_d[i],
// best_j[i]), the running minimum of query i by contract C19, takes them in
__global__ __launch_bounds__(kMatchLanes) void k_register_match(const float *__restrict__ rows, uint32_t first, uint32_t count,
                                                                 const float *__restrict__ cand, uint32_t c0, uint32_t c1, float *__restrict__ best_d,
                                                                 int32_t *__restrict__ best_j)
{
    __shared__ float tile[kMatchTile * kRegisterWidth];
    const uint32_t offset = blockIdx.x * kMatchLanes + threadIdx.x;
    const bool live = offset < count;
    const size_t i = (size_t)first + offset;
    float mine[kRegisterWidth];
#pragma unroll
    for (int b = 0; b < kRegisterWidth; ++b) {
        mine[b] = live ? rows[i * kRegisterWidth + b] : 0.0f;
    }
    float best = live ? best_d[i] : INFINITY;
    int32_t best_at = live ? best_j[i] : -1;
    for (uint32_t t0 = c0; t0 < c1; t0 += kMatchTile) {
        const uint32_t here = c1 - t0 < (uint32_t)kMatchTile ? c1 - t0 : (uint32_t)kMatchTile;
        __syncthreads();  // the tile before is read
        for (uint32_t e = threadIdx.x; e < here * kRegisterWidth; e += kMatchLanes) {
            tile[e] = cand[(size_t)t0 * kRegisterWidth + e];
        }
        __syncthreads();
        for (uint32_t r = 0; r < here; ++r) {
            const float d = apd_fusion::register_distance2(mine, tile + r * kRegisterWidth);
            if (d < best) {
                best = d;
                best_at = (int32_t)(t0 + r);
            }
        }
    }
    if (live) {
        best_d[i] = best;
        best_j[i] = best_at;
    }
}

// Compacted query c < count with a match that stands (mutual: whose match's match it is): index and distance, either may be
// null, of its input index; the others keep what they have
__global__ __launch_bounds__(256) void k_register_matches(const float *__restrict__ best_d, const int32_t *__restrict__ best_j, uint32_t count,
                                                           const int32_t *__restrict__ back, const int32_t *__restrict__ origin_p,
                                                           const int32_t *__restrict__ origin_q, int32_t *__restrict__ index, float *__restrict__ distance)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= count) {
        return;
    }
    const int32_t j = best_j[c];
    if (j < 0 || (back && back[j] != (int32_t)c)) {
        return;
    }
    const size_t k = (size_t)origin_p[c];
    if (index) {
        index[k] = origin_q[j];
    }
    if (distance) {
        distance[k] = apd_fusion::nearest_distance(best_d[c]);
    }
}

// Admitted trial a < A: counts[a] = the inliers of moves[a] among the M matches, whose positions stand at six (P's, then Q's)
__global__ __launch_bounds__(kLanes) void k_register_count(const AlignMove *__restrict__ moves, uint32_t A, const float *__restrict__ six, uint32_t M,
                                                            float r2, uint32_t *__restrict__ counts)
{
    __shared__ float tile[kCountTile * 6];
    const uint32_t a = blockIdx.x * kLanes + threadIdx.x;
    const bool live = a < A;
    const AlignMove by = moves[live ? a : 0];  // A > 0
    uint32_t count = 0;
    for (uint32_t m0 = 0; m0 < M; m0 += kCountTile) {
        const uint32_t here = M - m0 < (uint32_t)kCountTile ? M - m0 : (uint32_t)kCountTile;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < here * 6; e += kLanes) {
            tile[e] = six[(size_t)m0 * 6 + e];
        }
        __syncthreads();
        for (uint32_t r = 0; r < here; ++r) {
            count += apd_fusion::register_inlier(by, tile + 6 * r, tile + 6 * r + 3, r2) ? 1u : 0u;
        }
    }
    if (live) {
        counts[a] = count;
    }
}

// Match e < M, of point from[e] of P to point to[e] of Q: six[6 e ..] = P's position, then Q's
__global__ __launch_bounds__(256) void k_register_gather(const int32_t *__restrict__ from, const int32_t *__restrict__ to, uint32_t M,
                                                          const float *__restrict__ xyz, const float *__restrict__ target, float *__restrict__ six)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M) {
        return;
    }
    const size_t i = (size_t)from[e], j = (size_t)to[e];
    for (int a = 0; a < 3; ++a) {
        six[6 * (size_t)e + a] = xyz[3 * i + a];
        six[6 * (size_t)e + 3 + a] = target[3 * j + a];
    }
}

// Match e < M, of point from[e] of P to point to[e] of Q: index[from[e]] = to[e] when it is an inlier of `by`, -1 otherwise
__global__ __launch_bounds__(256) void k_register_mark(const int32_t *__restrict__ from, const int32_t *__restrict__ to, uint32_t M,
                                                        const float *__restrict__ xyz, const float *__restrict__ target, AlignMove by, float r2,
                                                        int32_t *__restrict__ index)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M) {
        return;
    }
    const size_t i = (size_t)from[e], j = (size_t)to[e];
    const float P[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    const float Q[3] = {target[3 * j], target[3 * j + 1], target[3 * j + 2]};
    index[i] = apd_fusion::register_inlier(by, P, Q, r2) ? (int32_t)j : apd_fusion::kNearestNoIndex;
}

// The descriptors of one cloud that have one, in input order
struct Rows {
    size_t count = 0;
    const float *rows = nullptr;
    const int32_t *origin = nullptr;  // the input index of row c
};

// One call of any of the three entry points
struct Call : AlignSums {
    unsigned min_neighbours = 0;
    unsigned long long pair_bound = kMatchLaunchPairs;

    // What the calls refuse on top of Search::check
    int check_neighbours(unsigned want)
    {
        if (want < apd_fusion::kRegisterMinNeighbours) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: min_neighbours = %u, below %u", who, want, apd_fusion::kRegisterMinNeighbours);
        }
        min_neighbours = want;
        return APD_OK;
    }

    // The match costs the product of the two counts
    int check_size(apd_points_t p) const
    {
        if (p->count > apd_fusion::kRegisterMaxPoints) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED,
                                  "%s: %lld points, more than %lld: matching costs the product of the two counts; thin the cloud first "
                                  "(apd_points_merge_voxels)",
                                  who, p->count, apd_fusion::kRegisterMaxPoints);
        }
        return APD_OK;
    }

    int check_options(const apd_fusion::RegisterOptions &o) const
    {
        if (o.trials < 1 || o.trials > apd_fusion::kRegisterMaxTrials) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: trials = %u, not in 1 .. %u", who, o.trials, apd_fusion::kRegisterMaxTrials);
        }
        const float r2 = o.inlier_distance * o.inlier_distance;
        if (!(isfinite(o.inlier_distance) && o.inlier_distance > 0.0f && isfinite(r2) && r2 > 0.0f)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: an inlier distance of %g, not a positive finite number with such a square", who,
                                  (double)o.inlier_distance);
        }
        if (!(o.edge_ratio > 0.0f && o.edge_ratio <= 1.0f)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: an edge ratio of %g, not in (0, 1]", who, (double)o.edge_ratio);
        }
        return APD_OK;
    }

    // features (33 n floats) and has (n bytes) of the n > 0 points at xyz with the normals `normal`; all device memory
    int describe(const float *xyz, const float *normal, size_t n, float *features, uint8_t *has) const
    {
        Scratch scratch;
        HIP_TRY(hipMemsetAsync(features, 0, n * kRegisterWidth * 4, 0));
        HIP_TRY(hipMemsetAsync(has, 0, n, 0));
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK || s.m == 0) {
            return rc;
        }
        phase(kPhaseSort);
        double *unit = nullptr, *spfh = nullptr;
        uint32_t *admitted = nullptr;
        HIP_TRY(scratch.alloc(s.m * 24, &unit));
        HIP_TRY(scratch.alloc(s.m * kRegisterWidth * 8, &spfh));
        HIP_TRY(scratch.alloc(s.m * 4, &admitted));
        const float r2 = grid.size * grid.size;
        const unsigned blocks = (unsigned)((s.m + kLanes - 1) / kLanes);
        hipLaunchKernelGGL(k_register_frames, grid_of(s.m), dim3(256), 0, 0, normal, s.member, s.m, unit);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_register_spfh, dim3(blocks), dim3(kLanes), 0, 0, s.keys, s.xyz, (const double *)unit, (uint32_t)s.m, r2,
                           (uint32_t)min_neighbours, spfh, admitted);
        HIP_TRY(hipGetLastError());
        phase(kPhaseSpfh);
        hipLaunchKernelGGL(k_register_fpfh, dim3(blocks), dim3(kLanes), 0, 0, s.keys, s.xyz, (const double *)unit, s.member, (uint32_t)s.m, r2,
                           (const double *)spfh, (const uint32_t *)admitted, features, has);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // before the sort's memory goes
        phase(kPhaseFpfh);
        return APD_OK;
    }

    // The descriptors of p (count > 0, its device current) in the caller's scratch: features, has, and the compacted rows
    int rows_of(Scratch &scratch, apd_points_t p, const float *xyz, Rows &out) const
    {
        const size_t n = (size_t)p->count;
        const float *normal = nullptr;
        float *features = nullptr, *rows = nullptr;
        uint8_t *has = nullptr;
        uint32_t *keep = nullptr;
        uint64_t *at = nullptr;
        int32_t *origin = nullptr;
        if (const int rc = readable(scratch, p, (const float *)p->arrays.normal, n * 12, &normal); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(scratch.alloc(n * kRegisterWidth * 4, &features));
        HIP_TRY(scratch.alloc(n, &has));
        HIP_TRY(scratch.alloc(n * 4, &keep));
        HIP_TRY(scratch.alloc((n + 1) * 8, &at));
        if (const int rc = describe(xyz, normal, n, features, has); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_register_flags, grid_of(n), dim3(256), 0, 0, (const uint8_t *)has, n, keep);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(keep, at, n));
        uint64_t count = 0;
        HIP_TRY(hipMemcpy(&count, at + n, 8, hipMemcpyDeviceToHost));
        out.count = (size_t)count;
        HIP_TRY(scratch.alloc(out.count * kRegisterWidth * 4, &rows));
        HIP_TRY(scratch.alloc(out.count * 4, &origin));
        hipLaunchKernelGGL(k_register_compact, grid_of(n), dim3(256), 0, 0, (const float *)features, (const uint32_t *)keep, (const uint64_t *)at, n, rows,
                           origin);
        HIP_TRY(hipGetLastError());
        out.rows = rows;
        out.origin = origin;
        return APD_OK;
    }

    // (best_d, best_j), from.count entries each in the caller's scratch: every row of `from` against every row of `in`
    int nearest_rows(Scratch &scratch, const Rows &from, const Rows &in, float **best_d, int32_t **best_j) const
    {
        HIP_TRY(scratch.alloc(from.count * 4, best_d));
        HIP_TRY(scratch.alloc(from.count * 4, best_j));
        if (from.count == 0) {
            return APD_OK;
        }
        hipLaunchKernelGGL(k_fill<float>, grid_of(from.count), dim3(256), 0, 0, *best_d, from.count, apd_fusion::nearest_no_distance());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fill<int32_t>, grid_of(from.count), dim3(256), 0, 0, *best_j, from.count, apd_fusion::kNearestNoIndex);
        HIP_TRY(hipGetLastError());
        const unsigned long long bound = pair_bound > 0 ? pair_bound : 1;
        const size_t queries = (size_t)std::min<unsigned long long>(from.count, bound);
        const size_t candidates = (size_t)std::max<unsigned long long>(1, bound / queries);
        for (size_t q0 = 0; q0 < from.count; q0 += queries) {
            const size_t qn = std::min(queries, from.count - q0);
            for (size_t c0 = 0; c0 < in.count; c0 += candidates) {
                const size_t c1 = std::min(in.count, c0 + candidates);
                hipLaunchKernelGGL(k_register_match, dim3((unsigned)((qn + kMatchLanes - 1) / kMatchLanes)), dim3(kMatchLanes), 0, 0, from.rows,
                                   (uint32_t)q0, (uint32_t)qn, in.rows, (uint32_t)c0, (uint32_t)c1, *best_d, *best_j);
                HIP_TRY(hipGetLastError());
            }
        }
        return APD_OK;
    }

    // index and distance (either may be null; n_p entries each, device memory) of p's matches in q, both with points; xyz_p and
    // xyz_q: their positions, readable.  features_*: how many points of each have a descriptor
    int matches(Scratch &scratch, apd_points_t p, apd_points_t q, const float *xyz_p, const float *xyz_q, bool mutual, int32_t *index, float *distance,
                long long *features_p, long long *features_q) const
    {
        const size_t n = (size_t)p->count;
        Rows rp, rq;
        if (const int rc = rows_of(scratch, p, xyz_p, rp); rc != APD_OK) {
            return rc;
        }
        rq = rp;
        if (q != p) {
            if (const int rc = rows_of(scratch, q, xyz_q, rq); rc != APD_OK) {
                return rc;
            }
        }
        *features_p = (long long)rp.count;
        *features_q = (long long)rq.count;
        if (index) {
            hipLaunchKernelGGL(k_fill<int32_t>, grid_of(n), dim3(256), 0, 0, index, n, apd_fusion::kNearestNoIndex);
            HIP_TRY(hipGetLastError());
        }
        if (distance) {
            hipLaunchKernelGGL(k_fill<float>, grid_of(n), dim3(256), 0, 0, distance, n, apd_fusion::nearest_no_distance());
            HIP_TRY(hipGetLastError());
        }
        if (rp.count == 0 || rq.count == 0) {
            return APD_OK;
        }
        float *best_d = nullptr, *back_d = nullptr;
        int32_t *best_j = nullptr, *back_j = nullptr;
        if (const int rc = nearest_rows(scratch, rp, rq, &best_d, &best_j); rc != APD_OK) {
            return rc;
        }
        if (mutual) {
            if (const int rc = nearest_rows(scratch, rq, rp, &back_d, &back_j); rc != APD_OK) {
                return rc;
            }
        }
        hipLaunchKernelGGL(k_register_matches, grid_of(rp.count), dim3(256), 0, 0, (const float *)best_d, (const int32_t *)best_j, (uint32_t)rp.count,
                           (const int32_t *)back_j, rp.origin, rq.origin, index, distance);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // Both clouds' positions readable on p's device, which it selects
    int both_positions(Scratch &scratch, apd_points_t p, apd_points_t q, const float **xyz_p, const float **xyz_q) const
    {
        if (const int rc = positions(scratch, p, xyz_p); rc != APD_OK) {
            return rc;
        }
        *xyz_q = *xyz_p;
        return q == p ? (int)APD_OK : readable(scratch, q, (const float *)q->arrays.xyz, (size_t)q->count * 12, xyz_q);
    }

    // apd_points_features of p (count > 0)
    int features_of(apd_points_t p, float *features, uint8_t *has) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        const float *xyz = nullptr, *normal = nullptr;
        Staged<float> out_features;
        Staged<uint8_t> out_has;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : readable(scratch, p, (const float *)p->arrays.normal, n * 12, &normal);
        rc = rc != APD_OK ? rc : stage(scratch, p, features, n * kRegisterWidth * 4, out_features);
        rc = rc != APD_OK ? rc : stage(scratch, p, has, n, out_has);
        if (rc == APD_OK && !out_has.device) {
            HIP_TRY(scratch.alloc(n, &out_has.device));
        }
        rc = rc != APD_OK ? rc : describe(xyz, normal, n, out_features.device, out_has.device);
        rc = rc != APD_OK ? rc : download(out_features);
        return rc != APD_OK ? rc : download(out_has);
    }

    // apd_points_match_features of p in q, both with points
    int match_of(apd_points_t p, apd_points_t q, bool mutual, int32_t *index, float *distance) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        const float *xyz_p = nullptr, *xyz_q = nullptr;
        Staged<int32_t> out_index;
        Staged<float> out_distance;
        long long fp = 0, fq = 0;
        int rc = both_positions(scratch, p, q, &xyz_p, &xyz_q);
        rc = rc != APD_OK ? rc : stage(scratch, p, index, n * 4, out_index);
        rc = rc != APD_OK ? rc : stage(scratch, p, distance, n * 4, out_distance);
        rc = rc != APD_OK ? rc : matches(scratch, p, q, xyz_p, xyz_q, mutual, out_index.device, out_distance.device, &fp, &fq);
        rc = rc != APD_OK ? rc : download(out_index);
        return rc != APD_OK ? rc : download(out_distance);
    }

    // The answer of device-resident points without candidates
    int no_matches(apd_points_t p, int32_t *index, float *distance) const
    {
        const size_t n = (size_t)p->count;
        HIP_TRY(hipSetDevice(p->device));
        if (index) {
            hipLaunchKernelGGL(k_fill<int32_t>, grid_of(n), dim3(256), 0, 0, index, n, apd_fusion::kNearestNoIndex);
            HIP_TRY(hipGetLastError());
        }
        if (distance) {
            hipLaunchKernelGGL(k_fill<float>, grid_of(n), dim3(256), 0, 0, distance, n, apd_fusion::nearest_no_distance());
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_points_register of p onto q, both with points
    int register_of(apd_points_t p, apd_points_t q, const apd_fusion::RegisterOptions &o, apd_fusion::Registration &out) const
    {
        const size_t n = (size_t)p->count, chunks = (n + kKnnChunk - 1) / kKnnChunk;
        Scratch scratch;
        const float *own = nullptr, *target = nullptr;
        int32_t *index = nullptr;
        if (const int rc = both_positions(scratch, p, q, &own, &target); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(scratch.alloc(n * 4, &index));
        if (const int rc = matches(scratch, p, q, own, target, o.mutual != 0, index, nullptr, &out.features_p, &out.features_q); rc != APD_OK) {
            return rc;
        }
        // the matches in ascending i, and their positions, on the host
        std::vector<int32_t> all(n), from, to;
        HIP_TRY(hipMemcpy(all.data(), index, n * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (all[i] >= 0) {
                from.push_back((int32_t)i);
                to.push_back(all[i]);
            }
        }
        const size_t M = from.size();
        const float r2 = o.inlier_distance * o.inlier_distance;
        const int32_t *d_from = nullptr, *d_to = nullptr;
        float *d_six = nullptr, *moved = nullptr;
        double *sums = nullptr;
        HIP_TRY(scratch.upload(from.data(), M * 4, &d_from));
        HIP_TRY(scratch.upload(to.data(), M * 4, &d_to));
        HIP_TRY(scratch.alloc(M * 24, &d_six));
        std::vector<float> six(6 * M), mp(3 * M), mq(3 * M);
        if (M > 0) {
            hipLaunchKernelGGL(k_register_gather, grid_of(M), dim3(256), 0, 0, d_from, d_to, (uint32_t)M, own, target, d_six);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(six.data(), d_six, M * 24, hipMemcpyDeviceToHost));
        }
        for (size_t e = 0; e < M; ++e) {
            for (int a = 0; a < 3; ++a) {
                mp[3 * e + a] = six[6 * e + a];
                mq[3 * e + a] = six[6 * e + 3 + a];
            }
        }
        phase(kPhaseMatch);
        HIP_TRY(scratch.alloc(n * 12, &moved));
        HIP_TRY(scratch.alloc(chunks * (size_t)kAlignSums2 * 8, &sums));
        std::vector<double> host(chunks * (size_t)kAlignSums2);
        const auto count = [&](const std::vector<AlignMove> &moves, std::vector<uint32_t> &counts) -> int {
            phase(kPhaseTrials);
            Scratch of_count;
            const size_t A = moves.size();
            const AlignMove *d_moves = nullptr;
            uint32_t *d_counts = nullptr;
            HIP_TRY(of_count.upload(moves.data(), A * sizeof(AlignMove), &d_moves));
            HIP_TRY(of_count.alloc(A * 4, &d_counts));
            hipLaunchKernelGGL(k_register_count, dim3((unsigned)((A + kLanes - 1) / kLanes)), dim3(kLanes), 0, 0, d_moves, (uint32_t)A, d_six, (uint32_t)M, r2,
                               d_counts);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(counts.data(), d_counts, A * 4, hipMemcpyDeviceToHost));
            phase(kPhaseCount);
            return APD_OK;
        };
        const auto mark = [&](const AlignMove &by) -> int {
            hipLaunchKernelGGL(k_fill<int32_t>, grid_of(n), dim3(256), 0, 0, index, n, apd_fusion::kNearestNoIndex);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_register_mark, grid_of(M), dim3(256), 0, 0, d_from, d_to, (uint32_t)M, own, target, by, r2, index);
            HIP_TRY(hipGetLastError());
            return APD_OK;
        };
        const auto pass1 = [&](const AlignMove *by, double *s) -> int {
            const float *at = own;
            if (by) {
                if (const int rc = move(own, n, *by, moved); rc != APD_OK) {
                    return rc;
                }
                at = moved;
            }
            hipLaunchKernelGGL(k_align_sums1, dim3((unsigned)chunks), dim3(256), 0, 0, at, (const int32_t *)index, target, n, sums);
            HIP_TRY(hipGetLastError());
            return totals(sums, chunks, kAlignSums1, host, s);
        };
        const auto pass2 = [&](const double mean[6], double *s) -> int {
            AlignMeans about;
            for (int a = 0; a < 6; ++a) {
                about.mean[a] = mean[a];
            }
            hipLaunchKernelGGL(k_align_sums2, dim3((unsigned)chunks), dim3(256), 0, 0, own, (const int32_t *)index, target, n, about, sums);
            HIP_TRY(hipGetLastError());
            return totals(sums, chunks, kAlignSums2, host, s);
        };
        const int rc = apd_fusion::register_run(o, M, mp.data(), mq.data(), count, mark, pass1, pass2, out);
        phase(out.trials_admitted > 0 ? kPhaseRefit : kPhaseTrials);
        return rc;
    }
};

apd_fusion::RegisterOptions options_of(const apd_points_register_options *opt, float radius)
{
    if (!opt) {
        return {4096, 0, radius * 0.5f, 0.9f, 5, 1, 0};
    }
    return {opt->trials, opt->seed, opt->inlier_distance, opt->edge_ratio, opt->min_neighbours, opt->mutual, opt->with_scale};
}

int match_features(apd_points_t p, apd_points_t q, float radius, const float *origin3, unsigned min_neighbours, int mutual, unsigned long long pair_bound,
                   int32_t *index, float *distance)
{
    Call call{{{{"apd_points_match_features"}}}};
    call.pair_bound = pair_bound;
    const void *output = index ? (const void *)index : (const void *)distance;
    if (const int rc = call.check(p, output, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, q, output, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_neighbours(min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (pair_bound == 0) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a launch bound of 0 pairs", call.who);
    }
    if (const int rc = call.check_size(p); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_size(q); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    if (q->count == 0 && !p->on_device) {  // no device is touched
        for (long long k = 0; k < p->count; ++k) {
            if (index) {
                index[k] = apd_fusion::kNearestNoIndex;
            }
            if (distance) {
                distance[k] = apd_fusion::nearest_no_distance();
            }
        }
        return APD_OK;
    }
    DeviceScope scope(true);
    if (q->count == 0) {
        return call.no_matches(p, index, distance);
    }
    return call.match_of(p, q, mutual != 0, index, distance);
}

}  // namespace

extern "C" int apd_points_features(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *features, unsigned char *has)
{
    Call call{{{{"apd_points_features"}}}};
    if (const int rc = call.check(p, features, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_neighbours(min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.features_of(p, features, has);
}

extern "C" int apd_points_match_features(apd_points_t p, apd_points_t q, float radius, const float *origin3, unsigned min_neighbours, int mutual,
                                         int32_t *index, float *distance)
{
    return match_features(p, q, radius, origin3, min_neighbours, mutual, kMatchLaunchPairs, index, distance);
}

// Not declared in include/apd_mi355x.h and no part of the interface: for tools/points_register_time.py.  on != 0: from now on the
// calls of this file add their time per phase; the sums so far go to ms7 (may be null) -- the sort into cells, SPFH, FPFH, the
// match with its compaction and transfers, the trials on the host, the inlier count, the refit -- and start again from 0
extern "C" void apd_points_register_time_phases(int on, double *ms7)
{
    for (int k = 0; k < kPhases; ++k) {
        if (ms7) {
            ms7[k] = g_phase_ms[k];
        }
        g_phase_ms[k] = 0.0;
    }
    g_time_phases = on != 0;
    g_phase_start = std::chrono::steady_clock::now();
}

// Not declared in include/apd_mi355x.h and no part of the interface: apd_points_match_features with the largest number of (query,
// candidate) pairs of one kernel launch given by the caller (> 0) in place of kMatchLaunchPairs.  The results do not depend on it,
// which is what tests/test_gpu_points_register.py uses it for
extern "C" int apd_points_match_features_bounded(apd_points_t p, apd_points_t q, float radius, const float *origin3, unsigned min_neighbours, int mutual,
                                                 unsigned long long pair_bound, int32_t *index, float *distance)
{
    return match_features(p, q, radius, origin3, min_neighbours, mutual, pair_bound, index, distance);
}

extern "C" int apd_points_register(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_register_options *opt,
                                   apd_points_registration_t *out)
{
    Call call{{{{"apd_points_register"}}}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_other(p, q, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    const apd_fusion::RegisterOptions options = options_of(opt, radius);
    if (const int rc = call.check_neighbours(options.min_neighbours); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_options(options); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_size(p); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_size(q); rc != APD_OK) {
        return rc;
    }
    apd_fusion::Registration result = apd_fusion::register_identity(apd_fusion::kRegisterTooFewMatches);
    if (p->count > 0 && q->count > 0) {
        DeviceScope scope(true);
        if (const int rc = call.register_of(p, q, options, result); rc != APD_OK) {
            return rc;
        }
    }
    static_assert(sizeof(*out) == sizeof(result), "one layout");
    memcpy(out, &result, sizeof(result));
    return APD_OK;
}
