// apd_mesh_nearest.hip -- apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score of include/apd_mi355x.h: the closest point of a
// mesh's surface for every point of a cloud, points drawn on the surface by area, and the precision / recall / F-score of a surface
// against a ground-truth cloud (arithmetic contract C27; the rules: apd_mesh_nearest_math.h).  The first search here that
// is point against triangle; it stands on the walk and the host frame of apd_points_search.h like the six point searches.
//
// apd_mesh_nearest, on the mesh's device, on its null stream:
//   1. k_mesh_face_records, one lane per face: the nine coordinates of a face that can be a candidate at all (distinct indices,
//      finite, on the grid, a cross product that is not zero) as one record of 36 bytes, and the number of cells it is binned into:
//      those of its bounding box on the grid, one more on a side whose corner stands within binary32 rounding of a cell boundary
//      (mesh_cell_range: with it the walk of the 27 cells meets every candidate, apd_mesh_nearest_math.h), 0 for any other face,
//      capped at 2^31 (a face may span 2^21 cells per axis: mesh_face_cells).
//   2. apd_sort::exclusive_scan of the counts; the total comes down and is held against the pair limit.
//   3. k_mesh_emit_pairs, one lane per face: (cell key, face) for every cell of the box, at the scan's positions.
//   4. one stable apd_sort::sort_pairs of the pairs by key.
//   5. Search::sort_into_cells of the queries.
//   6. k_mesh_nearest: one lane per query in the QUERIES' sorted order, so that the lanes of a wave mostly share their cell and with
//      it the nine rows of pairs they walk (for_each_position_around: the walk of the point searches, handing out a position); per
//      pair the face's record is read -- ONE dependent load of 36 consecutive bytes through the face id, where the mesh's own layout
//      costs three indices and then three vertices at unrelated addresses -- and the closest point computed in binary64; (best d2,
//      best face, best point) stay in registers, a face met in several cells is evaluated again and the tie rule makes that
//      harmless; the result goes to the query's input index.  No atomics, no LDS, no array indexed by a runtime value, no scratch
//      memory (profiles/mesh_score/kres.txt).
// The record per face in face order is the only layout that was built and timed (profiles/mesh_score/timing.txt); a record per PAIR
// in pair order (no dependent load at all, 36 bytes a pair instead of 4) was not tried, so the choice between the two is
// unverified by measurement: it rests on the memory of the call, which the other layout multiplies by nine.
// apd_mesh_sample_points: k_mesh_sample_counts (one lane per face: n_f), the scan, k_mesh_sample_emit (one lane per SAMPLE, which
// finds its face by a binary search of the scan, so that a large face is not one lane's loop).
// apd_mesh_score: the samples against the truth by k_nearest_in (apd_points_nearest.h), the truth against the surface by steps 1-6 on
// the one sort of the truth, and of both lists of distances only the chunk sums of contract C12 come down.
// There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>

#include <atomic>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_host.h"
#include "apd_mesh_nearest_math.h"
#include "apd_nearest_math.h"
#include "apd_points_host.h"
#include "apd_points_nearest.h"
#include "apd_points_search.h"
#include "apd_sort.h"

namespace {

using apd_fusion::MeshFace;
using apd_nearest_search::NearestSearch;
using apd_points_grid::Grid;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_points_search::err;
using apd_points_search::for_each_position_around;
using apd_points_search::k_fill;
using apd_points_search::Sorted;
using apd_points_search::Staged;

static_assert(sizeof(apd_points_score_t) == sizeof(apd_fusion::NearestScore), "apd_points_score_t is NearestScore");

constexpr long long kPairLimit = 1LL << 31;  // the walk and the sort carry 32-bit positions
std::atomic<long long> g_pair_limit{0};      // > 0: apd_mesh_nearest_pair_limit's

// the corners of face f
__device__ __forceinline__ void face_corners(const int32_t *__restrict__ index, const float *__restrict__ xyz, size_t f, int32_t id[3], float A[3],
                                             float B[3], float C[3])
{
    for (int c = 0; c < 3; ++c) {
        id[c] = index[3 * f + c];
    }
    for (int a = 0; a < 3; ++a) {
        A[a] = xyz[3 * (size_t)id[0] + a];
        B[a] = xyz[3 * (size_t)id[1] + a];
        C[a] = xyz[3 * (size_t)id[2] + a];
    }
}

// Face f < faces: record[9 f ..] = its corners and cells[f] = the cells of its bounding box (capped), or cells[f] = 0 for a face that
// is nobody's candidate (its record is then not written and never read)
__global__ __launch_bounds__(256) void k_mesh_face_records(const int32_t *__restrict__ index, const float *__restrict__ xyz, size_t faces, Grid grid,
                                                            float *__restrict__ record, uint32_t *__restrict__ cells)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    int32_t id[3];
    float A[3], B[3], C[3];
    face_corners(index, xyz, f, id, A, B, C);
    int lo[3], hi[3];
    if (!apd_fusion::mesh_face_proper(id, A, B, C) || !apd_fusion::mesh_face_on_grid(A, B, C, grid.origin, grid.size, lo, hi)) {
        cells[f] = 0u;
        return;
    }
    for (int a = 0; a < 3; ++a) {
        record[9 * f + a] = A[a];
        record[9 * f + 3 + a] = B[a];
        record[9 * f + 6 + a] = C[a];
    }
    cells[f] = apd_fusion::mesh_face_cells(lo, hi);
}

// Face f < faces with cells[f] > 0: its (cell key, f) pairs at positions at[f] .. at[f] + cells[f] - 1, all below `pairs`
__global__ __launch_bounds__(256) void k_mesh_emit_pairs(const float *__restrict__ record, const uint32_t *__restrict__ cells,
                                                          const uint64_t *__restrict__ at, size_t faces, Grid grid, uint64_t pairs,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ face)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces || cells[f] == 0u) {
        return;
    }
    const float *r = record + 9 * f;
    const float A[3] = {r[0], r[1], r[2]}, B[3] = {r[3], r[4], r[5]}, C[3] = {r[6], r[7], r[8]};
    int lo[3], hi[3];
    if (!apd_fusion::mesh_face_on_grid(A, B, C, grid.origin, grid.size, lo, hi)) {
        return;  // cells[f] > 0 says it is
    }
    uint64_t to = at[f];
    const uint64_t end = to + cells[f] < pairs ? to + cells[f] : pairs;
    for (int z = lo[2]; z <= hi[2]; ++z) {
        for (int y = lo[1]; y <= hi[1]; ++y) {
            for (int x = lo[0]; x <= hi[0] && to < end; ++x, ++to) {
                keys[to] = apd_fusion::radius_key(x, y, z);
                face[to] = (uint32_t)f;
            }
        }
    }
}

// Sorted query i < m with a candidate among the faces: distance, face and closest (any may be null) at its input index member[i] by
// contract C27; the others keep what they have.  keys / xyz / member: the queries in cell order; pair_keys / pair_face: the
// `pairs` > 0 (cell, face) pairs in key order on the same grid; record: nine floats per face
__global__ __launch_bounds__(256) void k_mesh_nearest(const uint64_t *__restrict__ keys, const float *__restrict__ xyz, const uint32_t *__restrict__ member,
                                                       uint32_t m, const uint64_t *__restrict__ pair_keys, const uint32_t *__restrict__ pair_face,
                                                       uint32_t pairs, const float *__restrict__ record, double r2, float *__restrict__ distance,
                                                       int32_t *__restrict__ face, float *__restrict__ closest)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const double P[3] = {(double)xyz[3 * (size_t)i], (double)xyz[3 * (size_t)i + 1], (double)xyz[3 * (size_t)i + 2]};
    int cell[3];
    apd_fusion::radius_cells_of_key(keys[i], cell);
    bool have = false;
    double best = 0.0, best_x[3] = {0.0, 0.0, 0.0};
    uint32_t best_f = 0;
    for_each_position_around(pair_keys, cell, pairs, [&](uint32_t at) {
        const uint32_t f = pair_face[at];
        const float *r = record + 9 * (size_t)f;
        MeshFace t;
        for (int a = 0; a < 3; ++a) {
            t.a[a] = (double)r[a];
            t.b[a] = (double)r[3 + a];
            t.c[a] = (double)r[6 + a];
        }
        double X[3];
        const double d2 = apd_fusion::mesh_closest_point(t, P, X);
        if (d2 <= r2 && apd_fusion::mesh_nearest_takes(d2, f, have, best, best_f)) {
            have = true;
            best = d2;
            best_f = f;
            best_x[0] = X[0];
            best_x[1] = X[1];
            best_x[2] = X[2];
        }
        return false;
    });
    if (!have) {
        return;  // the fill
    }
    const size_t k = member[i];
    if (distance) {
        distance[k] = apd_fusion::mesh_nearest_distance(best);
    }
    if (face) {
        face[k] = (int32_t)best_f;  // fewer than 2^31 faces
    }
    if (closest) {
        closest[3 * k] = (float)best_x[0];
        closest[3 * k + 1] = (float)best_x[1];
        closest[3 * k + 2] = (float)best_x[2];
    }
}

// Face f < faces: count[f] = its samples n_f, kMeshSampleCap for 2^31 or more
__global__ __launch_bounds__(256) void k_mesh_sample_counts(const int32_t *__restrict__ index, const float *__restrict__ xyz, size_t faces, double density,
                                                             unsigned long long seed, uint32_t *__restrict__ count)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    int32_t id[3];
    float A[3], B[3], C[3];
    face_corners(index, xyz, f, id, A, B, C);
    uint32_t n = 0u;
    if (apd_fusion::mesh_face_proper(id, A, B, C)) {
        double normal[3];
        const double n2 = apd_fusion::mesh_face_area2(apd_fusion::mesh_face_of(A, B, C), normal);
        n = apd_fusion::mesh_sample_count(n2, density, apd_fusion::mesh_sample_unit(seed, (uint64_t)f, 0, 0));
    }
    count[f] = n;
}

// Sample s < total: it is sample s - at[f] of the face f with at[f] <= s < at[f + 1] (at: faces + 1 entries, the scan of the counts)
__global__ __launch_bounds__(256) void k_mesh_sample_emit(const int32_t *__restrict__ index, const float *__restrict__ xyz, const uint8_t *__restrict__ bgr,
                                                           const uint64_t *__restrict__ at, size_t faces, size_t total, unsigned long long seed,
                                                           float *__restrict__ out_xyz, float *__restrict__ out_normal, uint8_t *__restrict__ out_bgr,
                                                           int32_t *__restrict__ out_face)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= total) {
        return;
    }
    size_t lo = 0, hi = faces - 1;  // the first f with at[f + 1] > s: at[faces] = total > s, so there is one
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (at[mid + 1] > s) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    const size_t f = lo;
    int32_t id[3];
    float A[3], B[3], C[3];
    face_corners(index, xyz, f, id, A, B, C);
    float position[3], normal[3];
    uint8_t colour[3];
    apd_fusion::mesh_sample_point(apd_fusion::mesh_face_of(A, B, C), seed, (uint64_t)f, (uint64_t)(s - at[f]), bgr ? bgr + 3 * (size_t)id[0] : nullptr,
                                  bgr ? bgr + 3 * (size_t)id[1] : nullptr, bgr ? bgr + 3 * (size_t)id[2] : nullptr, position, normal, colour);
    for (int a = 0; a < 3; ++a) {
        out_xyz[3 * s + a] = position[a];
        out_normal[3 * s + a] = normal[a];
        out_bgr[3 * s + a] = colour[a];
    }
    out_face[s] = (int32_t)f;
}

// One call of an entry point
struct Call : NearestSearch {
    int invalid(const char *what) const { return apd::set_error(err(), APD_ERR_INVALID, "%s: %s", who, what); }

    // What the calls with a points object refuse on top of Search::check of it
    int check_mesh(apd_mesh_t m, apd_points_t p) const
    {
        if (!m) {
            return invalid("null argument");
        }
        if (p->on_device && p->device != m->device) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: the points live on device %d, the computation runs on the mesh's device %d", who,
                                  p->device, m->device);
        }
        return APD_OK;
    }

    // The answers of the n > 0 queries of which q holds those inside the grid, against the surface of m, whose device is the
    // current one: distance and face n entries each, closest 3 n, device memory, any may be null
    int surface(const apd_mesh *m, const Sorted &q, size_t n, float *distance, int32_t *face, float *closest) const
    {
        auto t0 = std::chrono::steady_clock::now();
        const size_t nf = (size_t)m->faces;
        const bool searching = nf > 0 && q.m > 0;
        Scratch scratch;
        float *record = nullptr;
        uint32_t *cells = nullptr;
        uint64_t *at = nullptr, total = 0;
        if (searching) {  // the counting pass first: a call refused at the pair limit has written nothing
            HIP_TRY(scratch.alloc(nf * 36, &record));
            HIP_TRY(scratch.alloc(nf * 4, &cells));
            HIP_TRY(scratch.alloc((nf + 1) * 8, &at));
            hipLaunchKernelGGL(k_mesh_face_records, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (const float *)m->xyz, nf, grid, record, cells);
            HIP_TRY(hipGetLastError());
            HIP_TRY(apd_sort::exclusive_scan(cells, at, nf));
            HIP_TRY(hipMemcpy(&total, at + nf, 8, hipMemcpyDeviceToHost));
            const long long chosen = g_pair_limit.load();
            const long long limit = chosen > 0 && chosen < kPairLimit ? chosen : kPairLimit;
            if (total >= (uint64_t)limit) {
                return apd::set_error(err(), APD_ERR_UNSUPPORTED,
                                      "%s: %llu (cell, face) pairs at a radius of %g, %lld or more: the faces are put into every cell of size radius that "
                                      "their bounding boxes overlap; take a larger radius, or apd_mesh_simplify or a subdivision of the large faces first",
                                      who, (unsigned long long)total, (double)grid.size, limit);
            }
        }
        if (distance) {
            hipLaunchKernelGGL(k_fill<float>, grid_of(n), dim3(256), 0, 0, distance, n, apd_fusion::nearest_no_distance());
            HIP_TRY(hipGetLastError());
        }
        if (face) {
            hipLaunchKernelGGL(k_fill<int32_t>, grid_of(n), dim3(256), 0, 0, face, n, apd_fusion::kMeshNearestNoFace);
            HIP_TRY(hipGetLastError());
        }
        if (closest) {
            hipLaunchKernelGGL(k_fill<float>, grid_of(3 * n), dim3(256), 0, 0, closest, 3 * n, (float)NAN);
            HIP_TRY(hipGetLastError());
        }
        if (total == 0) {
            return APD_OK;  // no face can be a candidate
        }
        uint64_t *keys[2] = {nullptr, nullptr};
        uint32_t *faces[2] = {nullptr, nullptr};
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(scratch.alloc((size_t)total * 8, &keys[b]));
            HIP_TRY(scratch.alloc((size_t)total * 4, &faces[b]));
        }
        hipLaunchKernelGGL(k_mesh_emit_pairs, grid_of(nf), dim3(256), 0, 0, (const float *)record, (const uint32_t *)cells, (const uint64_t *)at, nf, grid,
                           total, keys[0], faces[0]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        int side = 0;
        HIP_TRY(apd_sort::sort_pairs(keys[0], keys[1], faces[0], faces[1], (size_t)total, &side, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        apd_fusion::g_fusion_ms[1] += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_mesh_nearest, grid_of(q.m), dim3(256), 0, 0, q.keys, q.xyz, q.member, (uint32_t)q.m, (const uint64_t *)keys[side],
                           (const uint32_t *)faces[side], (uint32_t)total, (const float *)record, apd_fusion::mesh_nearest_r2(grid.size), distance, face,
                           closest);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // before the pairs' memory goes
        apd_fusion::g_fusion_ms[2] = ms_since(t0);
        return APD_OK;
    }

    // apd_mesh_nearest of p (count > 0)
    int nearest_of(const apd_mesh *m, apd_points_t p, float *distance, int32_t *face, float *closest) const
    {
        const size_t n = (size_t)p->count;
        HIP_TRY(hipSetDevice(m->device));
        Scratch scratch;
        const float *xyz = nullptr;
        Sorted sp;
        Staged<float> out_distance, out_closest;
        Staged<int32_t> out_face;
        int rc = readable(scratch, p, (const float *)p->arrays.xyz, n * 12, &xyz);
        const auto t0 = std::chrono::steady_clock::now();
        rc = rc != APD_OK ? rc : sort_into_cells(scratch, xyz, n, sp);
        if (rc == APD_OK) {
            HIP_TRY(hipDeviceSynchronize());
            apd_fusion::g_fusion_ms[1] = ms_since(t0);  // surface() adds the pairs' sort
        }
        rc = rc != APD_OK ? rc : stage(scratch, p, distance, n * 4, out_distance);
        rc = rc != APD_OK ? rc : stage(scratch, p, face, n * 4, out_face);
        rc = rc != APD_OK ? rc : stage(scratch, p, closest, n * 12, out_closest);
        rc = rc != APD_OK ? rc : surface(m, sp, n, out_distance.device, out_face.device, out_closest.device);
        if (rc != APD_OK) {
            return rc;
        }
        HIP_TRY(hipDeviceSynchronize());
        rc = download(out_distance);
        rc = rc != APD_OK ? rc : download(out_face);
        return rc != APD_OK ? rc : download(out_closest);
    }

    // apd_mesh_sample_points of m (with faces) into `result` (no arrays so far); face: null, or host memory for every sample
    int sample_into(const apd_mesh *m, double density, unsigned long long seed, apd_points *result, int32_t *face) const
    {
        HIP_TRY(hipSetDevice(m->device));
        const size_t nf = (size_t)m->faces;
        Scratch scratch, made;
        uint32_t *count = nullptr;
        uint64_t *at = nullptr, total = 0;
        HIP_TRY(scratch.alloc(nf * 4, &count));
        HIP_TRY(scratch.alloc((nf + 1) * 8, &at));
        hipLaunchKernelGGL(k_mesh_sample_counts, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (const float *)m->xyz, nf, density, seed, count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(count, at, nf));
        HIP_TRY(hipMemcpy(&total, at + nf, 8, hipMemcpyDeviceToHost));
        if (total >= (1ull << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %llu samples or more at a density of %g, 2^31 or more (a points object carries a 32-bit index)",
                                  who, (unsigned long long)total, density);
        }
        if (total == 0) {
            return APD_OK;
        }
        const size_t n = (size_t)total;
        apd_fusion::PointArrays device;
        int32_t *faces = nullptr;
        HIP_TRY(apd_fusion::alloc_arrays(made, device, n));
        HIP_TRY(scratch.alloc(n * 4, &faces));
        HIP_TRY(hipMemsetAsync(device.support, 0, n, 0));
        HIP_TRY(hipMemsetAsync(device.view, 0, n * 4, 0));
        HIP_TRY(hipMemsetAsync(device.pixel, 0, n * 4, 0));
        HIP_TRY(hipMemsetAsync(device.sources, 0, n * 4, 0));
        hipLaunchKernelGGL(k_mesh_sample_emit, grid_of(n), dim3(256), 0, 0, (const int32_t *)m->index, (const float *)m->xyz,
                           (const uint8_t *)(m->colour ? m->bgr : nullptr), (const uint64_t *)at, nf, n, seed, device.xyz, device.normal, device.bgr, faces);
        HIP_TRY(hipGetLastError());
        if (face) {
            HIP_TRY(hipMemcpy(face, faces, n * 4, hipMemcpyDeviceToHost));
        }
        HIP_TRY(hipDeviceSynchronize());
        if (result->on_device) {
            apd_fusion::keep_arrays(made, device);
            result->arrays = device;
        } else {
            apd_fusion::PointArrays host;
            if (!apd_fusion::alloc_host_arrays(host, n)) {
                apd_fusion::free_arrays(host, false);
                return apd::set_error(err(), APD_ERR_HIP, "%s: no host memory for %zu samples", who, n);
            }
            if (const hipError_t e = apd_fusion::copy_arrays(host, device, n, hipMemcpyDeviceToHost); e != hipSuccess) {
                apd_fusion::free_arrays(host, false);
                return hip_failed("copy_arrays", e, __FILE__, __LINE__);
            }
            result->arrays = host;
        }
        result->count = (long long)n;
        return APD_OK;
    }

    // The new points object of apd_mesh_sample_points; on failure the message is set and *out is untouched
    int samples(const apd_mesh *m, double density, unsigned long long seed, int on_device, apd_points_t *out, int32_t *face) const
    {
        const int rows[1] = {1}, cols[1] = {1}, pair_offsets[2] = {0, 0};  // apd_points_read_ply's: one view of 1 x 1 without sources
        apd_points *result = apd_points_host::new_points(m->device, on_device, 1, rows, cols, pair_offsets, pair_offsets);
        if (m->faces > 0) {  // a mesh without faces has no surface: no device is touched
            DeviceScope scope(true);
            if (const int rc = sample_into(m, density, seed, result, face); rc != APD_OK) {
                const std::string why = err();
                apd_points_destroy(result);  // it has no arrays yet
                err() = why;
                return rc;
            }
        }
        *out = result;
        return APD_OK;
    }

    // The finite ones of the n > 0 distances at `distance`: their number and their binary64 sum in contract C12's order
    int finite(const float *distance, size_t n, unsigned long long *count, double *sum) const { return chunk_totals(distance, n, sum, nullptr, count); }

    // apd_mesh_score of m against truth (count > 0) with the samples s, which live on m's device
    int score_of(const apd_mesh *m, apd_points_t s, apd_points_t truth, apd_points_score_t *out) const
    {
        HIP_TRY(hipSetDevice(m->device));
        const size_t ns = (size_t)s->count, nt = (size_t)truth->count;
        Scratch scratch;
        const float *xyz = nullptr;
        Sorted ss, st;
        float *distance = nullptr;
        unsigned long long a = 0, b = 0;
        double sum_p = 0.0, sum_q = 0.0;
        int rc = readable(scratch, truth, (const float *)truth->arrays.xyz, nt * 12, &xyz);
        rc = rc != APD_OK ? rc : sort_into_cells(scratch, xyz, nt, st);
        rc = rc != APD_OK ? rc : sorted(scratch, (const float *)s->arrays.xyz, ns, ss);
        if (rc != APD_OK) {
            return rc;
        }
        HIP_TRY(scratch.alloc((ns > nt ? ns : nt) * 4, &distance));
        if (ns > 0) {
            rc = search(ss, ns, st, distance, nullptr);
            rc = rc != APD_OK ? rc : finite(distance, ns, &a, &sum_p);
        }
        rc = rc != APD_OK ? rc : surface(m, st, nt, distance, nullptr, nullptr);
        rc = rc != APD_OK ? rc : finite(distance, nt, &b, &sum_q);
        if (rc != APD_OK) {
            return rc;
        }
        HIP_TRY(hipDeviceSynchronize());  // before the sorts' memory goes
        set(out, apd_fusion::nearest_score((unsigned long long)ns, (unsigned long long)nt, a, b, sum_p, sum_q));
        return APD_OK;
    }

    static void set(apd_points_score_t *out, const apd_fusion::NearestScore &s)
    {
        *out = {s.n_p, s.n_q, s.p_within, s.q_within, s.precision, s.recall, s.fscore, s.mean_p, s.mean_q};
    }
};

void clear_timing() { apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0; }

}  // namespace

// The number of (cell, face) pairs at which apd_mesh_nearest refuses: pairs > 0 sets it (2^31 at the most), 0 restores 2^31.  The
// results do not depend on it: it exists so that a test reaches the refusal with a dozen faces
extern "C" void apd_mesh_nearest_pair_limit(long long pairs) { g_pair_limit.store(pairs > 0 ? pairs : 0); }

extern "C" int apd_mesh_device(apd_mesh_t m) { return m ? m->device : -1; }

extern "C" int apd_mesh_nearest(apd_mesh_t m, apd_points_t p, float radius, const float *origin3, float *distance, int32_t *face, float *closest3)
{
    Call call{{"apd_mesh_nearest"}};
    const void *output = distance ? (const void *)distance : face ? (const void *)face : (const void *)closest3;
    if (const int rc = call.check(p, output, radius, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_mesh(m, p); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    if (p->count == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.nearest_of(m, p, distance, face, closest3);
}

extern "C" int apd_mesh_sample_points(apd_mesh_t m, double density, unsigned long long seed, int on_device, apd_points_t *out, int32_t *face)
{
    const Call call{{"apd_mesh_sample_points"}};
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    if (!(isfinite(density) && density > 0.0)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a density of %g, not a positive finite number", call.who, density);
    }
    clear_timing();
    return call.samples(m, density, seed, on_device, out, face);
}

extern "C" int apd_mesh_score(apd_mesh_t m, apd_points_t truth, float threshold, const float *origin3, double density, unsigned long long seed,
                              apd_points_score_t *out)
{
    Call call{{"apd_mesh_score"}};
    if (const int rc = call.check(truth, out, threshold, origin3); rc != APD_OK) {
        return rc;
    }
    if (const int rc = call.check_mesh(m, truth); rc != APD_OK) {
        return rc;
    }
    if (!isfinite(density)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a density of %g, not a finite number", call.who, density);
    }
    if (!(density > 0.0)) {
        density = 4.0 / ((double)threshold * (double)threshold);
    }
    clear_timing();
    apd_points_t drawn = nullptr;
    if (const int rc = call.samples(m, density, seed, 1, &drawn, nullptr); rc != APD_OK) {
        return rc;
    }
    int rc = APD_OK;
    if (truth->count == 0) {  // no distance is finite: the counts, and zeros
        Call::set(out, apd_fusion::nearest_score((unsigned long long)drawn->count, 0, 0, 0, 0.0, 0.0));
    } else {
        DeviceScope scope(true);
        apd_points_score_t found;
        rc = call.score_of(m, drawn, truth, &found);
        if (rc == APD_OK) {
            *out = found;
        }
    }
    const std::string why = err();
    apd_points_destroy(drawn);
    err() = why;
    return rc;
}
