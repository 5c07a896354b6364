// apd_mesh_simplify.hip -- apd_mesh_simplify of include/apd_mi355x.h: a mesh thinned by vertex clustering on a cubic grid, each
// cluster's vertex placed at the members' mean or by the quadric of the faces around them (arithmetic contract C23; the
// rules: apd_simplify_math.h).  A new mesh on the input's device, on its null stream; the input stays as it is; there is no host
// path.  Everything is a function of the input alone: positions come from scans and stable sorts, every sum is walked by one lane
// in the contract's order, and there is no floating-point atomic.
//   1. Search::sort_into_cells: the vertices inside the grid as (key, vertex) pairs, sorted stably -- ascending key, ascending vertex
//      within a key -- with their positions gathered into that order.
//   2. k_simplify_heads, a scan, k_simplify_members: the first sorted position of every cluster (first[c], first[K] = the inside
//      count) and cluster_of[v] (kNoCluster outside the grid).
//   3. k_simplify_faces: per face its three clusters (mapped), whether it is live -- all inside, not degenerate --, the last entry of
//      its rotated triple as the key of the first face sort, and for QUADRIC the three corner pairs (cluster, 3 f + k), the key
//      kNoKey where the face names an outside vertex.
//   4. Duplicates: the rotated triple is 96 bits and a sort key 64, so the faces are sorted twice, stably: by the triple's last
//      entry, then (k_simplify_face_keys) by its first two; a face that is not live sorts behind every live one.  Always two sorts:
//      one path for every cluster count, and a pass over a digit that is the same in every key is skipped by the sort.
//      k_simplify_mark_duplicates: a live face whose predecessor in that order is live with the same rotated triple goes; the first of
//      a run of equals is the one with the smallest input index and stays.
//   5. QUADRIC: the corner pairs sorted stably by cluster, k_simplify_corner_starts: where each cluster's run starts.
//   6. k_simplify_place, one lane per cluster: the members in order for colour, the binary32 mean or the binary64 mean offset; for
//      QUADRIC the run of corners in ascending 3 f + k for the nine sums and the solve in the same lane.  A cluster of very many
//      members or corners is one long lane, accepted as in the voxel merge: the order of the sum is the contract.
//   7. MeshCall::compact (apd_mesh_compact.h) of the clusters as vertices and the mapped faces: the clusters a kept face names, in key
//      order, and the kept faces in input order, renumbered.
// No LDS, no scratch memory (profiles/mesh_simplify/kres.txt).
#include <hip/hip_runtime.h>

#include <math.h>

#include <chrono>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_simplify_math.h"
#include "apd_sort.h"

namespace {

using apd_mesh_compact::err;
using apd_mesh_compact::into_new_mesh;
using apd_mesh_compact::MeshCall;
using apd_mesh_compact::new_mesh_like;
using apd_points_grid::Grid;
using apd_points_grid::grid_of;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_points_search::k_fill;
using apd_points_search::Sorted;

constexpr uint32_t kNoRun = 0xFFFFFFFFu;
constexpr int32_t kNoCluster = -1;
constexpr uint64_t kNoKey = ~(uint64_t)0;  // above every cluster and every pair of clusters: clusters are fewer than 2^31

// Sorted position i < m: head[i] = 1 where a cluster starts
__global__ __launch_bounds__(256) void k_simplify_heads(const uint64_t *__restrict__ keys, size_t m, uint32_t *__restrict__ head)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    }
}

// Sorted position i < m, rank[i] = heads before i: cluster_of[member[i]], first[c] where c starts, first[clusters] = m
__global__ __launch_bounds__(256) void k_simplify_members(const uint32_t *__restrict__ head, const uint64_t *__restrict__ rank,
                                                           const uint32_t *__restrict__ member, size_t m, int32_t *__restrict__ cluster_of,
                                                           uint32_t *__restrict__ first)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) {
        return;
    }
    const size_t c = (size_t)rank[i] + head[i] - 1;
    cluster_of[member[i]] = (int32_t)c;
    if (head[i]) {
        first[c] = (uint32_t)i;
    }
    if (i == m - 1) {
        first[c + 1] = (uint32_t)m;
    }
}

// Face f < faces: mapped[3 f + k], live[f], the first sort's pair (the rotated triple's last entry, f); corner_key non-null: the
// pairs (cluster, 3 f + k) of its corners
__global__ __launch_bounds__(256) void k_simplify_faces(const int32_t *__restrict__ index, const int32_t *__restrict__ cluster_of, size_t faces,
                                                         int32_t *__restrict__ mapped, uint32_t *__restrict__ live, uint64_t *__restrict__ face_key,
                                                         uint32_t *__restrict__ face_val, uint64_t *__restrict__ corner_key,
                                                         uint32_t *__restrict__ corner_val)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    const int32_t a = cluster_of[index[3 * f]], b = cluster_of[index[3 * f + 1]], c = cluster_of[index[3 * f + 2]];
    const bool inside = a != kNoCluster && b != kNoCluster && c != kNoCluster;
    const bool alive = inside && !apd_fusion::mesh_face_degenerate(a, b, c);
    mapped[3 * f] = inside ? a : 0;
    mapped[3 * f + 1] = inside ? b : 0;
    mapped[3 * f + 2] = inside ? c : 0;
    live[f] = alive ? 1u : 0u;
    int32_t r[3];
    apd_fusion::simplify_rotated(a, b, c, r);
    face_key[f] = alive ? (uint64_t)(uint32_t)r[2] : kNoKey;
    face_val[f] = (uint32_t)f;
    if (corner_key) {
        corner_key[3 * f] = inside ? (uint64_t)(uint32_t)a : kNoKey;
        corner_key[3 * f + 1] = inside ? (uint64_t)(uint32_t)b : kNoKey;
        corner_key[3 * f + 2] = inside ? (uint64_t)(uint32_t)c : kNoKey;
        corner_val[3 * f] = (uint32_t)(3 * f);
        corner_val[3 * f + 1] = (uint32_t)(3 * f + 1);
        corner_val[3 * f + 2] = (uint32_t)(3 * f + 2);
    }
}

// Position p < faces of the first sort: the second sort's key of face val[p], the first two entries of its rotated triple
__global__ __launch_bounds__(256) void k_simplify_face_keys(const int32_t *__restrict__ mapped, const uint32_t *__restrict__ live,
                                                             const uint32_t *__restrict__ val, size_t faces, uint64_t *__restrict__ key)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= faces) {
        return;
    }
    const size_t f = val[p];
    int32_t r[3];
    apd_fusion::simplify_rotated(mapped[3 * f], mapped[3 * f + 1], mapped[3 * f + 2], r);
    key[p] = live[f] ? ((uint64_t)(uint32_t)r[0] << 32) | (uint64_t)(uint32_t)r[1] : kNoKey;
}

// Position p < faces of the second sort: keep[val[p]] = the face is live and not the duplicate of its predecessor
__global__ __launch_bounds__(256) void k_simplify_mark_duplicates(const int32_t *__restrict__ mapped, const uint32_t *__restrict__ live,
                                                                   const uint32_t *__restrict__ val, size_t faces, uint32_t *__restrict__ keep)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= faces) {
        return;
    }
    const size_t f = val[p];
    bool kept = live[f] != 0;
    if (kept && p > 0) {
        const size_t g = val[p - 1];
        if (live[g]) {
            int32_t r[3], q[3];
            apd_fusion::simplify_rotated(mapped[3 * f], mapped[3 * f + 1], mapped[3 * f + 2], r);
            apd_fusion::simplify_rotated(mapped[3 * g], mapped[3 * g + 1], mapped[3 * g + 2], q);
            kept = !(r[0] == q[0] && r[1] == q[1] && r[2] == q[2]);
        }
    }
    keep[f] = kept ? 1u : 0u;
}

// Sorted position p < corners: start[key[p]] = p where a cluster's run starts; start: kNoRun before, one entry per cluster
__global__ __launch_bounds__(256) void k_simplify_corner_starts(const uint64_t *__restrict__ key, size_t corners, uint32_t *__restrict__ start)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < corners && key[p] != kNoKey && (p == 0 || key[p] != key[p - 1])) {
        start[key[p]] = (uint32_t)p;
    }
}

// Cluster c < clusters: its position and colour by contract C23.  sorted_xyz, keys, member: the inside vertices in cluster order;
// corner_key / corner_val / corner_start: the sorted corners, read for APD_SIMPLIFY_QUADRIC alone
__global__ __launch_bounds__(256) void k_simplify_place(const float *__restrict__ sorted_xyz, const uint64_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ member, const uint32_t *__restrict__ first, size_t clusters,
                                                         const uint8_t *__restrict__ bgr, Grid grid, int placement, const float *__restrict__ xyz,
                                                         const int32_t *__restrict__ index, const uint64_t *__restrict__ corner_key,
                                                         const uint32_t *__restrict__ corner_val, size_t corners,
                                                         const uint32_t *__restrict__ corner_start, float *__restrict__ out_xyz,
                                                         uint8_t *__restrict__ out_bgr)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= clusters) {
        return;
    }
    const size_t begin = first[c], end = first[c + 1];
    const uint64_t m = end - begin;
    if (bgr) {
        uint64_t sum0 = 0, sum1 = 0, sum2 = 0;
        for (size_t i = begin; i < end; ++i) {
            const size_t v = member[i];
            sum0 += bgr[3 * v];
            sum1 += bgr[3 * v + 1];
            sum2 += bgr[3 * v + 2];
        }
        out_bgr[3 * c] = apd_fusion::simplify_colour(sum0, m);
        out_bgr[3 * c + 1] = apd_fusion::simplify_colour(sum1, m);
        out_bgr[3 * c + 2] = apd_fusion::simplify_colour(sum2, m);
    }
    if (placement == APD_SIMPLIFY_MEAN) {
        float s0 = sorted_xyz[3 * begin], s1 = sorted_xyz[3 * begin + 1], s2 = sorted_xyz[3 * begin + 2];
        for (size_t i = begin + 1; i < end; ++i) {
            s0 += sorted_xyz[3 * i];
            s1 += sorted_xyz[3 * i + 1];
            s2 += sorted_xyz[3 * i + 2];
        }
        const float count = (float)m;
        out_xyz[3 * c] = s0 / count;
        out_xyz[3 * c + 1] = s1 / count;
        out_xyz[3 * c + 2] = s2 / count;
        return;
    }
    int cell[3];
    apd_fusion::simplify_cell(keys[begin], cell);
    const double c0 = apd_fusion::simplify_centre(grid.origin[0], cell[0], grid.size);
    const double c1 = apd_fusion::simplify_centre(grid.origin[1], cell[1], grid.size);
    const double c2 = apd_fusion::simplify_centre(grid.origin[2], cell[2], grid.size);
    double mu0 = 0.0, mu1 = 0.0, mu2 = 0.0;
    for (size_t i = begin; i < end; ++i) {
        const double d0 = (double)sorted_xyz[3 * i] - c0, d1 = (double)sorted_xyz[3 * i + 1] - c1, d2 = (double)sorted_xyz[3 * i + 2] - c2;
        mu0 = mu0 + d0;
        mu1 = mu1 + d1;
        mu2 = mu2 + d2;
    }
    const double count = (double)m;
    mu0 = mu0 / count;
    mu1 = mu1 / count;
    mu2 = mu2 / count;
    apd_fusion::SimplifySums sums;
    const uint32_t from = corner_start[c];
    for (size_t p = from; from != kNoRun && p < corners && corner_key[p] == (uint64_t)c; ++p) {
        const size_t f = corner_val[p] / 3u;
        const float *A = xyz + 3 * (size_t)index[3 * f], *B = xyz + 3 * (size_t)index[3 * f + 1], *C = xyz + 3 * (size_t)index[3 * f + 2];
        apd_fusion::simplify_add(sums, A, B, C, c0, c1, c2);
    }
    double x0, x1, x2;
    apd_fusion::simplify_place(sums, mu0, mu1, mu2, grid.size, x0, x1, x2);
    out_xyz[3 * c] = (float)(c0 + x0);
    out_xyz[3 * c + 1] = (float)(c1 + x1);
    out_xyz[3 * c + 2] = (float)(c2 + x2);
}

struct Call : MeshCall {
    // apd_mesh_simplify of m (with vertices; 3 * faces < 2^32) into `out`, which has colour as m and no normals
    int simplify(const apd_mesh *m, int placement, apd_mesh *out) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces, corners = 3 * nf;
        if (nf == 0) {
            return APD_OK;  // no face names a cluster
        }
        const bool quadric = placement == APD_SIMPLIFY_QUADRIC;
        Scratch scratch;
        int32_t *cluster_of = nullptr, *mapped = nullptr;
        uint32_t *live = nullptr, *keep_face = nullptr, *face_val[2] = {nullptr, nullptr}, *corner_val[2] = {nullptr, nullptr};
        uint64_t *face_key[2] = {nullptr, nullptr}, *corner_key[2] = {nullptr, nullptr};
        HIP_TRY(scratch.alloc(nv * 4, &cluster_of));
        HIP_TRY(scratch.alloc(nf * 12, &mapped));
        HIP_TRY(scratch.alloc(nf * 4, &live));
        HIP_TRY(scratch.alloc(nf * 4, &keep_face));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(scratch.alloc(nf * 8, &face_key[b]));
            HIP_TRY(scratch.alloc(nf * 4, &face_val[b]));
            if (quadric) {
                HIP_TRY(scratch.alloc(corners * 8, &corner_key[b]));
                HIP_TRY(scratch.alloc(corners * 4, &corner_val[b]));
            }
        }
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        const int rc = clustered(scratch, m, placement, cluster_of, mapped, live, keep_face, face_key, face_val, corner_key, corner_val, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return rc;
    }

    int clustered(Scratch &scratch, const apd_mesh *m, int placement, int32_t *cluster_of, int32_t *mapped, uint32_t *live, uint32_t *keep_face,
                  uint64_t *face_key[2], uint32_t *face_val[2], uint64_t *corner_key[2], uint32_t *corner_val[2], apd_mesh *out) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces, corners = 3 * nf;
        const bool quadric = placement == APD_SIMPLIFY_QUADRIC;
        Sorted s;
        if (const int rc = sort_into_cells(scratch, m->xyz, nv, s); rc != APD_OK) {
            return rc;
        }
        if (s.m == 0) {
            return APD_OK;  // every vertex is outside the grid
        }
        uint32_t *head = nullptr, *first = nullptr, *corner_start = nullptr;
        uint64_t *rank = nullptr;
        HIP_TRY(scratch.alloc(s.m * 4, &head));
        HIP_TRY(scratch.alloc((s.m + 1) * 8, &rank));
        hipLaunchKernelGGL(k_simplify_heads, grid_of(s.m), dim3(256), 0, 0, s.keys, s.m, head);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(head, rank, s.m));
        uint64_t found = 0;
        HIP_TRY(hipMemcpy(&found, rank + s.m, 8, hipMemcpyDeviceToHost));
        const size_t clusters = (size_t)found;  // >= 1
        HIP_TRY(scratch.alloc((clusters + 1) * 4, &first));
        hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(nv), dim3(256), 0, 0, (uint32_t *)cluster_of, nv, (uint32_t)kNoCluster);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_simplify_members, grid_of(s.m), dim3(256), 0, 0, (const uint32_t *)head, (const uint64_t *)rank, s.member, s.m, cluster_of,
                           first);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_simplify_faces, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (const int32_t *)cluster_of, nf, mapped, live,
                           face_key[0], face_val[0], corner_key[0], corner_val[0]);
        HIP_TRY(hipGetLastError());
        // the faces by their rotated triple: its last entry, then its first two
        int side = 0, turned = 0;
        HIP_TRY(apd_sort::sort_pairs(face_key[0], face_key[1], face_val[0], face_val[1], nf, &side, nullptr));
        hipLaunchKernelGGL(k_simplify_face_keys, grid_of(nf), dim3(256), 0, 0, (const int32_t *)mapped, (const uint32_t *)live,
                           (const uint32_t *)face_val[side], nf, face_key[side]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::sort_pairs(face_key[side], face_key[1 - side], face_val[side], face_val[1 - side], nf, &turned, nullptr));
        side = turned ? 1 - side : side;
        hipLaunchKernelGGL(k_simplify_mark_duplicates, grid_of(nf), dim3(256), 0, 0, (const int32_t *)mapped, (const uint32_t *)live,
                           (const uint32_t *)face_val[side], nf, keep_face);
        HIP_TRY(hipGetLastError());
        int corner_side = 0;
        if (quadric) {
            HIP_TRY(scratch.alloc(clusters * 4, &corner_start));
            HIP_TRY(apd_sort::sort_pairs(corner_key[0], corner_key[1], corner_val[0], corner_val[1], corners, &corner_side, nullptr));
            hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(clusters), dim3(256), 0, 0, corner_start, clusters, kNoRun);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_simplify_corner_starts, grid_of(corners), dim3(256), 0, 0, (const uint64_t *)corner_key[corner_side], corners,
                               corner_start);
            HIP_TRY(hipGetLastError());
        }
        // the clusters as the vertices of a mesh with the mapped faces: what the compaction takes
        apd_mesh all;
        all.device = m->device;
        all.vertices = (long long)clusters;
        all.faces = m->faces;
        all.colour = m->colour;
        all.index = mapped;
        HIP_TRY(scratch.alloc(clusters * 12, &all.xyz));
        if (m->colour) {
            HIP_TRY(scratch.alloc(clusters * 3, &all.bgr));
        }
        hipLaunchKernelGGL(k_simplify_place, grid_of(clusters), dim3(256), 0, 0, s.xyz, s.keys, s.member, (const uint32_t *)first, clusters,
                           (const uint8_t *)m->bgr, grid, placement, (const float *)m->xyz, (const int32_t *)m->index,
                           (const uint64_t *)corner_key[corner_side], (const uint32_t *)corner_val[corner_side], corners,
                           (const uint32_t *)corner_start, all.xyz, all.bgr);
        HIP_TRY(hipGetLastError());
        return compact(scratch, &all, mapped, keep_face, out);
    }
};

}  // namespace

extern "C" int apd_mesh_simplify(apd_mesh_t m, float cell, const float *origin3, int placement, apd_mesh_t *out, long long *removed_vertices,
                                 long long *removed_faces)
{
    Call call{{{"apd_mesh_simplify"}}};
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    if (!(isfinite(cell) && cell > 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a cell of %g, not a positive finite number", call.who, (double)cell);
    }
    call.grid.size = cell;
    for (int a = 0; origin3 && a < 3; ++a) {
        if (!isfinite(origin3[a])) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: origin component %d is %g", call.who, a, (double)origin3[a]);
        }
        call.grid.origin[a] = origin3[a];
    }
    if (placement != APD_SIMPLIFY_MEAN && placement != APD_SIMPLIFY_QUADRIC) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: placement %d, neither APD_SIMPLIFY_MEAN nor APD_SIMPLIFY_QUADRIC", call.who, placement);
    }
    if (3 * m->faces >= (1LL << 32)) {
        return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld faces, whose 3 corners each are 2^32 or more (the sort carries a 32-bit corner)", call.who,
                              m->faces);
    }
    apd_mesh *like = new_mesh_like(m);
    like->normals = 0;
    apd_mesh_t result = nullptr;
    const int rc = into_new_mesh(m, like, &result, [&](apd_mesh *r) { return call.simplify(m, placement, r); });
    if (rc != APD_OK) {
        return rc;
    }
    *out = result;
    if (removed_vertices) {
        *removed_vertices = m->vertices - result->vertices;
    }
    if (removed_faces) {
        *removed_faces = m->faces - result->faces;
    }
    return APD_OK;
}
