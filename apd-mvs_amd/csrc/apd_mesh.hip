// apd_mesh.hip -- the apd_mesh_* calls of include/apd_mi355x.h: the life and the files of the mesh object, and what is done to a
// mesh once it exists -- welding of close vertices, the connected components of its faces and the removal of the small ones,
// area-weighted vertex normals (arithmetic contract C22; the rules: apd_mesh_math.h).  Every operation gives a new
// mesh on the input's device, on its null stream, and leaves the input as it is; there is no host path.
//
// apd_mesh_weld:
//   1. rep[v] by contract C13 over the positions: Labelling::label_points of apd_union_find.h, the labelling of
//      apd_points_components -- cell order, k_cluster_link, flatten, reduce, emit.
//   2. k_mesh_weld_faces: per face the three representatives and whether the face survives (no two equal).
//   3. the compaction (MeshCall::compact, apd_mesh_compact.h, shared with apd_mesh_simplify.hip).
// apd_mesh_components, on a parent array over the VERTICES:
//   1. k_cluster_init; k_mesh_link, one lane per face: unite(v0, v1), unite(v0, v2) -- the lock-free union-find of apd_union_find.h.
//   2. k_cluster_flatten, a launch of its own: root[v].
//   3. k_mesh_face_roots: per face root[v0].
//   4. k_cluster_reduce over the faces, the lanes of a wave that hold one root combined first -- a surface is one component of
//      millions of faces --, integer min / add per root; k_cluster_emit: label[f], size[f]; the count of label[f] == f by a scan.
// apd_mesh_remove_small_components: the flags size[f] >= min_faces, and the compaction.
// The compaction (apd_mesh_compact.h): used[v] = 1 for every index of a kept face (plain stores of the one value 1), a 64-bit scan of the
// vertex flags and one of the face flags, a gather of the kept vertices' arrays and of the kept faces with their indices renumbered
// by the vertex scan.  Every output element has one writer and every position is a scan's.
// apd_mesh_with_vertex_normals -- a GATHER, so that the order of every binary64 sum is the contract's and not the order of arrival
// of an atomic, which no floating-point sum survives bit for bit:
//   1. k_mesh_corner_keys: the 3 F keys index[3 f + c] with payload 3 f + c; apd_sort::sort_pairs, stable, so equal keys stay in
//      payload order; the passes over digits that are the same in every key are skipped.
//   2. k_mesh_run_starts: the position where each vertex's run of corners starts (2^32 - 1: no face names it).
//   3. k_mesh_vertex_normals: one lane per vertex walks its run, ascending 3 f + c, and adds each face's binary64 cross product.
// No LDS, no scratch memory, no floating-point atomic.  A call that fails leaves its result without arrays: what it allocated
// goes with its Scratch, and the entry point deletes the bare object.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_mesh_math.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_sort.h"
#include "apd_union_find.h"

namespace {

using apd_mesh_compact::clear_timing;
using apd_mesh_compact::err;
using apd_mesh_compact::into_new_mesh;
using apd_mesh_compact::MeshCall;
using apd_mesh_compact::new_mesh_like;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;
using apd_points_search::k_fill;
using apd_points_search::k_keep_flags;
using apd_points_search::Search;
using apd_union_find::k_cluster_emit;
using apd_union_find::k_cluster_flatten;
using apd_union_find::k_cluster_init;
using apd_union_find::k_cluster_reduce;

constexpr uint32_t kNoRun = 0xFFFFFFFFu;

// *bad = 1 when one of the n indices is outside [0, vertices)
__global__ __launch_bounds__(256) void k_mesh_check_indices(const int32_t *__restrict__ index, size_t n, int32_t vertices, uint32_t *bad)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n && (index[k] < 0 || index[k] >= vertices)) {
        *bad = 1u;
    }
}

// Face f < faces: mapped[3 f + c] = rep[index[3 f + c]], keep[f] = 1 where the three differ
__global__ __launch_bounds__(256) void k_mesh_weld_faces(const int32_t *__restrict__ index, const uint32_t *__restrict__ rep, size_t faces,
                                                          int32_t *__restrict__ mapped, uint32_t *__restrict__ keep)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    const int32_t a = (int32_t)rep[index[3 * f]], b = (int32_t)rep[index[3 * f + 1]], c = (int32_t)rep[index[3 * f + 2]];
    mapped[3 * f] = a;
    mapped[3 * f + 1] = b;
    mapped[3 * f + 2] = c;
    keep[f] = apd_fusion::mesh_face_degenerate(a, b, c) ? 0u : 1u;
}

// Face f < faces: its three vertices are in one tree of parent[] when the kernel ends
__global__ __launch_bounds__(256) void k_mesh_link(const int32_t *__restrict__ index, uint32_t faces, uint32_t *parent)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;  // faces < 2^31
    if (f >= faces) {
        return;
    }
    const uint32_t v0 = (uint32_t)index[3 * (size_t)f], v1 = (uint32_t)index[3 * (size_t)f + 1], v2 = (uint32_t)index[3 * (size_t)f + 2];
    apd_union_find::unite(parent, v0, v1);
    apd_union_find::unite(parent, v0, v2);
}

__global__ __launch_bounds__(256) void k_mesh_face_roots(const int32_t *__restrict__ index, const uint32_t *__restrict__ root, uint32_t faces,
                                                          uint32_t *__restrict__ face_root)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < faces) {
        face_root[f] = root[index[3 * (size_t)f]];
    }
}

// Corner k < corners (= 3 F < 2^32): the pair (its vertex, k)
__global__ __launch_bounds__(256) void k_mesh_corner_keys(const int32_t *__restrict__ index, size_t corners, uint64_t *__restrict__ key,
                                                           uint32_t *__restrict__ val)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < corners) {
        key[k] = (uint64_t)(uint32_t)index[k];
        val[k] = (uint32_t)k;
    }
}

// Sorted position p < corners: start[key[p]] = p where a run starts; start: kNoRun before
__global__ __launch_bounds__(256) void k_mesh_run_starts(const uint64_t *__restrict__ key, size_t corners, uint32_t *__restrict__ start)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < corners && (p == 0 || key[p] != key[p - 1])) {
        start[key[p]] = (uint32_t)p;
    }
}

// Vertex v < vertices: its normal by contract C22, from the corners key[p] == v, p from start[v] on, in that order
__global__ __launch_bounds__(256) void k_mesh_vertex_normals(const float *__restrict__ xyz, const int32_t *__restrict__ index,
                                                              const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, size_t corners,
                                                              const uint32_t *__restrict__ start, size_t vertices, float *__restrict__ normal)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};
    const uint32_t first = start[v];
    for (size_t p = first; first != kNoRun && p < corners && key[p] == (uint64_t)v; ++p) {
        const size_t f = val[p] / 3u;
        const float *A = xyz + 3 * (size_t)index[3 * f], *B = xyz + 3 * (size_t)index[3 * f + 1], *C = xyz + 3 * (size_t)index[3 * f + 2];
        double g[3];
        apd_fusion::mesh_face_normal(A, B, C, g);
        apd_fusion::mesh_add(s, g);
    }
    float n[3];
    apd_fusion::mesh_vertex_normal(s, n);
    normal[3 * v] = n[0];
    normal[3 * v + 1] = n[1];
    normal[3 * v + 2] = n[2];
}

// One call: its name, which starts every message; for welding the grid of the search
struct Call : MeshCall {
    // apd_mesh_create after its refusals: the arrays into m on its device, which is made the current one
    int create(apd_mesh *m, size_t vertices, const float *xyz, const uint8_t *bgr, size_t faces, const int32_t *index, bool on_device) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        Scratch scratch;
        if (const int rc = alloc(scratch, m, vertices, faces); rc != APD_OK) {
            return rc;
        }
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (vertices > 0) {
            HIP_TRY(hipMemcpy(m->xyz, xyz, vertices * 12, kind));
            if (bgr) {
                HIP_TRY(hipMemcpy(m->bgr, bgr, vertices * 3, kind));
            }
        }
        if (faces > 0) {
            HIP_TRY(hipMemcpy(m->index, index, faces * 12, kind));
        }
        if (on_device && faces > 0) {
            uint32_t *bad = nullptr, found = 0;
            HIP_TRY(scratch.alloc(4, &bad));
            HIP_TRY(hipMemset(bad, 0, 4));
            hipLaunchKernelGGL(k_mesh_check_indices, grid_of(3 * faces), dim3(256), 0, 0, (const int32_t *)m->index, 3 * faces, (int32_t)vertices, bad);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&found, bad, 4, hipMemcpyDeviceToHost));
            if (found) {
                return apd::set_error(err(), APD_ERR_INVALID, "%s: a face index outside 0 .. %zu", who, vertices);
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        keep(scratch, m);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // apd_mesh_weld of m (with vertices) into `out`
    int weld(const apd_mesh *m, apd_mesh *out) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *rep = nullptr, *size = nullptr, *keep_face = nullptr;
        int32_t *mapped = nullptr;
        HIP_TRY(scratch.alloc(nv * 4, &rep));
        HIP_TRY(scratch.alloc(nv * 4, &size));
        HIP_TRY(scratch.alloc(nf * 4, &keep_face));
        HIP_TRY(scratch.alloc(nf * 12, &mapped));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (const int rc = apd_union_find::Labelling{*this}.label_points(m->xyz, nv, rep, size, nullptr); rc != APD_OK) {
            return rc;
        }
        if (nf > 0) {
            hipLaunchKernelGGL(k_mesh_weld_faces, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (const uint32_t *)rep, nf, mapped, keep_face);
            HIP_TRY(hipGetLastError());
        }
        const int rc = compact(scratch, m, mapped, keep_face, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return rc;
    }

    // label[f] and size[f] of the nf > 0 faces of m, device memory on the current device, and their number of components (may be
    // null)
    int label_faces(const apd_mesh *m, uint32_t *label, uint32_t *size, long long *components) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *parent = nullptr, *root = nullptr, *root_min = nullptr, *root_size = nullptr, *face_root = nullptr;
        HIP_TRY(scratch.alloc(nv * 4, &parent));
        HIP_TRY(scratch.alloc(nv * 4, &root));
        HIP_TRY(scratch.alloc(nv * 4, &root_min));
        HIP_TRY(scratch.alloc(nv * 4, &root_size));
        HIP_TRY(scratch.alloc(nf * 4, &face_root));
        hipLaunchKernelGGL(k_cluster_init, grid_of(nv), dim3(256), 0, 0, (uint32_t)nv, parent, root_min, root_size);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_link, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (uint32_t)nf, parent);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_cluster_flatten, grid_of(nv), dim3(256), 0, 0, (uint32_t)nv, parent, root);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_face_roots, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, (const uint32_t *)root, (uint32_t)nf, face_root);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_cluster_reduce, grid_of(nf), dim3(256), 0, 0, (const uint32_t *)face_root, (const uint32_t *)nullptr, (uint32_t)nf, root_min,
                           root_size);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_cluster_emit, grid_of(nf), dim3(256), 0, 0, (const uint32_t *)face_root, (const uint32_t *)nullptr, (uint32_t)nf,
                           (const uint32_t *)root_min, (const uint32_t *)root_size, label, size);
        HIP_TRY(hipGetLastError());
        if (components) {
            if (const int rc = apd_union_find::Labelling{*this}.count_own(label, nf, components); rc != APD_OK) {
                return rc;
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_mesh_components of m (with faces): label and size (may be null) are host memory
    int components_of(const apd_mesh *m, uint32_t *label, uint32_t *size, long long *components) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *d_label = nullptr, *d_size = nullptr;
        HIP_TRY(scratch.alloc(nf * 4, &d_label));
        HIP_TRY(scratch.alloc(nf * 4, &d_size));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (const int rc = label_faces(m, d_label, d_size, components); rc != APD_OK) {
            return rc;
        }
        HIP_TRY(hipMemcpy(label, d_label, nf * 4, hipMemcpyDeviceToHost));
        if (size) {
            HIP_TRY(hipMemcpy(size, d_size, nf * 4, hipMemcpyDeviceToHost));
        }
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // apd_mesh_remove_small_components of m (with vertices) into `out`
    int remove_small(const apd_mesh *m, uint32_t min_faces, apd_mesh *out, long long *components) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nf = (size_t)m->faces;
        Scratch scratch;
        uint32_t *label = nullptr, *size = nullptr, *keep_face = nullptr;
        HIP_TRY(scratch.alloc(nf * 4, &label));
        HIP_TRY(scratch.alloc(nf * 4, &size));
        HIP_TRY(scratch.alloc(nf * 4, &keep_face));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (nf > 0) {
            if (min_faces <= 1 && !components) {  // every face stays and nobody asks for the components
                hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(nf), dim3(256), 0, 0, keep_face, nf, 1u);
                HIP_TRY(hipGetLastError());
            } else {
                if (const int rc = label_faces(m, label, size, components); rc != APD_OK) {
                    return rc;
                }
                hipLaunchKernelGGL(k_keep_flags, grid_of(nf), dim3(256), 0, 0, (const uint32_t *)size, nf, min_faces, keep_face);
                HIP_TRY(hipGetLastError());
            }
        }
        const int rc = compact(scratch, m, m->index, keep_face, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return rc;
    }

    // apd_mesh_with_vertex_normals of m (with vertices; 3 * faces < 2^32) into `out`, which has colour as m and normals
    int with_normals(const apd_mesh *m, apd_mesh *out) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces, corners = 3 * nf;
        Scratch scratch, made;
        if (const int rc = alloc(made, out, nv, nf); rc != APD_OK) {
            return rc;
        }
        uint64_t *keys[2] = {nullptr, nullptr};
        uint32_t *vals[2] = {nullptr, nullptr}, *start = nullptr;
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(scratch.alloc(corners * 8, &keys[b]));
            HIP_TRY(scratch.alloc(corners * 4, &vals[b]));
        }
        HIP_TRY(scratch.alloc(nv * 4, &start));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpyAsync(out->xyz, m->xyz, nv * 12, hipMemcpyDeviceToDevice, 0));
        if (m->colour) {
            HIP_TRY(hipMemcpyAsync(out->bgr, m->bgr, nv * 3, hipMemcpyDeviceToDevice, 0));
        }
        int side = 0;
        if (nf > 0) {
            HIP_TRY(hipMemcpyAsync(out->index, m->index, nf * 12, hipMemcpyDeviceToDevice, 0));
            hipLaunchKernelGGL(k_mesh_corner_keys, grid_of(corners), dim3(256), 0, 0, (const int32_t *)m->index, corners, keys[0], vals[0]);
            HIP_TRY(hipGetLastError());
            HIP_TRY(apd_sort::sort_pairs(keys[0], keys[1], vals[0], vals[1], corners, &side, nullptr));
        }
        hipLaunchKernelGGL(k_fill<uint32_t>, grid_of(nv), dim3(256), 0, 0, start, nv, kNoRun);
        HIP_TRY(hipGetLastError());
        if (nf > 0) {
            hipLaunchKernelGGL(k_mesh_run_starts, grid_of(corners), dim3(256), 0, 0, (const uint64_t *)keys[side], corners, start);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_mesh_vertex_normals, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, (const int32_t *)m->index,
                           (const uint64_t *)keys[side], (const uint32_t *)vals[side], corners, (const uint32_t *)start, nv, out->normal);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        keep(made, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // The arrays of m in host memory; any pointer may be null
    int download(const apd_mesh *m, float *xyz, uint8_t *bgr, float *normal, int32_t *faces) const
    {
        HIP_TRY(hipSetDevice(m->device));
        if (xyz && m->vertices > 0) {
            HIP_TRY(hipMemcpy(xyz, m->xyz, (size_t)m->vertices * 12, hipMemcpyDeviceToHost));
        }
        if (bgr && m->vertices > 0) {
            HIP_TRY(hipMemcpy(bgr, m->bgr, (size_t)m->vertices * 3, hipMemcpyDeviceToHost));
        }
        if (normal && m->vertices > 0) {
            HIP_TRY(hipMemcpy(normal, m->normal, (size_t)m->vertices * 12, hipMemcpyDeviceToHost));
        }
        if (faces && m->faces > 0) {
            HIP_TRY(hipMemcpy(faces, m->index, (size_t)m->faces * 12, hipMemcpyDeviceToHost));
        }
        return APD_OK;
    }
};

Call call_of(const char *who) { return Call{{{who}}}; }

}  // namespace

extern "C" int apd_mesh_create(int device, long long vertices, const float *xyz, const uint8_t *bgr, long long faces, const int32_t *index, int on_device,
                               apd_mesh_t *mesh)
{
    const Call call = call_of("apd_mesh_create");
    err().clear();
    if (!mesh) {
        return call.invalid("null argument");
    }
    if (vertices < 0 || faces < 0) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %lld vertices and %lld faces", call.who, vertices, faces);
    }
    if (vertices >= (1LL << 31) || faces >= (1LL << 31)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %lld vertices and %lld faces, 2^31 or more", call.who, vertices, faces);
    }
    if ((vertices > 0 && !xyz) || (faces > 0 && !index)) {
        return call.invalid("a null array with a count that is not 0");
    }
    if (device < 0) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: device %d", call.who, device);
    }
    if (!on_device) {
        for (long long k = 0; k < 3 * faces; ++k) {
            if (index[k] < 0 || index[k] >= vertices) {
                return apd::set_error(err(), APD_ERR_INVALID, "%s: face %lld names vertex %d, outside 0 .. %lld", call.who, k / 3, (int)index[k], vertices);
            }
        }
    }
    clear_timing();
    apd_mesh *m = new apd_mesh();
    m->device = device;
    m->colour = bgr ? 1 : 0;
    if (vertices > 0 || faces > 0) {
        DeviceScope scope(true);
        if (const int rc = call.create(m, (size_t)vertices, xyz, bgr, (size_t)faces, index, on_device != 0); rc != APD_OK) {
            delete m;
            return rc;
        }
    }
    *mesh = m;
    return APD_OK;
}

extern "C" int apd_mesh_weld(apd_mesh_t m, float tolerance, const float *origin3, apd_mesh_t *out, long long *removed_vertices, long long *removed_faces)
{
    Call call = call_of("apd_mesh_weld");
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    if (!(isfinite(tolerance) && tolerance > 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a tolerance of %g, not a positive finite number", call.who, (double)tolerance);
    }
    const float t2 = tolerance * tolerance;
    if (!(isfinite(t2) && t2 > 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a tolerance of %g, whose square %g is not a positive finite number", call.who, (double)tolerance,
                              (double)t2);
    }
    call.grid.size = tolerance;
    for (int a = 0; origin3 && a < 3; ++a) {
        if (!isfinite(origin3[a])) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: origin component %d is %g", call.who, a, (double)origin3[a]);
        }
        call.grid.origin[a] = origin3[a];
    }
    apd_mesh_t result = nullptr;
    const int rc = into_new_mesh(m, new_mesh_like(m), &result, [&](apd_mesh *r) { return call.weld(m, r); });
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

extern "C" int apd_mesh_components(apd_mesh_t m, uint32_t *label, uint32_t *size, long long *components)
{
    const Call call = call_of("apd_mesh_components");
    err().clear();
    if (!m || !label) {
        return call.invalid("null argument");
    }
    clear_timing();
    long long found = 0;
    if (m->faces > 0) {
        DeviceScope scope(true);
        if (const int rc = call.components_of(m, label, size, components ? &found : nullptr); rc != APD_OK) {
            return rc;
        }
    }
    if (components) {
        *components = found;
    }
    return APD_OK;
}

extern "C" int apd_mesh_remove_small_components(apd_mesh_t m, unsigned min_faces, apd_mesh_t *out, long long *removed_faces, long long *components)
{
    const Call call = call_of("apd_mesh_remove_small_components");
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    long long found = 0;
    apd_mesh_t result = nullptr;
    const int rc = into_new_mesh(m, new_mesh_like(m), &result, [&](apd_mesh *r) { return call.remove_small(m, min_faces, r, components ? &found : nullptr); });
    if (rc != APD_OK) {
        return rc;
    }
    *out = result;
    if (removed_faces) {
        *removed_faces = m->faces - result->faces;
    }
    if (components) {
        *components = found;
    }
    return APD_OK;
}

extern "C" int apd_mesh_with_vertex_normals(apd_mesh_t m, apd_mesh_t *out)
{
    const Call call = call_of("apd_mesh_with_vertex_normals");
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    if (3 * m->faces >= (1LL << 32)) {
        return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld faces, whose 3 corners each are 2^32 or more (the sort carries a 32-bit corner)", call.who,
                              m->faces);
    }
    apd_mesh *like = new_mesh_like(m);
    like->normals = 1;
    apd_mesh_t result = nullptr;
    const int rc = into_new_mesh(m, like, &result, [&](apd_mesh *r) { return call.with_normals(m, r); });
    if (rc != APD_OK) {
        return rc;
    }
    *out = result;
    return APD_OK;
}

extern "C" int apd_mesh_counts(apd_mesh_t m, long long *vertices, long long *faces)
{
    const Call call = call_of("apd_mesh_counts");
    err().clear();
    if (!m || (!vertices && !faces)) {
        return call.invalid("null argument");
    }
    if (vertices) {
        *vertices = m->vertices;
    }
    if (faces) {
        *faces = m->faces;
    }
    return APD_OK;
}

extern "C" int apd_mesh_has_colour(apd_mesh_t m) { return m ? m->colour : 0; }

extern "C" int apd_mesh_has_normals(apd_mesh_t m) { return m ? m->normals : 0; }

extern "C" int apd_mesh_download(apd_mesh_t m, float *xyz, uint8_t *bgr, int32_t *faces)
{
    const Call call = call_of("apd_mesh_download");
    err().clear();
    if (!m || (!xyz && !bgr && !faces)) {
        return call.invalid("null argument");
    }
    if (bgr && !m->colour) {
        return call.invalid("a colour array for a mesh without colour");
    }
    if (m->vertices == 0 && m->faces == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.download(m, xyz, bgr, nullptr, faces);
}

extern "C" int apd_mesh_download_normals(apd_mesh_t m, float *nxyz)
{
    const Call call = call_of("apd_mesh_download_normals");
    err().clear();
    if (!m || !nxyz) {
        return call.invalid("null argument");
    }
    if (!m->normals) {
        return call.invalid("a mesh without normals");
    }
    if (m->vertices == 0) {
        return APD_OK;
    }
    DeviceScope scope(true);
    return call.download(m, nullptr, nullptr, nxyz, nullptr);
}

extern "C" int apd_mesh_write_ply(apd_mesh_t m, const char *path)
{
    const Call call = call_of("apd_mesh_write_ply");
    err().clear();
    if (!m || !path) {
        return call.invalid("null argument");
    }
    clear_timing();
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
    std::vector<float> xyz(3 * nv), normal(m->normals ? 3 * nv : 0);
    std::vector<uint8_t> bgr(m->colour ? 3 * nv : 0);
    std::vector<int32_t> index(3 * nf);
    if (nv > 0 || nf > 0) {
        DeviceScope scope(true);
        if (const int rc = call.download(m, xyz.data(), m->colour ? bgr.data() : nullptr, m->normals ? normal.data() : nullptr, index.data()); rc != APD_OK) {
            return rc;
        }
    }
    apd_fusion::g_fusion_ms[1] = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    FILE *f = fopen(path, "wb");
    if (!f) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: cannot open %s for writing", call.who, path);
    }
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n%s%s"
               "element face %lld\nproperty list uchar int vertex_indices\nend_header\n", m->vertices,
            m->normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "",
            m->colour ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "", m->faces);
    const size_t colour_at = m->normals ? 24 : 12, vertex_bytes = colour_at + (m->colour ? 3 : 0);
    std::vector<uint8_t> packed(std::max(nv * vertex_bytes, nf * 13));
    for (size_t k = 0; k < nv; ++k) {  // little endian, as the host's memcpy writes them
        uint8_t *rec = packed.data() + k * vertex_bytes;
        memcpy(rec, xyz.data() + 3 * k, 12);
        if (m->normals) {
            memcpy(rec + 12, normal.data() + 3 * k, 12);
        }
        if (m->colour) {
            rec[colour_at] = bgr[3 * k + 2];
            rec[colour_at + 1] = bgr[3 * k + 1];
            rec[colour_at + 2] = bgr[3 * k];
        }
    }
    bool ok = fwrite(packed.data(), 1, nv * vertex_bytes, f) == nv * vertex_bytes;
    for (size_t k = 0; k < nf; ++k) {
        uint8_t *rec = packed.data() + k * 13;
        rec[0] = 3;
        memcpy(rec + 1, index.data() + 3 * k, 12);
    }
    ok = ok && fwrite(packed.data(), 1, nf * 13, f) == nf * 13;
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: writing %s failed", call.who, path);
    }
    apd_fusion::g_fusion_ms[2] = ms_since(t1);
    return APD_OK;
}

extern "C" int apd_mesh_destroy(apd_mesh_t m)
{
    if (!m) {
        return APD_OK;
    }
    if (m->xyz || m->bgr || m->normal || m->index) {
        DeviceScope scope(true);
        if (hipSetDevice(m->device) == hipSuccess) {
            hipFree(m->xyz);
            hipFree(m->bgr);
            hipFree(m->normal);
            hipFree(m->index);
        }
    }
    delete m;
    return APD_OK;
}
