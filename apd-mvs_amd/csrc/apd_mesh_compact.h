// apd_mesh_compact.h -- what the calls that answer with a new mesh share (apd_mesh.hip: weld, removal, normals; apd_mesh_simplify.hip):
// the device arrays of a result, the compaction of a mesh to its kept faces and the vertices they name, and the tail of such an entry
// point.  The compaction (compact): used[v] = 1 for every index of a kept face (plain stores of the one value 1), a 64-bit scan of
// the vertex flags and one of the face flags, a gather of the kept vertices' arrays and of the kept faces with their indices
// renumbered by the vertex scan.  Every output element has one writer and every position is a scan's.  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_host.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_sort.h"

namespace apd_mesh_compact {
namespace {

using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::Search;

// used[v] = 1 for the indices of the kept faces; used: zeros before.  Every writer writes the same value
__global__ __launch_bounds__(256) void k_mesh_mark_used(const int32_t *__restrict__ index, const uint32_t *__restrict__ keep, size_t faces,
                                                         uint32_t *used)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < faces && keep[f]) {
        used[index[3 * f]] = 1u;
        used[index[3 * f + 1]] = 1u;
        used[index[3 * f + 2]] = 1u;
    }
}

// Vertex v < vertices with used[v]: its arrays to position at[v]; bgr / normal null: the mesh has none
__global__ __launch_bounds__(256) void k_mesh_gather_vertices(const uint32_t *__restrict__ used, const uint64_t *__restrict__ at, size_t vertices,
                                                               const float *__restrict__ xyz, const uint8_t *__restrict__ bgr,
                                                               const float *__restrict__ normal, float *__restrict__ out_xyz,
                                                               uint8_t *__restrict__ out_bgr, float *__restrict__ out_normal)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices || !used[v]) {
        return;
    }
    const size_t to = (size_t)at[v];
    for (int a = 0; a < 3; ++a) {
        out_xyz[3 * to + a] = xyz[3 * v + a];
        if (bgr) {
            out_bgr[3 * to + a] = bgr[3 * v + a];
        }
        if (normal) {
            out_normal[3 * to + a] = normal[3 * v + a];
        }
    }
}

// Face f < faces with keep[f]: to position at[f], its indices renumbered by vertex_at
__global__ __launch_bounds__(256) void k_mesh_gather_faces(const int32_t *__restrict__ index, const uint32_t *__restrict__ keep,
                                                            const uint64_t *__restrict__ at, size_t faces, const uint64_t *__restrict__ vertex_at,
                                                            int32_t *__restrict__ out_index)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces || !keep[f]) {
        return;
    }
    const size_t to = (size_t)at[f];
    for (int c = 0; c < 3; ++c) {
        out_index[3 * to + c] = (int32_t)vertex_at[index[3 * f + c]];
    }
}

std::string &err() { return apd_fusion::g_fusion_error; }

void clear_timing() { apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0; }

// One call on a mesh: its name, which starts every message; where it searches a grid, that grid
struct MeshCall : Search {
    int invalid(const char *what) const { return apd::set_error(err(), APD_ERR_INVALID, "%s: %s", who, what); }

    // Device arrays for `vertices` vertices and `faces` faces in m (which has none so far), owned by `scratch` until keep()
    int alloc(Scratch &scratch, apd_mesh *m, size_t vertices, size_t faces) const
    {
        m->vertices = (long long)vertices;
        m->faces = (long long)faces;
        if (vertices > 0) {
            HIP_TRY(scratch.alloc(vertices * 12, &m->xyz));
            if (m->colour) {
                HIP_TRY(scratch.alloc(vertices * 3, &m->bgr));
            }
            if (m->normals) {
                HIP_TRY(scratch.alloc(vertices * 12, &m->normal));
            }
        }
        if (faces > 0) {
            HIP_TRY(scratch.alloc(faces * 12, &m->index));
        }
        return APD_OK;
    }

    static void keep(Scratch &scratch, const apd_mesh *m)
    {
        for (void *q : {(void *)m->xyz, (void *)m->bgr, (void *)m->normal, (void *)m->index}) {
            if (q) {
                scratch.keep(q);
            }
        }
    }

    // The faces f of m with keep[f] != 0, their indices read from `index` (m's own or a welded copy: 3 per face of m, each a vertex of
    // m), and the vertices those faces name, both in m's order and renumbered, into `out` (no arrays so far; colour and normals
    // as m).  m has vertices; its device is the current one
    int compact(Scratch &scratch, const apd_mesh *m, const int32_t *index, const uint32_t *keep_face, apd_mesh *out) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        uint32_t *used = nullptr;
        uint64_t *vertex_at = nullptr, *face_at = nullptr;
        HIP_TRY(scratch.alloc(nv * 4, &used));
        HIP_TRY(scratch.alloc((nv + 1) * 8, &vertex_at));
        HIP_TRY(scratch.alloc((nf + 1) * 8, &face_at));
        HIP_TRY(hipMemsetAsync(used, 0, nv * 4, 0));
        if (nf > 0) {
            hipLaunchKernelGGL(k_mesh_mark_used, grid_of(nf), dim3(256), 0, 0, index, keep_face, nf, used);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(apd_sort::exclusive_scan(used, vertex_at, nv));
        HIP_TRY(apd_sort::exclusive_scan(keep_face, face_at, nf));
        uint64_t vertices = 0, faces = 0;
        HIP_TRY(hipMemcpy(&vertices, vertex_at + nv, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&faces, face_at + nf, 8, hipMemcpyDeviceToHost));
        Scratch made;
        if (const int rc = alloc(made, out, (size_t)vertices, (size_t)faces); rc != APD_OK) {
            return rc;
        }
        if (vertices > 0) {
            hipLaunchKernelGGL(k_mesh_gather_vertices, grid_of(nv), dim3(256), 0, 0, (const uint32_t *)used, (const uint64_t *)vertex_at, nv,
                               (const float *)m->xyz, (const uint8_t *)m->bgr, (const float *)m->normal, out->xyz, out->bgr, out->normal);
            HIP_TRY(hipGetLastError());
        }
        if (faces > 0) {
            hipLaunchKernelGGL(k_mesh_gather_faces, grid_of(nf), dim3(256), 0, 0, index, keep_face, (const uint64_t *)face_at, nf,
                               (const uint64_t *)vertex_at, out->index);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());
        keep(made, out);
        return APD_OK;
    }
};

// A new mesh like m without vertices or faces: its device and whether it carries colour and normals
apd_mesh *new_mesh_like(const apd_mesh *m)
{
    apd_mesh *out = new apd_mesh();
    out->device = m->device;
    out->colour = m->colour;
    out->normals = m->normals;
    return out;
}

// The tail of an entry point that answers with a new mesh: body(result) fills it from m (which has vertices) or fails with its
// message set; a mesh without vertices gives one without, and touches no device
template <typename Body> int into_new_mesh(apd_mesh_t m, apd_mesh *result, apd_mesh_t *out, Body &&body)
{
    clear_timing();
    if (m->vertices > 0) {
        DeviceScope scope(true);
        if (const int rc = body(result); rc != APD_OK) {
            delete result;  // it holds nothing: what the call allocated went with its scratch
            return rc;
        }
    }
    *out = result;
    return APD_OK;
}

}  // namespace
}  // namespace apd_mesh_compact
