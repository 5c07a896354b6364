// apd_mesh_render_device.h -- the rasteriser of contract C25 as device code, for the calls that need the key image of a mesh in a
// camera on the device: apd_mesh_render.hip (the maps, the face visibility, the trimming) and apd_mesh_colour.hip (the vertex colours,
// which read the depth map of every view without a download).  The kernels of steps 1, 3 and 5 of apd_mesh_render.hip's header text,
// the device memory they draw in (Canvas) and the launches of one camera (RenderCall::draw).  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_mesh_render_math.h"
#include "apd_points_host.h"
#include "apd_render_device.h"
#include "apd_sort.h"
#include "apd_tuning.h"

namespace apd_mesh_render_device {

// > 0: the split of apd_mesh_render_split; 0: APD_MESH_RENDER_SPLIT (apd_mesh_render.hip)
extern std::atomic<int> g_render_split;

namespace {

using apd_fusion::RenderFace;
using apd_fusion::RenderVertex;
using apd_fusion::View;
using apd_mesh_compact::err;
using apd_mesh_compact::MeshCall;
using apd_points_grid::grid_of;
using apd_points_host::Scratch;
using apd_render_device::k_render_clear;
using apd_render_device::render_offer;

static_assert(sizeof(RenderVertex) == 16, "one 128-bit load a corner");

constexpr int kTile = 8;          // a wave's tile: 8 x 8 pixels
constexpr int64_t kMaxSlices = 64;
constexpr int64_t kTilesPerSlice = 256;  // a large face gets one wave per this many tiles of its box, up to kMaxSlices

// Vertex v < vertices
__global__ __launch_bounds__(256) void k_mesh_project(const float *__restrict__ xyz, size_t vertices, View view, RenderVertex *__restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    const float P[3] = {xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]};
    out[v] = apd_fusion::mesh_render_vertex(view, P);
}

// Whether face f is drawn into the image, and then the face
__device__ __forceinline__ bool face_of(const RenderVertex *__restrict__ verts, const int32_t *__restrict__ index, size_t f, int cull, int cols, int rows,
                                        RenderFace &face)
{
    const RenderVertex v0 = verts[index[3 * f]], v1 = verts[index[3 * f + 1]], v2 = verts[index[3 * f + 2]];
    return apd_fusion::mesh_render_face(v0, v1, v2, cull, cols, rows, face);
}

// The 8 x 8 tiles of a face's box (which is not empty)
__device__ __forceinline__ int64_t tiles_of(const RenderFace &face, int &across)
{
    across = (face.c1 - face.c0) / kTile + 1;
    return (int64_t)across * (int64_t)((face.r1 - face.r0) / kTile + 1);
}

// Face f < faces: drawn here when its box has at most `split` pixels; otherwise slices[f] = the waves of k_mesh_raster_large that
// will draw it; slices[f] = 0 for every face drawn here or not at all.  keys: rows x cols, cleared
__global__ __launch_bounds__(256) void k_mesh_raster_small(const RenderVertex *__restrict__ verts, const int32_t *__restrict__ index, size_t faces, int cull,
                                                            int cols, int rows, int64_t split, uint64_t *keys, uint32_t *__restrict__ slices)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    RenderFace face;
    const bool drawn = face_of(verts, index, f, cull, cols, rows, face);
    const int64_t box = drawn ? apd_fusion::mesh_render_box_pixels(face) : 0;
    const bool big = box > split;
    uint32_t waves = 0;
    if (big) {
        int across;
        const int64_t wanted = (tiles_of(face, across) + kTilesPerSlice - 1) / kTilesPerSlice;
        waves = (uint32_t)(wanted < kMaxSlices ? wanted : kMaxSlices);  // at least 1: the box is not empty
    }
    slices[f] = waves;
    if (box == 0 || big) {
        return;
    }
    for (int y = face.r0; y <= face.r1; ++y) {
        uint64_t *row = keys + (size_t)y * (size_t)cols;
        for (int x = face.c0; x <= face.c1; ++x) {
            float z;
            if (apd_fusion::mesh_render_pixel(face, x, y, z)) {
                render_offer(row + x, apd_fusion::render_key(z, (uint32_t)f));
            }
        }
    }
}

// The largest value of edge a -> b's function over the pixel centres of [x0, x1] x [y0, y1]: at a corner, the function being linear
__device__ __forceinline__ int64_t edge_max(const RenderFace &face, int a, int b, int x0, int y0, int x1, int y1)
{
    const int64_t dx = face.X[b] - face.X[a], dy = face.Y[b] - face.Y[a];
    const int py = dx > 0 ? y1 : y0, px = dy > 0 ? x0 : x1;  // dx * py grows with py when dx > 0; -dy * px grows with px when dy < 0
    return dx * (int64_t)(256 * py - face.Y[a]) - dy * (int64_t)(256 * px - face.X[a]);
}

// Wave w < waves (= at[faces], the sum of slices[]): the face f with at[f] <= w < at[f] + slices[f], and of the tiles of its box the
// tiles slice, slice + slices[f], ... with slice = w - at[f].  Four waves a workgroup
__global__ __launch_bounds__(256) void k_mesh_raster_large(const RenderVertex *__restrict__ verts, const int32_t *__restrict__ index,
                                                            const uint64_t *__restrict__ at, const uint32_t *__restrict__ slices, uint32_t faces,
                                                            uint64_t waves, int cull, int cols, int rows, uint64_t *keys)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u;
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= waves) {
        return;
    }
    uint32_t lo = 0, hi = faces;  // at[lo] <= w < at[hi]: at[0] = 0 and at[faces] = waves
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (at[mid] <= w) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    const uint32_t f = lo;  // the last face with at[f] <= w: at[f + 1] > w, so slices[f] > 0
    const int64_t slice = (int64_t)(w - at[f]), step = (int64_t)slices[f];
    RenderFace face;
    if (step == 0 || !face_of(verts, index, f, cull, cols, rows, face)) {
        return;  // not reached: only drawn faces have slices
    }
    int across;
    const int64_t tiles = tiles_of(face, across);
    for (int64_t t = slice; t < tiles; t += step) {
        const int x0 = face.c0 + (int)(t % across) * kTile, y0 = face.r0 + (int)(t / across) * kTile;
        const int x1 = x0 + kTile - 1 < face.c1 ? x0 + kTile - 1 : face.c1, y1 = y0 + kTile - 1 < face.r1 ? y0 + kTile - 1 : face.r1;
        if (edge_max(face, 0, 1, x0, y0, x1, y1) < 0 || edge_max(face, 1, 2, x0, y0, x1, y1) < 0 || edge_max(face, 2, 0, x0, y0, x1, y1) < 0) {
            continue;  // the whole wave: no centre of the tile is inside that edge
        }
        const int x = x0 + (lane & (kTile - 1)), y = y0 + lane / kTile;
        float z;
        if (x <= x1 && y <= y1 && apd_fusion::mesh_render_pixel(face, x, y, z)) {
            render_offer(keys + (size_t)y * (size_t)cols + (size_t)x, apd_fusion::render_key(z, f));
        }
    }
}

// What drawing one mesh into the cameras of a call needs on the device
struct Canvas {
    RenderVertex *verts = nullptr;
    uint64_t *keys = nullptr, *at = nullptr;
    uint32_t *slices = nullptr;
};

// A call that draws a mesh
struct RenderCall : MeshCall {
    int bad_camera(const apd_camera &c, int s) const
    {
        if (c.width <= 0 || c.height <= 0) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels", who, s, c.width, c.height);
        }
        if ((long long)c.width * c.height >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels, 2^31 or more", who, s, c.width, c.height);
        }
        return APD_OK;
    }

    int canvas(Scratch &scratch, const apd_mesh *m, size_t max_px, Canvas &c) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        HIP_TRY(scratch.alloc(nv * sizeof(RenderVertex), &c.verts));
        HIP_TRY(scratch.alloc(max_px * 8, &c.keys));
        HIP_TRY(scratch.alloc((nf + 1) * 8, &c.at));
        HIP_TRY(scratch.alloc(nf * 4, &c.slices));
        return APD_OK;
    }

    // The key image of `camera` from the faces of m (which has faces) into c.keys; c.verts: the vertices in that camera
    int draw(const apd_mesh *m, const apd_camera &camera, int cull, const Canvas &c, View &view) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        const int cols = camera.width, rows = camera.height;
        const size_t px = (size_t)cols * (size_t)rows;
        const int chosen = g_render_split.load();
        const int64_t split = chosen > 0 ? chosen : APD_MESH_RENDER_SPLIT;
        apd_fusion::view_geometry(camera, rows, cols, view);
        hipLaunchKernelGGL(k_mesh_project, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, nv, view, c.verts);
        hipLaunchKernelGGL(k_render_clear, grid_of(px), dim3(256), 0, 0, c.keys, px);
        hipLaunchKernelGGL(k_mesh_raster_small, grid_of(nf), dim3(256), 0, 0, (const RenderVertex *)c.verts, (const int32_t *)m->index, nf, cull, cols, rows,
                           split, c.keys, c.slices);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(c.slices, c.at, nf));
        uint64_t waves = 0;
        HIP_TRY(hipMemcpy(&waves, c.at + nf, 8, hipMemcpyDeviceToHost));
        if ((waves + 3) / 4 >= (1ull << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: the large faces need %llu waves, more than one launch holds", who, (unsigned long long)waves);
        }
        if (waves > 0) {
            hipLaunchKernelGGL(k_mesh_raster_large, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, 0, (const RenderVertex *)c.verts,
                               (const int32_t *)m->index, (const uint64_t *)c.at, (const uint32_t *)c.slices, (uint32_t)nf, waves, cull, cols, rows, c.keys);
            HIP_TRY(hipGetLastError());
        }
        return APD_OK;
    }
};

}  // namespace
}  // namespace apd_mesh_render_device
