// apd_volume.hip -- the apd_volume_* calls of include/apd_mi355x.h: a truncated signed distance volume integrated from depth maps,
// and the indexed triangle mesh that marching tetrahedra on the six-tetrahedra split of each cell takes from it (arithmetic
// contract C21; the relation: apd_volume_math.h).  The mesh object and everything done to one: apd_mesh.hip.
//
// The volume: per sample a distance D and a weight W, 4 bytes each, and with colour four more floats (blue, green, red, colour
// weight) interleaved; allocated and set to (1, 0, 0 ..) on the first call that needs the device, so that apd_volume_create itself
// touches none.
//
// apd_volume_integrate, on the volume's device, on its null stream: k_volume_integrate, one lane per sample in linear order -- lanes
// run along i, so D, W and the colour are read and written coalesced, once per launch -- loops over the views of the launch, which
// it gets as a table in its kernel arguments (wave-uniform: scalar loads); per view the projection, one gathered read of the depth
// map and, with colour, of the image.  A call with more than kVolumeViewChunk views is launched in chunks of that many, in order;
// host maps go up per chunk.
// There is no culling: every sample projects into every view.
//
// apd_volume_extract_mesh:
//   1. k_volume_codes: per sample the code (known, inside, the 7-bit mask of the edges that carry a vertex) and the mask's popcount.
//   2. apd_sort::exclusive_scan of the counts: the id of the first vertex of every sample.  The id of (sample, direction) is that
//      plus the rank of the direction in the mask; no table of ids per edge exists.
//   3. k_volume_cell_counts: per cell the faces of its six tetrahedra.
//   4. the scan of those: the first face of every cell.
//   5. k_volume_vertices writes positions and colours, k_volume_faces the index triples.
// No atomics anywhere: every output element has one writer, and every position in the output is a scan's.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_lab.h"
#include "apd_mesh_host.h"
#include "apd_points_host.h"
#include "apd_sort.h"
#include "apd_volume_math.h"

struct apd_volume {
    int device = 0;
    apd_fusion::VolumeGrid grid;
    int colour = 0;
    size_t samples = 0;
    float *D = nullptr, *W = nullptr, *C = nullptr;  // device memory once `ready`
    bool ready = false;
};

namespace {

using apd_fusion::View;
using apd_fusion::VolumeGrid;
using apd_fusion::VolumeView;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;

constexpr int kVolumeViewChunk = APD_VOLUME_VIEW_CHUNK;  // views of one launch: 128 bytes each in the kernel arguments

inline dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }  // blocks of 256 lanes over n < 2^32 elements

struct ViewTable {
    VolumeView v[kVolumeViewChunk];
};

__global__ __launch_bounds__(256) void k_volume_init(float *__restrict__ D, float *__restrict__ W, float4 *__restrict__ C, size_t n)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) {
        return;
    }
    D[s] = 1.0f;
    W[s] = 0.0f;
    if (C) {
        C[s] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// (i, j, k) of linear sample s < nx * ny * nz
__device__ inline void sample_of(const VolumeGrid &g, size_t s, int &i, int &j, int &k)
{
    const uint32_t row = (uint32_t)(s / (uint32_t)g.nx);  // s < 2^31
    i = (int)(s - (size_t)row * (uint32_t)g.nx);
    k = (int)(row / (uint32_t)g.ny);
    j = (int)(row - (uint32_t)k * (uint32_t)g.ny);
}

// Sample s < n: the `count` views of the table, in order
__global__ __launch_bounds__(256) void k_volume_integrate(VolumeGrid g, size_t n, ViewTable table, int count, float *__restrict__ D,
                                                           float *__restrict__ W, float4 *__restrict__ C)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) {
        return;
    }
    int i, j, k;
    sample_of(g, s, i, j, k);
    float P[3];
    apd_fusion::volume_position(g, i, j, k, P);
    float d = D[s], w = W[s];
    float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (C) {
        const float4 c = C[s];
        col[0] = c.x;
        col[1] = c.y;
        col[2] = c.z;
        col[3] = c.w;
    }
    for (int v = 0; v < count; ++v) {
        apd_fusion::volume_integrate(table.v[v], P, g.trunc, g.max_weight, d, w, C != nullptr, col);
    }
    D[s] = d;
    W[s] = w;
    if (C) {
        C[s] = make_float4(col[0], col[1], col[2], col[3]);
    }
}

__global__ __launch_bounds__(256) void k_volume_codes(VolumeGrid g, size_t n, const float *__restrict__ D, const float *__restrict__ W,
                                                       uint16_t *__restrict__ code, uint32_t *__restrict__ count)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) {
        return;
    }
    int i, j, k;
    sample_of(g, s, i, j, k);
    const uint32_t c = apd_fusion::volume_code(g, D, W, i, j, k);
    code[s] = (uint16_t)c;
    count[s] = (uint32_t)apd_fusion::volume_carried(c);
}

// (i, j, k) of cell c < (nx - 1) * (ny - 1) * (nz - 1)
__device__ inline void cell_of(const VolumeGrid &g, size_t c, int &i, int &j, int &k)
{
    const uint32_t cx = (uint32_t)g.nx - 1u, cy = (uint32_t)g.ny - 1u;
    const uint32_t row = (uint32_t)(c / cx);
    i = (int)(c - (size_t)row * cx);
    k = (int)(row / cy);
    j = (int)(row - (uint32_t)k * cy);
}

__global__ __launch_bounds__(256) void k_volume_cell_counts(VolumeGrid g, size_t cells, const uint16_t *__restrict__ code, uint32_t *__restrict__ count)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) {
        return;
    }
    int i, j, k;
    cell_of(g, c, i, j, k);
    uint32_t known8, inside8;
    apd_fusion::volume_cell_corners(g, code, i, j, k, known8, inside8);
    count[c] = (uint32_t)apd_fusion::volume_cell_faces(known8, inside8);
}

// Sample s < n: its vertices, from id at[s] on in ascending direction.  bgr null: no colours.
__global__ __launch_bounds__(256) void k_volume_vertices(VolumeGrid g, size_t n, const float *__restrict__ D, const float *__restrict__ C,
                                                          const uint16_t *__restrict__ code, const uint64_t *__restrict__ at, float *__restrict__ xyz,
                                                          uint8_t *__restrict__ bgr)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) {
        return;
    }
    const uint32_t c = code[s];
    if ((c & 0x7fu) == 0) {
        return;
    }
    int i, j, k;
    sample_of(g, s, i, j, k);
    size_t id = (size_t)at[s];
    for (int dir = 0; dir < 7; ++dir) {
        if (!((c >> dir) & 1u)) {
            continue;
        }
        float P[3];
        uint8_t col[3];
        apd_fusion::volume_vertex(g, D, bgr ? C : nullptr, i, j, k, dir, P, col);
        for (int a = 0; a < 3; ++a) {
            xyz[3 * id + a] = P[a];
            if (bgr) {
                bgr[3 * id + a] = col[a];
            }
        }
        ++id;
    }
}

// Cell c < cells: its faces, from face at[c] on
__global__ __launch_bounds__(256) void k_volume_faces(VolumeGrid g, size_t cells, const uint16_t *__restrict__ code, const uint64_t *__restrict__ vertex_at,
                                                       const uint64_t *__restrict__ at, int32_t *__restrict__ faces)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells || at[c + 1] == at[c]) {
        return;
    }
    int i, j, k;
    cell_of(g, c, i, j, k);
    uint32_t known8, inside8;
    apd_fusion::volume_cell_corners(g, code, i, j, k, known8, inside8);
    apd_fusion::volume_emit_faces(g, code, vertex_at, i, j, k, known8, inside8, faces + 3 * (size_t)at[c]);
}

std::string &err() { return apd_fusion::g_fusion_error; }

bool positive_finite(float v) { return v > 0.0f && isfinite(v); }

void clear_timing() { apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0; }

// One call: its name, which starts every message
struct Call {
    const char *const who;

    int hip_failed(const char *expr, hipError_t e, const char *, int) const  // what HIP_TRY returns
    {
        return apd::set_error(err(), APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
    }

    int invalid(const char *what) const { return apd::set_error(err(), APD_ERR_INVALID, "%s: %s", who, what); }

    // The volume's memory on its device, which is made the current one: allocated and set to the initial state the first time
    int ready(apd_volume *v) const
    {
        HIP_TRY(hipSetDevice(v->device));
        if (v->ready) {
            return APD_OK;
        }
        Scratch scratch;
        float *D = nullptr, *W = nullptr, *C = nullptr;
        HIP_TRY(scratch.alloc(v->samples * 4, &D));
        HIP_TRY(scratch.alloc(v->samples * 4, &W));
        if (v->colour) {
            HIP_TRY(scratch.alloc(v->samples * 16, &C));
        }
        hipLaunchKernelGGL(k_volume_init, grid_of(v->samples), dim3(256), 0, 0, D, W, (float4 *)C, v->samples);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        scratch.keep(D);
        scratch.keep(W);
        if (C) {
            scratch.keep(C);
        }
        v->D = D;
        v->W = W;
        v->C = C;
        v->ready = true;
        return APD_OK;
    }

    int integrate(apd_volume *v, int num_views, const apd_camera *cameras, const float *const *depths, const float *const *images, int channels,
                  const float *weights, int maps_on_device) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = ready(v); rc != APD_OK) {
            return rc;
        }
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        // host maps go up chunk by chunk and are released when the chunk's launch has ended: a call of many views holds the maps of
        // at most kVolumeViewChunk of them on the device
        for (int first = 0; first < num_views; first += kVolumeViewChunk) {
            const int count = std::min(kVolumeViewChunk, num_views - first);
            Scratch scratch;
            ViewTable table;
            memset(&table, 0, sizeof(table));
            for (int k = 0; k < count; ++k) {
                const int s = first + k;
                VolumeView &view = table.v[k];
                const apd_camera &c = cameras[s];
                apd_fusion::view_geometry(c, c.height, c.width, view.geo);
                const size_t px = (size_t)c.width * (size_t)c.height;
                view.depth = depths[s];
                view.image = images ? images[s] : nullptr;
                view.channels = images ? channels : 1;
                view.weight = weights ? weights[s] : 1.0f;
                if (!maps_on_device) {
                    HIP_TRY(scratch.upload(depths[s], px * 4, &view.depth));
                    if (images) {
                        HIP_TRY(scratch.upload(images[s], px * 4 * (size_t)channels, &view.image));
                    }
                }
            }
            hipLaunchKernelGGL(k_volume_integrate, grid_of(v->samples), dim3(256), 0, 0, v->grid, v->samples, table, count, v->D, v->W, (float4 *)v->C);
            HIP_TRY(hipGetLastError());
            if (!maps_on_device) {
                HIP_TRY(hipDeviceSynchronize());  // before the chunk's maps are freed
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // The mesh of v into m (empty so far, on v's device)
    int extract(apd_volume *v, apd_mesh *m) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = ready(v); rc != APD_OK) {
            return rc;
        }
        const VolumeGrid &g = v->grid;
        const size_t n = v->samples, cells = (size_t)(g.nx - 1) * (size_t)(g.ny - 1) * (size_t)(g.nz - 1);
        Scratch scratch;
        uint16_t *code = nullptr;
        uint32_t *vertex_count = nullptr, *face_count = nullptr;
        uint64_t *vertex_at = nullptr, *face_at = nullptr;
        HIP_TRY(scratch.alloc(n * 2, &code));
        HIP_TRY(scratch.alloc(n * 4, &vertex_count));
        HIP_TRY(scratch.alloc((n + 1) * 8, &vertex_at));
        HIP_TRY(scratch.alloc(cells * 4, &face_count));
        HIP_TRY(scratch.alloc((cells + 1) * 8, &face_at));
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_volume_codes, grid_of(n), dim3(256), 0, 0, g, n, (const float *)v->D, (const float *)v->W, code, vertex_count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(vertex_count, vertex_at, n));
        hipLaunchKernelGGL(k_volume_cell_counts, grid_of(cells), dim3(256), 0, 0, g, cells, (const uint16_t *)code, face_count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(face_count, face_at, cells));
        uint64_t vertices = 0, faces = 0;
        HIP_TRY(hipMemcpy(&vertices, vertex_at + n, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&faces, face_at + cells, 8, hipMemcpyDeviceToHost));
        if (vertices >= (1ull << 31) || faces >= (1ull << 31)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %llu vertices and %llu faces, 2^31 or more", who, (unsigned long long)vertices,
                                  (unsigned long long)faces);
        }
        float *xyz = nullptr;
        uint8_t *bgr = nullptr;
        int32_t *index = nullptr;
        if (vertices > 0) {
            HIP_TRY(scratch.alloc((size_t)vertices * 12, &xyz));
            if (v->colour) {
                HIP_TRY(scratch.alloc((size_t)vertices * 3, &bgr));
            }
            hipLaunchKernelGGL(k_volume_vertices, grid_of(n), dim3(256), 0, 0, g, n, (const float *)v->D, (const float *)v->C, (const uint16_t *)code,
                               (const uint64_t *)vertex_at, xyz, bgr);
            HIP_TRY(hipGetLastError());
        }
        if (faces > 0) {
            HIP_TRY(scratch.alloc((size_t)faces * 12, &index));
            hipLaunchKernelGGL(k_volume_faces, grid_of(cells), dim3(256), 0, 0, g, cells, (const uint16_t *)code, (const uint64_t *)vertex_at,
                               (const uint64_t *)face_at, index);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());
        for (void *q : {(void *)xyz, (void *)bgr, (void *)index}) {
            if (q) {
                scratch.keep(q);
            }
        }
        m->vertices = (long long)vertices;
        m->faces = (long long)faces;
        m->xyz = xyz;
        m->bgr = bgr;
        m->index = index;
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    int copy(apd_volume *v, float *tsdf, float *weight, float *colour4, bool up) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = ready(v); rc != APD_OK) {
            return rc;
        }
        float *const host[3] = {tsdf, weight, colour4};
        float *const device[3] = {v->D, v->W, v->C};
        for (int a = 0; a < 3; ++a) {
            if (!host[a]) {
                continue;
            }
            const size_t bytes = v->samples * (a == 2 ? 16 : 4);
            if (up) {
                HIP_TRY(hipMemcpy(device[a], host[a], bytes, hipMemcpyHostToDevice));
            } else {
                HIP_TRY(hipMemcpy(host[a], device[a], bytes, hipMemcpyDeviceToHost));
            }
        }
        apd_fusion::g_fusion_ms[1] = ms_since(t0);
        return APD_OK;
    }
};

// What apd_volume_download and apd_volume_upload refuse
int check_copy(const Call &call, apd_volume_t v, const float *tsdf, const float *weight, const float *colour4)
{
    err().clear();
    if (!v || (!tsdf && !weight && !colour4)) {
        return call.invalid("null argument");
    }
    if (colour4 && !v->colour) {
        return call.invalid("a colour array for a volume without colour");
    }
    return APD_OK;
}

}  // namespace

extern "C" int apd_volume_view_chunk(void) { return kVolumeViewChunk; }

extern "C" int apd_volume_create(int device, int nx, int ny, int nz, const float *origin3, float voxel, float trunc, float max_weight, int with_colour,
                                 apd_volume_t *volume)
{
    const Call call{"apd_volume_create"};
    err().clear();
    if (!origin3 || !volume) {
        return call.invalid("null argument");
    }
    if (nx < 2 || ny < 2 || nz < 2) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d x %d x %d samples, fewer than 2 along an axis", call.who, nx, ny, nz);
    }
    if ((long long)nx * ny >= (1LL << 31) || (long long)nx * ny * nz >= (1LL << 31)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d x %d x %d samples, 2^31 or more", call.who, nx, ny, nz);
    }
    if (device < 0) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: device %d", call.who, device);
    }
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(origin3[a])) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: an origin of %g, %g, %g", call.who, (double)origin3[0], (double)origin3[1], (double)origin3[2]);
        }
    }
    if (!positive_finite(voxel)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a voxel size of %g, not a positive finite number", call.who, (double)voxel);
    }
    if (!positive_finite(trunc)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a truncation distance of %g, not a positive finite number", call.who, (double)trunc);
    }
    if (!positive_finite(max_weight) || max_weight < 1.0f) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a maximal weight of %g, not a finite number of at least 1", call.who, (double)max_weight);
    }
    apd_volume *v = new apd_volume();
    v->device = device;
    v->grid.nx = nx;
    v->grid.ny = ny;
    v->grid.nz = nz;
    std::copy(origin3, origin3 + 3, v->grid.origin);
    v->grid.voxel = voxel;
    v->grid.trunc = trunc;
    v->grid.max_weight = max_weight;
    v->colour = with_colour ? 1 : 0;
    v->samples = (size_t)nx * (size_t)ny * (size_t)nz;
    *volume = v;
    return APD_OK;
}

extern "C" int apd_volume_destroy(apd_volume_t v)
{
    if (!v) {
        return APD_OK;
    }
    if (v->ready) {
        DeviceScope scope(true);
        if (hipSetDevice(v->device) == hipSuccess) {
            hipFree(v->D);
            hipFree(v->W);
            hipFree(v->C);
        }
    }
    delete v;
    return APD_OK;
}

extern "C" int apd_volume_integrate(apd_volume_t v, int num_views, const apd_camera *cameras, const float *const *depths, const float *const *images,
                                    int image_channels, const float *weights, int maps_on_device)
{
    const Call call{"apd_volume_integrate"};
    err().clear();
    if (!v || !cameras || !depths) {
        return call.invalid("null argument");
    }
    if (num_views < 1) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d views", call.who, num_views);
    }
    if (images && !v->colour) {
        return call.invalid("images for a volume without colour");
    }
    if (images && image_channels != 1 && image_channels != 3) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: images of %d channels, not 1 or 3", call.who, image_channels);
    }
    for (int s = 0; s < num_views; ++s) {
        const apd_camera &c = cameras[s];
        if (c.width <= 0 || c.height <= 0) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels", call.who, s, c.width, c.height);
        }
        if ((long long)c.width * c.height >= (1LL << 31)) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: camera %d has %d x %d pixels, 2^31 or more", call.who, s, c.width, c.height);
        }
        if (!depths[s] || (images && !images[s])) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: view %d has a null map", call.who, s);
        }
        if (weights && !positive_finite(weights[s])) {
            return apd::set_error(err(), APD_ERR_INVALID, "%s: view %d has a weight of %g, not a positive finite number", call.who, s, (double)weights[s]);
        }
    }
    clear_timing();
    DeviceScope scope(true);
    return call.integrate(v, num_views, cameras, depths, images, image_channels, weights, maps_on_device);
}

extern "C" int apd_volume_download(apd_volume_t v, float *tsdf, float *weight, float *colour4)
{
    const Call call{"apd_volume_download"};
    if (const int rc = check_copy(call, v, tsdf, weight, colour4); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    DeviceScope scope(true);
    return call.copy(v, tsdf, weight, colour4, false);
}

extern "C" int apd_volume_upload(apd_volume_t v, const float *tsdf, const float *weight, const float *colour4)
{
    const Call call{"apd_volume_upload"};
    if (const int rc = check_copy(call, v, tsdf, weight, colour4); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    DeviceScope scope(true);
    return call.copy(v, const_cast<float *>(tsdf), const_cast<float *>(weight), const_cast<float *>(colour4), true);
}

extern "C" int apd_volume_extract_mesh(apd_volume_t v, apd_mesh_t *mesh)
{
    const Call call{"apd_volume_extract_mesh"};
    err().clear();
    if (!v || !mesh) {
        return call.invalid("null argument");
    }
    clear_timing();
    apd_mesh *m = new apd_mesh();
    m->device = v->device;
    m->colour = v->colour;
    DeviceScope scope(true);
    if (const int rc = call.extract(v, m); rc != APD_OK) {
        delete m;  // it holds nothing yet: what the call allocated went with its scratch
        return rc;
    }
    *mesh = m;
    return APD_OK;
}
