// apd_mesh_smooth.hip -- apd_mesh_adjacency and apd_mesh_smooth of include/apd_mi355x.h: the vertex-to-vertex adjacency of a mesh with
// its edge multiplicities, and Laplacian / Taubin smoothing of the positions over it (arithmetic contract C24; the rules:
// apd_mesh_smooth_math.h).  On the input's device, on its null stream; the input stays as it is; there is no host path.  Everything
// is a function of the input alone: positions come from one stable sort and scans, every sum is walked by one lane in the
// contract's order, every output element has one writer, and there is no atomic.
//   1. k_mesh_edge_keys: one lane per face, its six keys (v << 32) | w; a pair with equal ends gets the key 2^64 - 1, which sorts
//      last.  apd_sort::sort_pairs without a payload over the 6 F keys.
//   2. k_mesh_edge_heads: one lane per sorted position; a head is where the key differs from the one before it and is not 2^64 - 1;
//      a head's lane walks to the end of its run, whose length is the multiplicity of the edge.
//   3. apd_sort::exclusive_scan of the head flags: the position of every distinct pair, and their number, read back.
//      k_mesh_edge_compact: the neighbour lists, w with bit 31 set for an edge of multiplicity 1 (vertices are fewer than 2^31, so one
//      bit is free; whether an edge is non-manifold stays with the multiplicities and is read by the counts alone).
//      k_mesh_row_bounds: where the list of every vertex begins and ends (0 and 0 for a vertex no pair names).
//   4. k_mesh_vertex_flags: one lane per vertex walks its list: valence and boundary flag.
//   5. apd_mesh_adjacency: k_mesh_edge_kinds flags the heads with v < w of multiplicity 1 and of 3 or more; a scan of each counts
//      them.  The undirected edges are half the distinct pairs: (v, w) occurs as often as (w, v).
//   6. apd_mesh_smooth: k_mesh_smooth_moves and a scan count the vertices that move in the first step; k_mesh_smooth_step, one lane
//      per vertex, once per step, walks the list in ascending w, gathers the neighbours' positions and applies the step.  The
//      positions between the steps live in two buffers; the last step writes the result's own array.  The positions stay 12 bytes a
//      vertex, three 32-bit loads a neighbour; staged once per call as 16 bytes, one 128-bit load, a step takes the same time and
//      gives the same bits (profiles/mesh_smooth/timing.txt has both times; apd_mesh_smooth_layout switches, for that tool).
// No LDS, no scratch memory (profiles/mesh_smooth/kres.txt).
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_mesh_compact.h"
#include "apd_mesh_host.h"
#include "apd_mesh_smooth_math.h"
#include "apd_points_host.h"
#include "apd_sort.h"

namespace {

using apd_fusion::kSmoothNoPair;
using apd_mesh_compact::clear_timing;
using apd_mesh_compact::err;
using apd_mesh_compact::into_new_mesh;
using apd_mesh_compact::MeshCall;
using apd_mesh_compact::new_mesh_like;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::ms_since;
using apd_points_host::Scratch;

static_assert(APD_SMOOTH_BOUNDARY_FIXED == apd_fusion::kSmoothFixed && APD_SMOOTH_BOUNDARY_ALONG == apd_fusion::kSmoothAlong &&
                  APD_SMOOTH_BOUNDARY_FREE == apd_fusion::kSmoothFree,
              "the modes of the header are the modes of the rules");

// 1: positions staged as 16 bytes a vertex; 0: read as they are.  On an MI355X a step takes the same time either way on a mesh of
// a million faces (profiles/mesh_smooth/timing.txt), so the layout that needs no staging is the one in use
std::atomic<int> g_smooth_wide{0};

// Face f < faces: its six keys
__global__ __launch_bounds__(256) void k_mesh_edge_keys(const int32_t *__restrict__ index, size_t faces, uint64_t *__restrict__ key)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= faces) {
        return;
    }
    uint64_t k[6];
    apd_fusion::smooth_face_keys(index[3 * f], index[3 * f + 1], index[3 * f + 2], k);
    for (int i = 0; i < 6; ++i) {
        key[6 * f + i] = k[i];
    }
}

// Sorted position i < n: head[i] = 1 where a distinct pair starts, multiplicity[i] = the length of its run there and 0 elsewhere
__global__ __launch_bounds__(256) void k_mesh_edge_heads(const uint64_t *__restrict__ key, size_t n, uint32_t *__restrict__ head,
                                                          uint32_t *__restrict__ multiplicity)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t mine = key[i];
    const bool first = mine != kSmoothNoPair && (i == 0 || key[i - 1] != mine);
    size_t j = i;
    if (first) {
        for (j = i + 1; j < n && key[j] == mine; ++j) {
        }
    }
    head[i] = first ? 1u : 0u;
    multiplicity[i] = (uint32_t)(j - i);
}

// Sorted position i < n with head[i], at[i] = heads before i: the entry of its pair in the neighbour lists
__global__ __launch_bounds__(256) void k_mesh_edge_compact(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                            const uint32_t *__restrict__ multiplicity, const uint64_t *__restrict__ at, size_t n,
                                                            uint32_t *__restrict__ neighbour)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && head[i]) {
        neighbour[at[i]] = apd_fusion::smooth_entry((uint32_t)key[i], multiplicity[i]);
    }
}

// Sorted position i < n of a pair (v, w): begin[v] where the pairs of v start, end[v] where they end; begin, end: zeros before
__global__ __launch_bounds__(256) void k_mesh_row_bounds(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                          const uint64_t *__restrict__ at, size_t n, uint32_t *__restrict__ begin,
                                                          uint32_t *__restrict__ end)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || key[i] == kSmoothNoPair) {
        return;
    }
    const uint32_t v = (uint32_t)(key[i] >> 32);
    if (i == 0 || (uint32_t)(key[i - 1] >> 32) != v) {
        begin[v] = (uint32_t)at[i];  // a head: the first pair of v
    }
    if (i == n - 1 || (uint32_t)(key[i + 1] >> 32) != v) {
        end[v] = (uint32_t)(at[i] + head[i]);
    }
}

// Vertex v < vertices: its number of neighbours, and whether one of its edges is a boundary edge
__global__ __launch_bounds__(256) void k_mesh_vertex_flags(const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                                                            const uint32_t *__restrict__ neighbour, size_t vertices, uint32_t *__restrict__ valence,
                                                            uint8_t *__restrict__ boundary)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    const uint32_t from = begin[v], to = end[v];
    bool open = false;
    for (uint32_t e = from; e < to; ++e) {
        open = open || apd_fusion::smooth_entry_boundary(neighbour[e]);
    }
    valence[v] = to - from;
    boundary[v] = open ? 1 : 0;
}

// Sorted position i < n: open[i] = 1 for the head of a pair v < w of multiplicity 1, many[i] = 1 for one of multiplicity 3 or more
__global__ __launch_bounds__(256) void k_mesh_edge_kinds(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                          const uint32_t *__restrict__ multiplicity, size_t n, uint32_t *__restrict__ open,
                                                          uint32_t *__restrict__ many)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const bool counted = head[i] && (uint32_t)(key[i] >> 32) < (uint32_t)key[i];
    open[i] = counted && multiplicity[i] == 1u ? 1u : 0u;
    many[i] = counted && apd_fusion::smooth_nonmanifold(multiplicity[i]) ? 1u : 0u;
}

// The position of vertex w in an array of Stride floats a vertex; Stride 4: 16-byte aligned, one load
template <int Stride> __device__ __forceinline__ void position(const float *__restrict__ p, size_t w, float &x, float &y, float &z)
{
    if constexpr (Stride == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p + 4 * w);
        x = q.x, y = q.y, z = q.z;
    } else {
        x = p[3 * w], y = p[3 * w + 1], z = p[3 * w + 2];
    }
}

// The step of contract C24 for vertex v: its new position in q; whether it moves
template <int Stride>
__device__ __forceinline__ bool smooth_vertex(const float *__restrict__ p, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                                              const uint32_t *__restrict__ neighbour, const uint8_t *__restrict__ boundary, size_t v, int mode, double k,
                                              float q[3])
{
    position<Stride>(p, v, q[0], q[1], q[2]);
    const bool open = boundary[v] != 0;
    if (apd_fusion::smooth_held(mode, open) || !apd_fusion::smooth_finite(q[0], q[1], q[2])) {
        return false;
    }
    double s[3] = {0.0, 0.0, 0.0};
    uint32_t count = 0;
    const uint32_t to = end[v];
    for (uint32_t e = begin[v]; e < to; ++e) {
        const uint32_t entry = neighbour[e];
        if (!apd_fusion::smooth_takes(mode, open, entry)) {
            continue;
        }
        float x, y, z;
        position<Stride>(p, apd_fusion::smooth_entry_vertex(entry), x, y, z);
        if (apd_fusion::smooth_finite(x, y, z)) {
            apd_fusion::smooth_add(s, x, y, z);
            ++count;
        }
    }
    if (count == 0) {
        return false;
    }
    q[0] = apd_fusion::smooth_place(q[0], s[0], count, k);
    q[1] = apd_fusion::smooth_place(q[1], s[1], count, k);
    q[2] = apd_fusion::smooth_place(q[2], s[2], count, k);
    return true;
}

// Vertex v < vertices: moves[v] = 1 where a step from p moves it
__global__ __launch_bounds__(256) void k_mesh_smooth_moves(const float *__restrict__ p, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                                                            const uint32_t *__restrict__ neighbour, const uint8_t *__restrict__ boundary, size_t vertices,
                                                            int mode, uint32_t *__restrict__ moves)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < vertices) {
        float q[3];
        moves[v] = smooth_vertex<3>(p, begin, end, neighbour, boundary, v, mode, 0.0, q) ? 1u : 0u;
    }
}

// Vertex v < vertices: its position as 16 bytes
__global__ __launch_bounds__(256) void k_mesh_smooth_stage(const float *__restrict__ xyz, size_t vertices, float4 *__restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < vertices) {
        out[v] = make_float4(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], 0.0f);
    }
}

// Vertex v < vertices: one step with the factor k from p (In floats a vertex) into out (Out floats a vertex); p and out are two arrays
template <int In, int Out>
__global__ __launch_bounds__(256) void k_mesh_smooth_step(const float *__restrict__ p, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                                                           const uint32_t *__restrict__ neighbour, const uint8_t *__restrict__ boundary, size_t vertices,
                                                           int mode, double k, float *__restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= vertices) {
        return;
    }
    float q[3];
    smooth_vertex<In>(p, begin, end, neighbour, boundary, v, mode, k, q);
    if constexpr (Out == 4) {
        *reinterpret_cast<float4 *>(out + 4 * v) = make_float4(q[0], q[1], q[2], 0.0f);
    } else {
        out[3 * v] = q[0];
        out[3 * v + 1] = q[1];
        out[3 * v + 2] = q[2];
    }
}

// The adjacency of one mesh in device memory of a call's scratch
struct Adjacency {
    size_t n = 0, pairs = 0;                        // sorted positions (6 F), distinct directed pairs
    uint64_t *key = nullptr, *at = nullptr;         // sorted keys; heads before each position, n + 1 entries
    uint32_t *head = nullptr, *multiplicity = nullptr;
    uint32_t *neighbour = nullptr, *begin = nullptr, *end = nullptr, *valence = nullptr;
    uint8_t *boundary = nullptr;
};

struct Call : MeshCall {
    // Steps 1 to 4 for m (with vertices and faces; 6 * faces < 2^32; its device is the current one)
    int adjacency(Scratch &scratch, const apd_mesh *m, Adjacency &a) const
    {
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        a.n = 6 * nf;
        uint64_t *keys[2] = {nullptr, nullptr};
        HIP_TRY(scratch.alloc(a.n * 8, &keys[0]));
        HIP_TRY(scratch.alloc(a.n * 8, &keys[1]));
        HIP_TRY(scratch.alloc((a.n + 1) * 8, &a.at));
        HIP_TRY(scratch.alloc(a.n * 4, &a.head));
        HIP_TRY(scratch.alloc(a.n * 4, &a.multiplicity));
        HIP_TRY(scratch.alloc(nv * 4, &a.begin));
        HIP_TRY(scratch.alloc(nv * 4, &a.end));
        HIP_TRY(scratch.alloc(nv * 4, &a.valence));
        HIP_TRY(scratch.alloc(nv, &a.boundary));
        hipLaunchKernelGGL(k_mesh_edge_keys, grid_of(nf), dim3(256), 0, 0, (const int32_t *)m->index, nf, keys[0]);
        HIP_TRY(hipGetLastError());
        int side = 0;
        HIP_TRY(apd_sort::sort_pairs(keys[0], keys[1], nullptr, nullptr, a.n, &side, nullptr));
        a.key = keys[side];
        hipLaunchKernelGGL(k_mesh_edge_heads, grid_of(a.n), dim3(256), 0, 0, (const uint64_t *)a.key, a.n, a.head, a.multiplicity);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(a.head, a.at, a.n));
        uint64_t found = 0;
        HIP_TRY(hipMemcpy(&found, a.at + a.n, 8, hipMemcpyDeviceToHost));
        a.pairs = (size_t)found;
        HIP_TRY(scratch.alloc(a.pairs * 4, &a.neighbour));
        HIP_TRY(hipMemsetAsync(a.begin, 0, nv * 4, 0));
        HIP_TRY(hipMemsetAsync(a.end, 0, nv * 4, 0));
        hipLaunchKernelGGL(k_mesh_edge_compact, grid_of(a.n), dim3(256), 0, 0, (const uint64_t *)a.key, (const uint32_t *)a.head,
                           (const uint32_t *)a.multiplicity, (const uint64_t *)a.at, a.n, a.neighbour);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_row_bounds, grid_of(a.n), dim3(256), 0, 0, (const uint64_t *)a.key, (const uint32_t *)a.head, (const uint64_t *)a.at, a.n,
                           a.begin, a.end);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_vertex_flags, grid_of(nv), dim3(256), 0, 0, (const uint32_t *)a.begin, (const uint32_t *)a.end,
                           (const uint32_t *)a.neighbour, nv, a.valence, a.boundary);
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // apd_mesh_adjacency of m (with vertices and faces) into host arrays of the call's own; counts[3]: edges, boundary, non-manifold
    int adjacency_of(const apd_mesh *m, uint32_t *valence, uint8_t *boundary, bool kinds, long long counts[3]) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices;
        Scratch scratch;
        Adjacency a;
        if (const int rc = adjacency(scratch, m, a); rc != APD_OK) {
            return rc;
        }
        counts[0] = (long long)(a.pairs / 2);
        if (kinds) {
            uint32_t *open = nullptr, *many = nullptr;
            uint64_t *sum = nullptr, total[2] = {0, 0};
            HIP_TRY(scratch.alloc(a.n * 4, &open));
            HIP_TRY(scratch.alloc(a.n * 4, &many));
            HIP_TRY(scratch.alloc((a.n + 1) * 8, &sum));
            hipLaunchKernelGGL(k_mesh_edge_kinds, grid_of(a.n), dim3(256), 0, 0, (const uint64_t *)a.key, (const uint32_t *)a.head,
                               (const uint32_t *)a.multiplicity, a.n, open, many);
            HIP_TRY(hipGetLastError());
            HIP_TRY(apd_sort::exclusive_scan(open, sum, a.n));
            HIP_TRY(hipMemcpy(&total[0], sum + a.n, 8, hipMemcpyDeviceToHost));
            HIP_TRY(apd_sort::exclusive_scan(many, sum, a.n));
            HIP_TRY(hipMemcpy(&total[1], sum + a.n, 8, hipMemcpyDeviceToHost));
            counts[1] = (long long)total[0];
            counts[2] = (long long)total[1];
        }
        if (valence) {
            HIP_TRY(hipMemcpy(valence, a.valence, nv * 4, hipMemcpyDeviceToHost));
        }
        if (boundary) {
            HIP_TRY(hipMemcpy(boundary, a.boundary, nv, hipMemcpyDeviceToHost));
        }
        HIP_TRY(hipDeviceSynchronize());
        apd_fusion::g_fusion_ms[1] = ms_since(t0);
        return APD_OK;
    }

    template <int In, int Out>
    int step(const Adjacency &a, const float *from, size_t nv, int mode, double k, float *to) const
    {
        hipLaunchKernelGGL((k_mesh_smooth_step<In, Out>), grid_of(nv), dim3(256), 0, 0, from, (const uint32_t *)a.begin, (const uint32_t *)a.end,
                           (const uint32_t *)a.neighbour, (const uint8_t *)a.boundary, nv, mode, k, to);
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // apd_mesh_smooth of m (with vertices; 6 * faces < 2^32) into `out`, which has colour as m and no normals
    int smooth(const apd_mesh *m, int iterations, float lambda, float mu, int mode, apd_mesh *out, long long *moved) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(m->device));
        const size_t nv = (size_t)m->vertices, nf = (size_t)m->faces;
        const bool wide = g_smooth_wide.load() != 0;
        Scratch scratch, made;
        if (const int rc = alloc(made, out, nv, nf); rc != APD_OK) {
            return rc;
        }
        float *between[2] = {nullptr, nullptr};
        uint32_t *moves = nullptr;
        uint64_t *moves_before = nullptr;
        if (nf > 0) {
            HIP_TRY(scratch.alloc(nv * (wide ? 16 : 12), &between[0]));
            HIP_TRY(scratch.alloc(nv * (wide ? 16 : 12), &between[1]));
            HIP_TRY(scratch.alloc(nv * 4, &moves));
            HIP_TRY(scratch.alloc((nv + 1) * 8, &moves_before));
        }
        apd_fusion::g_fusion_ms[0] = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (m->colour) {
            HIP_TRY(hipMemcpyAsync(out->bgr, m->bgr, nv * 3, hipMemcpyDeviceToDevice, 0));
        }
        *moved = 0;
        if (nf == 0) {
            HIP_TRY(hipMemcpyAsync(out->xyz, m->xyz, nv * 12, hipMemcpyDeviceToDevice, 0));
        } else {
            HIP_TRY(hipMemcpyAsync(out->index, m->index, nf * 12, hipMemcpyDeviceToDevice, 0));
            Adjacency a;
            if (const int rc = adjacency(scratch, m, a); rc != APD_OK) {
                return rc;
            }
            hipLaunchKernelGGL(k_mesh_smooth_moves, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, (const uint32_t *)a.begin, (const uint32_t *)a.end,
                               (const uint32_t *)a.neighbour, (const uint8_t *)a.boundary, nv, mode, moves);
            HIP_TRY(hipGetLastError());
            HIP_TRY(apd_sort::exclusive_scan(moves, moves_before, nv));
            uint64_t found = 0;
            HIP_TRY(hipMemcpy(&found, moves_before + nv, 8, hipMemcpyDeviceToHost));
            *moved = (long long)found;
            const int per = mu != 0.0f ? 2 : 1, steps = iterations * per;
            const float *from = m->xyz;
            if (wide) {
                hipLaunchKernelGGL(k_mesh_smooth_stage, grid_of(nv), dim3(256), 0, 0, (const float *)m->xyz, nv, reinterpret_cast<float4 *>(between[1]));
                HIP_TRY(hipGetLastError());
                from = between[1];
            }
            for (int s = 0; s < steps; ++s) {
                const double k = (double)(s % per == 0 ? lambda : mu);
                const bool last = s == steps - 1;
                float *to = last ? out->xyz : between[s & 1];
                const int rc = wide ? (last ? step<4, 3>(a, from, nv, mode, k, to) : step<4, 4>(a, from, nv, mode, k, to)) : step<3, 3>(a, from, nv, mode, k, to);
                if (rc != APD_OK) {
                    return rc;
                }
                from = to;
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        keep(made, out);
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }

    // What both calls refuse of a mesh
    int too_many_faces(const apd_mesh *m) const
    {
        if (6 * m->faces >= (1LL << 32)) {
            return apd::set_error(err(), APD_ERR_UNSUPPORTED, "%s: %lld faces, whose 6 directed pairs each are 2^32 or more (a neighbour list's position is 32-bit)",
                                  who, m->faces);
        }
        return APD_OK;
    }
};

}  // namespace

// Which layout apd_mesh_smooth gives the positions between its steps: 1, 16 bytes a vertex; 0, 12.  Returns the one before.  The
// result's bits do not depend on it; tools/mesh_smooth_time.py times both and tests/test_gpu_mesh_smooth.py compares them
extern "C" int apd_mesh_smooth_layout(int wide) { return g_smooth_wide.exchange(wide != 0 ? 1 : 0); }

extern "C" int apd_mesh_adjacency(apd_mesh_t m, uint32_t *valence, uint8_t *boundary, long long *edges, long long *boundary_edges,
                                  long long *nonmanifold_edges)
{
    const Call call{{{"apd_mesh_adjacency"}}};
    err().clear();
    if (!m) {
        return call.invalid("null argument");
    }
    if (!valence && !boundary && !edges && !boundary_edges && !nonmanifold_edges) {
        return call.invalid("every output is null");
    }
    if (const int rc = call.too_many_faces(m); rc != APD_OK) {
        return rc;
    }
    clear_timing();
    const size_t nv = (size_t)m->vertices;
    long long counts[3] = {0, 0, 0};
    std::vector<uint32_t> degree(valence ? nv : 0, 0u);
    std::vector<uint8_t> open(boundary ? nv : 0, (uint8_t)0);
    if (m->faces > 0) {
        DeviceScope scope(true);
        if (const int rc = call.adjacency_of(m, valence ? degree.data() : nullptr, boundary ? open.data() : nullptr, boundary_edges || nonmanifold_edges, counts);
            rc != APD_OK) {
            return rc;
        }
    }
    std::copy(degree.begin(), degree.end(), valence);
    std::copy(open.begin(), open.end(), boundary);
    if (edges) {
        *edges = counts[0];
    }
    if (boundary_edges) {
        *boundary_edges = counts[1];
    }
    if (nonmanifold_edges) {
        *nonmanifold_edges = counts[2];
    }
    return APD_OK;
}

extern "C" int apd_mesh_smooth(apd_mesh_t m, int iterations, float lambda, float mu, int boundary, apd_mesh_t *out, long long *moved)
{
    const Call call{{{"apd_mesh_smooth"}}};
    err().clear();
    if (!m || !out) {
        return call.invalid("null argument");
    }
    if (iterations < 1 || iterations > 1000) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: %d iterations, outside 1 .. 1000", call.who, iterations);
    }
    if (!(lambda > 0.0f && lambda <= 1.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a lambda of %g, not in (0, 1]", call.who, (double)lambda);
    }
    if (!(mu >= -2.0f && mu <= 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: a mu of %g, not in [-2, 0]", call.who, (double)mu);
    }
    if (boundary != APD_SMOOTH_BOUNDARY_FIXED && boundary != APD_SMOOTH_BOUNDARY_ALONG && boundary != APD_SMOOTH_BOUNDARY_FREE) {
        return apd::set_error(err(), APD_ERR_INVALID, "%s: boundary mode %d, none of APD_SMOOTH_BOUNDARY_FIXED, _ALONG and _FREE", call.who, boundary);
    }
    if (const int rc = call.too_many_faces(m); rc != APD_OK) {
        return rc;
    }
    apd_mesh *like = new_mesh_like(m);
    like->normals = 0;
    apd_mesh_t result = nullptr;
    long long found = 0;
    const int rc = into_new_mesh(m, like, &result, [&](apd_mesh *r) { return call.smooth(m, iterations, lambda, mu, boundary, r, &found); });
    if (rc != APD_OK) {
        return rc;
    }
    *out = result;
    if (moved) {
        *moved = found;
    }
    return APD_OK;
}
