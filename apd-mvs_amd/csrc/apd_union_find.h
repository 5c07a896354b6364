// apd_union_find.h -- the lock-free union-find of the library and the kernels around it, shared by apd_points_clusters.hip (the
// components of a cloud, contract C13) and apd_mesh.hip (welding: C13 over the vertex positions; the components of the faces: the
// same forest over the vertex indices).  Device code: hipcc only.
//
// parent[]: one slot per element, set to its own index by k_cluster_init.
//   find(v)      follows parent[] to the slot that names itself, halving the path on the way (fetch_min of the grandparent into
//                the slot it came from);
//   unite(a, b)  finds both roots, and hooks the larger under the smaller with a compare-and-swap on parent[larger] that expects
//                `larger` itself; when the swap fails the slot holds somebody else's hook, and the lane goes on from the value the
//                swap returned.
// Invariants of parent[], kept by every one of these writes:
//   (a) parent[v] <= v;
//   (b) a slot only ever decreases: the swap replaces v by something smaller, fetch_min cannot increase;
//   (c) a slot always names an element of the same component of the graph: a hook joins the roots of the two ends of an edge, and
//       the halving writes an ancestor, which by induction is in the component.
// From (a): no cycles, and the root of a tree is its smallest element.  From (b): the halving cannot undo a hook -- a slot that no
// longer names itself never names itself again --, and being in one tree is for good.  A failed swap means that another lane's swap
// on that slot succeeded: somebody made progress, nobody waits for anybody, and the number of hooks is below the number of
// elements.  When the kernel that unites ends, every edge has been united, so the trees are the components.
// Every access to parent[] while lanes unite is a relaxed atomic of agent scope: a plain store can stay invisible to a wave on
// another XCD, whose L2 is not coherent with this one's, and a plain load can be served from a stale L1 line.  No order between
// different slots is needed: whatever a lane reads from a slot is a value the slot held, and (a) to (c) hold for every such value.
//
// The steps of a labelling, each a launch of its own:
//   k_cluster_init     parent[v] = v, root_min[v] = 2^32 - 1, root_size[v] = 0.
//   (the caller's link kernel: k_cluster_link here for the neighbour pairs of contract C11, k_mesh_link of apd_mesh.hip for faces)
//   k_cluster_flatten  root[i] = find(i), in a forest nobody hooks in: the smallest element of the component.
//   k_cluster_reduce   root_min[root[i]] = min over the component of member[i], root_size[root[i]] = its number, by integer
//                      atomics, whose result does not depend on the order of arrival.  A surface is one component of millions of
//                      elements, and one atomic per lane would queue them all on one address; so the lanes of a wave that hold the
//                      same root are combined first (a loop over the distinct roots of the wave: broadcast of the first pending
//                      lane's root, ballot of the lanes that hold it, a butterfly minimum) and the wave issues one min and one add
//                      per distinct root it holds.  -DAPD_LAB_CLUSTER_REDUCE_NAIVE (apd_lab.h) builds the one-atomic-per-lane form,
//                      for tools/points_clusters_time.py.
//   k_cluster_fill     label[k] = k, size[k] = 1 (what an element without edges keeps); k_cluster_emit: label[member[i]] =
//                      root_min[root[i]], size[member[i]] = root_size[root[i]].
//   k_cluster_own_flags and apd_sort::exclusive_scan: the number of components, the k with label[k] == k.
// label_points is contract C13 whole, for the n points at xyz on the grid of a Search: what apd_points_components writes and what
// apd_mesh_weld takes its representatives from.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "apd_lab.h"
#include "apd_points_search.h"
#include "apd_radius_math.h"

namespace apd_union_find {
namespace {

using apd_points_grid::grid_of;
using apd_points_host::Scratch;

__device__ __forceinline__ uint32_t parent_of(uint32_t *parent, uint32_t v)
{
    return __hip_atomic_load(&parent[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of v's tree at some moment between the call and the return; halves the path it walks
__device__ __forceinline__ uint32_t find(uint32_t *parent, uint32_t v)
{
    for (;;) {
        const uint32_t p = parent_of(parent, v);
        if (p == v) {
            return v;
        }
        const uint32_t g = parent_of(parent, p);
        if (g == p) {
            return p;
        }
        __hip_atomic_fetch_min(&parent[v], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // g < p <= what the slot held
        v = g;
    }
}

// a and b, the two ends of an edge, are in one tree when this returns
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) {
            return;
        }
        const uint32_t larger = a > b ? a : b, smaller = a > b ? b : a;
        uint32_t held = larger;
        if (__hip_atomic_compare_exchange_strong(&parent[larger], &held, smaller, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            return;
        }
        a = held;  // somebody else's hook of `larger`: below it, in the component
        b = smaller;
    }
}

__global__ __launch_bounds__(256) void k_cluster_init(uint32_t m, uint32_t *__restrict__ parent, uint32_t *__restrict__ root_min,
                                                       uint32_t *__restrict__ root_size)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i < m) {
        parent[i] = i;
        root_min[i] = 0xFFFFFFFFu;
        root_size[i] = 0;
    }
}

// Sorted element i < m: unites i with every neighbour (contract C11) at a sorted position below i.  keys: ascending; xyz: in the
// same order; parent: k_cluster_init's.  The walk's searches and runs end at position i, which no read of a candidate reaches or
// passes.  Before a full unite the lane compares the two parents it has just loaded: equal means one tree already.  In a dense cell
// nearly every edge ends there.
__global__ __launch_bounds__(256) void k_cluster_link(const uint64_t *__restrict__ keys, const float *__restrict__ xyz, uint32_t m, float r2,
                                                       uint32_t *parent)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    apd_points_search::for_each_candidate(keys, xyz, i, i, [&](uint32_t at, const float Q[3]) {
        if (apd_fusion::radius_within(P, Q, r2) && parent_of(parent, i) != parent_of(parent, at)) {
            unite(parent, i, at);
        }
        return false;
    });
}

__global__ __launch_bounds__(256) void k_cluster_flatten(uint32_t m, uint32_t *parent, uint32_t *__restrict__ root)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        root[i] = find(parent, i);
    }
}

// root_min[r] = min of member[i] (member null: of i itself), root_size[r] = number of the i with root[i] == r; both
// k_cluster_init's.  Every lane of the workgroup stays to the end: the loop's ballots and shuffles are the whole wave's
__global__ __launch_bounds__(256) void k_cluster_reduce(const uint32_t *__restrict__ root, const uint32_t *__restrict__ member, uint32_t m,
                                                         uint32_t *root_min, uint32_t *root_size)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool mine = i < m;
    const uint32_t r = mine ? root[i] : 0xFFFFFFFFu, k = mine ? (member ? member[i] : i) : 0xFFFFFFFFu;
#if APD_CLUSTER_REDUCE_COMBINED
    const uint32_t lane = threadIdx.x & 63;
    uint64_t pending = __ballot(mine);
    while (pending != 0) {  // the same in every lane
        const int first = __ffsll((unsigned long long)pending) - 1;
        const uint32_t r0 = __shfl(r, first, 64);
        const uint64_t same = __ballot(mine && r == r0);  // holds `first`
        uint32_t least = mine && r == r0 ? k : 0xFFFFFFFFu;
        if (same != ((uint64_t)1 << first)) {
            for (int step = 32; step >= 1; step >>= 1) {
                const uint32_t other = __shfl_xor(least, step, 64);
                least = other < least ? other : least;
            }
        }
        if (lane == (uint32_t)first) {
            __hip_atomic_fetch_min(&root_min[r0], least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&root_size[r0], (uint32_t)__popcll((unsigned long long)same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        pending &= ~same;
    }
#else
    if (mine) {
        __hip_atomic_fetch_min(&root_min[r], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&root_size[r], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
}

__global__ __launch_bounds__(256) void k_cluster_fill(size_t n, uint32_t *__restrict__ label, uint32_t *__restrict__ size)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        label[k] = (uint32_t)k;
        size[k] = 1;
    }
}

// member null: element i is its own member
__global__ __launch_bounds__(256) void k_cluster_emit(const uint32_t *__restrict__ root, const uint32_t *__restrict__ member, uint32_t m,
                                                       const uint32_t *__restrict__ root_min, const uint32_t *__restrict__ root_size,
                                                       uint32_t *__restrict__ label, uint32_t *__restrict__ size)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        const uint32_t r = root[i], k = member ? member[i] : i;
        label[k] = root_min[r];
        size[k] = root_size[r];
    }
}

// flag[k] = 1 where label[k] == k: one per component
__global__ __launch_bounds__(256) void k_cluster_own_flags(const uint32_t *__restrict__ label, size_t n, uint32_t *__restrict__ flag)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        flag[k] = label[k] == (uint32_t)k ? 1u : 0u;
    }
}

// The host side of one labelling, for a call whose refusals and grid are `search`'s (its hip_failed names the entry point)
struct Labelling {
    const apd_points_search::Search &search;

    int hip_failed(const char *expr, hipError_t e, const char *file, int line) const { return search.hip_failed(expr, e, file, line); }

    // label[k] = k and size[k] = 1 for the n > 0 elements; all in device memory on the current device
    int fill(size_t n, uint32_t *label, uint32_t *size) const
    {
        hipLaunchKernelGGL(k_cluster_fill, grid_of(n), dim3(256), 0, 0, n, label, size);
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // *components = the number of k < n with label[k] == k
    int count_own(const uint32_t *label, size_t n, long long *components) const
    {
        Scratch scratch;
        uint32_t *own = nullptr;
        uint64_t *before = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &own));
        HIP_TRY(scratch.alloc((n + 1) * 8, &before));
        hipLaunchKernelGGL(k_cluster_own_flags, grid_of(n), dim3(256), 0, 0, label, n, own);
        HIP_TRY(hipGetLastError());
        HIP_TRY(apd_sort::exclusive_scan(own, before, n));
        uint64_t total = 0;
        HIP_TRY(hipMemcpy(&total, before + n, 8, hipMemcpyDeviceToHost));
        *components = (long long)total;
        return APD_OK;
    }

    // label[k] and size[k] by contract C13 for the n > 0 points at xyz, and their number of components (may be null)
    int label_points(const float *xyz, size_t n, uint32_t *label, uint32_t *size, long long *components) const
    {
        Scratch scratch;
        if (const int rc = fill(n, label, size); rc != APD_OK) {
            return rc;
        }
        apd_points_search::Sorted s;
        if (const int rc = search.sort_into_cells(scratch, xyz, n, s); rc != APD_OK) {
            return rc;
        }
        if (s.m > 0) {
            const uint32_t m = (uint32_t)s.m;
            uint32_t *parent = nullptr, *root = nullptr, *root_min = nullptr, *root_size = nullptr;
            HIP_TRY(scratch.alloc(s.m * 4, &parent));
            HIP_TRY(scratch.alloc(s.m * 4, &root));
            HIP_TRY(scratch.alloc(s.m * 4, &root_min));
            HIP_TRY(scratch.alloc(s.m * 4, &root_size));
            hipLaunchKernelGGL(k_cluster_init, grid_of(s.m), dim3(256), 0, 0, m, parent, root_min, root_size);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_cluster_link, grid_of(s.m), dim3(256), 0, 0, s.keys, s.xyz, m, search.grid.size * search.grid.size, parent);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_cluster_flatten, grid_of(s.m), dim3(256), 0, 0, m, parent, root);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_cluster_reduce, grid_of(s.m), dim3(256), 0, 0, (const uint32_t *)root, s.member, m, root_min, root_size);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_cluster_emit, grid_of(s.m), dim3(256), 0, 0, (const uint32_t *)root, s.member, m, (const uint32_t *)root_min,
                               (const uint32_t *)root_size, label, size);
            HIP_TRY(hipGetLastError());
        }
        if (components) {
            if (const int rc = count_own(label, n, components); rc != APD_OK) {
                return rc;
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }
};

}  // namespace
}  // namespace apd_union_find
