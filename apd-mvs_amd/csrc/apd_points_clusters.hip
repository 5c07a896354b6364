// apd_points_clusters.hip -- apd_points_components and apd_points_remove_small_components of include/apd_mi355x.h: the connected
// components of the graph whose edges are the neighbour pairs of contract C11, and the object without the points of the
// components that have too few (contract C13).
//
// Contract C13.  Vertices: the points of the object.  Edge {i, j}: j is a neighbour of i by C11 (apd_radius_math.h) on the grid of
// cell size `radius` at the origin given; the relation is symmetric.  A point outside the grid has no edge and is a component of
// its own.  label[i] = the smallest input index among the points of i's component, size[i] = their number (below 2^31).  Both
// are functions of the input alone.  Kept by the removal: size[i] >= min_size, in input order; min_size 0 and 1 keep every point.
//
// On the points' device, on its null stream, after the refusals and the cell order of apd_points_search.h.  Everything between
// the sort and the last step works on SORTED POSITIONS: lanes of a wave are neighbours in space.
//   1. k_cluster_init: parent[v] = v, root_min[v] = 2^32 - 1, root_size[v] = 0.
//   2. k_cluster_link: one lane per sorted position i.  The walk over the 27 cells (for_each_candidate of apd_points_search.h, the
//      one of the other three searches) with end = i: it visits the positions in ascending order and stops before the first one
//      >= i, everything after that being above i too, and since the relation is symmetric every edge is seen exactly once, from
//      its higher end.  Every candidate within the radius is unite(i, at) on parent[], a lock-free union-find:
//        find(v)      follows parent[] to the slot that names itself, halving the path on the way (fetch_min of the
//                     grandparent into the slot it came from);
//        unite(a, b)  finds both roots, and hooks the larger under the smaller with a compare-and-swap on parent[larger] that
//                     expects `larger` itself; when the swap fails the slot holds somebody else's hook, and the lane goes on from
//                     the value the swap returned.
//      Invariants of parent[], kept by every one of these writes:
//        (a) parent[v] <= v;
//        (b) a slot only ever decreases: the swap replaces v by something smaller, fetch_min cannot increase;
//        (c) a slot always names a point of the same component of the graph: a hook joins the roots of the two ends of an edge,
//            and the halving writes an ancestor, which by induction is in the component.
//      From (a): no cycles, and the root of a tree is its smallest position.  From (b): the halving cannot undo a hook -- a slot
//      that no longer names itself never names itself again --, and being in one tree is for good.  A failed swap means that
//      another lane's swap on that slot succeeded: somebody made progress, nobody waits for anybody, and the number of hooks is
//      below m.  When the kernel ends every edge has been united, so the trees are the components.
//      Every access to parent[] in this kernel is a relaxed atomic of agent scope: a plain store can stay invisible to a wave
//      on another XCD, whose L2 is not coherent with this one's, and a plain load can be served from a stale L1 line.  No order
//      between different slots is needed: whatever a lane reads from a slot is a value the slot held, and (a) to (c) hold for
//      every such value.
//      Before a full unite the lane compares the two parents it has just loaded: equal means one tree already.  In a dense cell
//      nearly every edge ends there.
//   3. k_cluster_flatten, a launch of its own, so that its finds read a forest nobody hooks in: root[i] = find(i), the smallest
//      sorted position of the component.
//   4. k_cluster_reduce: root_min[root[i]] = min over the component of member[i], root_size[root[i]] = its number, by integer
//      atomics, whose result does not depend on the order of arrival.  A surface is one component of millions of points, and
//      one atomic per lane would queue them all on one address; so the lanes of a wave that hold the same root are combined
//      first (a loop over the distinct roots of the wave: broadcast of the first pending lane's root, ballot of the lanes that
//      hold it, a butterfly minimum) and the wave issues one min and one add per distinct root it holds.
//      -DAPD_LAB_CLUSTER_REDUCE_NAIVE (apd_lab.h) builds the one-atomic-per-lane form, for tools/points_clusters_time.py.
//   5. k_cluster_fill: label[k] = k, size[k] = 1 (what a point outside the grid keeps); k_cluster_emit: label[member[i]] =
//      root_min[root[i]], size[member[i]] = root_size[root[i]].
//   6. the number of components: the flags label[k] == k through apd_sort::exclusive_scan.
//   7. removal: flags size[k] >= min_size (k_keep_flags of apd_points_search.h), compact_points (apd_points.hip).  With
//      min_size <= 1 and no caller for the number of components nothing is labelled.
// No LDS, no scratch memory.  The work of the link step is half that of apd_points_neighbour_counts without a cap.  There is no
// host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_lab.h"
#include "apd_points_host.h"
#include "apd_points_search.h"
#include "apd_radius_math.h"

namespace {

using apd_fusion::PointArrays;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::for_each_candidate;
using apd_points_search::k_keep_flags;
using apd_points_search::Search;
using apd_points_search::Sorted;
using apd_points_search::Staged;

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
// passes.
__global__ __launch_bounds__(256) void k_cluster_link(const uint64_t *__restrict__ keys, const float *__restrict__ xyz, uint32_t m, float r2,
                                                       uint32_t *parent)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // m < 2^31
    if (i >= m) {
        return;
    }
    const float P[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    for_each_candidate(keys, xyz, i, i, [&](uint32_t at, const float Q[3]) {
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

// root_min[r] = min of member[i], root_size[r] = number of the i with root[i] == r; both k_cluster_init's.  Every lane of the
// workgroup stays to the end: the loop's ballots and shuffles are the whole wave's
__global__ __launch_bounds__(256) void k_cluster_reduce(const uint32_t *__restrict__ root, const uint32_t *__restrict__ member, uint32_t m,
                                                         uint32_t *root_min, uint32_t *root_size)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool mine = i < m;
    const uint32_t r = mine ? root[i] : 0xFFFFFFFFu, k = mine ? member[i] : 0xFFFFFFFFu;
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

__global__ __launch_bounds__(256) void k_cluster_emit(const uint32_t *__restrict__ root, const uint32_t *__restrict__ member, uint32_t m,
                                                       const uint32_t *__restrict__ root_min, const uint32_t *__restrict__ root_size,
                                                       uint32_t *__restrict__ label, uint32_t *__restrict__ size)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        const uint32_t r = root[i], k = member[i];
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

// One call of either entry point: the refusals and the cell order of apd_points_search.h, and the steps the two share
struct Call : Search {
    // label[k] = k and size[k] = 1 for the n > 0 points; all in device memory on the current device
    int fill(size_t n, uint32_t *label, uint32_t *size) const
    {
        hipLaunchKernelGGL(k_cluster_fill, grid_of(n), dim3(256), 0, 0, n, label, size);
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // label[k] and size[k] by contract C13 for the n > 0 points at xyz, and their number of components (may be null)
    int label_points(const float *xyz, size_t n, uint32_t *label, uint32_t *size, long long *components) const
    {
        Scratch scratch;
        if (const int rc = fill(n, label, size); rc != APD_OK) {
            return rc;
        }
        Sorted s;
        if (const int rc = sort_into_cells(scratch, xyz, n, s); rc != APD_OK) {
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
            hipLaunchKernelGGL(k_cluster_link, grid_of(s.m), dim3(256), 0, 0, s.keys, s.xyz, m, grid.size * grid.size, parent);
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
            uint32_t *own = nullptr;
            uint64_t *before = nullptr;
            HIP_TRY(scratch.alloc(n * 4, &own));
            HIP_TRY(scratch.alloc((n + 1) * 8, &before));
            hipLaunchKernelGGL(k_cluster_own_flags, grid_of(n), dim3(256), 0, 0, (const uint32_t *)label, n, own);
            HIP_TRY(hipGetLastError());
            HIP_TRY(apd_sort::exclusive_scan(own, before, n));
            uint64_t total = 0;
            HIP_TRY(hipMemcpy(&total, before + n, 8, hipMemcpyDeviceToHost));
            *components = (long long)total;
        }
        HIP_TRY(hipDeviceSynchronize());
        return APD_OK;
    }

    // apd_points_components of p (count > 0); the sizes are computed whether the caller wants them or not
    int components_of(apd_points_t p, uint32_t *label, uint32_t *size, long long *components) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        const float *xyz = nullptr;
        Staged<uint32_t> out_label, out_size;
        int rc = positions(scratch, p, &xyz);
        rc = rc != APD_OK ? rc : stage(scratch, p, label, n * 4, out_label);
        rc = rc != APD_OK ? rc : stage(scratch, p, size, n * 4, out_size);
        if (rc != APD_OK) {
            return rc;
        }
        if (!size) {  // not wanted and so not staged, but label_points writes the sizes: scratch that nothing brings down (host is null)
            HIP_TRY(scratch.alloc(n * 4, &out_size.device));
        }
        rc = label_points(xyz, n, out_label.device, out_size.device, components);
        rc = rc != APD_OK ? rc : download(out_label);
        return rc != APD_OK ? rc : download(out_size);
    }

    // apd_points_remove_small_components of p (count > 0) into `result`
    int remove_small(apd_points_t p, uint32_t min_size, apd_points *result, long long *components) const
    {
        const size_t n = (size_t)p->count;
        Scratch scratch;
        PointArrays in;
        if (const int rc = device_arrays(scratch, p, in); rc != APD_OK) {
            return rc;
        }
        uint32_t *label = nullptr, *size = nullptr, *keep = nullptr;
        HIP_TRY(scratch.alloc(n * 4, &label));
        HIP_TRY(scratch.alloc(n * 4, &size));
        HIP_TRY(scratch.alloc(n * 4, &keep));
        if (min_size <= 1 && !components) {  // every point stays, those outside the grid too, and nobody asks for the components
            if (const int rc = fill(n, label, size); rc != APD_OK) {
                return rc;
            }
        } else if (const int rc = label_points(in.xyz, n, label, size, components); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_keep_flags, grid_of(n), dim3(256), 0, 0, (const uint32_t *)size, n, min_size, keep);
        HIP_TRY(hipGetLastError());
        return apd_points_host::compact_points(who, p, in, keep, result);
    }
};

}  // namespace

extern "C" int apd_points_components(apd_points_t p, float radius, const float *origin3, uint32_t *label, uint32_t *size, long long *components)
{
    Call call{{"apd_points_components"}};
    if (const int rc = call.check(p, label, radius, origin3); rc != APD_OK) {
        return rc;
    }
    long long found = 0;
    if (p->count > 0) {
        DeviceScope scope(true);
        if (const int rc = call.components_of(p, label, size, components ? &found : nullptr); rc != APD_OK) {
            return rc;
        }
    }
    if (components) {
        *components = found;
    }
    return APD_OK;
}

extern "C" int apd_points_remove_small_components(apd_points_t p, float radius, const float *origin3, unsigned min_size, apd_points_t *out,
                                                  long long *removed, long long *components)
{
    Call call{{"apd_points_remove_small_components"}};
    if (const int rc = call.check(p, out, radius, origin3); rc != APD_OK) {
        return rc;
    }
    long long found = 0;
    const auto body = [&](apd_points *result) { return call.remove_small(p, min_size, result, components ? &found : nullptr); };
    const int rc = call.into_new_points(p, out, removed, body);
    if (rc == APD_OK && components) {
        *components = found;
    }
    return rc;
}
