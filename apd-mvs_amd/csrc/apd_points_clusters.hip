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
//   1. - 6. the labelling of apd_union_find.h (Labelling::label_points), which apd_mesh_weld shares: k_cluster_init; k_cluster_link,
//      one lane per sorted position i, the walk over the 27 cells (for_each_candidate of apd_points_search.h, the one of the other
//      three searches) with end = i: it visits the positions in ascending order and stops before the first one >= i, everything
//      after that being above i too, and since the relation is symmetric every edge is seen exactly once, from its higher end;
//      every candidate within the radius is unite(i, at) on parent[], the lock-free union-find whose invariants that header
//      states; k_cluster_flatten, a launch of its own, so that its finds read a forest nobody hooks in; k_cluster_reduce, integer
//      atomics combined per wave; k_cluster_fill and k_cluster_emit; the number of components through apd_sort::exclusive_scan.
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
#include "apd_union_find.h"

namespace {

using apd_fusion::PointArrays;
using apd_points_grid::grid_of;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_search::k_keep_flags;
using apd_points_search::Search;
using apd_points_search::Sorted;
using apd_points_search::Staged;

// One call of either entry point: the refusals and the cell order of apd_points_search.h, and the steps the two share
struct Call : Search {
    apd_union_find::Labelling labelling() const { return apd_union_find::Labelling{*this}; }

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
        rc = labelling().label_points(xyz, n, out_label.device, out_size.device, components);
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
            if (const int rc = labelling().fill(n, label, size); rc != APD_OK) {
                return rc;
            }
        } else if (const int rc = labelling().label_points(in.xyz, n, label, size, components); rc != APD_OK) {
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
