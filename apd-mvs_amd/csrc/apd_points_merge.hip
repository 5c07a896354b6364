// apd_points_merge.hip -- apd_points_merge_voxels of include/apd_mi355x.h: one point per occupied cell of a cubic grid, with the
// union of its members' visibility lists (arithmetic contract C10; the cell and the key: apd_voxel_math.h).
//
// On the points' device, on top of the sort and the scan of apd_sort.h (steps 1 and 2: apd_points_grid.h, shared with
// apd_points_radius.hip):
//   1. k_voxel_keys: the key of every point and whether it is kept.
//   2. scan of the keep flags, k_voxel_compact: (key, input index) of the kept points, in input order.
//   3. sort_pairs: stable, so the members of a cell stand in ascending input index.
//   4. k_run_heads, scan: the first element of every cell, and from the scan the rank of every element's cell.
//   5. k_cell_starts, k_cell_merge: one lane per cell adds its members up in member order.
//   6. the lists: k_list_lengths, scan, k_list_expand write rank * num_views + view for every entry of every member's input list;
//      sort_pairs (keys only); k_run_heads, scan, k_list_emit keep the first of every run: per cell its distinct views, ascending;
//      k_cell_offsets: every cell's offset, also of a cell whose members have no entries.
//   7. k_cell_support: support from the length of a cell's list.
// There is no host path: host-resident points go up, the result comes down.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <chrono>
#include <string>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_grid.h"
#include "apd_points_host.h"
#include "apd_sort.h"
#include "apd_voxel_math.h"

namespace {

using apd_fusion::PointArrays;
using apd_points_grid::Grid;
using apd_points_grid::grid_of;
using apd_points_grid::k_voxel_compact;
using apd_points_grid::k_voxel_keys;
using apd_points_host::DeviceScope;
using apd_points_host::Scratch;
using apd_points_host::ms_since;

// head[i] = 1 where sorted key i differs from its predecessor: the first element of a cell, or of a (cell, view) run of the lists
__global__ __launch_bounds__(256) void k_run_heads(const uint64_t *__restrict__ keys, size_t n, uint32_t *__restrict__ head)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    }
}

// before[i]: heads before element i, so the head of cell c has before == c.  start[c]: the cell's first element; start[cells] = m
__global__ __launch_bounds__(256) void k_cell_starts(const uint32_t *__restrict__ head, const uint64_t *__restrict__ before, size_t m,
                                                      uint32_t *__restrict__ start)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) {
        return;
    }
    if (head[i]) {
        start[before[i]] = (uint32_t)i;
    }
    if (i == 0) {
        start[before[m]] = (uint32_t)m;
    }
}

// Cell c < cells: the sums of contract C10 over its members index[start[c] .. start[c + 1]), in that order.  One lane per cell,
// because the order of a binary32 sum is the contract: a cell with very many members (a whole cloud in one cell) is one long
// lane, and that is accepted.  Gathers through `index`; no LDS, no atomics.
__global__ __launch_bounds__(256) void k_cell_merge(size_t cells, const uint32_t *__restrict__ start, const uint32_t *__restrict__ index,
                                                     PointArrays in, PointArrays out)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) {
        return;
    }
    const uint32_t first = start[c], end = start[c + 1];
    const size_t r = index[first];  // the representative
    float sumP[3] = {in.xyz[3 * r], in.xyz[3 * r + 1], in.xyz[3 * r + 2]};
    float sumN[3] = {in.normal[3 * r], in.normal[3 * r + 1], in.normal[3 * r + 2]};
    uint64_t sumC[3] = {in.bgr[3 * r], in.bgr[3 * r + 1], in.bgr[3 * r + 2]};
    for (uint32_t e = first + 1; e < end; ++e) {
        const size_t k = index[e];
        for (int a = 0; a < 3; ++a) {
            sumP[a] += in.xyz[3 * k + a];
            sumN[a] += in.normal[3 * k + a];
            sumC[a] += in.bgr[3 * k + a];
        }
    }
    const uint64_t m = end - first;
    const float count = (float)m;
    float meanN[3];
    apd_fusion::mean_normal(sumN, count, meanN);
    for (int a = 0; a < 3; ++a) {
        out.xyz[3 * c + a] = sumP[a] / count;
        out.normal[3 * c + a] = meanN[a];
        out.bgr[3 * c + a] = (uint8_t)((sumC[a] + m / 2) / m);
    }
    out.view[c] = in.view[r];
    out.pixel[c] = in.pixel[r];
    out.sources[c] = in.sources[r];
}

// length[i]: entries of the input list of sorted element i
__global__ __launch_bounds__(256) void k_list_lengths(const uint32_t *__restrict__ index, size_t m, const long long *__restrict__ offsets,
                                                       uint32_t *__restrict__ length)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        const size_t k = index[i];
        length[i] = (uint32_t)(offsets[k + 1] - offsets[k]);
    }
}

// keys[at[i] + j] = cell of element i * num_views + the j-th view of its input list; the cell is (heads up to and with i) - 1
__global__ __launch_bounds__(256) void k_list_expand(const uint32_t *__restrict__ index, size_t m, const long long *__restrict__ offsets,
                                                      const int32_t *__restrict__ views, const uint64_t *__restrict__ before,
                                                      const uint64_t *__restrict__ at, uint64_t num_views, uint64_t *__restrict__ keys)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) {
        return;
    }
    const size_t k = index[i];
    const uint64_t cell = before[i + 1] - 1;
    uint64_t *to = keys + at[i];
    for (long long e = offsets[k]; e < offsets[k + 1]; ++e) {
        *to++ = cell * num_views + (uint64_t)views[e];
    }
}

// The first entry of every (cell, view) run of the sorted list keys goes to position before[i] of the merged lists; the first of
// a cell is the cell's offset (k_cell_offsets writes the same, and that of a cell without entries).
__global__ __launch_bounds__(256) void k_list_emit(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ head,
                                                    const uint64_t *__restrict__ before, size_t entries, uint64_t num_views, size_t cells,
                                                    long long *__restrict__ vis_offsets, int32_t *__restrict__ vis_views)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= entries) {
        return;
    }
    if (head[i]) {
        const uint64_t cell = keys[i] / num_views;
        vis_views[before[i]] = (int32_t)(keys[i] - cell * num_views);
        if (i == 0 || keys[i - 1] / num_views != cell) {
            vis_offsets[cell] = (long long)before[i];
        }
    }
    if (i == 0) {
        vis_offsets[cells] = (long long)before[entries];
    }
}

// vis_offsets[c] for c <= cells: the distinct (cell, view) runs before the first sorted key of cell c or a later one, by binary
// search; that key starts a run, so before[] at its position counts exactly those.  k_list_emit writes the offset of every cell
// that has an entry; a cell whose members all have empty lists (a rendered visibility can have them) has none, and gets its
// offset here, like every other cell.
__global__ __launch_bounds__(256) void k_cell_offsets(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ before, size_t entries,
                                                       uint64_t num_views, size_t cells, long long *__restrict__ vis_offsets)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c > cells) {
        return;
    }
    const uint64_t want = (uint64_t)c * num_views;
    size_t lo = 0, hi = entries;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    vis_offsets[c] = (long long)before[lo];
}

__global__ __launch_bounds__(256) void k_cell_support(const long long *__restrict__ vis_offsets, size_t cells, uint8_t *__restrict__ support)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c < cells) {
        const long long others = vis_offsets[c + 1] - vis_offsets[c] - 1;
        support[c] = (uint8_t)(others < 255 ? others : 255);
    }
}

std::string &err() { return apd_fusion::g_fusion_error; }

int hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(err(), APD_ERR_HIP, "apd_points_merge_voxels: %s: %s", expr, hipGetErrorString(e));
}

constexpr long long kMaxEntries = 1LL << 32;

int too_many_entries(long long entries)
{
    return apd::set_error(err(), APD_ERR_UNSUPPORTED, "apd_points_merge_voxels: %lld visibility entries, 2^32 or more", entries);
}

// `bytes` device bytes at `from` as host memory (malloc) in *to
template <typename T> int download(const T *from, size_t bytes, T **to)
{
    *to = static_cast<T *>(malloc(bytes > 0 ? bytes : 1));
    if (!*to) {
        return apd::set_error(err(), APD_ERR_HIP, "apd_points_merge_voxels: out of host memory");
    }
    HIP_TRY(hipMemcpy(*to, from, bytes, hipMemcpyDeviceToHost));
    return APD_OK;
}

// The merge of p (count > 0) into `result` (where p lives, without arrays so far); *dropped: the points without a cell.
// offsets / views: p's lists, where p lives.
int merge(apd_points_t p, const Grid &grid, const long long *offsets, const int32_t *views, apd_points *result, long long *dropped)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)p->count;
    const uint64_t num_views = (uint64_t)p->rows.size();
    Scratch scratch;
    PointArrays in = p->arrays;
    if (!p->on_device) {
        long long entries = offsets[n];
        constexpr unsigned kRead = apd_fusion::kAllArrays & ~apd_fusion::kSupport;  // the merge counts its own support
        HIP_TRY(alloc_arrays(scratch, in, n, kRead));
        HIP_TRY(copy_arrays(in, p->arrays, n, hipMemcpyHostToDevice, kRead));
        HIP_TRY(scratch.upload(offsets, (n + 1) * sizeof(long long), &offsets));
        HIP_TRY(scratch.upload(views, (size_t)entries * sizeof(int32_t), &views));
    }
    uint64_t *key = nullptr, *at = nullptr, *keys[2] = {nullptr, nullptr};
    uint32_t *keep = nullptr, *index[2] = {nullptr, nullptr};
    HIP_TRY(scratch.alloc(n * 8, &key));
    HIP_TRY(scratch.alloc(n * 4, &keep));
    HIP_TRY(scratch.alloc((n + 1) * 8, &at));
    apd_fusion::g_fusion_ms[0] = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();

    // 1, 2: keys, and the kept points in input order
    hipLaunchKernelGGL(k_voxel_keys, grid_of(n), dim3(256), 0, 0, (const float *)in.xyz, n, grid, key, keep);
    HIP_TRY(hipGetLastError());
    HIP_TRY(apd_sort::exclusive_scan(keep, at, n));
    uint64_t kept = 0;
    HIP_TRY(hipMemcpy(&kept, at + n, 8, hipMemcpyDeviceToHost));
    const size_t m = (size_t)kept;
    *dropped = (long long)(n - m);
    if (m == 0) {  // every point dropped: an object without points
        apd_fusion::g_fusion_ms[1] = ms_since(t1);
        return APD_OK;
    }
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(scratch.alloc(m * 8, &keys[b]));
        HIP_TRY(scratch.alloc(m * 4, &index[b]));
    }
    hipLaunchKernelGGL(k_voxel_compact, grid_of(n), dim3(256), 0, 0, (const uint64_t *)key, (const uint32_t *)keep, (const uint64_t *)at, n, keys[0],
                       index[0]);
    HIP_TRY(hipGetLastError());

    // 3: cells together, members in ascending input index
    int side = 0;
    HIP_TRY(apd_sort::sort_pairs(keys[0], keys[1], index[0], index[1], m, &side, nullptr));
    const uint64_t *sorted = keys[side];
    const uint32_t *member = index[side];

    // 4: heads and ranks of the cells
    uint32_t *head = nullptr, *start = nullptr;
    uint64_t *before = nullptr;
    HIP_TRY(scratch.alloc(m * 4, &head));
    HIP_TRY(scratch.alloc((m + 1) * 8, &before));
    hipLaunchKernelGGL(k_run_heads, grid_of(m), dim3(256), 0, 0, sorted, m, head);
    HIP_TRY(hipGetLastError());
    HIP_TRY(apd_sort::exclusive_scan(head, before, m));
    uint64_t ncells = 0;
    HIP_TRY(hipMemcpy(&ncells, before + m, 8, hipMemcpyDeviceToHost));
    const size_t cells = (size_t)ncells;

    // 5: the merged points
    PointArrays out;
    HIP_TRY(alloc_arrays(scratch, out, cells));
    HIP_TRY(scratch.alloc((cells + 1) * 4, &start));
    hipLaunchKernelGGL(k_cell_starts, grid_of(m), dim3(256), 0, 0, (const uint32_t *)head, (const uint64_t *)before, m, start);
    hipLaunchKernelGGL(k_cell_merge, grid_of(cells), dim3(256), 0, 0, cells, (const uint32_t *)start, member, in, out);
    HIP_TRY(hipGetLastError());

    // 6: the lists.  Entries of the kept members, keyed by (cell, view), sorted, first of every run kept
    uint32_t *length = nullptr;
    uint64_t *entry_at = nullptr;
    HIP_TRY(scratch.alloc(m * 4, &length));
    HIP_TRY(scratch.alloc((m + 1) * 8, &entry_at));
    hipLaunchKernelGGL(k_list_lengths, grid_of(m), dim3(256), 0, 0, member, m, offsets, length);
    HIP_TRY(hipGetLastError());
    HIP_TRY(apd_sort::exclusive_scan(length, entry_at, m));
    uint64_t nentries = 0;
    HIP_TRY(hipMemcpy(&nentries, entry_at + m, 8, hipMemcpyDeviceToHost));
    if (nentries >= (uint64_t)kMaxEntries) {  // p's own total was below: cannot happen, and must not reach a 32-bit grid
        return too_many_entries((long long)nentries);
    }
    const size_t entries = (size_t)nentries;
    uint64_t *list_keys[2] = {nullptr, nullptr}, *list_before = nullptr;
    uint32_t *list_head = nullptr;
    HIP_TRY(scratch.alloc(entries * 8, &list_keys[0]));
    HIP_TRY(scratch.alloc(entries * 8, &list_keys[1]));
    HIP_TRY(scratch.alloc(entries * 4, &list_head));
    HIP_TRY(scratch.alloc((entries + 1) * 8, &list_before));
    hipLaunchKernelGGL(k_list_expand, grid_of(m), dim3(256), 0, 0, member, m, offsets, views, (const uint64_t *)before, (const uint64_t *)entry_at,
                       num_views, list_keys[0]);
    HIP_TRY(hipGetLastError());
    if (entries > 0) {  // every list may be empty: a rendered visibility that no camera sees
        HIP_TRY(apd_sort::sort_pairs(list_keys[0], list_keys[1], nullptr, nullptr, entries, &side, nullptr));
    }
    const uint64_t *list_sorted = list_keys[entries > 0 ? side : 0];
    if (entries > 0) {
        hipLaunchKernelGGL(k_run_heads, grid_of(entries), dim3(256), 0, 0, list_sorted, entries, list_head);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(apd_sort::exclusive_scan(list_head, list_before, entries));
    uint64_t distinct = 0;
    HIP_TRY(hipMemcpy(&distinct, list_before + entries, 8, hipMemcpyDeviceToHost));
    long long *vis_offsets = nullptr;
    int32_t *vis_views = nullptr;
    HIP_TRY(scratch.alloc((cells + 1) * sizeof(long long), &vis_offsets));
    HIP_TRY(scratch.alloc((size_t)distinct * sizeof(int32_t), &vis_views));
    if (entries > 0) {
        hipLaunchKernelGGL(k_list_emit, grid_of(entries), dim3(256), 0, 0, list_sorted, (const uint32_t *)list_head, (const uint64_t *)list_before, entries,
                           num_views, cells, vis_offsets, vis_views);
    }
    hipLaunchKernelGGL(k_cell_offsets, grid_of(cells + 1), dim3(256), 0, 0, list_sorted, (const uint64_t *)list_before, entries, num_views, cells, vis_offsets);
    // 7
    hipLaunchKernelGGL(k_cell_support, grid_of(cells), dim3(256), 0, 0, (const long long *)vis_offsets, cells, out.support);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());

    result->count = (long long)cells;
    if (p->on_device) {
        keep_arrays(scratch, out);
        scratch.keep(vis_offsets);
        scratch.keep(vis_views);
        result->arrays = out;
        result->vis_offsets = vis_offsets;
        result->vis_views = vis_views;
    } else {  // freed with `result` by the caller if a download fails
        if (!alloc_host_arrays(result->arrays, cells)) {
            return apd::set_error(err(), APD_ERR_HIP, "apd_points_merge_voxels: out of host memory");
        }
        HIP_TRY(copy_arrays(result->arrays, out, cells, hipMemcpyDeviceToHost));
        int rc = download(vis_offsets, (cells + 1) * sizeof(long long), &result->vis_offsets);
        rc = rc != APD_OK ? rc : download(vis_views, (size_t)distinct * sizeof(int32_t), &result->vis_views);
        if (rc != APD_OK) {
            return rc;
        }
    }
    apd_fusion::g_fusion_ms[1] = ms_since(t1);
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_merge_voxels(apd_points_t p, float voxel_size, const float *origin3, apd_points_t *out, long long *dropped)
{
    err().clear();
    if (!p || !out) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_merge_voxels: null argument");
    }
    if (!(isfinite(voxel_size) && voxel_size > 0.0f)) {
        return apd::set_error(err(), APD_ERR_INVALID, "apd_points_merge_voxels: a voxel size of %g, not a positive finite number", (double)voxel_size);
    }
    Grid grid = {{0.0f, 0.0f, 0.0f}, voxel_size};
    for (int a = 0; origin3 && a < 3; ++a) {
        if (!isfinite(origin3[a])) {
            return apd::set_error(err(), APD_ERR_INVALID, "apd_points_merge_voxels: origin component %d is %g", a, (double)origin3[a]);
        }
        grid.origin[a] = origin3[a];
    }
    if (p->count >= (1LL << 31)) {
        return apd::set_error(err(), APD_ERR_UNSUPPORTED, "apd_points_merge_voxels: %lld points, 2^31 or more (the sort carries a 32-bit index)", p->count);
    }
    apd_points *result = apd_points_host::new_points_like(p);
    result->merged = 1;
    long long lost = 0;
    apd_fusion::g_fusion_ms[0] = apd_fusion::g_fusion_ms[1] = apd_fusion::g_fusion_ms[2] = 0.0;
    if (p->count > 0) {
        // p's lists, where p lives: host-resident points are counted here, before any device is touched; the lists of
        // device-resident points are built (if they are not yet) and counted on their device
        DeviceScope scope(true);
        const long long *offsets = nullptr;
        const int32_t *views = nullptr;
        int rc = apd_points_visibility(p, &offsets, &views);
        long long entries = 0;
        if (rc == APD_OK && !p->on_device) {
            entries = offsets[p->count];
        } else if (rc == APD_OK) {
            hipError_t e = hipSetDevice(p->device);
            e = e != hipSuccess ? e : hipMemcpy(&entries, offsets + p->count, sizeof(long long), hipMemcpyDeviceToHost);
            rc = e == hipSuccess ? APD_OK : hip_failed("download of the list total", e, __FILE__, __LINE__);
        }
        if (rc == APD_OK && entries >= kMaxEntries) {
            rc = too_many_entries(entries);
        }
        if (rc == APD_OK) {
            const hipError_t e = hipSetDevice(p->device);
            rc = e == hipSuccess ? merge(p, grid, offsets, views, result, &lost) : hip_failed("hipSetDevice", e, __FILE__, __LINE__);
        }
        if (rc != APD_OK) {
            const std::string why = err();
            apd_points_destroy(result);  // its arrays are host memory, or none yet
            err() = why;
            return rc;
        }
    }
    *out = result;
    if (dropped) {
        *dropped = lost;
    }
    return APD_OK;
}

extern "C" int apd_points_merged(apd_points_t p) { return p && p->merged ? 1 : 0; }
