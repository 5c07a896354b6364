// apd_points_vis.hip -- apd_points_visibility of include/apd_mi355x.h: the visibility lists of a points object, built on the
// first call where the arrays live -- the plain loop for host-resident points, three kernels for device-resident ones.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_points_host.h"
#include "apd_scan.h"

namespace {

// The lists of device-resident points.
// Point k has 1 + popcount(sources[k]) entries: its own view, then the views behind the set bits in ascending bit order.  Three
// kernels: per block of 256 points the number of entries (k_vis_count), an exclusive 64-bit scan of those block sums by one
// workgroup (k_vis_scan: a full ETH3D or 152-view run has more than 10^8 points, so the entries can pass 2^31 and every offset
// is 64-bit; 1024 lanes, each over a run of consecutive blocks, so up to kVisScanSpan points every lane has one block), and the
// scatter, which repeats the block's own scan in LDS (k_vis_scatter).

constexpr long long kVisScanSpan = 1024LL * 256;  // points up to which every lane of k_vis_scan scans at most one block sum

// the bits of sources[k] that name a source of the point's view: all of them, by construction of the mask
__device__ __forceinline__ uint32_t vis_mask(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                             const int *__restrict__ pair_offsets, size_t k, int &first)
{
    const int v = view[k];
    first = pair_offsets[v];
    const int ns = pair_offsets[v + 1] - first;
    return sources[k] & (ns >= 32 ? 0xFFFFFFFFu : ((1u << ns) - 1u));
}

// exclusive scan of one value per lane over the 256 lanes of the block; *block_total: the sum
__device__ __forceinline__ int vis_block_scan(int value, int *block_total)
{
    __shared__ int part[256];
    const int before = apd_scan::block_inclusive_scan(part, (int)threadIdx.x, value) - value;
    *block_total = part[255];
    return before;
}

__global__ __launch_bounds__(256) void k_vis_count(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                                    const int *__restrict__ pair_offsets, size_t n, long long *__restrict__ block_sums)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int first;
    const int entries = k < n ? 1 + __popc(vis_mask(sources, view, pair_offsets, k, first)) : 0;
    int total;
    vis_block_scan(entries, &total);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = total;
    }
}

// block_sums[b] becomes the number of entries before block b; *total: all entries
__global__ __launch_bounds__(1024) void k_vis_scan(long long *__restrict__ block_sums, size_t nblocks, long long *__restrict__ total)
{
    __shared__ long long part[1024];
    const long long sum = apd_scan::scan_sums_in_place(block_sums, nblocks, part);
    if (threadIdx.x == 1023) {
        *total = sum;
    }
}

// offsets[k] = entries before point k (offsets[n] = all of them); views[offsets[k] ..]: the point's view, then its agreeing sources
__global__ __launch_bounds__(256) void k_vis_scatter(const uint32_t *__restrict__ sources, const int32_t *__restrict__ view,
                                                      const int *__restrict__ pair_offsets, const int *__restrict__ pair_indices, size_t n,
                                                      const long long *__restrict__ block_prefix, const long long *__restrict__ total,
                                                      long long *__restrict__ offsets, int32_t *__restrict__ views)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int first = 0;
    uint32_t m = 0;
    int entries = 0;
    if (k < n) {
        m = vis_mask(sources, view, pair_offsets, k, first);
        entries = 1 + __popc(m);
    }
    int block_total;
    const long long at = block_prefix[blockIdx.x] + vis_block_scan(entries, &block_total);
    if (k < n) {
        offsets[k] = at;
        int32_t *list = views + at;
        *list++ = view[k];
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            *list++ = pair_indices[first + j];
        }
    }
    if (k == 0) {
        offsets[n] = *total;
    }
}

int vis_hip_failed(const char *expr, hipError_t e, const char *, int)
{
    return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: %s: %s", expr, hipGetErrorString(e));
}

// The lists of host-resident points: the plain loop
int build_visibility_host(apd_points *p)
{
    const size_t n = (size_t)p->count;
    long long *offsets = (long long *)malloc((n + 1) * sizeof(long long));
    if (!offsets) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: out of host memory");
    }
    const apd_fusion::PointArrays &a = p->arrays;
    long long total = 0;
    for (size_t k = 0; k < n; ++k) {
        offsets[k] = total;
        total += 1 + __builtin_popcount(a.sources[k]);
    }
    offsets[n] = total;
    int32_t *views = (int32_t *)malloc(total > 0 ? (size_t)total * sizeof(int32_t) : sizeof(int32_t));
    if (!views) {
        free(offsets);
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_HIP, "apd_points_visibility: out of host memory");
    }
    for (size_t k = 0; k < n; ++k) {
        int32_t *list = views + offsets[k];
        *list++ = a.view[k];
        const int first = p->pair_offsets[(size_t)a.view[k]];
        for (int j = 0; j < 32; ++j) {
            if ((a.sources[k] >> j) & 1u) {
                *list++ = p->pair_indices[(size_t)(first + j)];
            }
        }
    }
    p->vis_offsets = offsets;
    p->vis_views = views;
    return APD_OK;
}

// The lists of device-resident points, on their device: k_vis_count, k_vis_scan, k_vis_scatter
int build_visibility_device(apd_points *p)
{
    const auto hip_failed = vis_hip_failed;  // what HIP_TRY returns here
    const size_t n = (size_t)p->count;
    const size_t nblocks = (n + 255) / 256;
    apd_points_host::Scratch scratch;
    long long *offsets = nullptr, *block_sums = nullptr, *dtotal = nullptr;
    int32_t *views = nullptr;
    const int *pair_offsets = nullptr, *pair_indices = nullptr;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(scratch.alloc((n + 1) * sizeof(long long), &offsets));
    long long total = 0;
    if (n == 0) {
        HIP_TRY(hipMemset(offsets, 0, sizeof(long long)));
    } else {
        HIP_TRY(scratch.alloc(nblocks * sizeof(long long), &block_sums));
        HIP_TRY(scratch.alloc(sizeof(long long), &dtotal));
        HIP_TRY(scratch.upload(p->pair_offsets.data(), p->pair_offsets.size() * sizeof(int), &pair_offsets));
        HIP_TRY(scratch.upload(p->pair_indices.data(), p->pair_indices.size() * sizeof(int), &pair_indices));
        const apd_fusion::PointArrays &a = p->arrays;
        hipLaunchKernelGGL(k_vis_count, dim3((unsigned)nblocks), dim3(256), 0, 0, (const uint32_t *)a.sources, (const int32_t *)a.view,
                           pair_offsets, n, block_sums);
        hipLaunchKernelGGL(k_vis_scan, dim3(1), dim3(1024), 0, 0, block_sums, nblocks, dtotal);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&total, dtotal, sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIP_TRY(scratch.alloc(total > 0 ? (size_t)total * sizeof(int32_t) : sizeof(int32_t), &views));
    if (n > 0) {
        const apd_fusion::PointArrays &a = p->arrays;
        hipLaunchKernelGGL(k_vis_scatter, dim3((unsigned)nblocks), dim3(256), 0, 0, (const uint32_t *)a.sources, (const int32_t *)a.view,
                           pair_offsets, pair_indices, n, (const long long *)block_sums, (const long long *)dtotal,
                           offsets, views);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    scratch.keep(offsets);
    scratch.keep(views);
    p->vis_offsets = offsets;
    p->vis_views = views;
    return APD_OK;
}

}  // namespace

extern "C" int apd_points_visibility(apd_points_t p, const long long **offsets, const int32_t **views)
{
    apd_fusion::g_fusion_error.clear();
    if (!p || !offsets || !views) {
        return apd::set_error(apd_fusion::g_fusion_error, APD_ERR_INVALID, "apd_points_visibility: null argument");
    }
    if (!p->vis_offsets) {
        apd_points_host::DeviceScope scope(p->on_device != 0);
        if (const int rc = p->on_device ? build_visibility_device(p) : build_visibility_host(p); rc != APD_OK) {
            return rc;
        }
    }
    *offsets = p->vis_offsets;
    *views = p->vis_views;
    return APD_OK;
}
