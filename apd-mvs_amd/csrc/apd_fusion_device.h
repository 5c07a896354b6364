// apd_fusion_device.h -- what the device fusions share (apd_fusion.hip: ETH, apd_fusion_tat.hip: Tanks and Temples): the raster-order
// compaction of a view's points into the 15-byte PLY records, the PLY writer, and the per-thread error / timing that
// apd_fusion_last_error and apd_fusion_last_timing report.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

namespace apd_fusion {

extern thread_local std::string g_fusion_error;
extern thread_local double g_fusion_ms[3];  // last fusion: set-up (allocations, uploads), views (kernels + point downloads), PLY file

// ExportPointCloud (APD.cpp:214-254): header + the views' records in order.  APD_OK, or APD_ERR_IO with g_fusion_error set
// (`who` prefixes the message).
int write_ply(const char *who, const char *ply_path, long long count, const std::vector<std::vector<uint8_t>> &body);

}  // namespace apd_fusion

// Internal linkage: every fusion source gets its own copy of the two kernels.
namespace {

// exclusive scan of the block counts (one workgroup; a view has at most a few hundred thousand blocks)
__global__ __launch_bounds__(1024) void k_fusion_scan(int *__restrict__ counts, int nblocks, int *__restrict__ total)
{
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, nblocks);
    int sum = 0;
    for (int b = b0; b < b1; ++b) {
        sum += counts[b];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int b = b0; b < b1; ++b) {
        const int c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (t == 1023) {
        *total = part[1023];
    }
}

// Packs the points of a view (pixels p < n with state[p] == accepted) in raster order as the 15-byte records of the PLY body
// (x y z float, diffuse_blue / green / red uchar, APD.cpp:214-254): one download per view straight into the file image, no
// per-point loop on the host.  block_offsets: k_fusion_scan of the per-256-pixel point counts.
__global__ __launch_bounds__(256) void k_fusion_compact(const uint8_t *__restrict__ state, uint8_t accepted, int n,
                                                         const float *__restrict__ xyz_sparse, const uint8_t *__restrict__ bgr_sparse,
                                                         const int *__restrict__ block_offsets, uint8_t *__restrict__ records)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool acc = p < n && state[p] == accepted;
    const unsigned long long m = __ballot(acc);
    __shared__ int wave_counts[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        wave_counts[wave] = __popcll(m);
    }
    __syncthreads();
    if (acc) {
        int pos = block_offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) {
            pos += wave_counts[w];
        }
        uint8_t *rec = records + (size_t)pos * 15;
        for (int k = 0; k < 3; ++k) {
            const uint32_t bits = __float_as_uint(xyz_sparse[3 * (size_t)p + k]);  // little endian, as the host's memcpy wrote them
            rec[4 * k + 0] = (uint8_t)(bits & 0xFFu);
            rec[4 * k + 1] = (uint8_t)((bits >> 8) & 0xFFu);
            rec[4 * k + 2] = (uint8_t)((bits >> 16) & 0xFFu);
            rec[4 * k + 3] = (uint8_t)(bits >> 24);
        }
        rec[12] = bgr_sparse[3 * (size_t)p + 0];
        rec[13] = bgr_sparse[3 * (size_t)p + 1];
        rec[14] = bgr_sparse[3 * (size_t)p + 2];
    }
}

}  // namespace
