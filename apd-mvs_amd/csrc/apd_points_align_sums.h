// apd_points_align_sums.h -- passes 1 and 2 of contract C18 (the relation: apd_align_math.h) and the move of positions
// by a transform, as the entry points that fit a transform to matched pairs share them: the kernels k_align_sums1, k_align_sums2
// and k_align_move and, as methods of AlignSums on the host frame of apd_points_nearest.h, the launch of the move and the totals
// of the chunk sums.  Used by apd_points_align.hip (apd_points_align, apd_points_transformed) and apd_points_register.hip (the
// refit of apd_points_register).  Device code: hipcc only.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_align_math.h"
#include "apd_fusion_device.h"
#include "apd_points_nearest.h"
#include "apd_points_search.h"

namespace apd_align_sums {
namespace {

using apd_fusion::AlignMove;
using apd_fusion::kAlignSums1;
using apd_fusion::kAlignSums2;
using apd_fusion::kKnnChunk;
using apd_nearest_search::NearestSearch;
using apd_points_grid::grid_of;
using apd_points_search::err;

static_assert(kKnnChunk == 256, "one lane per slot of a chunk, four waves");

// The tree of contract C18 over the workgroup's 256 slots, for each of the N sums: v is the lane's slot; sums[0 .. N): the chunk's.
// Every lane of the workgroup calls it.  A lane s >= d of a ladder step adds what no lane below it reads afterwards
template <int N> __device__ __forceinline__ void align_reduce(double (&v)[N], double *__restrict__ sums)
{
    __shared__ double of_wave[4][N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int d = 32; d >= 1; d /= 2) {
            v[j] = v[j] + __shfl_down(v[j], d, 64);
        }
    }
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            of_wave[wave][j] = v[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double low = of_wave[0][j] + of_wave[1][j], high = of_wave[2][j] + of_wave[3][j];
            sums[j] = low + high;
        }
    }
}

// The lane's slot k and whether point k < n is matched; then P its position and Q that of its match.  index[k] is -1 or below n_q
__device__ __forceinline__ bool align_pair(const float *__restrict__ xyz, const int32_t *__restrict__ index, const float *__restrict__ target, size_t n,
                                           float P[3], float Q[3])
{
    const size_t k = (size_t)blockIdx.x * kKnnChunk + threadIdx.x;
    const int32_t j = k < n ? index[k] : apd_fusion::kNearestNoIndex;
    if (j < 0) {
        return false;
    }
    for (int a = 0; a < 3; ++a) {
        P[a] = xyz[3 * k + a];
        Q[a] = target[3 * (size_t)j + a];
    }
    return true;
}

// Chunk blockIdx.x of the n points at xyz: sums[8 * chunk ..] by pass 1 of contract C18.  index: n matches; target: q's positions
__global__ __launch_bounds__(256) void k_align_sums1(const float *__restrict__ xyz, const int32_t *__restrict__ index, const float *__restrict__ target,
                                                      size_t n, double *__restrict__ sums)
{
    float P[3], Q[3];
    double v[kAlignSums1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (align_pair(xyz, index, target, n, P, Q)) {
        apd_fusion::align_terms1(P, Q, v);
    }
    align_reduce(v, sums + (size_t)blockIdx.x * kAlignSums1);
}

// Its means: pm then qm, as pass 1 gave them
struct AlignMeans {
    double mean[6];
};

// Likewise sums[10 * chunk ..] by pass 2
__global__ __launch_bounds__(256) void k_align_sums2(const float *__restrict__ xyz, const int32_t *__restrict__ index, const float *__restrict__ target,
                                                      size_t n, AlignMeans about, double *__restrict__ sums)
{
    float P[3], Q[3];
    double v[kAlignSums2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (align_pair(xyz, index, target, n, P, Q)) {
        apd_fusion::align_terms2(P, Q, about.mean, v);
    }
    align_reduce(v, sums + (size_t)blockIdx.x * kAlignSums2);
}

// out[k] = in[k] moved by `by` (contract C18, step 5), k < n; out is not in
__global__ __launch_bounds__(256) void k_align_move(const float *__restrict__ in, size_t n, AlignMove by, float *__restrict__ out)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) {
        return;
    }
    const float X[3] = {in[3 * k], in[3 * k + 1], in[3 * k + 2]};
    float Y[3];
    apd_fusion::align_moved(by, X, Y);
    out[3 * k] = Y[0];
    out[3 * k + 1] = Y[1];
    out[3 * k + 2] = Y[2];
}

// One call of an entry point that sums over matched pairs
struct AlignSums : NearestSearch {
    int move(const float *in, size_t n, const AlignMove &by, float *out) const
    {
        hipLaunchKernelGGL(k_align_move, grid_of(n), dim3(256), 0, 0, in, n, by, out);
        HIP_TRY(hipGetLastError());
        return APD_OK;
    }

    // The `width` totals of the chunk sums at `sums` (device memory): they come down and are added in ascending order from 0.0
    int totals(const double *sums, size_t chunks, int width, std::vector<double> &host, double *total) const
    {
        HIP_TRY(hipMemcpy(host.data(), sums, chunks * (size_t)width * 8, hipMemcpyDeviceToHost));
        for (int j = 0; j < width; ++j) {
            total[j] = 0.0;
        }
        for (size_t c = 0; c < chunks; ++c) {
            for (int j = 0; j < width; ++j) {
                total[j] = total[j] + host[c * (size_t)width + j];
            }
        }
        return APD_OK;
    }
};

}  // namespace
}  // namespace apd_align_sums
