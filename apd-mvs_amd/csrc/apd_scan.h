// apd_scan.h -- the two scan bodies the kernels of the library share (device side only): a workgroup's inclusive scan of one value
// per lane in LDS, and the one-workgroup scan of a list of block sums in place.  Who uses them: k_fusion_scan
// (apd_fusion_call.hip), k_vis_count / k_vis_scan / k_vis_scatter (apd_points_vis.hip), k_scan_top / k_scan_apply (apd_sort.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace apd_scan {

// Hillis-Steele over the N lanes of the workgroup: returns value of lane 0 + ... + value of this lane t; afterwards part[i] is
// that sum of lane i, so part[N - 1] is the total.  Every lane of the workgroup calls it.
template <int N, typename T> __device__ __forceinline__ T block_inclusive_scan(T (&part)[N], int t, T value)
{
    part[t] = value;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const T v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    return part[t];
}

// One workgroup of N lanes: sums[b] becomes sums[0] + ... + sums[b - 1] for b < nblocks; returns the total.  Every lane adds up
// a run of consecutive sums, the runs are scanned across the lanes, and every lane writes the prefixes of its run.
template <int N, typename T, typename Index> __device__ __forceinline__ T scan_sums_in_place(T *__restrict__ sums, Index nblocks, T (&part)[N])
{
    const Index t = threadIdx.x;
    const Index per = (nblocks + (N - 1)) / N;
    const Index b0 = t * per < nblocks ? t * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    T sum = 0;
    for (Index b = b0; b < b1; ++b) {
        sum += sums[b];
    }
    T run = block_inclusive_scan(part, (int)t, sum) - sum;
    for (Index b = b0; b < b1; ++b) {
        const T c = sums[b];
        sums[b] = run;
        run += c;
    }
    return part[N - 1];
}

}  // namespace apd_scan
