// apd_fusion_call.hip -- the host driver every device fusion and the geometric filter share (apd_fusion::Call,
// apd_fusion_device.h), with the kernels only it launches (k_fusion_scan, k_fusion_compact, k_fusion_compact_soa) and the
// per-thread error and timing of the fusions (apd_fusion_last_error, apd_fusion_last_timing).
//
// Points in memory (apd_points_t, apd_points_host.h): the total is not known before the last view, so the arrays grow
// geometrically on the device (reserve_points: twice the capacity, one device-to-device copy of what is there) and
// k_fusion_compact_soa appends each view's points at the running count; a host result is one download at the end.  Nothing is sized
// by pixels x views.  Among the arrays is `sources`, per point the sources whose votes it was accepted with as a bit mask
// (k_fusion_emit / k_tat_decide write it per pixel, only when the points are asked for).
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_device.h"
#include "apd_scan.h"

namespace {

// exclusive scan of the block counts (one workgroup; a view has at most a few hundred thousand blocks)
__global__ __launch_bounds__(1024) void k_fusion_scan(int *__restrict__ counts, int nblocks, int *__restrict__ total)
{
    __shared__ int part[1024];
    const int sum = apd_scan::scan_sums_in_place(counts, nblocks, part);
    if (threadIdx.x == 1023) {
        *total = sum;
    }
}

// Packs the points of a view (pixels p < n with state[p] == accepted) in raster order as the 15-byte records of the PLY body
// (x y z float, diffuse_blue / green / red uchar, APD.cpp:214-254): one download per view straight into the file image, no
// per-point loop on the host.  block_offsets: k_fusion_scan of the per-256-pixel point counts.  kNormals: the 27-byte records
// x y z nx ny nz + colour, the normal read from the view's normal map at the pixel.
template <bool kNormals>
__global__ __launch_bounds__(256) void k_fusion_compact(const uint8_t *__restrict__ state, uint8_t accepted, int n,
                                                         const float *__restrict__ xyz_sparse, const uint8_t *__restrict__ bgr_sparse,
                                                         const float *__restrict__ normal_map, const int *__restrict__ block_offsets,
                                                         uint8_t *__restrict__ records)
{
    constexpr int kFloats = kNormals ? 6 : 3, kRecord = 4 * kFloats + 3;
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
        uint8_t *rec = records + (size_t)pos * kRecord;
        for (int k = 0; k < kFloats; ++k) {
            // little endian, as the host's memcpy wrote them
            const uint32_t bits = __float_as_uint(k < 3 ? xyz_sparse[3 * (size_t)p + k] : normal_map[3 * (size_t)p + (k - 3)]);
            rec[4 * k + 0] = (uint8_t)(bits & 0xFFu);
            rec[4 * k + 1] = (uint8_t)((bits >> 8) & 0xFFu);
            rec[4 * k + 2] = (uint8_t)((bits >> 16) & 0xFFu);
            rec[4 * k + 3] = (uint8_t)(bits >> 24);
        }
        rec[4 * kFloats + 0] = bgr_sparse[3 * (size_t)p + 0];
        rec[4 * kFloats + 1] = bgr_sparse[3 * (size_t)p + 1];
        rec[4 * kFloats + 2] = bgr_sparse[3 * (size_t)p + 2];
    }
}

// The same points as a structure of arrays, appended at `base`: point base + block offset + rank in the block gets xyz, the
// normal of the view's normal map at the pixel, colour, support, the agreeing sources, the view and the raster index.  One lane per
// pixel; the rank inside a wave from the ballot and mbcnt, across the four waves of the block through LDS.  Every offset is a size_t.
__global__ __launch_bounds__(256) void k_fusion_compact_soa(const uint8_t *__restrict__ state, uint8_t accepted, int n, int view,
                                                             const float *__restrict__ xyz_sparse, const uint8_t *__restrict__ bgr_sparse,
                                                             const uint8_t *__restrict__ support_sparse,
                                                             const uint32_t *__restrict__ agreeing_sparse,
                                                             const float *__restrict__ normal_map, const int *__restrict__ block_offsets,
                                                             size_t base, apd_fusion::PointArrays out)
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
        int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        for (int w = 0; w < wave; ++w) {
            rank += wave_counts[w];
        }
        const size_t pos = base + (size_t)block_offsets[blockIdx.x] + (size_t)rank;
        for (int k = 0; k < 3; ++k) {
            out.xyz[3 * pos + k] = xyz_sparse[3 * (size_t)p + k];
            out.normal[3 * pos + k] = normal_map[3 * (size_t)p + k];
            out.bgr[3 * pos + k] = bgr_sparse[3 * (size_t)p + k];
        }
        out.support[pos] = support_sparse[p];
        out.sources[pos] = agreeing_sparse[p];
        out.view[pos] = view;
        out.pixel[pos] = p;
    }
}

}  // namespace

namespace apd_fusion {

thread_local std::string g_fusion_error;
thread_local double g_fusion_ms[3] = {0.0, 0.0, 0.0};

namespace {

// ExportPointCloud (APD.cpp:214-254): header + the views' records in order.  APD_OK, or APD_ERR_IO with g_fusion_error set
int write_ply(const char *who, const char *ply_path, long long count, const std::vector<std::vector<uint8_t>> &body, bool normals)
{
    FILE *f = fopen(ply_path, "wb");
    if (!f) {
        g_fusion_error = std::string(who) + ": cannot write " + ply_path;  // no length limit: not through set_error
        return APD_ERR_IO;
    }
    apd_points_host::write_ply_header(f, count, normals);
    bool ok = true;
    for (const std::vector<uint8_t> &part : body) {
        ok = ok && (part.empty() || fwrite(part.data(), 1, part.size(), f) == part.size());
    }
    if (fclose(f) != 0 || !ok) {
        g_fusion_error = std::string(who) + ": short write to " + ply_path;
        return APD_ERR_IO;
    }
    return APD_OK;
}

}  // namespace

int check_options(const char *who, const apd_fusion_options *options, bool *preset_out)
{
    std::string &err = g_fusion_error;
    if (!options) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: null options", who);
    }
    if (options->struct_size != sizeof(apd_fusion_options)) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: struct_size %zu is not sizeof(apd_fusion_options) = %zu", who, options->struct_size,
                              sizeof(apd_fusion_options));
    }
    const apd_fusion_options o = *options, d = default_options();
    if (o.variant != APD_FUSION_ETH && o.variant != APD_FUSION_TAT_INTERMEDIATE && o.variant != APD_FUSION_TAT_ADVANCED) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: unknown variant %d", who, o.variant);
    }
    const struct {
        const char *name;
        float value, preset;
    } values[] = {{"max_reproj_error", o.max_reproj_error, d.max_reproj_error}, {"max_relative_depth", o.max_relative_depth, d.max_relative_depth},
                  {"max_angle", o.max_angle, d.max_angle},                      {"depth_weight", o.depth_weight, d.depth_weight},
                  {"angle_weight", o.angle_weight, d.angle_weight},             {"factor_strong", o.factor_strong, d.factor_strong},
                  {"factor_weak", o.factor_weak, d.factor_weak}};
    bool preset = o.min_consistent == d.min_consistent;
    for (const auto &v : values) {
        if (!(v.value >= 0.0f) || v.value > FLT_MAX) {
            return apd::set_error(err, APD_ERR_INVALID, "%s: %s is negative or not finite", who, v.name);
        }
        preset = preset && v.value == v.preset;
    }
    if (o.min_consistent < 1 || o.min_consistent > APD_MAX_IMAGES) {
        return apd::set_error(err, APD_ERR_INVALID, "%s: min_consistent %d is outside 1 .. %d", who, o.min_consistent, APD_MAX_IMAGES);
    }
    *preset_out = preset;
    return APD_OK;
}

int Call::begin(bool eth, bool points)
{
    g_fusion_error.clear();
    auto invalid = [this](const char *what) { return apd::set_error(g_fusion_error, APD_ERR_INVALID, "%s: %s", who, what); };
    if (a.num_views <= 0 || !a.cameras || (points && !a.images) || !a.depths || !a.normals || (eth && !a.weaks) || !a.rows || !a.cols ||
        !a.pair_offsets || !a.pair_indices || (points && ((!a.ply_path && !a.points) || !a.num_points))) {
        return invalid("null argument");
    }
    if (points && a.image_channels != 1 && a.image_channels != 3) {
        return invalid("images have 1 (grey) or 3 (blue, green, red) channels");
    }
    for (int i = 0; i < a.num_views; ++i) {
        const int ns = a.pair_offsets[i + 1] - a.pair_offsets[i];
        if (ns < 0 || ns > APD_MAX_IMAGES) {
            return invalid("a view has more than APD_MAX_IMAGES sources");
        }
        if (a.rows[i] < 0 || a.cols[i] < 0 || (long long)a.rows[i] * a.cols[i] > 0x7fffff00LL) {  // pixel indices are ints
            return invalid("view size out of range");
        }
        for (int k = a.pair_offsets[i]; k < a.pair_offsets[i + 1]; ++k) {
            if (a.pair_indices[k] < 0 || a.pair_indices[k] >= a.num_views) {
                return invalid("source index out of range");
            }
            // ETH: the consumption of a view's own pixels would be order dependent inside the vote kernel; T&T: the view would read the
            // masks it writes
            if (a.pair_indices[k] == i) {
                return invalid(eth ? "a view lists itself as a source (use the host fusion)" : "a view lists itself as a source");
            }
        }
    }
    for (int i = 0; i < a.num_views; ++i) {
        max_px = std::max(max_px, (size_t)pixels(i));
        max_src = std::max(max_src, sources(i));
    }
    body_.resize((size_t)a.num_views);
    HIP_TRY(hipSetDevice(a.device));
    return APD_OK;
}

Call::Call(const char *who_, const Args &args) : who(who_), a(args), t_lap_(std::chrono::steady_clock::now()) {}

void Call::release()
{
    scratch_.release();
    if (staging_) {
        hipHostFree(staging_);
        staging_ = nullptr;
    }
}

int Call::hip_failed(const char *expr, hipError_t e, const char *, int) const
{
    return apd::set_error(g_fusion_error, APD_ERR_HIP, "%s: %s: %s", who, expr, hipGetErrorString(e));
}

int Call::alloc_common()
{
    HIP_TRY(alloc(max_px * 12, &xyz));
    HIP_TRY(alloc(max_px * 3, &bgr));
    HIP_TRY(alloc(max_px, &support));
    if (a.points) {  // the PLY-only call has no such buffer and its emit kernels no such store
        HIP_TRY(alloc(max_px * 4, &agreeing));
    }
    HIP_TRY(alloc(max_blocks() * 4, &block_counts));
    HIP_TRY(alloc(sizeof(int), &total_));
    if (a.ply_path) {  // without a file no record is packed or downloaded
        const size_t bytes = max_px * (size_t)record_bytes();
        HIP_TRY(alloc(bytes, &records_));
        if (hipHostMalloc(&staging_, bytes > 0 ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
            staging_ = nullptr;  // pageable downloads then
        }
    }
    g_fusion_ms[0] = lap();
    return APD_OK;
}

double Call::lap()
{
    const double ms = apd_points_host::ms_since(t_lap_);
    t_lap_ = std::chrono::steady_clock::now();
    return ms;
}

int Call::collect(int i, const uint8_t *state, uint8_t accepted, const float *normal)
{
    const int n = pixels(i);
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_fusion_scan, dim3(1), dim3(1024), 0, 0, block_counts, blocks, total_);
    if (a.ply_path && a.opt.ply_normals) {
        hipLaunchKernelGGL(k_fusion_compact<true>, dim3(blocks), dim3(256), 0, 0, state, accepted, n, (const float *)xyz, (const uint8_t *)bgr,
                           normal, (const int *)block_counts, records_);
    } else if (a.ply_path) {
        hipLaunchKernelGGL(k_fusion_compact<false>, dim3(blocks), dim3(256), 0, 0, state, accepted, n, (const float *)xyz, (const uint8_t *)bgr,
                           normal, (const int *)block_counts, records_);
    }
    HIP_TRY(hipGetLastError());
    int npts = 0;
    HIP_TRY(hipMemcpy(&npts, total_, sizeof(int), hipMemcpyDeviceToHost));
    if (npts <= 0) {
        return APD_OK;
    }
    if (a.ply_path) {
        std::vector<uint8_t> &part = body_[i];
        part.resize((size_t)npts * record_bytes());
        if (staging_) {
            HIP_TRY(hipMemcpy(staging_, records_, part.size(), hipMemcpyDeviceToHost));
            memcpy(part.data(), staging_, part.size());
        } else {
            HIP_TRY(hipMemcpy(part.data(), records_, part.size(), hipMemcpyDeviceToHost));
        }
    }
    if (a.points) {
        if (const int rc = reserve_points(count_ + npts); rc != APD_OK) {
            return rc;
        }
        hipLaunchKernelGGL(k_fusion_compact_soa, dim3(blocks), dim3(256), 0, 0, state, accepted, n, i, (const float *)xyz, (const uint8_t *)bgr,
                           (const uint8_t *)support, (const uint32_t *)agreeing, normal, (const int *)block_counts, (size_t)count_, soa_);
        HIP_TRY(hipGetLastError());
    }
    count_ += npts;
    return APD_OK;
}

int Call::reserve_points(long long need)
{
    if (need <= soa_capacity_) {
        return APD_OK;
    }
    const long long capacity = std::max({need, 2 * soa_capacity_, 4096LL});
    apd_points_host::Scratch owner;  // of `grown` until the copy is made: a failure on the way frees what was allocated
    PointArrays grown;
    HIP_TRY(alloc_arrays(owner, grown, (size_t)capacity));
    if (count_ > 0) {
        HIP_TRY(copy_arrays(grown, soa_, (size_t)count_, hipMemcpyDeviceToDevice));
    }
    keep_arrays(owner, grown);
    release_points();
    soa_ = grown;
    soa_capacity_ = capacity;
    return APD_OK;
}

void Call::release_points()
{
    free_arrays(soa_, true);
    soa_capacity_ = 0;
}

int Call::finish()
{
    g_fusion_ms[1] = lap();
    apd_points *pts = nullptr;
    if (a.points) {
        HIP_TRY(hipDeviceSynchronize());  // the last view's compaction
        pts = apd_points_host::new_points(a.device, a.opt.result_on_device ? 1 : 0, a.num_views, a.rows, a.cols, a.pair_offsets, a.pair_indices);
        pts->count = count_;
        if (pts->on_device) {
            std::swap(pts->arrays, soa_);
            soa_capacity_ = 0;
        } else if (count_ > 0) {
            hipError_t e = alloc_host_arrays(pts->arrays, (size_t)count_) ? hipSuccess : hipErrorOutOfMemory;
            e = e != hipSuccess ? e : copy_arrays(pts->arrays, soa_, (size_t)count_, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                apd_points_destroy(pts);
                return hip_failed("download of the points", e, __FILE__, __LINE__);
            }
        }
        release_points();
    }
    release();
    if (a.ply_path) {
        const int written = write_ply(who, a.ply_path, count_, body_, a.opt.ply_normals != 0);
        if (written != APD_OK) {
            apd_points_destroy(pts);
            return written;
        }
    }
    *a.num_points = count_;
    if (a.points) {
        *a.points = pts;
    }
    g_fusion_ms[2] = apd_points_host::ms_since(t_lap_);
    return APD_OK;
}

}  // namespace apd_fusion

extern "C" const char *apd_fusion_last_error(void) { return apd_fusion::g_fusion_error.c_str(); }

extern "C" int apd_fusion_last_timing(double *setup_ms, double *views_ms, double *file_ms)
{
    if (setup_ms) {
        *setup_ms = apd_fusion::g_fusion_ms[0];
    }
    if (views_ms) {
        *views_ms = apd_fusion::g_fusion_ms[1];
    }
    if (file_ms) {
        *file_ms = apd_fusion::g_fusion_ms[2];
    }
    return APD_OK;
}

extern "C" void apd_fusion_default_options(apd_fusion_options *o)
{
    if (o) {
        *o = apd_fusion::default_options();
    }
}
