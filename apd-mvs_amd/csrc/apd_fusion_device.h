// apd_fusion_device.h -- the host driver the device fusions share (apd_fusion.hip: ETH, apd_fusion_tat.hip: Tanks and Temples).
// Implemented once, in apd_fusion_call.hip, together with the kernels only it launches (k_fusion_scan, k_fusion_compact): argument
// checks, the device memory of a call, the per-view geometry and maps, the scratch of the point compaction, the download of a
// view's points, the PLY file, the points in memory (apd_points_t), and the per-thread error / timing that apd_fusion_last_error
// and apd_fusion_last_timing report.
// A variant derives from Call and adds its own view members, scratch and kernels.  The geometric filter (apd_filter.hip,
// apd_filter_views) derives from it too: it shares the argument checks, the memory and the geometry-and-maps half of a view, and
// takes no images and makes no points.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"
#include "apd_fusion_math.h"
#include "apd_host_error.h"
#include "apd_points_host.h"

namespace apd_fusion {

extern thread_local std::string g_fusion_error;
extern thread_local double g_fusion_ms[3];  // last fusion: set-up (allocations, uploads), views (kernels + point downloads), PLY file

// apd_fusion_default_options: the reference's literals, a PLY of 15-byte records, host results
inline apd_fusion_options default_options()
{
    apd_fusion_options o;
    memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.variant = APD_FUSION_ETH;
    o.max_reproj_error = 2.0f;
    o.max_relative_depth = 0.01f;
    o.max_angle = 0.174533f;
    o.depth_weight = 200.0f;
    o.angle_weight = 10.0f;
    o.min_consistent = 1;
    o.factor_strong = 0.3f;
    o.factor_weak = 0.45f;
    return o;
}

// The geometry of camera c at rows x cols: K, R, t and the centre -R^T t in float, term order of Get3DPointonWorld (APD.cpp:795-798)
inline void view_geometry(const apd_camera &c, int rows, int cols, View &geo)
{
    memcpy(geo.K, c.K, sizeof(geo.K));
    memcpy(geo.R, c.R, sizeof(geo.R));
    memcpy(geo.t, c.t, sizeof(geo.t));
    geo.centre[0] = -(c.R[0] * c.t[0] + c.R[3] * c.t[1] + c.R[6] * c.t[2]);
    geo.centre[1] = -(c.R[1] * c.t[0] + c.R[4] * c.t[1] + c.R[7] * c.t[2]);
    geo.centre[2] = -(c.R[2] * c.t[0] + c.R[5] * c.t[1] + c.R[8] * c.t[2]);
    geo.rows = rows;
    geo.cols = cols;
}

// The arguments of apd_fuse_views / apd_fuse_views_variant / apd_fuse_views_opt (include/apd_mi355x.h)
struct Args {
    int device, num_views;
    const apd_camera *cameras;
    const float *const *images;
    int image_channels;
    const float *const *depths;
    const float *const *normals;
    const uint8_t *const *weaks;
    const uint8_t *const *blocks;
    const int *rows, *cols, *pair_offsets, *pair_indices;
    int maps_on_device;
    const char *ply_path;
    long long *num_points;
    apd_fusion_options opt = default_options();
    apd_points_t *points = nullptr;  // apd_fuse_views_opt: where the points in memory go; then ply_path may be null
};

// What apd_fuse_views_opt and apd_filter_views refuse in their options, APD_ERR_INVALID with "<who>: ...": null, a struct_size of
// another header, an unknown variant, one of the seven float values negative or not finite, min_consistent outside
// 1 .. APD_MAX_IMAGES.  *preset: the eight values are the defaults.
int check_options(const char *who, const apd_fusion_options *options, bool *preset);

// The ETH fusion (apd_fusion.hip) for apd_fuse_views_opt, which lives beside the T&T fusions (apd_fusion_tat.hip)
int run_eth(const char *who, const Args &args);

// One fusion call.  Owns every device allocation and the page-locked staging buffer of the call: whichever way the call returns,
// they are released, in the order they were made.
class Call {
public:
    Call(const char *who, const Args &args);  // the clock of the set-up starts here
    ~Call()
    {
        release();
        release_points();
    }
    Call(const Call &) = delete;
    Call &operator=(const Call &) = delete;

protected:
    const char *const who;  // the entry point, prefix of every message
    const Args a;
    size_t max_px = 0;      // pixels of the largest view
    int max_src = 1;        // sources of the view with the most
    float *xyz = nullptr;   // [pixel][3] of the view being fused: the points where they are, before the compaction
    uint8_t *bgr = nullptr; // [pixel][3]
    uint8_t *support = nullptr;  // [pixel]: votes the point was accepted with
    uint32_t *agreeing = nullptr;  // [pixel]: bit j = source j is one of those votes; null unless the points in memory are asked for
    int *block_counts = nullptr;  // points per block of 256 pixels

    int hip_failed(const char *expr, hipError_t e, const char *file, int line) const;  // what HIP_TRY returns
    int pixels(int i) const { return a.rows[i] * a.cols[i]; }  // begin(): fits
    size_t max_blocks() const { return (max_px + 255) / 256; }  // blocks of 256 pixels of the largest view
    int sources(int i) const { return a.pair_offsets[i + 1] - a.pair_offsets[i]; }

    template <typename T> hipError_t alloc(size_t bytes, T **out) { return scratch_.alloc(bytes, out); }

    // First step of every variant.  Clears the last error and checks the arguments: APD_ERR_INVALID with "<who>: ..." before any
    // device is touched.  eth: the weak maps are required, and a view that is its own source is pointed to the host fusion.  Then
    // selects the device.  points = false (the filter): no images, no PLY file and no points are asked for or looked at.
    int begin(bool eth, bool points = true);

    // *out = the caller's map if the maps are on the device, else a device copy of it
    template <typename T> hipError_t device_map(const T *map, size_t bytes, const T **out)
    {
        *out = map;
        return a.maps_on_device ? hipSuccess : scratch_.upload(map, bytes, out);
    }

    // The geometry of cameras[i] and the depth and normal maps: what every view of every variant and of the filter has
    template <typename V> int fill_maps(int i, V &v)
    {
        view_geometry(a.cameras[i], a.rows[i], a.cols[i], v.geo);
        HIP_TRY(device_map(a.depths[i], (size_t)pixels(i) * 4, &v.depth));
        HIP_TRY(device_map(a.normals[i], (size_t)pixels(i) * 12, &v.normal));
        return APD_OK;
    }

    // What DevView and TatView have in common, but for the block map: fill_maps and the image
    template <typename V> int fill_view(int i, V &v)
    {
        HIP_TRY(device_map(a.images[i], (size_t)pixels(i) * 4 * a.image_channels, &v.image));
        return fill_maps(i, v);
    }

    // The optional block map of view i, after the variant's own maps: the last upload of a view, as it always was
    template <typename V> int fill_block(int i, V &v)
    {
        v.block = nullptr;
        if (a.blocks && a.blocks[i]) {
            HIP_TRY(device_map(a.blocks[i], (size_t)pixels(i), &v.block));
        }
        return APD_OK;
    }

    // The view table on the device
    template <typename V> int upload_views(const std::vector<V> &views, V **dviews)
    {
        HIP_TRY(alloc(sizeof(V) * views.size(), dviews));
        HIP_TRY(hipMemcpy(*dviews, views.data(), sizeof(V) * views.size(), hipMemcpyHostToDevice));
        return APD_OK;
    }

    // The scratch every variant needs (xyz, bgr, support, agreeing, block_counts, and what collect() uses) and the staging buffer, sized for the
    // largest view.  Ends the set-up: its time is taken here.
    int alloc_common();
    // View i has its points in xyz / bgr, block_counts filled, and state[p] == accepted where pixel p is a point: packs them in
    // raster order as PLY records (k_fusion_scan, k_fusion_compact; 27-byte records with the normals of the view's map `normal`
    // when the options ask for them) and downloads them, if a file is wanted; appends them to the arrays of the points in memory
    // (k_fusion_compact_soa), if those are wanted.
    int collect(int i, const uint8_t *state, uint8_t accepted, const float *normal);
    // Takes the time of the views, brings a host result down, releases the device memory, writes the file, and then sets
    // *num_points and *points.
    int finish();
    // ms since the constructor or the last lap(): the set-up ends and the views end where a variant says so
    double lap();

private:
    void release();
    int record_bytes() const { return a.opt.ply_normals ? 27 : 15; }
    int reserve_points(long long need);  // room for `need` points in soa_, kept across a growth
    void release_points();

    apd_points_host::Scratch scratch_;  // every device allocation of the call but soa_
    void *staging_ = nullptr;  // page-locked buffer of the point downloads
    int *total_ = nullptr;     // points of the view
    uint8_t *records_ = nullptr;
    // PLY records: x y z float + diffuse_blue/green/red uchar (APD.cpp:214-254), one buffer per view (one growing vector re-allocates
    // and copies hundreds of megabytes at Tanks&Temples scale), downloaded through one page-locked staging buffer
    std::vector<std::vector<uint8_t>> body_;
    long long count_ = 0;
    PointArrays soa_;            // the points in memory so far, device memory outside scratch_: handed to the apd_points_t or freed
    long long soa_capacity_ = 0;
    std::chrono::steady_clock::time_point t_lap_;
};

}  // namespace apd_fusion
