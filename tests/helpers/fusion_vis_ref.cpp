// fusion_vis_ref.cpp -- the reference's three fusion loops (RunFusion, APD.cpp:892-974; RunFusion_TAT_Intermediate,
// APD.cpp:979-1147; RunFusion_TAT_advanced, APD.cpp:1149-1296) as the sequential loops they are, keeping what the reference
// throws away: `used_list` of the ETH loop (APD.cpp:917-964) and the sources with diff[j].use set in the emitting round of the
// T&T loops.  Per point: the fields of the PLY record, normal, support, view, pixel, the agreeing sources as a bit mask over
// the view's source list, and the list of views that see the point (its own first, then the agreeing sources in source order) --
// the lists are appended while the loop runs, not derived from the masks.  Writes the binary PLY of ExportPointCloud
// (APD.cpp:214-254) and COLMAP's fused.ply.vis.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_sources / apd_points_visibility / apd_points_write_vis
// (apd-mvs_amd/csrc/apd_fusion.hip, apd_fusion_tat.hip), compiled by tests/vis_checker.py.  tests/test_fusion_visibility.py ties
// it to the two existing checkers (eth_fusion_opt_ref.cpp, tat_fusion_ref.cpp) through the PLY bytes on the shared cases.  From the
// product it takes the arithmetic contract only (apd_fusion_math.h: acos_c9, exp_c9, lift, drop).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "apd_fusion_math.h"

namespace {

struct Camera {  // main.h:47-56 (== apd_camera of include/apd_mi355x.h)
    float K[9], R[9], t[3], c[3];
    int height, width;
    float depth_min, depth_max;
};

struct Rule {  // the literals of APD.cpp:941-951, in the order of apd_fusion_options
    float max_reproj_error, max_relative_depth, max_angle, depth_weight, angle_weight;
    int min_consistent;
    float factor_strong, factor_weak;
};

struct Point {
    float xyz[3], normal[3];
    uint8_t bgr[3], support;
    int view, pixel;
    uint32_t sources;
};

struct Diff {  // CostData, APD.cpp:1045-1064 (:1212-1225)
    float dist = FLT_MAX, depth = FLT_MAX, angle = FLT_MAX;
    int src_px = 0;
    bool use = false;
};

std::vector<Point> g_points;
std::vector<long long> g_offsets;  // g_points.size() + 1 entries
std::vector<int32_t> g_views;

apd_fusion::View view_of(const Camera &cam, int rows, int cols)
{
    apd_fusion::View v;
    memcpy(v.K, cam.K, sizeof(v.K));
    memcpy(v.R, cam.R, sizeof(v.R));
    memcpy(v.t, cam.t, sizeof(v.t));
    v.centre[0] = -(cam.R[0] * cam.t[0] + cam.R[3] * cam.t[1] + cam.R[6] * cam.t[2]);  // APD.cpp:791-794
    v.centre[1] = -(cam.R[1] * cam.t[0] + cam.R[4] * cam.t[1] + cam.R[7] * cam.t[2]);
    v.centre[2] = -(cam.R[2] * cam.t[0] + cam.R[5] * cam.t[1] + cam.R[8] * cam.t[2]);
    v.rows = rows;
    v.cols = cols;
    return v;
}

// int(v + 0.5f) (APD.cpp:925-926): where C++ leaves the conversion undefined (NaN, |v| >= 2^31) the reference's x86 build gets
// INT_MIN, a pixel outside every image
int to_pixel(float v)
{
    const float shifted = v + 0.5f;
    return (shifted > -2147483648.0f && shifted < 2147483648.0f) ? (int)shifted : -1;
}

// the three costs of a reference pixel against a source pixel (APD.cpp:934-939, :1098-1103, :1264-1269)
void costs(const apd_fusion::View &ref, const apd_fusion::View &src, int c, int r, float ref_depth, const float *ref_normal, int src_c,
           int src_r, float src_depth, const float *src_normal, float &dist, float &depth, float &angle)
{
    float tmp_X[3], tx, ty, proj_depth;
    apd_fusion::lift(src, src_c, src_r, src_depth, tmp_X);
    apd_fusion::drop(ref, tmp_X, tx, ty, proj_depth);
    dist = (float)sqrt(pow((double)(c - tx), 2) + pow((double)(r - ty), 2));
    depth = fabsf(proj_depth - ref_depth) / ref_depth;
    const float dot_product = ref_normal[0] * src_normal[0] + ref_normal[1] * src_normal[1] + ref_normal[2] * src_normal[2];
    angle = apd_fusion::acos_c9(dot_product);  // GetAngle, APD.cpp:814-823
    if (angle != angle) {
        angle = 0.0f;
    }
}

}  // namespace

extern "C" {

// variant 0: RunFusion with `rule`, 1: RunFusion_TAT_Intermediate, 2: RunFusion_TAT_advanced (rule and weaks are not read).
// Views in order, pixels in raster order.  images: floats 0..255, channels 1 or 3; blocks or blocks[i] may be null; ply_path may
// be null.  Returns the number of points, -1 if the file cannot be written or the variant is unknown.
long long vis_fuse(int variant, const Rule *rule, int num_views, const Camera *cameras, const float *const *images, int channels,
                   const float *const *depths, const float *const *normals, const uint8_t *const *weaks, const uint8_t *const *blocks,
                   const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, const char *ply_path, int ply_normals)
{
    g_points.clear();
    g_offsets.assign(1, 0);
    g_views.clear();
    if (variant < 0 || variant > 2) {
        return -1;
    }
    const bool intermediate = variant == 1;
    const float dist_base = 0.25f;  // APD.cpp:984-989, :1154-1155
    const float depth_base = intermediate ? 1.0f / 3500.0f : 1.0f / 3000.0f;
    const float angle_base = 0.06981317007977318f;
    const float angle_grad = 0.05235987755982988f;
    std::vector<apd_fusion::View> views;
    std::vector<std::vector<uint8_t>> masks;  // APD.cpp:884, :1038, :1205
    for (int i = 0; i < num_views; ++i) {
        views.push_back(view_of(cameras[i], rows[i], cols[i]));
        masks.emplace_back((size_t)rows[i] * cols[i], (uint8_t)0);
    }
    auto colour_at = [&](int view, size_t px, int k) { return images[view][px * channels + (channels == 3 ? k : 0)]; };
    for (int i = 0; i < num_views; ++i) {
        const apd_fusion::View &ref = views[i];
        const int num_ngb = pair_offsets[i + 1] - pair_offsets[i];
        const int *src_of = pair_indices + pair_offsets[i];
        std::vector<Diff> diff(num_ngb, Diff());  // T&T: once per view (APD.cpp:1069, :1233)
        for (int r = 0; r < ref.rows; ++r) {
            for (int c = 0; c < ref.cols; ++c) {
                const int p = r * ref.cols + c;
                if (blocks && blocks[i] && blocks[i][p] < 128) {
                    continue;
                }
                if (variant == 0 && masks[i][p] == 1) {  // :905; the T&T loops do not look at the reference's own mask
                    continue;
                }
                const float ref_depth = depths[i][p];
                if (ref_depth <= 0.0) {
                    continue;
                }
                const float *ref_normal = normals[i] + 3 * (size_t)p;
                float PointX[3];
                apd_fusion::lift(ref, c, r, ref_depth, PointX);
                std::vector<int> used(num_ngb, -1);  // `used_list`, as the raster index of the source pixel; -1: not used
                int count = 0;
                bool emit = false;
                if (variant == 0) {
                    float dynamic_consistency = 0.0f;
                    for (int j = 0; j < num_ngb; ++j) {
                        const apd_fusion::View &src = views[src_of[j]];
                        float px, py, proj_depth;
                        apd_fusion::drop(src, PointX, px, py, proj_depth);
                        const int src_r = to_pixel(py), src_c = to_pixel(px);
                        if (!(src_c >= 0 && src_c < src.cols && src_r >= 0 && src_r < src.rows)) {
                            continue;
                        }
                        const int s = src_r * src.cols + src_c;
                        if (masks[src_of[j]][s] == 1) {
                            continue;
                        }
                        const float src_depth = depths[src_of[j]][s];
                        if (src_depth <= 0.0) {
                            continue;
                        }
                        float dist, depth, angle;
                        costs(ref, src, c, r, ref_depth, ref_normal, src_c, src_r, src_depth, normals[src_of[j]] + 3 * (size_t)s, dist, depth, angle);
                        if (dist < rule->max_reproj_error && depth < rule->max_relative_depth && angle < rule->max_angle) {  // :941
                            used[j] = s;
                            const float tmp_index = dist + rule->depth_weight * depth + angle * rule->angle_weight;  // :944
                            dynamic_consistency += apd_fusion::exp_c9(-tmp_index);
                            count++;
                        }
                    }
                    const float factor = (weaks[i][p] == 0 /* WEAK */ ? rule->factor_weak : rule->factor_strong);  // :950
                    emit = count >= rule->min_consistent && (dynamic_consistency > factor * count);                 // :951
                } else {
                    for (int j = 0; j < num_ngb; ++j) {
                        const apd_fusion::View &src = views[src_of[j]];
                        float px, py, proj_depth;
                        apd_fusion::drop(src, PointX, px, py, proj_depth);
                        const int src_r = to_pixel(py), src_c = to_pixel(px);
                        if (!(src_c >= 0 && src_c < src.cols && src_r >= 0 && src_r < src.rows)) {
                            continue;
                        }
                        const int s = src_r * src.cols + src_c;
                        if (masks[src_of[j]][s] == 1) {
                            continue;
                        }
                        const float src_depth = depths[src_of[j]][s];
                        if (src_depth <= 0.0) {
                            continue;
                        }
                        costs(ref, src, c, r, ref_depth, ref_normal, src_c, src_r, src_depth, normals[src_of[j]] + 3 * (size_t)s, diff[j].dist,
                              diff[j].depth, diff[j].angle);
                        diff[j].src_px = s;
                    }
                    for (int k = 2; k <= num_ngb && !emit; ++k) {  // :1111-1144, :1277-1293
                        count = 0;
                        for (int j = 0; j < num_ngb; ++j) {
                            diff[j].use = diff[j].dist < k * dist_base && diff[j].depth < k * depth_base &&
                                          (!intermediate || diff[j].angle < (k * angle_grad + angle_base));
                            count += diff[j].use ? 1 : 0;
                        }
                        emit = count >= k;
                    }
                    for (int j = 0; j < num_ngb && emit; ++j) {
                        if (diff[j].use) {
                            used[j] = diff[j].src_px;
                        }
                    }
                }
                if (!emit) {
                    continue;
                }
                Point pt;
                memcpy(pt.xyz, PointX, sizeof(pt.xyz));
                memcpy(pt.normal, ref_normal, sizeof(pt.normal));
                float colour[3];
                for (int k = 0; k < 3; ++k) {
                    colour[k] = colour_at(i, (size_t)p, k);
                }
                pt.sources = 0;
                g_views.push_back(i);
                for (int j = 0; j < num_ngb; ++j) {
                    if (used[j] == -1) {
                        continue;
                    }
                    pt.sources |= 1u << j;
                    g_views.push_back(src_of[j]);
                    if (variant == 0) {
                        masks[src_of[j]][used[j]] = 1;  // :959
                    }
                    if (variant != 2) {  // the advanced loop keeps the reference pixel's colour
                        for (int k = 0; k < 3; ++k) {
                            colour[k] += colour_at(src_of[j], (size_t)used[j], k);
                        }
                    }
                }
                for (int k = 0; k < 3; ++k) {
                    if (variant == 0) {
                        colour[k] /= (count + 1);     // :965
                    } else if (variant == 1) {
                        colour[k] /= (count + 1.0f);  // :1131
                    }
                    pt.bgr[k] = static_cast<uint8_t>(colour[k]);  // :240
                }
                if (variant != 0) {
                    masks[i][p] = 1;
                }
                pt.support = (uint8_t)count;
                pt.view = i;
                pt.pixel = p;
                g_points.push_back(pt);
                g_offsets.push_back((long long)g_views.size());
            }
        }
    }
    if (ply_path) {
        FILE *f = fopen(ply_path, "wb");
        if (!f) {
            return -1;
        }
        fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n",
                (int)g_points.size());
        if (ply_normals) {
            fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
        }
        fprintf(f, "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n");
        for (const Point &pt : g_points) {
            fwrite(pt.xyz, 4, 3, f);
            if (ply_normals) {
                fwrite(pt.normal, 4, 3, f);
            }
            fwrite(pt.bgr, 1, 3, f);
        }
        if (fclose(f) != 0) {
            return -1;
        }
    }
    return (long long)g_points.size();
}

// The points of the last vis_fuse as arrays of its count (any pointer may be null)
void vis_points(float *xyz, float *normal, uint8_t *bgr, uint8_t *support, int *view, int *pixel, uint32_t *sources)
{
    for (size_t k = 0; k < g_points.size(); ++k) {
        const Point &pt = g_points[k];
        if (xyz) memcpy(xyz + 3 * k, pt.xyz, 12);
        if (normal) memcpy(normal + 3 * k, pt.normal, 12);
        if (bgr) memcpy(bgr + 3 * k, pt.bgr, 3);
        if (support) support[k] = pt.support;
        if (view) view[k] = pt.view;
        if (pixel) pixel[k] = pt.pixel;
        if (sources) sources[k] = pt.sources;
    }
}

long long vis_entries(void) { return (long long)g_views.size(); }

// offsets: count + 1 entries; views: vis_entries() entries
void vis_lists(long long *offsets, int32_t *views)
{
    memcpy(offsets, g_offsets.data(), g_offsets.size() * sizeof(long long));
    if (!g_views.empty()) {
        memcpy(views, g_views.data(), g_views.size() * sizeof(int32_t));
    }
}

// COLMAP's fused.ply.vis of the last vis_fuse: uint64 number of points, then per point uint32 n and n x uint32 view index.
// 0, or -1 if the file cannot be written.
int vis_write(const char *path)
{
    FILE *f = fopen(path, "wb");
    if (!f) {
        return -1;
    }
    const uint64_t n = g_points.size();
    fwrite(&n, 8, 1, f);
    for (size_t k = 0; k < g_points.size(); ++k) {
        const uint32_t len = (uint32_t)(g_offsets[k + 1] - g_offsets[k]);
        fwrite(&len, 4, 1, f);
        for (long long e = g_offsets[k]; e < g_offsets[k + 1]; ++e) {
            const uint32_t v = (uint32_t)g_views[(size_t)e];
            fwrite(&v, 4, 1, f);
        }
    }
    return fclose(f) == 0 ? 0 : -1;
}

}  // extern "C"
