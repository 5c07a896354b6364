// tat_fusion_ref.cpp -- the reference's two Tanks and Temples fusion loops as they are written: RunFusion_TAT_Intermediate
// (APD.cpp:979-1147) and RunFusion_TAT_advanced (APD.cpp:1149-1296), one sequential loop over views, rows, columns and
// source views, with the per-view `diff` entries that keep the values of the last pixel at which a source was valid, and the
// binary PLY of ExportPointCloud (APD.cpp:214-254).
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_fuse_views_variant (apd-mvs_amd/csrc/apd_fusion_tat.hip), compiled by
// tests/test_tat_fusion_checker.py.  It includes nothing from the product; the helpers below restate the reference lines they
// cite.  acosf is the fusion oracle's orc_fusion_acos (oracle/fusion_oracle.cpp), which tests/test_fusion_oracle.py pins to
// libm and to the product's kernel.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" float orc_fusion_acos(float x);

namespace {

struct Camera {  // main.h:47-56 (== apd_camera of include/apd_mi355x.h)
    float K[9], R[9], t[3], c[3];
    int height, width;
    float depth_min, depth_max;
};

struct float2 {
    float x, y;
};
struct float3 {
    float x, y, z;
};

// APD.cpp:776-803
float3 Get3DPointonWorld(int x, int y, float depth, const Camera &camera)
{
    float3 pointX, tmpX, C;
    pointX.x = depth * (x - camera.K[2]) / camera.K[0];
    pointX.y = depth * (y - camera.K[5]) / camera.K[4];
    pointX.z = depth;
    tmpX.x = camera.R[0] * pointX.x + camera.R[3] * pointX.y + camera.R[6] * pointX.z;
    tmpX.y = camera.R[1] * pointX.x + camera.R[4] * pointX.y + camera.R[7] * pointX.z;
    tmpX.z = camera.R[2] * pointX.x + camera.R[5] * pointX.y + camera.R[8] * pointX.z;
    C.x = -(camera.R[0] * camera.t[0] + camera.R[3] * camera.t[1] + camera.R[6] * camera.t[2]);
    C.y = -(camera.R[1] * camera.t[0] + camera.R[4] * camera.t[1] + camera.R[7] * camera.t[2]);
    C.z = -(camera.R[2] * camera.t[0] + camera.R[5] * camera.t[1] + camera.R[8] * camera.t[2]);
    return float3{tmpX.x + C.x, tmpX.y + C.y, tmpX.z + C.z};
}

// APD.cpp:805-815
void ProjectCamera(const float3 &PointX, const Camera &camera, float2 &point, float &depth)
{
    float3 tmp;
    tmp.x = camera.R[0] * PointX.x + camera.R[1] * PointX.y + camera.R[2] * PointX.z + camera.t[0];
    tmp.y = camera.R[3] * PointX.x + camera.R[4] * PointX.y + camera.R[5] * PointX.z + camera.t[1];
    tmp.z = camera.R[6] * PointX.x + camera.R[7] * PointX.y + camera.R[8] * PointX.z + camera.t[2];
    depth = camera.K[6] * tmp.x + camera.K[7] * tmp.y + camera.K[8] * tmp.z;
    point.x = (camera.K[0] * tmp.x + camera.K[1] * tmp.y + camera.K[2] * tmp.z) / depth;
    point.y = (camera.K[3] * tmp.x + camera.K[4] * tmp.y + camera.K[5] * tmp.z) / depth;
}

// APD.cpp:817-824
float GetAngle(const float *v1, const float *v2)
{
    const float dot_product = v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2];
    const float angle = orc_fusion_acos(dot_product);
    return angle != angle ? 0.0f : angle;
}

// int(v + 0.5f) (APD.cpp:1089-1090): undefined in C++ for NaN and |v| >= 2^31, where the reference's x86 build gets INT_MIN
// (cvttss2si), a pixel outside every image -- which `false` reports
bool RoundToPixel(float v, int &pixel)
{
    const float shifted = v + 0.5f;
    if (shifted > -2147483648.0f && shifted < 2147483648.0f) {
        pixel = (int)shifted;
        return true;
    }
    return false;
}

struct CostData {  // APD.cpp:1045-1064 (Intermediate), :1212-1225 (advanced)
    float dist = FLT_MAX, depth = FLT_MAX, angle = FLT_MAX;
    int src_r = 0, src_c = 0;
    bool use = false;
    bool fresh = false;  // not in the reference: written at the current pixel (else stale), for the tests' statistics
    long long writer = -1;  // not in the reference: the pixel (raster index) that wrote the entry last, for the tests' statistics
};

}  // namespace

// variant 1: RunFusion_TAT_Intermediate, 2: RunFusion_TAT_advanced.  Same flat arguments as apd_fuse_views_variant with host
// pointers (no weak maps).  Returns the number of points written, -1 on I/O failure or an unknown variant; *stale_points: how
// many of them used at least one diff entry written at an earlier pixel; *max_gap: the largest (pixel - writer) over the
// entries the points used, in raster pixels of the view (0: every used entry was fresh or there is no point).
extern "C" long long tat_fuse(int variant, int num_views, const void *cameras_v, const float *const *images, int image_channels,
                              const float *const *depths, const float *const *normals, const uint8_t *const *blocks, const int *rows_of,
                              const int *cols_of, const int *pair_offsets, const int *pair_indices, const char *ply_path,
                              long long *stale_points, long long *max_gap)
{
    if (variant != 1 && variant != 2) {
        return -1;
    }
    const bool intermediate = variant == 1;
    const float dist_base = 0.25f;
    const float depth_base = intermediate ? 1.0f / 3500.0f : 1.0f / 3000.0f;
    const float angle_base = 0.06981317007977318f;  // 4 degree
    const float angle_grad = 0.05235987755982988f;  // 3 degree
    const Camera *cameras = static_cast<const Camera *>(cameras_v);
    std::vector<std::vector<uint8_t>> masks(num_views);
    for (int i = 0; i < num_views; ++i) {
        masks[i].assign((size_t)rows_of[i] * cols_of[i], 0);
    }
    const int nc = image_channels;
    auto colour_at = [&](int view, size_t px, int k) { return images[view][px * nc + (nc == 3 ? k : 0)]; };
    std::vector<uint8_t> cloud;  // 15 bytes per point: x y z float, blue green red uchar (APD.cpp:236-247)
    long long count_points = 0, stale = 0, gap = 0;
    for (int ref_index = 0; ref_index < num_views; ++ref_index) {
        const int cols = cols_of[ref_index], rows = rows_of[ref_index];
        const int num_ngb = pair_offsets[ref_index + 1] - pair_offsets[ref_index];
        const int *src_of = pair_indices + pair_offsets[ref_index];
        std::vector<CostData> diff(num_ngb, CostData());  // once per view (APD.cpp:1069, :1233)
        for (int r = 0; r < rows; ++r) {
            for (int c = 0; c < cols; ++c) {
                const size_t ref_px = (size_t)r * cols + c;
                if (blocks && blocks[ref_index] && blocks[ref_index][ref_px] < 128) {
                    continue;
                }
                const float ref_depth = depths[ref_index][ref_px];
                if (ref_depth <= 0.0) {
                    continue;
                }
                const float *ref_normal = normals[ref_index] + 3 * ref_px;
                const float3 PointX = Get3DPointonWorld(c, r, ref_depth, cameras[ref_index]);
                for (int j = 0; j < num_ngb; ++j) {
                    diff[j].fresh = false;
                    const int src_index = src_of[j];
                    const int src_cols = cols_of[src_index], src_rows = rows_of[src_index];
                    float2 point;
                    float proj_depth;
                    ProjectCamera(PointX, cameras[src_index], point, proj_depth);
                    int src_r, src_c;
                    if (!RoundToPixel(point.y, src_r) || !RoundToPixel(point.x, src_c)) {
                        continue;
                    }
                    if (src_c >= 0 && src_c < src_cols && src_r >= 0 && src_r < src_rows) {
                        const size_t src_px = (size_t)src_r * src_cols + src_c;
                        if (masks[src_index][src_px] == 1) {
                            continue;
                        }
                        const float src_depth = depths[src_index][src_px];
                        if (src_depth <= 0.0) {
                            continue;
                        }
                        const float *src_normal = normals[src_index] + 3 * src_px;
                        const float3 tmp_X = Get3DPointonWorld(src_c, src_r, src_depth, cameras[src_index]);
                        float2 tmp_pt;
                        ProjectCamera(tmp_X, cameras[ref_index], tmp_pt, proj_depth);
                        // sqrt(pow(c - tmp_pt.x, 2) + pow(r - tmp_pt.y, 2)): float differences, double pow and sqrt
                        const double dx = (double)(c - tmp_pt.x), dy = (double)(r - tmp_pt.y);
                        diff[j].dist = (float)std::sqrt(dx * dx + dy * dy);
                        diff[j].depth = std::fabs(proj_depth - ref_depth) / ref_depth;
                        diff[j].angle = GetAngle(ref_normal, src_normal);
                        diff[j].src_r = src_r;
                        diff[j].src_c = src_c;
                        diff[j].fresh = true;
                        diff[j].writer = (long long)ref_px;
                    }
                }
                for (int k = 2; k <= num_ngb; ++k) {
                    int count = 0;
                    for (int j = 0; j < num_ngb; ++j) {
                        diff[j].use = false;
                        if (diff[j].dist < k * dist_base && diff[j].depth < k * depth_base &&
                            (!intermediate || diff[j].angle < (k * angle_grad + angle_base))) {
                            count++;
                            diff[j].use = true;
                        }
                    }
                    if (count >= k) {
                        float consistent_Color[3];
                        for (int ch = 0; ch < 3; ++ch) {
                            consistent_Color[ch] = colour_at(ref_index, ref_px, ch);
                        }
                        bool used_stale = false;
                        for (int j = 0; j < num_ngb; ++j) {
                            if (!diff[j].use) {
                                continue;
                            }
                            used_stale = used_stale || !diff[j].fresh;
                            gap = std::max(gap, (long long)ref_px - diff[j].writer);
                            if (intermediate) {
                                const int src_index = src_of[j];
                                const size_t src_px = (size_t)diff[j].src_r * cols_of[src_index] + diff[j].src_c;
                                for (int ch = 0; ch < 3; ++ch) {
                                    consistent_Color[ch] += colour_at(src_index, src_px, ch);
                                }
                            }
                        }
                        if (intermediate) {
                            for (int ch = 0; ch < 3; ++ch) {
                                consistent_Color[ch] /= (count + 1.0f);
                            }
                        }
                        uint8_t record[15];
                        memcpy(record, &PointX, 12);
                        for (int ch = 0; ch < 3; ++ch) {
                            record[12 + ch] = static_cast<uint8_t>(consistent_Color[ch]);  // (uchar) of the float colour, :240-242
                        }
                        cloud.insert(cloud.end(), record, record + 15);
                        ++count_points;
                        stale += used_stale ? 1 : 0;
                        masks[ref_index][ref_px] = 1;
                        break;
                    }
                }
            }
        }
    }
    if (stale_points) {
        *stale_points = stale;
    }
    if (max_gap) {
        *max_gap = gap;
    }
    FILE *f = fopen(ply_path, "wb");  // ExportPointCloud, APD.cpp:214-254
    if (!f) {
        return -1;
    }
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n", (int)count_points);
    const bool ok = cloud.empty() || fwrite(cloud.data(), 1, cloud.size(), f) == cloud.size();
    return (fclose(f) == 0 && ok) ? count_points : -1;
}
