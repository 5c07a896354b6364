// eth_fusion_opt_ref.cpp -- the reference's ETH fusion loop (RunFusion, APD.cpp:892-974) as the sequential loop it is, with the
// eight values of its acceptance rule as parameters instead of literals, the binary PLY of ExportPointCloud (APD.cpp:214-254)
// with or without normals, and per point its normal, support, view and pixel.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_fuse_views_opt (apd-mvs_amd/csrc/apd_fusion.hip) for options the fixed fusion
// oracle (oracle/fusion_oracle.cpp) cannot take; tests/test_fusion_options.py pins it to that oracle at the default values.
// Compiled by tests/eth_fusion_checker.py.  From the product it takes the arithmetic contract only (apd_fusion_math.h: acos_c9,
// exp_c9, lift, drop); the loop -- order of views, pixels and sources, the masks, the thresholds, the score, the acceptance, the
// colour -- is restated here from the reference lines cited.
#include <algorithm>
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
};

// a pixel that had exactly one vote, was rejected for it, and whose source pixel a later pixel of the same view then used
struct Reuse {
    int view, rejected, later;
};

std::vector<Point> g_points;
std::vector<Reuse> g_reuse;

apd_fusion::View view_of(const Camera &cam, int rows, int cols)
{
    apd_fusion::View v;
    memcpy(v.K, cam.K, sizeof(v.K));
    memcpy(v.R, cam.R, sizeof(v.R));
    memcpy(v.t, cam.t, sizeof(v.t));
    // C of Get3DPointonWorld, APD.cpp:791-794
    v.centre[0] = -(cam.R[0] * cam.t[0] + cam.R[3] * cam.t[1] + cam.R[6] * cam.t[2]);
    v.centre[1] = -(cam.R[1] * cam.t[0] + cam.R[4] * cam.t[1] + cam.R[7] * cam.t[2]);
    v.centre[2] = -(cam.R[2] * cam.t[0] + cam.R[5] * cam.t[1] + cam.R[8] * cam.t[2]);
    v.rows = rows;
    v.cols = cols;
    return v;
}

// int(v + 0.5f) (APD.cpp:925-926): where C++ leaves the conversion undefined (NaN, |v| >= 2^31) the reference's x86 build
// gets INT_MIN, a pixel outside every image
int to_pixel(float v)
{
    const float shifted = v + 0.5f;
    return (shifted > -2147483648.0f && shifted < 2147483648.0f) ? (int)shifted : -1;
}

}  // namespace

extern "C" {

// Views in order, pixels in raster order.  images: floats 0..255, channels 1 or 3; blocks or blocks[i] may be null.  ply_path
// may be null.  Returns the number of points, -1 if the file cannot be written.
long long eth_fuse_opt(const Rule *rule, int num_views, const Camera *cameras, const float *const *images, int channels,
                       const float *const *depths, const float *const *normals, const uint8_t *const *weaks, const uint8_t *const *blocks,
                       const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, const char *ply_path, int ply_normals)
{
    g_points.clear();
    g_reuse.clear();
    std::vector<apd_fusion::View> views;
    std::vector<std::vector<uint8_t>> masks;      // APD.cpp:884
    std::vector<std::vector<int>> sole_vote_of;   // per source pixel: the rejected one-vote pixel of the CURRENT view that voted here
    for (int i = 0; i < num_views; ++i) {
        views.push_back(view_of(cameras[i], rows[i], cols[i]));
        masks.emplace_back((size_t)rows[i] * cols[i], (uint8_t)0);
        sole_vote_of.emplace_back((size_t)rows[i] * cols[i], -1);
    }
    for (int i = 0; i < num_views; ++i) {  // APD.cpp:892
        const apd_fusion::View &ref = views[i];
        const int num_ngb = pair_offsets[i + 1] - pair_offsets[i];
        const int *src_of = pair_indices + pair_offsets[i];
        for (std::vector<int> &s : sole_vote_of) {
            std::fill(s.begin(), s.end(), -1);
        }
        for (int r = 0; r < ref.rows; ++r) {
            for (int c = 0; c < ref.cols; ++c) {
                const int p = r * ref.cols + c;
                if (blocks && blocks[i] && blocks[i][p] < 128) {  // :901
                    continue;
                }
                if (masks[i][p] == 1) {  // :905
                    continue;
                }
                const float ref_depth = depths[i][p];
                if (ref_depth <= 0.0) {  // :910
                    continue;
                }
                const float *ref_normal = normals[i] + 3 * (size_t)p;
                float PointX[3];
                apd_fusion::lift(ref, c, r, ref_depth, PointX);  // :913
                int num_consistent = 0;
                float dynamic_consistency = 0.0f;
                std::vector<int> used(num_ngb, -1);  // :917, as a raster index
                for (int j = 0; j < num_ngb; ++j) {
                    const apd_fusion::View &src = views[src_of[j]];
                    float px, py, proj_depth;
                    apd_fusion::drop(src, PointX, px, py, proj_depth);  // :924
                    const int src_r = to_pixel(py), src_c = to_pixel(px);
                    if (!(src_c >= 0 && src_c < src.cols && src_r >= 0 && src_r < src.rows)) {
                        continue;
                    }
                    const int s = src_r * src.cols + src_c;
                    if (masks[src_of[j]][s] == 1) {  // :928
                        continue;
                    }
                    const float src_depth = depths[src_of[j]][s];
                    if (src_depth <= 0.0) {  // :931
                        continue;
                    }
                    const float *src_normal = normals[src_of[j]] + 3 * (size_t)s;
                    float tmp_X[3], tx, ty;
                    apd_fusion::lift(src, src_c, src_r, src_depth, tmp_X);   // :934
                    apd_fusion::drop(ref, tmp_X, tx, ty, proj_depth);        // :936
                    const float reproj_error = (float)sqrt(pow((double)(c - tx), 2) + pow((double)(r - ty), 2));  // :937
                    const float relative_depth_diff = fabsf(proj_depth - ref_depth) / ref_depth;                 // :938
                    const float dot_product = ref_normal[0] * src_normal[0] + ref_normal[1] * src_normal[1] + ref_normal[2] * src_normal[2];
                    float angle = apd_fusion::acos_c9(dot_product);  // GetAngle, :814-823
                    if (angle != angle) {
                        angle = 0.0f;
                    }
                    if (reproj_error < rule->max_reproj_error && relative_depth_diff < rule->max_relative_depth && angle < rule->max_angle) {  // :941
                        used[j] = s;
                        const float tmp_index = reproj_error + rule->depth_weight * relative_depth_diff + angle * rule->angle_weight;  // :944
                        dynamic_consistency += apd_fusion::exp_c9(-tmp_index);
                        num_consistent++;
                    }
                }
                const float factor = (weaks[i][p] == 0 /* WEAK */ ? rule->factor_weak : rule->factor_strong);  // :950
                if (num_consistent >= rule->min_consistent && (dynamic_consistency > factor * num_consistent)) {  // :951
                    Point pt;
                    memcpy(pt.xyz, PointX, sizeof(pt.xyz));
                    memcpy(pt.normal, ref_normal, sizeof(pt.normal));
                    float colour[3];
                    for (int k = 0; k < 3; ++k) {
                        colour[k] = images[i][(size_t)p * channels + (channels == 3 ? k : 0)];
                    }
                    for (int j = 0; j < num_ngb; ++j) {
                        if (used[j] == -1) {
                            continue;
                        }
                        masks[src_of[j]][used[j]] = 1;  // :959
                        if (sole_vote_of[src_of[j]][used[j]] >= 0) {
                            g_reuse.push_back(Reuse{i, sole_vote_of[src_of[j]][used[j]], p});
                        }
                        for (int k = 0; k < 3; ++k) {
                            colour[k] += images[src_of[j]][(size_t)used[j] * channels + (channels == 3 ? k : 0)];
                        }
                    }
                    for (int k = 0; k < 3; ++k) {
                        colour[k] /= (num_consistent + 1);             // :965
                        pt.bgr[k] = static_cast<uint8_t>(colour[k]);   // :240
                    }
                    pt.support = (uint8_t)num_consistent;
                    pt.view = i;
                    pt.pixel = p;
                    g_points.push_back(pt);
                } else if (num_consistent == 1 && rule->min_consistent > 1 && dynamic_consistency > factor * num_consistent) {
                    for (int j = 0; j < num_ngb; ++j) {  // rejected for its count alone: remember where its one vote went
                        if (used[j] != -1 && sole_vote_of[src_of[j]][used[j]] < 0) {
                            sole_vote_of[src_of[j]][used[j]] = p;
                        }
                    }
                }
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

// The points of the last eth_fuse_opt as arrays of its count (any pointer may be null)
void eth_fuse_points(float *xyz, float *normal, uint8_t *bgr, uint8_t *support, int *view, int *pixel)
{
    for (size_t k = 0; k < g_points.size(); ++k) {
        const Point &pt = g_points[k];
        if (xyz) memcpy(xyz + 3 * k, pt.xyz, 12);
        if (normal) memcpy(normal + 3 * k, pt.normal, 12);
        if (bgr) memcpy(bgr + 3 * k, pt.bgr, 3);
        if (support) support[k] = pt.support;
        if (view) view[k] = pt.view;
        if (pixel) pixel[k] = pt.pixel;
    }
}

long long eth_fuse_reuse_count(void) { return (long long)g_reuse.size(); }

// (view, rejected pixel, later pixel) triples of the last eth_fuse_opt
void eth_fuse_reuse(int *triples) { memcpy(triples, g_reuse.data(), g_reuse.size() * sizeof(Reuse)); }

}  // extern "C"
