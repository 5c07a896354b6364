// points_average_ref.cpp -- the mean position and normal of fused points over their agreeing views, as one sequential loop over
// the points: for every point the masked loop over its view's source list, the sums from the stored position and normal, the
// divisions by the number of contributions and the renormalisation of the mean normal, all written out here.
//
// TEST INFRASTRUCTURE ONLY: the checker of apd_points_average (apd-mvs_amd/csrc/apd_points_average.hip), compiled by
// tests/points_average_checker.py.  From the product it takes lift, drop and vote_target of the arithmetic contract
// (apd_fusion_math.h) and nothing else: it does not call apd_fusion::mean_point, the code under test.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "apd_fusion_math.h"

namespace {

struct Camera {  // main.h:47-56 (== apd_camera of include/apd_mi355x.h)
    float K[9], R[9], t[3], c[3];
    int height, width;
    float depth_min, depth_max;
};

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

}  // namespace

extern "C" {

// Point k < n (xyz, normal, view, sources) -> out_xyz, out_normal, out_sources (the sources that contributed), out_support (their
// number).  contributions, normal_contributions (both may be null): per point 32 x 3 floats, the lifted point and the normal of
// source j at [k][j] (untouched where bit j did not contribute), for the tests that look at the terms behind a mean.
void points_average(int num_views, const Camera *cameras, const float *const *depths, const float *const *normals, const int *rows,
                    const int *cols, const int *pair_offsets, const int *pair_indices, long long n, const float *xyz, const float *normal,
                    const int32_t *view, const uint32_t *sources, float *out_xyz, float *out_normal, uint32_t *out_sources,
                    uint8_t *out_support, float *contributions, float *normal_contributions)
{
    std::vector<apd_fusion::View> geo;
    for (int i = 0; i < num_views; ++i) {
        geo.push_back(view_of(cameras[i], rows[i], cols[i]));
    }
    for (long long k = 0; k < n; ++k) {
        const float *P = xyz + 3 * k;
        float sum_p[3] = {P[0], P[1], P[2]};
        float sum_n[3] = {normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]};
        const int v = view[k];
        const int num_src = pair_offsets[v + 1] - pair_offsets[v];
        int used = 0;
        uint32_t kept = 0;
        for (int j = 0; j < 32; ++j) {
            if (!((sources[k] >> j) & 1u) || j >= num_src) {
                continue;
            }
            const int s = pair_indices[pair_offsets[v] + j];
            int sc, sr;
            if (!apd_fusion::vote_target(geo[s], P, sc, sr)) {
                continue;
            }
            const size_t idx = (size_t)sr * (size_t)cols[s] + (size_t)sc;
            const float d = depths[s][idx];
            if (d <= 0.0f) {
                continue;
            }
            float Q[3];
            apd_fusion::lift(geo[s], sc, sr, d, Q);
            for (int c = 0; c < 3; ++c) {
                sum_p[c] = sum_p[c] + Q[c];
                sum_n[c] = sum_n[c] + normals[s][3 * idx + c];
                if (contributions) {
                    contributions[(k * 32 + j) * 3 + c] = Q[c];
                }
                if (normal_contributions) {
                    normal_contributions[(k * 32 + j) * 3 + c] = normals[s][3 * idx + c];
                }
            }
            used = used + 1;
            kept = kept | (1u << j);
        }
        const float count = (float)(used + 1);
        float t[3];
        for (int c = 0; c < 3; ++c) {
            out_xyz[3 * k + c] = sum_p[c] / count;
            t[c] = sum_n[c] / count;
        }
        const float squares = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        const float len = sqrtf(squares);
        for (int c = 0; c < 3; ++c) {
            out_normal[3 * k + c] = len > 0.0f ? t[c] / len : 0.0f;
        }
        out_sources[k] = kept;
        out_support[k] = (uint8_t)used;
    }
}

}  // extern "C"
