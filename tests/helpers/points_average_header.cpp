// points_average_header.cpp -- apd_fusion::mean_point (apd_fusion_math.h), the arithmetic of apd_points_average, compiled by the
// host compiler and run over a list of points: what the device kernel computes per lane, on the CPU.
//
// TEST INFRASTRUCTURE ONLY: tests/test_points_average.py compares it bitwise with the independent loop of
// points_average_ref.cpp, so that the arithmetic contract (C9) of the function is checked on a machine without a device.
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

}  // namespace

extern "C" void points_average_header(int num_views, const Camera *cameras, const float *const *depths, const float *const *normals,
                                      const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, long long n,
                                      const float *xyz, const float *normal, const int32_t *view, const uint32_t *sources, float *out_xyz,
                                      float *out_normal, uint32_t *out_sources, uint8_t *out_support)
{
    std::vector<apd_fusion::MapView> views((size_t)num_views);
    for (int i = 0; i < num_views; ++i) {
        apd_fusion::View &g = views[i].geo;
        const Camera &cam = cameras[i];
        memcpy(g.K, cam.K, sizeof(g.K));
        memcpy(g.R, cam.R, sizeof(g.R));
        memcpy(g.t, cam.t, sizeof(g.t));
        g.centre[0] = -(cam.R[0] * cam.t[0] + cam.R[3] * cam.t[1] + cam.R[6] * cam.t[2]);
        g.centre[1] = -(cam.R[1] * cam.t[0] + cam.R[4] * cam.t[1] + cam.R[7] * cam.t[2]);
        g.centre[2] = -(cam.R[2] * cam.t[0] + cam.R[5] * cam.t[1] + cam.R[8] * cam.t[2]);
        g.rows = rows[i];
        g.cols = cols[i];
        views[i].depth = depths[i];
        views[i].normal = normals[i];
    }
    for (long long k = 0; k < n; ++k) {
        const int v = view[k];
        uint32_t kept;
        int used;
        apd_fusion::mean_point(views.data(), pair_indices + pair_offsets[v], pair_offsets[v + 1] - pair_offsets[v], xyz + 3 * k, normal + 3 * k,
                               sources[k], out_xyz + 3 * k, out_normal + 3 * k, kept, used);
        out_sources[k] = kept;
        out_support[k] = (uint8_t)used;
    }
}
