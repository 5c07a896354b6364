// filter_ref.cpp -- the geometric filter (apd_filter_views, apd-mvs_amd/csrc/apd_filter.hip) as a plain sequential loop over its
// definition (include/apd_mi355x.h): views, pixels and sources in order, nothing consumed.
//
// TEST INFRASTRUCTURE ONLY.  Compiled by tests/filter_checker.py.  From the product it takes the arithmetic contract only
// (apd_fusion_math.h: lift, vote_target, vote_check, accept_point).
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

struct Rule {  // the literals of APD.cpp:941-951, in the order of apd_fusion_options
    float max_reproj_error, max_relative_depth, max_angle, depth_weight, angle_weight;
    int min_consistent;
    float factor_strong, factor_weak;
};

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

}  // namespace

// blocks or blocks[i] may be null; so may each of the three output tables and each of their entries
extern "C" void filter_views_ref(const Rule *rule, int num_views, const Camera *cameras, const float *const *depths, const float *const *normals,
                                 const uint8_t *const *weaks, const uint8_t *const *blocks, const int *rows, const int *cols,
                                 const int *pair_offsets, const int *pair_indices, float *const *depth_out, uint8_t *const *votes_out,
                                 float *const *consistency_out)
{
    std::vector<apd_fusion::View> views;
    for (int i = 0; i < num_views; ++i) {
        views.push_back(view_of(cameras[i], rows[i], cols[i]));
    }
    for (int i = 0; i < num_views; ++i) {
        const apd_fusion::View &ref = views[i];
        for (int r = 0; r < ref.rows; ++r) {
            for (int c = 0; c < ref.cols; ++c) {
                const size_t p = (size_t)r * ref.cols + c;
                int votes = 0;
                float consistency = 0.0f, kept = 0.0f;
                const float depth = depths[i][p];
                const bool blocked = blocks && blocks[i] && blocks[i][p] < 128;
                if (!blocked && !(depth <= 0.0f)) {
                    float P[3];
                    apd_fusion::lift(ref, c, r, depth, P);
                    for (int k = pair_offsets[i]; k < pair_offsets[i + 1]; ++k) {
                        const int j = pair_indices[k];
                        int sc, sr;
                        if (!apd_fusion::vote_target(views[j], P, sc, sr)) {
                            continue;
                        }
                        const size_t s = (size_t)sr * views[j].cols + sc;
                        if (!(depths[j][s] > 0.0f)) {
                            continue;
                        }
                        float weight;
                        if (apd_fusion::vote_check(ref, views[j], c, r, depth, normals[i] + 3 * p, sc, sr, depths[j][s], normals[j] + 3 * s,
                                                   rule->max_reproj_error, rule->max_relative_depth, rule->max_angle, rule->depth_weight,
                                                   rule->angle_weight, weight)) {
                            votes += 1;
                            consistency += weight;
                        }
                    }
                    if (apd_fusion::accept_point(votes, consistency, weaks[i][p], rule->min_consistent, rule->factor_strong, rule->factor_weak)) {
                        kept = depth;
                    }
                }
                if (depth_out && depth_out[i]) {
                    depth_out[i][p] = kept;
                }
                if (votes_out && votes_out[i]) {
                    votes_out[i][p] = (uint8_t)votes;
                }
                if (consistency_out && consistency_out[i]) {
                    consistency_out[i][p] = consistency;
                }
            }
        }
    }
}
