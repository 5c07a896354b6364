/*
 * frame_limits_driver.c -- runs the CPU oracle alone over the tiny frames of tests/test_gpu_frame_limits.py.
 *
 * TEST INFRASTRUCTURE ONLY (see apd_oracle.h).  Bit equality between the HIP path and the oracle means nothing at a shape
 * where the oracle itself reads outside its arrays, so this program is built together with apd_oracle.c under
 * -fsanitize=address,undefined (Makefile target `frame_limits_asan`, host code only) and drives orc_run through the three
 * pass kinds -- FIRST_INIT, REFINE_INIT + APD, REFINE_ITER + APD + geometric term -- at every tiny shape, with 8-bit and
 * with non-integer images.  The prior of a pass is the post-processed result of the one before (main.cpp:105-115) with
 * the weak map replaced by a crafted one (central half-by-half block WEAK, the rest STRONG, one UNKNOWN pixel), so that
 * K3, K4, K9 and K10 have pixels to visit on frames K14 leaves all UNKNOWN.
 *
 * Images and cameras are procedural: a fronto-parallel ring of pinhole cameras with f = 0.9 W looking down +Z and an
 * integer hash texture.  Exit status 0 and no sanitizer report == the oracle is well defined at these shapes.
 *
 * Usage: frame_limits_asan            every shape of the table below
 *        frame_limits_asan W H N F    one shape, N sources, F = 1 for non-integer images
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "apd_oracle.h"

static const int kShapes[][2] = {{1, 1},  {2, 2},  {1, 40},  {40, 1},  {3, 5},   {5, 7},   {7, 8},   {8, 9},  {11, 11},
                                 {12, 10}, {16, 4}, {64, 5}, {5, 64}, {65, 9}, {24, 20}, {31, 32}, {33, 17}};

static uint32_t hash2(uint32_t x, uint32_t y, uint32_t k)
{
    uint32_t h = x * 0x9E3779B1u ^ (y + 0x7F4A7C15u) * 0x85EBCA77u ^ (k + 1u) * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

static void fill_camera(orc_camera *cam, int W, int H, int k)
{
    memset(cam, 0, sizeof(*cam));
    const float f = 0.9f * (float)W;
    cam->K[0] = f;
    cam->K[2] = 0.5f * (float)W;
    cam->K[4] = f;
    cam->K[5] = 0.5f * (float)H;
    cam->K[8] = 1.0f;
    cam->R[0] = cam->R[4] = cam->R[8] = 1.0f;
    const float rad = k == 0 ? 0.0f : 0.06f * (float)(1 + k % 3);
    const float ang = 2.399963f * (float)k;
    cam->c[0] = rad * cosf(ang);
    cam->c[1] = rad * sinf(ang);
    cam->c[2] = 0.0f;
    for (int j = 0; j < 3; ++j) {
        cam->t[j] = -cam->c[j]; /* R = I */
    }
    cam->width = W;
    cam->height = H;
    cam->depth_min = 1.0f;
    cam->depth_max = 4.0f;
}

static void fill_image(float *img, int W, int H, int k, int non_integer)
{
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            /* a smooth ramp shifted per view (so that views correlate) plus hash noise, 0..255 */
            const int v = (int)((uint32_t)(x * 23 + y * 37 + k * 5) % 200u) + (int)(hash2((uint32_t)x, (uint32_t)y, (uint32_t)k) % 56u);
            img[(size_t)y * W + x] = non_integer ? 0.731f * (float)v + 1.5f : (float)v;
        }
    }
}

static void fill_depth(float *d, int W, int H, int k)
{
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            float v = 2.2f + 0.1f * sinf(0.05f * (float)x + (float)k) + 0.05f * cosf(0.07f * (float)y);
            if (x % 17 == 0 && y % 13 == 0) {
                v = 0.0f;
            }
            d[(size_t)y * W + x] = v;
        }
    }
}

static int run_shape(int W, int H, int N, int non_integer)
{
    const size_t n = (size_t)W * H;
    const int views = N + 1;
    orc_camera cams[ORC_MAX_IMAGES];
    float *images[ORC_MAX_IMAGES], *depths[ORC_MAX_IMAGES];
    for (int k = 0; k < views; ++k) {
        fill_camera(&cams[k], W, H, k);
        images[k] = (float *)malloc(n * sizeof(float));
        depths[k] = (float *)malloc(n * sizeof(float));
        fill_image(images[k], W, H, k, non_integer);
        fill_depth(depths[k], W, H, k);
    }
    float *prior_planes = (float *)malloc(4 * n * sizeof(float));
    uint32_t *prior_views = (uint32_t *)malloc(n * sizeof(uint32_t));
    uint8_t *prior_weak = (uint8_t *)malloc(n);
    int weak_in = 0;
    for (int pass = 0; pass < 3; ++pass) {
        orc_params p;
        memset(&p, 0, sizeof(p));
        p.max_iterations = 2;
        p.num_images = views;
        p.top_k = 4;
        p.depth_min = 0.6f;
        p.depth_max = 4.8f;
        p.strong_radius = 5;
        p.strong_increment = 2;
        p.weak_radius = 5;
        p.weak_increment = 5;
        p.geom_factor = 0.2f;
        p.seed = 7;
        p.state = pass;
        p.use_APD = pass > 0;
        p.weak_peak_radius = pass == 2 ? 4 : 6;
        p.rotate_time = pass == 1 ? 2 : 4;
        p.ransac_threshold = pass == 1 ? 0.00875f : pass == 2 ? 0.0075f : 0.005f;
        p.geom_consistency = pass == 2;
        orc_state *s = orc_create(W, H, &p, cams, (const float *const *)images, pass == 2 ? (const float *const *)depths : NULL,
                                  pass ? prior_planes : NULL, pass ? prior_views : NULL, pass ? prior_weak : NULL);
        if (!s) {
            fprintf(stderr, "orc_create failed at %dx%d N=%d pass %d\n", W, H, N, pass);
            return 1;
        }
        if (pass && orc_weak_count(s) != weak_in) {
            fprintf(stderr, "weak_count %d != %d at %dx%d\n", orc_weak_count(s), weak_in, W, H);
            return 1;
        }
        orc_run(s);
        /* ProcessProblem post-processing (main.cpp:105-115), then the crafted weak map */
        memcpy(prior_planes, orc_planes(s), 4 * n * sizeof(float));
        memcpy(prior_views, orc_selected_views(s), n * sizeof(uint32_t));
        for (size_t c = 0; c < n; ++c) {
            const float d = prior_planes[4 * c + 3];
            if (d < p.depth_min || d > p.depth_max) {
                prior_planes[4 * c + 3] = 0.0f;
            }
        }
        weak_in = 0;
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x) {
                const int in_block = x >= W / 4 && x < W / 4 + W / 2 && y >= H / 4 && y < H / 4 + H / 2;
                prior_weak[(size_t)y * W + x] = in_block ? ORC_WEAK : ORC_STRONG;
                weak_in += in_block;
            }
        }
        if (W >= 3 && H >= 3) {
            prior_weak[n - 1] = ORC_UNKNOWN; /* the last pixel is outside the block */
        }
        orc_destroy(s);
    }
    for (int k = 0; k < views; ++k) {
        free(images[k]);
        free(depths[k]);
    }
    free(prior_planes);
    free(prior_views);
    free(prior_weak);
    return 0;
}

int main(int argc, char **argv)
{
    orc_set_threads(2);
    if (argc == 5) {
        return run_shape(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    }
    int runs = 0;
    for (size_t i = 0; i < sizeof(kShapes) / sizeof(kShapes[0]); ++i) {
        const int W = kShapes[i][0], H = kShapes[i][1];
        for (int non_integer = 0; non_integer < 2; ++non_integer) {
            if (run_shape(W, H, 2, non_integer)) {
                return 1;
            }
            ++runs;
            if (W == 24 && H == 20) { /* the wider view-count instantiations */
                if (run_shape(W, H, 17, non_integer)) {
                    return 1;
                }
                ++runs;
            }
        }
    }
    printf("frame_limits_driver: %d runs of three passes, no report\n", runs);
    return 0;
}
