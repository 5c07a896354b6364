// points_host_main.cpp -- host-resident points through their whole life, with its own main: apd_points_create, the accessors,
// apd_points_visibility, apd_points_write_ply, apd_points_write_vis, apd_points_destroy, and every refusal of apd_points_create.
// No device is touched.  Not a test of the suite: built by hand against the points sources with the host sanitizers and run,
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Wno-unused-value -Xarch_host -fsanitize=address,undefined -I apd-mvs_amd/_build
//         tests/helpers/points_host_main.cpp apd-mvs_amd/csrc/apd_points.hip apd-mvs_amd/csrc/apd_points_vis.hip
//         apd-mvs_amd/csrc/apd_fusion_call.hip -o points_host_main && ./points_host_main <directory for the files>
// to check the ownership of the host arrays on every path (exit status 0 and no sanitizer report).
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/apd_mi355x.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%s)\n", what, apd_fusion_last_error());
        ++failures;
    }
}

// `count` valid points over three views of 4 x 5 pixels with two sources each
struct Cloud {
    long long count;
    std::vector<float> xyz, normal;
    std::vector<uint8_t> bgr, support;
    std::vector<int32_t> view, pixel;
    std::vector<uint32_t> sources;
    int num_views = 3;
    std::vector<int> rows{4, 4, 4}, cols{5, 5, 5}, pair_offsets{0, 2, 4, 6}, pair_indices{1, 2, 2, 0, 0, 1};

    explicit Cloud(long long n) : count(n), xyz(3 * n), normal(3 * n), bgr(3 * n), support(n), view(n), pixel(n), sources(n)
    {
        for (long long k = 0; k < n; ++k) {
            for (int a = 0; a < 3; ++a) {
                xyz[3 * k + a] = 0.5f * (float)(3 * k + a);
                normal[3 * k + a] = a == 2 ? 1.0f : 0.0f;
                bgr[3 * k + a] = (uint8_t)(7 * k + a);
            }
            view[k] = (int32_t)(k % 3);
            pixel[k] = (int32_t)(k % 20);
            sources[k] = (uint32_t)(k % 4);
            support[k] = (uint8_t)__builtin_popcount(sources[k]);
        }
    }

    int create(apd_points_t *out) const
    {
        return apd_points_create(0, 0, count, xyz.data(), normal.data(), bgr.data(), support.data(), view.data(), pixel.data(), sources.data(),
                                 num_views, rows.data(), cols.data(), pair_offsets.data(), pair_indices.data(), out);
    }
};

void life(long long n, const std::string &dir)
{
    const Cloud c(n);
    apd_points_t p = nullptr;
    expect(c.create(&p) == APD_OK && p, "create");
    if (!p) {
        return;
    }
    expect(apd_points_count(p) == n && !apd_points_on_device(p), "count");
    if (n > 0) {
        expect(memcmp(apd_points_xyz(p), c.xyz.data(), 12 * n) == 0 && memcmp(apd_points_normal(p), c.normal.data(), 12 * n) == 0 &&
                   memcmp(apd_points_bgr(p), c.bgr.data(), 3 * n) == 0 && memcmp(apd_points_support(p), c.support.data(), n) == 0 &&
                   memcmp(apd_points_view(p), c.view.data(), 4 * n) == 0 && memcmp(apd_points_pixel(p), c.pixel.data(), 4 * n) == 0 &&
                   memcmp(apd_points_sources(p), c.sources.data(), 4 * n) == 0,
               "accessors");
    }
    const long long *offsets = nullptr;
    const int32_t *views = nullptr;
    expect(apd_points_visibility(p, &offsets, &views) == APD_OK, "visibility");
    long long entries = 0;
    for (long long k = 0; k < n; ++k) {
        expect(offsets[k] == entries && views[entries] == c.view[k], "list head");
        entries += 1 + c.support[k];
    }
    expect(offsets[n] == entries, "list total");
    for (int normals = 0; normals < 2; ++normals) {
        expect(apd_points_write_ply(p, (dir + "/points.ply").c_str(), normals) == APD_OK, "write_ply");
    }
    expect(apd_points_write_vis(p, (dir + "/points.ply.vis").c_str()) == APD_OK, "write_vis");
    expect(apd_points_write_ply(p, (dir + "/no/such/dir/points.ply").c_str(), 0) == APD_ERR_IO, "write_ply to nowhere");
    expect(apd_points_write_vis(p, (dir + "/no/such/dir/points.vis").c_str()) == APD_ERR_IO, "write_vis to nowhere");
    expect(apd_points_destroy(p) == APD_OK, "destroy");
}

void refusal(const char *what, const std::function<void(Cloud &)> &change)
{
    Cloud c(4);
    change(c);
    apd_points_t p = nullptr;
    expect(c.create(&p) == APD_ERR_INVALID && !p && strncmp(apd_fusion_last_error(), "apd_points_create: ", 19) == 0, what);
}

}  // namespace

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    for (long long n : {0LL, 1LL, 257LL, 70000LL}) {  // 70000: more than one chunk of the .vis writer
        life(n, dir);
    }
    refusal("negative count", [](Cloud &c) { c.count = -1; });
    refusal("no views", [](Cloud &c) { c.num_views = 0; });
    refusal("zero rows", [](Cloud &c) { c.rows[1] = 0; });
    refusal("negative cols", [](Cloud &c) { c.cols[2] = -5; });
    refusal("too many pixels", [](Cloud &c) { c.rows[0] = c.cols[0] = 50000; });
    refusal("offsets not from 0", [](Cloud &c) { c.pair_offsets[0] = 1; });
    refusal("offsets descend", [](Cloud &c) { c.pair_offsets[2] = 1; });
    refusal("index too large", [](Cloud &c) { c.pair_indices[4] = 3; });
    refusal("index negative", [](Cloud &c) { c.pair_indices[0] = -1; });
    refusal("own source", [](Cloud &c) { c.pair_indices[2] = 1; });
    refusal("view outside", [](Cloud &c) { c.view[1] = 3; });
    refusal("view negative", [](Cloud &c) { c.view[0] = -1; });
    refusal("pixel outside", [](Cloud &c) { c.pixel[2] = 20; });
    refusal("pixel negative", [](Cloud &c) { c.pixel[3] = -1; });
    refusal("bit above the list", [](Cloud &c) { c.sources[2] = 4; });
    refusal("support", [](Cloud &c) { c.support[1] = 2; });
    {  // too long a source list: 34 views, view 0 lists the 33 others
        Cloud c(0);
        c.num_views = 34;
        c.rows.assign(34, 4);
        c.cols.assign(34, 5);
        c.pair_offsets.assign(35, 33);
        c.pair_offsets[0] = 0;
        c.pair_indices.clear();
        for (int i = 1; i < 34; ++i) {
            c.pair_indices.push_back(i);
        }
        apd_points_t p = nullptr;
        expect(c.create(&p) == APD_ERR_INVALID && !p, "33 sources");
    }
    {  // null arguments
        const Cloud c(4);
        apd_points_t p = nullptr;
        expect(apd_points_create(0, 0, 4, nullptr, c.normal.data(), c.bgr.data(), c.support.data(), c.view.data(), c.pixel.data(), c.sources.data(), 3,
                                 c.rows.data(), c.cols.data(), c.pair_offsets.data(), c.pair_indices.data(), &p) == APD_ERR_INVALID, "null xyz");
        expect(apd_points_create(0, 0, 4, c.xyz.data(), c.normal.data(), c.bgr.data(), c.support.data(), c.view.data(), c.pixel.data(), c.sources.data(), 3,
                                 c.rows.data(), c.cols.data(), c.pair_offsets.data(), nullptr, &p) == APD_ERR_INVALID, "null pair_indices");
        expect(apd_points_create(0, 0, 4, c.xyz.data(), c.normal.data(), c.bgr.data(), c.support.data(), c.view.data(), c.pixel.data(), c.sources.data(), 3,
                                 c.rows.data(), c.cols.data(), c.pair_offsets.data(), c.pair_indices.data(), nullptr) == APD_ERR_INVALID, "null out");
        expect(apd_points_destroy(nullptr) == APD_OK, "destroy of null");
    }
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
