// host_capi.cpp -- flat C entry points over the host-side file-format helpers, so the Python tests
// can exercise ReadBinMat / WriteBinMat / ReadCamera / image decode / resampling without a GPU.
#include <cstdio>
#include <cstring>

#include "APD.h"
#include "schedule.h"
#include "wavefront.h"
#include "../csrc/apd_fusion_math.h"

bool DecodeJpegGray(const uint8_t *data, size_t size, std::vector<uint8_t> &gray, int &width, int &height);

extern "C" {

// returns 0 on success; *type gets the OpenCV type code; data copied into `out` (cap bytes)
int apdhost_read_bin_mat(const char *p, int *rows, int *cols, int *type, void *out, size_t cap)
{
    Mat m;
    if (!ReadBinMat(path(p), m)) {
        return -1;
    }
    *rows = m.rows;
    *cols = m.cols;
    *type = m.type;
    const size_t n = m.step() * (size_t)m.rows;
    if (out && n <= cap) {
        memcpy(out, m.data(), n);
    }
    return 0;
}

int apdhost_write_bin_mat(const char *p, int rows, int cols, int type, const void *data)
{
    Mat m(rows, cols, type);
    memcpy(m.data(), data, m.step() * (size_t)rows);
    return WriteBinMat(path(p), m) ? 0 : -1;
}

int apdhost_read_camera(const char *p, apd_camera *cam)
{
    memset(cam, 0, sizeof(*cam));
    return ReadCamera(path(p), *cam) ? 0 : -1;
}

int apdhost_read_gray_image(const char *stem, int *rows, int *cols, float *out, size_t cap_floats)
{
    Mat m;
    if (!ReadGrayImage(path(stem), m)) {
        return -1;
    }
    *rows = m.rows;
    *cols = m.cols;
    if (out && (size_t)m.rows * m.cols <= cap_floats) {
        memcpy(out, m.data(), (size_t)m.rows * m.cols * sizeof(float));
    }
    return 0;
}

// colour read (blue, green, red floats per pixel); `out` holds rows*cols*3 floats
int apdhost_read_color_image(const char *stem, int *rows, int *cols, float *out, size_t cap_floats)
{
    Mat m;
    if (!ReadColorImage(path(stem), m)) {
        return -1;
    }
    *rows = m.rows;
    *cols = m.cols;
    if (out && (size_t)m.rows * m.cols * 3 <= cap_floats) {
        memcpy(out, m.data(), (size_t)m.rows * m.cols * 3 * sizeof(float));
    }
    return 0;
}

int apdhost_resize_linear(const float *src, int rows, int cols, float *dst, int new_rows, int new_cols)
{
    Mat s(rows, cols, MAT_32FC1), d;
    memcpy(s.data(), src, (size_t)rows * cols * sizeof(float));
    ResizeLinear(s, d, new_cols, new_rows);
    memcpy(dst, d.data(), (size_t)new_rows * new_cols * sizeof(float));
    return 0;
}

int apdhost_rescale_nearest_f32(const float *src, int rows, int cols, float *dst, int new_rows, int new_cols)
{
    Mat s(rows, cols, MAT_32FC1), d;
    memcpy(s.data(), src, (size_t)rows * cols * sizeof(float));
    d = s;
    RescaleMatToTargetSize<float>(s, d, new_cols, new_rows);
    memcpy(dst, d.data(), (size_t)new_rows * new_cols * sizeof(float));
    return 0;
}

const char *apdhost_format_index(int index)
{
    static thread_local std::string s;
    s = ToFormatIndex(index);
    return s.c_str();
}

// acos / exp kernels of the fusion arithmetic (csrc/apd_fusion_math.h, contract C9): which = 0 acos_c9, 1 exp_c9
void apdhost_fusion_math(const float *in, int n, int which, float *out)
{
    for (int i = 0; i < n; ++i) {
        out[i] = which == 0 ? apd_fusion::acos_c9(in[i]) : apd_fusion::exp_c9(in[i]);
    }
}

// The pass table of the reference driver (main.cpp:72-88, :168-215) as host/schedule.h builds it for both C++ schedulers: the one
// implementation; apd-mvs_amd/pipeline.py reads it from here.  Row k of `rows` (9 ints) = level, iteration, scale_size, state,
// geom_consistency, use_APD, weak_peak_radius, rotate_time, and ransac_threshold as the bit pattern of the float.
int apdhost_round_num(int width, int height) { return RoundNum(width, height); }

int apdhost_schedule(int round_num, int single_level, int *rows, int cap_rows)
{
    const std::vector<Pass> plan = BuildSchedule(round_num, single_level != 0);
    if (rows) {
        for (size_t k = 0; k < plan.size() && (int)k < cap_rows; ++k) {
            const Pass &p = plan[k];
            int *r = rows + 9 * k;
            r[0] = p.level;
            r[1] = p.iteration;
            r[2] = p.scale_size;
            r[3] = (int)p.state;
            r[4] = p.geom_consistency ? 1 : 0;
            r[5] = p.use_APD ? 1 : 0;
            r[6] = p.weak_peak_radius;
            r[7] = p.rotate_time;
            memcpy(&r[8], &p.ransac_threshold, sizeof(float));
        }
    }
    return (int)plan.size();
}

// The task queue of a wavefront level (host/wavefront.h), as the in-memory scheduler drives it.  iterations / geom: per pass of the
// level; view v's sources (reconstructed views only) are src_index[src_begin[v] .. src_begin[v + 1]); lanes_per_pass <= 0: the
// scheduler's own cap.  take: 0 with a task in *pass_index / *view, 1 wait, 2 every task is handed out.  finish: 1 when the task was
// the last of its pass.
void *apdhost_wavefront_create(int num_passes, const int *iterations, const int *geom, int num_views, const int *src_begin, const int *src_index,
                               int gauss_seidel, int lanes_per_pass)
{
    std::vector<WavefrontQueue::PassInfo> passes;
    for (int p = 0; p < num_passes; ++p) {
        passes.push_back({iterations[p], geom[p] != 0});
    }
    std::vector<std::vector<int>> sources(num_views);
    for (int v = 0; v < num_views; ++v) {
        sources[v].assign(src_index + src_begin[v], src_index + src_begin[v + 1]);
    }
    return new WavefrontQueue(std::move(passes), std::move(sources), gauss_seidel != 0, lanes_per_pass > 0 ? lanes_per_pass : APD_GS_LANES_PER_PASS);
}

int apdhost_wavefront_take(void *queue, int *pass_index, int *view) { return (int)static_cast<WavefrontQueue *>(queue)->Take(*pass_index, *view); }
void apdhost_wavefront_publish(void *queue, int pass_index, int view) { static_cast<WavefrontQueue *>(queue)->Publish(pass_index, view); }
int apdhost_wavefront_finish(void *queue, int pass_index, int view) { return static_cast<WavefrontQueue *>(queue)->Finish(pass_index, view) ? 1 : 0; }
int apdhost_wavefront_published(void *queue, int view) { return static_cast<WavefrontQueue *>(queue)->Published(view); }
int apdhost_wavefront_source_iteration(void *queue, int pass_index, int view, int source)
{
    return static_cast<WavefrontQueue *>(queue)->SourceIteration(pass_index, view, source);
}
int apdhost_wavefront_lanes_per_pass(void) { return APD_GS_LANES_PER_PASS; }
void apdhost_wavefront_destroy(void *queue) { delete static_cast<WavefrontQueue *>(queue); }

// The value of a --ply-* flag as the command line reads it (host/ply_options.h), into options that are at their defaults.  0: the
// value is good, and `fields` holds every option as a `name value` line, the floats as %.9g, the three file names last since they
// end their lines, and for --ply-align-planes its own three fields after them; 1: it is bad, and `message` holds what the command line is told; -1: no such flag takes a value.
int apdhost_parse_ply_option(const char *flag, const char *value, char *fields, size_t fields_cap, char *message, size_t message_cap)
{
    if (!FindPlyFlag(flag)) {
        return -1;
    }
    PlyOptions o;
    const std::string why = ParsePlyOption(flag, value, o);
    snprintf(message, message_cap, "%s", why.c_str());
    snprintf(fields, fields_cap,
             "vis %d\nmean %d\nvoxel %.9g\nstat_radius %.9g\nstat_k %u\nstat_ratio %.9g\nradius %.9g\nradius_min %u\ncomponent_radius %.9g\ncomponent_min %u\n"
             "smooth_radius %.9g\nsmooth_min %u\nsmooth_iterations %u\nnormals_radius %.9g\nnormals_min %u\nrender_splat %d\nrender_tolerance %.9g\n"
             "register_radius %.9g\nregister_distance %.9g\nregister_trials %u\nregister_seed %llu\nalign_radius %.9g\nalign_iterations %u\nalign_scale %d\n"
             "score_threshold %.9g\nregister_truth %s\nalign_truth %s\nscore_truth %s\n",
             o.vis, o.mean, o.voxel, o.stat_radius, o.stat_k, o.stat_ratio, o.radius, o.radius_min, o.component_radius, o.component_min, o.smooth_radius,
             o.smooth_min, o.smooth_iterations, o.normals_radius, o.normals_min, o.render_splat, o.render_tolerance, o.register_radius, o.register_distance,
             o.register_trials, o.register_seed, o.align_radius, o.align_iterations, o.align_scale, o.score_threshold, o.register_truth.c_str(),
             o.align_truth.c_str(), o.score_truth.c_str());
    if (std::string(flag) == "--ply-align-planes") {   // the fields of a flag are reported when it is the one asked for
        const size_t used = strlen(fields);
        snprintf(fields + used, fields_cap - used, "planes_radius %.9g\nplanes_iterations %u\nplanes_truth %s\n", o.planes_radius, o.planes_iterations,
                 o.planes_truth.c_str());
    }
    return why.empty() ? 0 : 1;
}

// HIP device of the fusion started by apdhost_fuse / RunFusion (default 0)
void apdhost_set_fusion_device(int device) { SetFusionDevice(device); }

// Fusion loop of apdhost_fuse / RunFusion: APD_FUSION_ETH (default), APD_FUSION_TAT_INTERMEDIATE, APD_FUSION_TAT_ADVANCED
void apdhost_set_fusion_variant(int variant) { SetFusionVariant(variant); }

// Options of apdhost_fuse / RunFusion (apd_fusion_options, `variant` included); nullptr: the defaults
void apdhost_set_fusion_options(const apd_fusion_options *options)
{
    apd_fusion_options o;
    apd_fusion_default_options(&o);
    SetFusionOptions(options ? *options : o);
}

}  // extern "C"
