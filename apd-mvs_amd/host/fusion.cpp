// fusion.cpp -- depth-map fusion of the drop-in host: what the reference's RunFusion (ETH variant, APD.cpp:826-977) or, after
// SetFusionVariant, RunFusion_TAT_Intermediate / RunFusion_TAT_advanced (APD.cpp:979-1296), and ExportPointCloud
// (APD.cpp:214-254) produce, i.e. <dense>/APD/APD.ply.
//
// The fusion itself runs on the GPU (apd_fuse_views_opt, csrc/apd_fusion.hip and csrc/apd_fusion_tat.hip); this file is the drop-in entry point
// RunFusion, which reads the maps the way the reference does and hands them over.  There is no host fallback: a failing
// device fusion ends the program like any other device error.  (The reference's sequential loop lives in
// oracle/fusion_oracle.cpp as the checker of the device fusion.)
//
// Outside the PatchMatch path proper.  Like the reference, the images are re-read in colour for the
// point colours (cv::imread(IMREAD_COLOR), APD.cpp:859; host/jpeg_gray.cpp decodes to the same BGR bytes as libjpeg).
#include <atomic>
#include <chrono>
#include <sstream>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <thread>
#include <unordered_map>

#include "APD.h"
#include "schedule.h"

namespace {

int g_fusion_device = 0;
int g_fusion_variant = APD_FUSION_ETH;  // which of the reference's loops (APD_FUSION_*, include/apd_mi355x.h)
PlyOptions g_ply;                       // SetFusionPly: the --ply-* flags (host/ply_options.h)

// SetFusionOptions; `variant` is g_fusion_variant's at the moment of the call
apd_fusion_options &fusion_options()
{
    static apd_fusion_options o = [] {
        apd_fusion_options d;
        apd_fusion_default_options(&d);
        return d;
    }();
    return o;
}

apd_fusion_options call_options()
{
    apd_fusion_options o = fusion_options();
    o.variant = g_fusion_variant;
    return o;
}

struct FusionView {
    Camera cam;
    Camera full;   // the camera at the size of the image, before it is scaled to the maps: what --ply-render-vis draws into
    Mat image;     // float 0..255: 3 channels (blue, green, red, cv::imread(IMREAD_COLOR), APD.cpp:859) or 1 (grey)
    Mat depth;     // float, <= 0: no estimate
    Mat normal;    // 3 x float, world frame
    Mat weak;      // uint8 PixelState
    Mat block;     // optional uint8 mask of <dense>/blocks (APD.cpp:849-853); empty = none
};

void rework_and_write(apd_points_t &points, int num_views, const apd_camera *cameras, const apd_camera *full_cameras, const float *const *depths,
                      const float *const *normals, const int *rows, const int *cols, int maps_on_device, const path &ply_path);

// Device fusion through the C ABI (host pointers).  options: nullptr = those of SetFusionOptions; ply_path may be null when
// points is not.  mean_path (PlyOptions::from_points; points must be given): the fusion writes no file, *points become the
// reworked points and their PLY goes to *mean_path (rework_and_write).
long long fuse_dispatch(std::vector<FusionView> &views, const std::vector<std::vector<int>> &sources, const char *ply_path,
                        const apd_fusion_options *options = nullptr, apd_points_t *points = nullptr, const path *mean_path = nullptr)
{
    const int V = (int)views.size();
    std::vector<apd_camera> cams(V), full(V);
    std::vector<const float *> imgs(V), deps(V), nors(V);
    std::vector<const uint8_t *> weaks(V), blocks(V, nullptr);
    bool any_block = false;
    std::vector<int> rows(V), cols(V), offs(V + 1, 0), idx;
    for (int i = 0; i < V; ++i) {
        cams[i] = views[i].cam;
        full[i] = views[i].full;
        imgs[i] = views[i].image.ptr<float>();
        deps[i] = views[i].depth.ptr<float>();
        nors[i] = views[i].normal.ptr<float>();
        weaks[i] = views[i].weak.empty() ? nullptr : views[i].weak.ptr<uint8_t>();
        if (!views[i].block.empty()) {
            blocks[i] = views[i].block.ptr<uint8_t>();
            any_block = true;
        }
        rows[i] = views[i].depth.rows;
        cols[i] = views[i].depth.cols;
        idx.insert(idx.end(), sources[i].begin(), sources[i].end());
        offs[i + 1] = (int)idx.size();
    }
    if (idx.empty()) {
        idx.push_back(0);
    }
    long long n = 0;
    const int channels = (V > 0 && views[0].image.type == MAT_32FC3) ? 3 : 1;
    const apd_fusion_options opt = options ? *options : call_options();
    const int st = apd_fuse_views_opt(&opt, g_fusion_device, V, cams.data(), imgs.data(), channels, deps.data(), nors.data(), weaks.data(),
                                      any_block ? blocks.data() : nullptr, rows.data(), cols.data(), offs.data(), idx.data(), 0,
                                      mean_path ? nullptr : ply_path, &n, points);
    if (st != APD_OK) {
        std::cerr << apd_fusion_last_error() << std::endl;
        return -1;
    }
    if (mean_path) {
        rework_and_write(*points, V, cams.data(), full.data(), deps.data(), nors.data(), rows.data(), cols.data(), 0, *mean_path);
    }
    return n;
}

}  // namespace

void SetFusionDevice(int device) { g_fusion_device = device; }

void SetFusionVariant(int variant) { g_fusion_variant = variant; }

void SetFusionPly(const PlyOptions &ply) { g_ply = ply; }

namespace {

// The cloud of a truth file of --ply-register, --ply-align, --ply-align-planes and --ply-score (apd_points_read_ply into host memory): read once when
// several name the same file
struct Truth {
    apd_points_t points = nullptr;
    std::string file;
    ~Truth() { apd_points_destroy(points); }  // leaves the message of a failed call as it is
    int read(const std::string &from)
    {
        if (points && file == from) {
            return APD_OK;
        }
        apd_points_destroy(points);
        points = nullptr;
        file = from;
        return apd_points_read_ply(from.c_str(), g_fusion_device, 0, &points);
    }
};

void write_lines_or_exit(const std::string &to, const std::string &lines)
{
    FILE *f = fopen(to.c_str(), "wb");
    const bool ok = f && fwrite(lines.data(), 1, lines.size(), f) == lines.size();
    if ((f && fclose(f) != 0) || !ok) {
        std::cerr << "cannot write " << to << std::endl;
        exit(EXIT_FAILURE);
    }
}

// What --ply-register, --ply-align, --ply-align-planes and --ply-score report: every figure once in the printed line and once as a `name value` line of
// the file beside APD.ply
struct Report {
    std::string line, lines;
    void add(const std::string &name, const char *format, ...)
    {
        char text[64];
        va_list value;
        va_start(value, format);
        vsnprintf(text, sizeof(text), format, value);
        va_end(value);
        line += " " + name + " " + text;
        lines += name + " " + text + "\n";
    }
    void real(const std::string &name, double v) { add(name, "%.17g", v); }  // the double, back to the bit
    void integer(const std::string &name, long long v) { add(name, "%lld", v); }
    // what apd_points_registration_t and apd_points_alignment_t begin with; the rotation row-major
    void transform(double scale, const double *rotation, const double *translation)
    {
        real("scale", scale);
        for (int e = 0; e < 9; ++e) {
            real("rotation" + std::to_string(e), rotation[e]);
        }
        for (int e = 0; e < 3; ++e) {
            real("translation" + std::to_string(e), translation[e]);
        }
    }
    void write(const std::string &to)   // ends the line whose lead-in the caller has printed
    {
        std::cout << ":" << line << std::endl;
        write_lines_or_exit(to, lines);
    }
};

// The end of a reworking step: with APD_OK the new points take the place of the old ones, which are released, and the step's line
// is due.  *was: how many the old ones were
bool took(int st, apd_points_t &points, apd_points_t fresh, long long *was = nullptr)
{
    if (st != APD_OK) {
        return false;
    }
    if (was) {
        *was = apd_points_count(points);
    }
    apd_points_destroy(points);
    points = fresh;
    return true;
}

// --ply-register: replaces the points by themselves moved onto the cloud of the truth file from any start (apd_points_register on
// the fusion's device with the defaults of its other options, apd_points_transformed by its answer): one line with every field, and
// the same as `name value` lines in <ply_path>.register
int register_beside(apd_points_t &points, Truth &truth, const path &ply_path)
{
    int st = truth.read(g_ply.register_truth);
    const apd_points_register_options options = {g_ply.register_trials, g_ply.register_seed, g_ply.register_distance, 0.9f, 5, 1, 0};
    apd_points_registration_t r;
    st = st != APD_OK ? st : apd_points_register(points, truth.points, g_ply.register_radius, nullptr, &options, &r);
    apd_points_t moved = nullptr;
    st = st != APD_OK ? st : apd_points_transformed(points, r.scale, r.rotation, r.translation, &moved);
    if (!took(st, points, moved)) {
        return st;
    }
    Report report;
    report.transform(r.scale, r.rotation, r.translation);
    report.integer("features_p", r.features_p);
    report.integer("features_q", r.features_q);
    report.integer("matches", r.matches);
    report.integer("trials_admitted", r.trials_admitted);
    report.integer("best_trial", r.best_trial);
    report.integer("inliers", r.inliers);
    report.integer("inliers_after", r.inliers_after);
    report.real("rms_after", r.rms_after);
    report.integer("stopped", r.stopped);
    std::cout << "Registered to " << g_ply.register_truth << " at " << g_ply.register_radius << " within " << g_ply.register_distance;
    report.write(ply_path.string() + ".register");
    return APD_OK;
}

// --ply-align: replaces the points by themselves moved onto the cloud of the truth file (apd_points_align on the fusion's device,
// apd_points_transformed by its answer): one line with every field, and the same as `name value` lines in <ply_path>.align
int align_beside(apd_points_t &points, Truth &truth, const path &ply_path)
{
    int st = truth.read(g_ply.align_truth);
    const apd_points_align_options options = {g_ply.align_iterations, 1e-6, g_ply.align_scale ? 1 : 0};
    apd_points_alignment_t a;
    st = st != APD_OK ? st : apd_points_align(points, truth.points, g_ply.align_radius, nullptr, &options, &a);
    apd_points_t moved = nullptr;
    st = st != APD_OK ? st : apd_points_transformed(points, a.scale, a.rotation, a.translation, &moved);
    if (!took(st, points, moved)) {
        return st;
    }
    Report report;
    report.transform(a.scale, a.rotation, a.translation);
    report.integer("matched_before", a.matched_before);
    report.integer("matched_after", a.matched_after);
    report.real("rms_before", a.rms_before);
    report.real("rms_after", a.rms_after);
    report.integer("steps", a.steps);
    report.integer("stopped", a.stopped);
    std::cout << "Aligned to " << g_ply.align_truth << " within " << g_ply.align_radius;
    report.write(ply_path.string() + ".align");
    return APD_OK;
}

// --ply-align-planes: replaces the points by themselves moved onto the tangent planes of the cloud of the truth file, whose stored
// normals are used as they are -- a file without nx ny nz has none that is usable, which gives APD_ALIGN_TOO_FEW and the identity
// (apd_points_align_planes on the fusion's device, apd_points_transformed by its answer): one line with every field, and the same
// as `name value` lines in <ply_path>.align_planes
int align_planes_beside(apd_points_t &points, Truth &truth, const path &ply_path)
{
    int st = truth.read(g_ply.planes_truth);
    const apd_points_align_planes_options options = {g_ply.planes_iterations, 1e-6};
    apd_points_plane_alignment_t a;
    st = st != APD_OK ? st : apd_points_align_planes(points, truth.points, g_ply.planes_radius, nullptr, &options, &a);
    apd_points_t moved = nullptr;
    st = st != APD_OK ? st : apd_points_transformed(points, a.scale, a.rotation, a.translation, &moved);
    if (!took(st, points, moved)) {
        return st;
    }
    Report report;
    report.transform(a.scale, a.rotation, a.translation);
    report.integer("matched_before", a.matched_before);
    report.integer("matched_after", a.matched_after);
    report.real("rms_before", a.rms_before);
    report.real("rms_after", a.rms_after);
    report.integer("steps", a.steps);
    report.integer("stopped", a.stopped);
    report.integer("planes_before", a.planes_before);
    report.integer("planes_after", a.planes_after);
    report.real("plane_rms_before", a.plane_rms_before);
    report.real("plane_rms_after", a.plane_rms_after);
    std::cout << "Aligned to planes of " << g_ply.planes_truth << " within " << g_ply.planes_radius;
    report.write(ply_path.string() + ".align_planes");
    return APD_OK;
}

// --ply-score: the points ply_path was written from against the cloud of the truth file (apd_points_score on the fusion's
// device): one line with the nine fields, and the same as `key value` lines in <ply_path>.score
int score_beside(apd_points_t points, Truth &truth, const path &ply_path)
{
    int st = truth.read(g_ply.score_truth);
    apd_points_score_t s;
    st = st != APD_OK ? st : apd_points_score(points, truth.points, g_ply.score_threshold, nullptr, &s);
    if (st != APD_OK) {
        return st;
    }
    Report report;
    report.integer("n_p", s.n_p);
    report.integer("n_q", s.n_q);
    report.integer("p_within", s.p_within);
    report.integer("q_within", s.q_within);
    report.real("precision", s.precision);
    report.real("recall", s.recall);
    report.real("fscore", s.fscore);
    report.real("mean_p", s.mean_p);
    report.real("mean_q", s.mean_q);
    std::cout << "Score against " << g_ply.score_truth << " at " << g_ply.score_threshold;
    report.write(ply_path.string() + ".score");
    return APD_OK;
}

// The --ply-* steps that are asked for (host/ply_options.h), in the order of their fields: each replaces the points of a fusion,
// which wrote no file, by what it makes of them and prints its figures -- the mean over the fusion's own cameras and maps, the
// rendering into full_cameras, the views' cameras at the size of their images.  Then writes ply_path from them
// (apd_points_write_ply) and, with --ply-score, scores the points the file was written from, which changes none of them.
void rework_and_write(apd_points_t &points, int num_views, const apd_camera *cameras, const apd_camera *full_cameras, const float *const *depths,
                      const float *const *normals, const int *rows, const int *cols, int maps_on_device, const path &ply_path)
{
    const PlyOptions &o = g_ply;
    int st = APD_OK;
    apd_points_t fresh = nullptr;
    long long was = 0, gone = 0;   // the points a step was given, and those it removed or changed
    if (o.mean) {
        st = apd_points_average(points, num_views, cameras, depths, normals, rows, cols, maps_on_device, &fresh);
        took(st, points, fresh);
    }
    if (st == APD_OK && o.voxel > 0.0f) {
        st = apd_points_merge_voxels(points, o.voxel, nullptr, &fresh, &gone);
        double ms_setup = 0, ms_kernels = 0;
        apd_fusion_last_timing(&ms_setup, &ms_kernels, nullptr);
        if (took(st, points, fresh, &was)) {
            std::cout << "Merged " << was << " points into " << apd_points_count(points) << " cells of size " << o.voxel << ", dropped " << gone << ": "
                      << (long long)(ms_setup + ms_kernels) << " ms (set-up " << (long long)ms_setup << ", kernels " << (long long)ms_kernels << ")" << std::endl;
        }
    }
    if (st == APD_OK && o.stat_radius > 0.0f) {
        double threshold = 0.0;
        st = apd_points_remove_statistical(points, o.stat_radius, nullptr, o.stat_k, o.stat_ratio, &fresh, &gone, &threshold);
        if (took(st, points, fresh, &was)) {
            std::cout << "Removed " << gone << " of " << was << " points whose mean distance to their " << o.stat_k << " nearest neighbours within "
                      << o.stat_radius << " is above " << threshold << std::endl;
        }
    }
    if (st == APD_OK && o.radius > 0.0f) {
        st = apd_points_remove_sparse(points, o.radius, nullptr, o.radius_min, &fresh, &gone);
        if (took(st, points, fresh, &was)) {
            std::cout << "Removed " << gone << " of " << was << " points with fewer than " << o.radius_min << " neighbours within " << o.radius << std::endl;
        }
    }
    if (st == APD_OK && o.component_radius > 0.0f) {
        long long components = 0;
        st = apd_points_remove_small_components(points, o.component_radius, nullptr, o.component_min, &fresh, &gone, &components);
        if (took(st, points, fresh, &was)) {
            std::cout << "Removed " << gone << " of " << was << " points in connected components of fewer than " << o.component_min << " points, of "
                      << components << " components within " << o.component_radius << std::endl;
        }
    }
    if (st == APD_OK && o.smooth_radius > 0.0f) {
        st = apd_points_with_smoothed_positions(points, o.smooth_radius, nullptr, o.smooth_min, o.smooth_iterations, &fresh, &gone);
        if (took(st, points, fresh, &was)) {
            std::cout << "Smoothed the positions of " << gone << " of " << was << " points with at least " << o.smooth_min << " neighbours within "
                      << o.smooth_radius << " in " << o.smooth_iterations << " iteration(s)" << std::endl;
        }
    }
    if (st == APD_OK && o.normals_radius > 0.0f) {
        st = apd_points_with_estimated_normals(points, o.normals_radius, nullptr, o.normals_min, &fresh, &gone);
        if (took(st, points, fresh, &was)) {
            std::cout << "Estimated the normals of " << gone << " of " << was << " points from at least " << o.normals_min << " neighbours within "
                      << o.normals_radius << std::endl;
        }
    }
    if (st == APD_OK && o.render_splat >= 0) {
        st = apd_points_rendered_visibility(points, num_views, full_cameras, o.render_splat, o.render_tolerance, &fresh, &gone);
        if (took(st, points, fresh, &was)) {
            std::cout << "Rendered the visibility of " << was << " points in " << num_views << " views with a splat of " << o.render_splat
                      << " and a tolerance of " << o.render_tolerance << ": " << gone << " points are seen by no view" << std::endl;
        }
    }
    Truth truth;
    if (st == APD_OK && !o.register_truth.empty()) {
        st = register_beside(points, truth, ply_path);
    }
    if (st == APD_OK && !o.align_truth.empty()) {
        st = align_beside(points, truth, ply_path);
    }
    if (st == APD_OK && !o.planes_truth.empty()) {
        st = align_planes_beside(points, truth, ply_path);
    }
    st = st != APD_OK ? st : apd_points_write_ply(points, ply_path.string().c_str(), fusion_options().ply_normals);
    std::string err = st != APD_OK ? apd_fusion_last_error() : "";
    if (st == APD_OK && !o.score_truth.empty() && (st = score_beside(points, truth, ply_path)) != APD_OK) {
        err = apd_fusion_last_error();
    }
    if (st != APD_OK) {
        apd_points_destroy(points);
        std::cerr << err << std::endl;
        exit(EXIT_FAILURE);
    }
}

// The end of both fusions: releases the points ply_path was written from (null: none were kept), after <ply_path>.vis has been written
// from them with --ply-vis
void write_vis_beside(const path &ply_path, apd_points_t points)
{
    const std::string vis_path = ply_path.string() + ".vis";
    if (!g_ply.vis) {
        apd_points_destroy(points);
        return;
    }
    const int st = apd_points_write_vis(points, vis_path.c_str());
    const std::string err = st != APD_OK ? apd_fusion_last_error() : "";
    apd_points_destroy(points);
    if (st != APD_OK) {
        std::cerr << err << std::endl;
        exit(EXIT_FAILURE);
    }
    std::cout << "Visibility lists in " << vis_path << std::endl;
}

}  // namespace

void SetFusionOptions(const apd_fusion_options &options)
{
    fusion_options() = options;
    g_fusion_variant = options.variant;
}

// Reads every view's final maps from <dense>/APD/<id>/ and fuses them into APD/APD.ply (APD.cpp:826-977).
void RunFusion(const path &dense_folder, const std::vector<Problem> &problems) { RunFusionWithMaps(dense_folder, problems, nullptr); }

// Inputs of the fusion besides the maps: colour image, camera, optional block mask of every view, resampled to the size of
// the maps when that differs from the image's (RescaleImageAndCamera, APD.cpp:729-750), and the sources of every view as view
// indices.  maps: host maps (RunFusionWithMaps) or nullptr with map_cols x map_rows > 0 (the maps are on the device) or
// nullptr with 0 x 0 (read the files).  for_filter: the inputs of the geometric filter (--filtered-maps) -- no colour image (its
// size is the grey image's, which the passes have decoded), the weak maps whatever the fusion variant, and no progress lines.
// with_weak: the weak maps whatever the fusion variant, beside the colour image (--mesh).
namespace {

// log: where the reference's progress lines go ("Reading image ...", "Fusing image ...", APD.cpp:855, :899); the prefetch worker
// collects them and RunFusionOnDevice prints them where the reference would, after the passes' own lines.
bool prepare_fusion_inputs(const path &dense_folder, const std::vector<Problem> &problems, const std::vector<FinalMaps> *maps, int map_cols,
                           int map_rows, std::vector<FusionView> &views, std::vector<std::vector<int>> &sources, unsigned threads = 0,
                           std::ostream *log = nullptr, bool for_filter = false, bool with_weak = false)
{
    std::ostringstream unheard;
    std::ostream &out = for_filter ? unheard : log ? *log : std::cout;
    const bool need_weak = for_filter || with_weak || g_fusion_variant == APD_FUSION_ETH;
    const bool on_device = !maps && map_cols > 0 && map_rows > 0;
    views.assign(problems.size(), FusionView());
    std::unordered_map<int, int> index_of_id;
    const path block_folder = dense_folder / path("blocks");
    const bool use_block = std::filesystem::exists(block_folder);  // APD.cpp:849-853
    for (size_t i = 0; i < problems.size(); ++i) {
        out << "Reading image " << std::setw(8) << std::setfill('0') << i << "..." << std::endl;
        index_of_id.emplace(problems[i].ref_image_id, (int)i);
    }
    // the views are independent here: decode, read and rescale them on several host threads
    std::vector<int> failed(problems.size(), 0);
    ParallelFor(problems.size(), [&](size_t i) {
        const Problem &problem = problems[i];
        FusionView &v = views[i];
        const path image_stem = dense_folder / path("images") / path(ToFormatIndex(problem.ref_image_id));
        if (!(for_filter ? ReadGrayImageShared(image_stem, v.image) : ReadColorImage(image_stem, v.image))) {
            failed[i] = 1;
            return;
        }
        memset(&v.cam, 0, sizeof(v.cam));
        ReadCamera(dense_folder / path("cams") / path(ToFormatIndex(problem.ref_image_id) + "_cam.txt"), v.cam);
        v.full = v.cam;
        v.full.width = v.image.cols;
        v.full.height = v.image.rows;
        int cols = map_cols, rows = map_rows;
        if (!on_device) {
            if (maps) {
                v.depth = (*maps)[i].depth;
                v.normal = (*maps)[i].normal;
                v.weak = (*maps)[i].weak.clone();  // resampled in place below
            } else {
                ReadBinMat(problem.result_folder / path("depths.dmb"), v.depth);
                ReadBinMat(problem.result_folder / path("normals.dmb"), v.normal);
                if (need_weak) {  // the T&T loops read depths and normals only (APD.cpp:1023-1024, :1190-1191)
                    ReadBinMat(problem.result_folder / path("weak.bin"), v.weak);
                }
            }
            if (v.depth.empty() || v.normal.empty() || (v.weak.empty() && need_weak)) {
                std::cerr << "Missing maps of view " << problem.ref_image_id << " in " << problem.result_folder << std::endl;
                failed[i] = 1;
                return;
            }
            cols = v.depth.cols;
            rows = v.depth.rows;
        }
        if (cols != v.image.cols || rows != v.image.rows) {  // RescaleImageAndCamera, APD.cpp:729-750
            const float scale_x = cols / static_cast<float>(v.image.cols);
            const float scale_y = rows / static_cast<float>(v.image.rows);
            v.cam.K[0] *= scale_x;
            v.cam.K[2] *= scale_x;
            v.cam.K[4] *= scale_y;
            v.cam.K[5] *= scale_y;
        }
        if (for_filter) {
            v.image = Mat();  // the cache's matrix: looked at for its size only
        } else if (cols != v.image.cols || rows != v.image.rows) {
            // the reference resizes the 8-bit colour image: each channel resampled, then rounded back to 8 bit
            const size_t n_in = (size_t)v.image.rows * v.image.cols, n_out = (size_t)rows * cols;
            Mat out(rows, cols, MAT_32FC3), plane(v.image.rows, v.image.cols, MAT_32FC1), scaled;
            for (int ch = 0; ch < 3; ++ch) {
                for (size_t k = 0; k < n_in; ++k) {
                    plane.ptr<float>()[k] = v.image.ptr<float>()[3 * k + ch];
                }
                ResizeLinear(plane, scaled, cols, rows);
                for (size_t k = 0; k < n_out; ++k) {
                    out.ptr<float>()[3 * k + ch] = std::nearbyint(scaled.ptr<float>()[k]);
                }
            }
            v.image = out;
        }
        v.cam.width = cols;
        v.cam.height = rows;
        if (!on_device && !v.weak.empty()) {  // device maps: the weak map already has the size of the depth map
            RescaleMatToTargetSize<uint8_t>(v.weak, v.weak, cols, rows);
        }
        if (use_block) {  // blocks/mask_<id>.jpg, read as grey (APD.cpp:871-875); must have the size of the depth map
            Mat grey;
            if (ReadGrayImage(block_folder / path("mask_" + std::to_string(problem.ref_image_id)), grey) && grey.rows == rows && grey.cols == cols) {
                v.block.create(grey.rows, grey.cols, MAT_8UC1);
                for (size_t k = 0; k < (size_t)grey.rows * grey.cols; ++k) {
                    v.block.ptr<uint8_t>()[k] = (uint8_t)grey.ptr<float>()[k];
                }
            }
        }
    }, threads);
    for (int f : failed) {
        if (f) {
            return false;
        }
    }
    sources.assign(problems.size(), std::vector<int>());
    for (size_t i = 0; i < problems.size(); ++i) {
        out << "Fusing image " << std::setw(8) << std::setfill('0') << i << "..." << std::endl;
        for (int id : problems[i].src_image_ids) {
            // A source without a problem of its own has no maps to check against and is skipped.  (The reference's
            // imageIdToindexMap[id] default-inserts 0 for it, APD.cpp:919, i.e. silently checks against view 0 instead.)
            const auto it = index_of_id.find(id);
            if (it != index_of_id.end()) {
                sources[i].push_back(it->second);
            }
        }
    }
    return true;
}

}  // namespace

// The same with the final maps already in memory (maps[i] belongs to problems[i]; nullptr reads the files).
void RunFusionWithMaps(const path &dense_folder, const std::vector<Problem> &problems, const std::vector<FinalMaps> *maps)
{
    const auto t_inputs = std::chrono::steady_clock::now();
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    if (!prepare_fusion_inputs(dense_folder, problems, maps, 0, 0, views, sources)) {
        exit(EXIT_FAILURE);
    }
    const path ply_path = dense_folder / path("APD") / path("APD.ply");
    const auto t_fuse = std::chrono::steady_clock::now();
    std::cout << "Fusion inputs ready: " << std::chrono::duration_cast<std::chrono::milliseconds>(t_fuse - t_inputs).count() << " ms" << std::endl;
    apd_points_t points = nullptr;
    const long long n = fuse_dispatch(views, sources, ply_path.string().c_str(), nullptr, g_ply.vis || g_ply.from_points() ? &points : nullptr,
                                      g_ply.from_points() ? &ply_path : nullptr);
    std::cout << "Fusion + PLY: " << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_fuse).count() << " ms" << std::endl;
    if (n < 0) {
        exit(EXIT_FAILURE);  // like every other device error of the reference (CudaSafeCall, APD.cpp:315-323)
    }
    std::cout << "Fused " << n << " points into " << ply_path << std::endl;
    write_vis_beside(ply_path, points);
}

// The final maps are on `device` already (host/multi_device.cpp keeps every view's state there and gathers the other devices'
// into it): only the colour images (and block masks) go up; nothing comes down but the points.  The inputs that do not depend
// on the passes -- colour decode (cv::imread(IMREAD_COLOR), APD.cpp:859), cameras, masks, their upload -- are prepared on a
// background thread WHILE the passes run (StartFusionInputs right after the grey images are loaded): at 152 views of 1920 x 1080
// they take 4 s, as long as half of an 8-device run's passes.
struct FusionPrefetch {
    std::thread worker;
    path dense_folder;
    std::vector<Problem> problems;
    int device = 0, cols = 0, rows = 0;
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    std::vector<void *> owned;
    std::vector<const float *> imgs;
    std::vector<const uint8_t *> blocks;
    bool any_block = false, ok = false;
    std::atomic<bool> failed{false};  // set by the worker as soon as it gives up: RunMultiDevice polls it between levels (FusionInputsFailed)
    int channels = 3;
    long long prepare_ms = 0;
    std::string error;
    std::ostringstream log;           // the reference's progress lines, printed by RunFusionOnDevice
};

FusionPrefetch *StartFusionInputs(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows, unsigned threads)
{
    FusionPrefetch *f = new FusionPrefetch();
    f->dense_folder = dense_folder;
    f->problems = problems;
    f->device = device;
    f->cols = cols;
    f->rows = rows;
    f->worker = std::thread([f, threads]() {
        const auto t0 = std::chrono::steady_clock::now();
        // every way out of this worker releases the upload stream and the staging buffer, and a failure is published at once
        void *stream = nullptr, *staging = nullptr;
        struct Guard {
            FusionPrefetch *f;
            void *&stream, *&staging;
            ~Guard()
            {
                if (stream) {
                    apd_stream_destroy(f->device, stream);
                }
                if (staging) {
                    apd_host_free(staging);
                }
                if (!f->ok) {
                    f->failed.store(true);
                }
            }
        } guard{f, stream, staging};
        if (!prepare_fusion_inputs(f->dense_folder, f->problems, nullptr, f->cols, f->rows, f->views, f->sources, threads, &f->log)) {
            f->error = "fusion inputs could not be read";
            return;
        }
        const int V = (int)f->views.size();
        const size_t n = (size_t)f->rows * f->cols;
        f->channels = (V > 0 && f->views[0].image.type == MAT_32FC3) ? 3 : 1;
        f->imgs.assign(V, nullptr);
        f->blocks.assign(V, nullptr);
        auto upload = [&](const void *host, size_t bytes) -> void * {
            void *p = nullptr;
            if (apd_device_malloc(f->device, bytes, &p) != APD_OK) {
                f->error = std::string("fusion: device allocation failed: ") + apd_exchange_last_error();
                return nullptr;
            }
            f->owned.push_back(p);
            if (apd_device_memcpy(f->device, p, host, bytes) != APD_OK) {
                f->error = std::string("fusion: device upload failed: ") + apd_exchange_last_error();
                return nullptr;
            }
            return p;
        };
        // one allocation for every view's colour image: device allocations are not free while other threads launch kernels
        const size_t image_bytes = n * 4 * (size_t)f->channels;
        void *all_images = nullptr;
        if (apd_device_malloc(f->device, image_bytes * (size_t)std::max(V, 1), &all_images) != APD_OK) {
            f->error = std::string("fusion: device allocation failed: ") + apd_exchange_last_error();
            return;
        }
        f->owned.push_back(all_images);
        // Uploads on a stream of their own through ONE page-locked staging buffer.  Measured on 24 views of 1920 x 1080 with the
        // passes running beside it: a plain hipMemcpy of the pageable image, and just as much hipHostRegister + asynchronous copy +
        // unregister per image, cost the passes what the early start saved (8.2 -> 8.6 s): every map / unmap of host pages holds
        // the device's queues up; one mapping for the whole run does not.
        if (apd_stream_create(f->device, &stream) != APD_OK) {
            stream = nullptr;
        } else if (apd_host_alloc(image_bytes, &staging) != APD_OK) {
            staging = nullptr;
        }
        for (int i = 0; i < V; ++i) {
            void *dst = (char *)all_images + (size_t)i * image_bytes;
            const void *src = f->views[i].image.data();
            int rc;
            if (stream && staging) {
                memcpy(staging, src, image_bytes);
                rc = apd_device_memcpy_async(f->device, stream, dst, staging, image_bytes);
                rc = rc != APD_OK ? rc : apd_stream_synchronize(f->device, stream);
            } else {
                rc = apd_device_memcpy(f->device, dst, src, image_bytes);
            }
            if (rc != APD_OK) {
                f->error = std::string("fusion: device upload failed: ") + apd_exchange_last_error();
                return;
            }
            f->imgs[i] = (const float *)dst;
            f->views[i].image = Mat();  // the host copy is done with
            if (!f->views[i].block.empty()) {
                f->blocks[i] = (const uint8_t *)upload(f->views[i].block.data(), n);
                if (!f->blocks[i]) {
                    return;
                }
                f->any_block = true;
            }
        }
        f->prepare_ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        f->ok = true;
    });
    return f;
}

// true as soon as the prefetch worker has given up (unreadable colour image, device out of memory): the caller stops before the
// next level instead of learning it after every pass has run
bool FusionInputsFailed(const FusionPrefetch *f, std::string *why)
{
    if (!f || !f->failed.load()) {
        return false;
    }
    if (why) {
        *why = f->error;   // written before the flag was set
    }
    return true;
}

void CancelFusionInputs(FusionPrefetch *f)
{
    if (!f) {
        return;
    }
    if (f->worker.joinable()) {
        f->worker.join();
    }
    for (void *p : f->owned) {
        apd_device_free(f->device, p);
    }
    delete f;
}

void RunFusionOnDevice(FusionPrefetch *f, const std::vector<const float *> &depths, const std::vector<const float *> &normals,
                       const std::vector<const uint8_t *> &weaks)
{
    const auto t_wait = std::chrono::steady_clock::now();
    f->worker.join();
    if (!f->ok) {
        std::cerr << f->error << std::endl;
        exit(EXIT_FAILURE);
    }
    const int V = (int)f->views.size();
    std::vector<apd_camera> cams(V), full(V);
    std::vector<int> rws(V, f->rows), cls(V, f->cols), offs(V + 1, 0), idx;
    for (int i = 0; i < V; ++i) {
        cams[i] = f->views[i].cam;
        full[i] = f->views[i].full;
        idx.insert(idx.end(), f->sources[i].begin(), f->sources[i].end());
        offs[i + 1] = (int)idx.size();
    }
    if (idx.empty()) {
        idx.push_back(0);
    }
    const path ply_path = f->dense_folder / path("APD") / path("APD.ply");
    const auto t_fuse = std::chrono::steady_clock::now();
    std::cout << f->log.str();   // "Reading image ..." / "Fusing image ...": here, where the reference prints them (after the passes)
    std::cout << "Fusion inputs ready: prepared in " << f->prepare_ms << " ms behind the passes, waited "
              << std::chrono::duration_cast<std::chrono::milliseconds>(t_fuse - t_wait).count() << " ms" << std::endl;
    long long count = 0;
    apd_fusion_options fusion = call_options();
    apd_points_t points = nullptr;
    const bool keep_points = g_ply.vis || g_ply.from_points();
    if (keep_points) {
        fusion.result_on_device = 1;  // the maps are here already: the lists and the means are built here too and only they come down
    }
    const int st = apd_fuse_views_opt(&fusion, f->device, V, cams.data(), f->imgs.data(), f->channels, depths.data(), normals.data(), weaks.data(),
                                      f->any_block ? f->blocks.data() : nullptr, rws.data(), cls.data(), offs.data(), idx.data(), 1,
                                      g_ply.from_points() ? nullptr : ply_path.string().c_str(), &count, keep_points ? &points : nullptr);
    double ms_setup = 0, ms_views = 0, ms_file = 0;
    apd_fusion_last_timing(&ms_setup, &ms_views, &ms_file);
    std::cout << "Fusion + PLY: " << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_fuse).count() << " ms (set-up "
              << (long long)ms_setup << ", views " << (long long)ms_views << ", file " << (long long)ms_file << ")" << std::endl;
    const std::string err = st != APD_OK ? apd_fusion_last_error() : "";
    CancelFusionInputs(f);
    if (st != APD_OK) {
        std::cerr << err << std::endl;
        exit(EXIT_FAILURE);
    }
    if (g_ply.from_points()) {
        rework_and_write(points, V, cams.data(), full.data(), depths.data(), normals.data(), rws.data(), cls.data(), 1, ply_path);
    }
    std::cout << "Fused " << count << " points into " << ply_path << std::endl;
    write_vis_beside(ply_path, points);
}

// ---- --filtered-maps: the geometric filter (apd_filter_views, csrc/apd_filter.hip) ----

namespace {

// The filter of --filtered-maps and --mesh on the views whose maps are given: the three outputs per view in host memory
struct Filtered {
    std::vector<Mat> depth, votes, consistency;
    std::vector<apd_camera> cams;
    double ms_setup = 0, ms_views = 0;
};

void filter_views(const std::vector<FusionView> &views, const std::vector<std::vector<int>> &sources, const float *const *depths,
                  const float *const *normals, const uint8_t *const *weaks, const uint8_t *const *blocks, int cols, int rows, int maps_on_device,
                  Filtered &out)
{
    const int V = (int)views.size();
    out.cams.resize(V);
    out.depth.resize(V);
    out.votes.resize(V);
    out.consistency.resize(V);
    std::vector<int> rws(V), cls(V), offs(V + 1, 0), idx;
    std::vector<float *> depth_out(V), consistency_out(V);
    std::vector<uint8_t *> votes_out(V);
    for (int i = 0; i < V; ++i) {
        out.cams[i] = views[i].cam;
        rws[i] = rows > 0 ? rows : views[i].depth.rows;
        cls[i] = cols > 0 ? cols : views[i].depth.cols;
        idx.insert(idx.end(), sources[i].begin(), sources[i].end());
        offs[i + 1] = (int)idx.size();
        out.depth[i].create(rws[i], cls[i], MAT_32FC1);
        out.votes[i].create(rws[i], cls[i], MAT_8UC1);
        out.consistency[i].create(rws[i], cls[i], MAT_32FC1);
        depth_out[i] = out.depth[i].ptr<float>();
        votes_out[i] = out.votes[i].ptr<uint8_t>();
        consistency_out[i] = out.consistency[i].ptr<float>();
    }
    if (idx.empty()) {
        idx.push_back(0);
    }
    apd_fusion_options rule = fusion_options();
    rule.variant = APD_FUSION_ETH;
    const int st = apd_filter_views(&rule, g_fusion_device, V, out.cams.data(), depths, normals, weaks, blocks, rws.data(), cls.data(), offs.data(),
                                    idx.data(), maps_on_device, depth_out.data(), votes_out.data(), consistency_out.data(), 0);
    if (st != APD_OK) {
        std::cerr << apd_fusion_last_error() << std::endl;
        exit(EXIT_FAILURE);
    }
    apd_fusion_last_timing(&out.ms_setup, &out.ms_views, nullptr);
}

// Filters the views whose maps are given (host pointers, or device pointers on the fusion device with maps_on_device; blocks may be
// null) and writes depths_filtered.dmb, consistency.dmb and votes.bin into every view's result folder.  The rule is the fusion's
// (--fusion-*); a Tanks and Temples variant has refused those flags, so the filter then runs the defaults.
void filter_and_write(const std::vector<Problem> &problems, const std::vector<FusionView> &views, const std::vector<std::vector<int>> &sources,
                      const float *const *depths, const float *const *normals, const uint8_t *const *weaks, const uint8_t *const *blocks,
                      int cols, int rows, int maps_on_device)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int V = (int)views.size();
    Filtered f;
    filter_views(views, sources, depths, normals, weaks, blocks, cols, rows, maps_on_device, f);
    for (int i = 0; i < V; ++i) {
        const path &folder = problems[i].result_folder;
        std::filesystem::create_directories(folder);
        const std::pair<const char *, const Mat *> files[3] = {{"depths_filtered.dmb", &f.depth[i]}, {"consistency.dmb", &f.consistency[i]}, {"votes.bin", &f.votes[i]}};
        for (const auto &file : files) {
            if (!WriteBinMat(folder / file.first, *file.second)) {
                std::cerr << "cannot write " << (folder / file.first).string() << std::endl;
                exit(EXIT_FAILURE);
            }
        }
    }
    std::cout << "Filtered maps of " << V << " views: " << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count()
              << " ms (set-up " << (long long)f.ms_setup << ", views " << (long long)f.ms_views << ")" << std::endl;
}

// --mesh: the filter, then the volume over the box of the finite points of ply_path grown by trunc -- origin = lo - trunc and per
// axis the fewest samples, at least 2, whose last one is at or past hi + trunc, in the arithmetic of the Python binding's
// Volume.around --, the filtered maps with the views' colour images (3 channels) into it, every view weighing 1, and the mesh
// into <ply_path>.mesh, after the steps of `clean` in their fixed order -- weld, trimming of unseen faces, small components, smoothing,
// simplification, normals --, each a new mesh that replaces the one before and a printed line with the counts before and after.  With
// clean.depth_maps the final mesh is rendered into every view and written as depths_mesh.dmb into its result folder.  A failure ends
// the program like every other device error.
void mesh_and_write(const path &ply_path, const std::vector<Problem> &problems, const std::vector<FusionView> &views, const std::vector<std::vector<int>> &sources, const float *const *depths,
                    const float *const *normals, const uint8_t *const *weaks, const uint8_t *const *blocks, int cols, int rows, int maps_on_device,
                    float voxel, float trunc, const MeshClean &clean)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int V = (int)views.size();
    Filtered f;
    filter_views(views, sources, depths, normals, weaks, blocks, cols, rows, maps_on_device, f);
    auto failed = [](const std::string &why) {
        std::cerr << why << std::endl;
        exit(EXIT_FAILURE);
    };
    apd_points_t cloud = nullptr;
    if (apd_points_read_ply(ply_path.string().c_str(), g_fusion_device, 0, &cloud) != APD_OK) {
        failed(apd_fusion_last_error());
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float *xyz = apd_points_xyz(cloud);
    for (long long k = 0; k < apd_points_count(cloud); ++k) {
        const float *P = xyz + 3 * k;
        if (std::isfinite(P[0]) && std::isfinite(P[1]) && std::isfinite(P[2])) {
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], P[a]);
                hi[a] = std::max(hi[a], P[a]);
            }
        }
    }
    apd_points_destroy(cloud);
    if (!(lo[0] <= hi[0])) {
        failed("--mesh: " + ply_path.string() + " holds no point with a finite position: no box to mesh in");
    }
    float origin[3];
    int dims[3];
    for (int a = 0; a < 3; ++a) {
        origin[a] = lo[a] - trunc;
        const float top = hi[a] + trunc;
        const float extent = top - origin[a];
        const double samples = std::ceil((double)extent / (double)voxel) + 1.0;
        if (!(samples < 2147483648.0)) {
            failed("--mesh: a voxel of " + std::to_string(voxel) + " gives too many samples in the box of " + ply_path.string());
        }
        dims[a] = std::max(2, (int)samples);
    }
    std::vector<const float *> filtered(V), images(V);
    for (int i = 0; i < V; ++i) {
        filtered[i] = f.depth[i].ptr<float>();
        images[i] = views[i].image.ptr<float>();
    }
    apd_volume_t volume = nullptr;
    apd_mesh_t mesh = nullptr;
    const std::string mesh_path = ply_path.string() + ".mesh";
    long long vertices = 0, faces = 0;
    // --mesh-recolour: the colours come from the images at the end, so the volume carries none and is integrated without them
    if (apd_volume_create(g_fusion_device, dims[0], dims[1], dims[2], origin, voxel, trunc, 64.0f, clean.recolour ? 0 : 1, &volume) != APD_OK ||
        apd_volume_integrate(volume, V, f.cams.data(), filtered.data(), clean.recolour ? nullptr : images.data(), 3, nullptr, 0) != APD_OK ||
        apd_volume_extract_mesh(volume, &mesh) != APD_OK || apd_mesh_counts(mesh, &vertices, &faces) != APD_OK) {
        failed(apd_fusion_last_error());
    }
    // one step of `clean`: `next` replaces the mesh, and a line tells what the step did to the counts
    auto replaced = [&](int rc, apd_mesh_t next, const std::string &what) {
        long long nv = 0, nf = 0;
        if (rc != APD_OK || apd_mesh_counts(next, &nv, &nf) != APD_OK) {
            failed(apd_fusion_last_error());
        }
        std::cout << "Mesh " << what << ": " << vertices << " vertices and " << faces << " faces -> " << nv << " vertices and " << nf << " faces" << std::endl;
        apd_mesh_destroy(mesh);
        mesh = next;
        vertices = nv;
        faces = nf;
    };
    if (clean.weld > 0.0f) {
        apd_mesh_t next = nullptr;
        const int rc = apd_mesh_weld(mesh, clean.weld, nullptr, &next, nullptr, nullptr);
        replaced(rc, next, "welded within " + std::to_string(clean.weld));
    }
    std::vector<apd_camera> cams = f.cams;  // the views at the size of their maps: what the mesh is trimmed by and rendered into
    for (int i = 0; i < V; ++i) {
        cams[i].width = f.depth[i].cols;
        cams[i].height = f.depth[i].rows;
    }
    if (clean.trim > 0) {
        apd_mesh_t next = nullptr;
        const int rc = apd_mesh_remove_unseen(mesh, V, cams.data(), APD_RENDER_CULL_BACK, clean.trim_pixels, clean.trim_tolerance, clean.trim, &next, nullptr,
                                              nullptr);
        replaced(rc, next, "without the faces that fewer than " + std::to_string(clean.trim) + " of " + std::to_string(V) + " views see");
    }
    if (clean.remove_small) {
        apd_mesh_t next = nullptr;
        long long components = 0;
        const int rc = apd_mesh_remove_small_components(mesh, clean.min_component, &next, nullptr, &components);
        replaced(rc, next, "without the components of fewer than " + std::to_string(clean.min_component) + " faces among " + std::to_string(components));
    }
    if (clean.smooth > 0) {
        apd_mesh_t next = nullptr;
        long long moved = 0;
        const int rc = apd_mesh_smooth(mesh, clean.smooth, clean.smooth_lambda, clean.smooth_mu, clean.smooth_boundary, &next, &moved);
        if (rc != APD_OK) {
            failed(apd_fusion_last_error());
        }
        static const char *const modes[3] = {"fixed", "along", "free"};
        printf("Mesh smoothed in %d iterations (lambda %f, mu %f, %s boundary): %lld of %lld vertices moved\n", clean.smooth, (double)clean.smooth_lambda,
               (double)clean.smooth_mu, modes[clean.smooth_boundary], moved, vertices);
        fflush(stdout);
        apd_mesh_destroy(mesh);
        mesh = next;
    }
    if (clean.simplify > 0.0f) {
        apd_mesh_t next = nullptr;
        const int rc = apd_mesh_simplify(mesh, clean.simplify, nullptr, clean.simplify_mean ? APD_SIMPLIFY_MEAN : APD_SIMPLIFY_QUADRIC, &next, nullptr, nullptr);
        replaced(rc, next, "simplified in cells of " + std::to_string(clean.simplify) + (clean.simplify_mean ? " (mean)" : " (quadric)"));
    }
    if (clean.normals) {
        apd_mesh_t next = nullptr;
        const int rc = apd_mesh_with_vertex_normals(mesh, &next);
        replaced(rc, next, "with vertex normals");
    }
    if (clean.recolour) {
        apd_mesh_t next = nullptr;
        long long uncoloured = 0;
        if (apd_mesh_colour_from_views(mesh, V, cams.data(), images.data(), 3, 0, clean.recolour_tolerance, clean.recolour_min_cos, &next, nullptr,
                                       &uncoloured) != APD_OK) {
            failed(apd_fusion_last_error());
        }
        printf("Mesh recoloured from %d views (tolerance %f, min_cos %f): %lld vertices, %lld left uncoloured\n", V, (double)clean.recolour_tolerance,
               (double)clean.recolour_min_cos, vertices, uncoloured);
        fflush(stdout);
        apd_mesh_destroy(mesh);
        mesh = next;
    }
    if (apd_mesh_write_ply(mesh, mesh_path.c_str()) != APD_OK) {
        failed(apd_fusion_last_error());
    }
    for (int i = 0; clean.depth_maps && i < V; ++i) {
        Mat rendered;
        rendered.create(cams[i].height, cams[i].width, MAT_32FC1);
        if (apd_mesh_render(mesh, &cams[i], APD_RENDER_CULL_NONE, rendered.ptr<float>(), nullptr) != APD_OK) {
            failed(apd_fusion_last_error());
        }
        const path file = problems[i].result_folder / "depths_mesh.dmb";
        std::filesystem::create_directories(problems[i].result_folder);
        if (!WriteBinMat(file, rendered)) {
            failed("cannot write " + file.string());
        }
    }
    if (!clean.score_truth.empty()) {   // --mesh-score: last, the file has its bytes
        Truth truth;
        apd_points_score_t s;
        if (truth.read(clean.score_truth) != APD_OK ||
            apd_mesh_score(mesh, truth.points, clean.score_threshold, nullptr, clean.score_density, clean.score_seed, &s) != APD_OK) {
            failed(apd_fusion_last_error());
        }
        Report report;
        report.integer("n_p", s.n_p);
        report.integer("n_q", s.n_q);
        report.integer("p_within", s.p_within);
        report.integer("q_within", s.q_within);
        report.real("precision", s.precision);
        report.real("recall", s.recall);
        report.real("fscore", s.fscore);
        report.real("mean_p", s.mean_p);
        report.real("mean_q", s.mean_q);
        std::cout << "Mesh score against " << clean.score_truth << " at " << clean.score_threshold;
        report.write(mesh_path + ".score");
    }
    apd_mesh_destroy(mesh);
    apd_volume_destroy(volume);
    std::cout << "Mesh of " << vertices << " vertices and " << faces << " faces on " << dims[0] << " x " << dims[1] << " x " << dims[2] << " samples in "
              << mesh_path << ": " << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() << " ms" << std::endl;
}

}  // namespace

// From the four state files of every view, as RunFusion reads them
void RunFilter(const path &dense_folder, const std::vector<Problem> &problems)
{
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    if (!prepare_fusion_inputs(dense_folder, problems, nullptr, 0, 0, views, sources, 0, nullptr, true)) {
        exit(EXIT_FAILURE);
    }
    const int V = (int)views.size();
    std::vector<const float *> deps(V), nors(V);
    std::vector<const uint8_t *> weaks(V), blocks(V, nullptr);
    bool any_block = false;
    for (int i = 0; i < V; ++i) {
        deps[i] = views[i].depth.ptr<float>();
        nors[i] = views[i].normal.ptr<float>();
        weaks[i] = views[i].weak.ptr<uint8_t>();
        if (!views[i].block.empty()) {
            blocks[i] = views[i].block.ptr<uint8_t>();
            any_block = true;
        }
    }
    filter_and_write(problems, views, sources, deps.data(), nors.data(), weaks.data(), any_block ? blocks.data() : nullptr, 0, 0, 0);
}

// The final maps are on `device` (cols x rows each): cameras and block masks are read here, the masks go up, only the outputs come
// down
void RunFilterOnDevice(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows,
                       const std::vector<const float *> &depths, const std::vector<const float *> &normals, const std::vector<const uint8_t *> &weaks)
{
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    if (!prepare_fusion_inputs(dense_folder, problems, nullptr, cols, rows, views, sources, 0, nullptr, true)) {
        exit(EXIT_FAILURE);
    }
    const int V = (int)views.size();
    std::vector<const uint8_t *> blocks(V, nullptr);
    std::vector<void *> owned;
    for (int i = 0; i < V; ++i) {
        if (views[i].block.empty()) {
            continue;
        }
        void *p = nullptr;
        if (apd_device_malloc(device, (size_t)rows * cols, &p) != APD_OK || apd_device_memcpy(device, p, views[i].block.data(), (size_t)rows * cols) != APD_OK) {
            std::cerr << "filter: upload of a block mask failed: " << apd_exchange_last_error() << std::endl;
            exit(EXIT_FAILURE);
        }
        owned.push_back(p);
        blocks[i] = (const uint8_t *)p;
    }
    const int fusion_device = g_fusion_device;
    g_fusion_device = device;
    filter_and_write(problems, views, sources, depths.data(), normals.data(), weaks.data(), owned.empty() ? nullptr : blocks.data(), cols, rows, 1);
    g_fusion_device = fusion_device;
    for (void *p : owned) {
        apd_device_free(device, p);
    }
}

// --mesh from the four state files of every view, as RunFusion reads them, after it has written APD.ply
void RunMesh(const path &dense_folder, const std::vector<Problem> &problems, float voxel, float trunc, const MeshClean &clean)
{
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    std::ostringstream unheard;
    if (!prepare_fusion_inputs(dense_folder, problems, nullptr, 0, 0, views, sources, 0, &unheard, false, true)) {
        exit(EXIT_FAILURE);
    }
    const int V = (int)views.size();
    std::vector<const float *> deps(V), nors(V);
    std::vector<const uint8_t *> weaks(V), blocks(V, nullptr);
    bool any_block = false;
    for (int i = 0; i < V; ++i) {
        deps[i] = views[i].depth.ptr<float>();
        nors[i] = views[i].normal.ptr<float>();
        weaks[i] = views[i].weak.ptr<uint8_t>();
        if (!views[i].block.empty()) {
            blocks[i] = views[i].block.ptr<uint8_t>();
            any_block = true;
        }
    }
    mesh_and_write(dense_folder / path("APD") / path("APD.ply"), problems, views, sources, deps.data(), nors.data(), weaks.data(), any_block ? blocks.data() : nullptr,
                   0, 0, 0, voxel, trunc, clean);
}

// The final maps are on `device` (cols x rows each): colour images, cameras and block masks are read here, the masks go up
void RunMeshOnDevice(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows,
                     const std::vector<const float *> &depths, const std::vector<const float *> &normals, const std::vector<const uint8_t *> &weaks,
                     float voxel, float trunc, const MeshClean &clean)
{
    std::vector<FusionView> views;
    std::vector<std::vector<int>> sources;
    std::ostringstream unheard;
    if (!prepare_fusion_inputs(dense_folder, problems, nullptr, cols, rows, views, sources, 0, &unheard, false, true)) {
        exit(EXIT_FAILURE);
    }
    const int V = (int)views.size();
    std::vector<const uint8_t *> blocks(V, nullptr);
    std::vector<void *> owned;
    for (int i = 0; i < V; ++i) {
        if (views[i].block.empty()) {
            continue;
        }
        void *p = nullptr;
        if (apd_device_malloc(device, (size_t)rows * cols, &p) != APD_OK || apd_device_memcpy(device, p, views[i].block.data(), (size_t)rows * cols) != APD_OK) {
            std::cerr << "mesh: upload of a block mask failed: " << apd_exchange_last_error() << std::endl;
            exit(EXIT_FAILURE);
        }
        owned.push_back(p);
        blocks[i] = (const uint8_t *)p;
    }
    const int fusion_device = g_fusion_device;
    g_fusion_device = device;
    mesh_and_write(dense_folder / path("APD") / path("APD.ply"), problems, views, sources, depths.data(), normals.data(), weaks.data(),
                   owned.empty() ? nullptr : blocks.data(), cols, rows, 1, voxel, trunc, clean);
    g_fusion_device = fusion_device;
    for (void *p : owned) {
        apd_device_free(device, p);
    }
}

extern "C" {

// Flat entry for the Python pipeline (maps already in memory after the all-gather): per-view pointers, all maps of view
// i are rows[i] x cols[i]; sources of view i are pair_indices[pair_offsets[i] .. pair_offsets[i+1]).  Returns the
// number of points written to `ply_path`.  apdhost_fuse_opt: with the options of this call (nullptr: those of
// apdhost_set_fusion_options), a file, the points in memory (*points, apd_points_destroy) or both, as apd_fuse_views_opt.
long long apdhost_fuse_opt(const apd_fusion_options *options, int num_views, const apd_camera *cameras, const float *const *images,
                           int image_channels, const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                           const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices,
                           const char *ply_path, apd_points_t *points)
{
    std::vector<FusionView> views(num_views);
    std::vector<std::vector<int>> sources(num_views);
    for (int i = 0; i < num_views; ++i) {
        const size_t n = (size_t)rows[i] * cols[i];
        FusionView &v = views[i];
        v.cam = cameras[i];
        v.cam.width = cols[i];
        v.cam.height = rows[i];
        v.image.create(rows[i], cols[i], image_channels == 3 ? MAT_32FC3 : MAT_32FC1);
        v.depth.create(rows[i], cols[i], MAT_32FC1);
        v.normal.create(rows[i], cols[i], MAT_32FC3);
        v.weak.create(rows[i], cols[i], MAT_8UC1);
        memcpy(v.image.data(), images[i], n * 4 * (image_channels == 3 ? 3 : 1));
        memcpy(v.depth.data(), depths[i], n * 4);
        memcpy(v.normal.data(), normals[i], n * 12);
        memcpy(v.weak.data(), weaks[i], n);
        if (blocks && blocks[i]) {
            v.block.create(rows[i], cols[i], MAT_8UC1);
            memcpy(v.block.data(), blocks[i], n);
        }
        sources[i].assign(pair_indices + pair_offsets[i], pair_indices + pair_offsets[i + 1]);
    }
    return fuse_dispatch(views, sources, ply_path, options, points);  // -1: the device fusion failed (message on stderr)
}

long long apdhost_fuse(int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                       const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                       const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets,
                       const int *pair_indices, const char *ply_path)
{
    return apdhost_fuse_opt(nullptr, num_views, cameras, images, image_channels, depths, normals, weaks, blocks, rows, cols, pair_offsets,
                            pair_indices, ply_path, nullptr);
}

}  // extern "C"
