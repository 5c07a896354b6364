// schedule.h -- what the two schedulers of the drop-in host share: the command-line options, the pass table of the
// reference driver (main.cpp:168-215) and the per-pass parameters of a problem.  host/main.cpp runs the table view by view
// through files like the reference (Gauss-Seidel over views); host/multi_device.cpp runs it in memory on several devices
// (RunMultiDevice: a Scheduler whose lanes take the (pass, view) tasks of a level from host/wavefront.h's queue on one rank,
// in order with an all-gather after every pass on several).
#ifndef APD_MI355X_HOST_SCHEDULE_H_
#define APD_MI355X_HOST_SCHEDULE_H_

#include <algorithm>
#include <cstdint>
#include <vector>

#include "APD.h"
#include "ply_options.h"

// What --mesh does to its mesh between extraction and the file, in this fixed order: apd_mesh_weld, apd_mesh_remove_unseen,
// apd_mesh_remove_small_components, apd_mesh_smooth, apd_mesh_simplify, apd_mesh_with_vertex_normals, apd_mesh_colour_from_views.  All off: the file has the bytes
// of the extracted mesh.  --mesh-score comes after the file and changes nothing of it.
struct MeshClean {
    float weld = 0.0f;                 // --mesh-weld TOL: 0 is off
    unsigned trim = 0;                 // --mesh-trim MIN_VIEWS[,MIN_PIXELS[,TOL]]: 0 is off
    unsigned trim_pixels = 1;
    float trim_tolerance = 0.01f;
    bool depth_maps = false;           // --mesh-depth-maps: depths_mesh.dmb of every view, the final mesh rendered into it
    bool remove_small = false;         // --mesh-min-component FACES
    unsigned min_component = 0;
    int smooth = 0;                    // --mesh-smooth ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]]: 0 is off
    float smooth_lambda = 0.5f, smooth_mu = -0.53f;
    int smooth_boundary = 1;           // APD_SMOOTH_BOUNDARY_ALONG
    float simplify = 0.0f;             // --mesh-simplify CELL[,mean|quadric]: 0 is off
    bool simplify_mean = false;        // ,mean: APD_SIMPLIFY_MEAN; otherwise APD_SIMPLIFY_QUADRIC
    bool normals = false;              // --mesh-normals
    bool recolour = false;             // --mesh-recolour [TOL[,MIN_COS]]: the colours from the views' images, not from the volume
    float recolour_tolerance = 0.01f, recolour_min_cos = 0.1f;
    std::string score_truth;           // --mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]: the final mesh scored against the cloud of TRUTH.ply; empty is off
    float score_threshold = 0.0f;
    double score_density = 0.0;        // 0: apd_mesh_score's own, 4 / TAU^2
    unsigned long long score_seed = 0;
};

struct Options {
    path dense_folder;
    int gpu_index = 0;
    std::vector<int> devices;   // "0,1,2,3": one scheduler rank per entry (an entry may repeat: two ranks on one device)
    bool jacobi = false;        // the in-memory scheduler of host/multi_device.cpp even with a single device
    int ranks_per_device = 0;   // --ranks N: scheduler ranks on a single device (0: by frame size, host/multi_device.cpp)
    bool files = false;         // --files: state moves between passes through the four files per view, as in the reference
    bool in_memory = false;     // --in-memory: the in-memory scheduler on one device in the reference's own order (one rank, a view reads the
                                // depth maps its sources have at that moment): the file-based driver's bytes without the files
    bool use_rccl = true;       // --no-rccl: exchange maps with direct copies
    bool exchange_device_sync = false;  // --exchange-device-sync: the per-pass exchange synchronises every device first, as in rounds 2-4 (A/B measurements)
    bool force_rccl = false;    // --rccl: RCCL even for a single rank (which has nothing to exchange between devices and uses direct copies otherwise)
    uint64_t seed = 12345;
    int iters = 3;          // PatchMatchParams::max_iterations of every pass (reference: 3)
    int max_src = 0;        // > 0: keep only the first N sources of each pair.txt entry (they are sorted by score)
    bool single_level = false, keep_maps = false, no_fusion = false;
    int fusion_variant = APD_FUSION_ETH;  // --fusion eth | tat-intermediate | tat-advanced
    // --fusion-min-consistent N, --fusion-reproj PX, --fusion-depth REL, --fusion-angle RAD, --fusion-factors STRONG,WEAK, --ply-normals
    apd_fusion_options fusion = [] {
        apd_fusion_options o;
        apd_fusion_default_options(&o);
        return o;
    }();
    PlyOptions ply;                       // every other --ply-* flag: what becomes of the fused points before APD.ply is written (host/ply_options.h)
    bool filtered_maps = false;           // --filtered-maps: depths_filtered.dmb, consistency.dmb and votes.bin of every view (apd_filter_views)
    float mesh_voxel = 0.0f;              // --mesh VOXEL[,TRUNC]: APD/APD.ply.mesh, the marching-tetrahedra mesh of the filtered maps fused into a signed
    float mesh_trunc = 0.0f;              // distance volume with samples VOXEL apart in the box of the points of APD.ply (apd_volume_*); voxel 0: off
    MeshClean mesh_clean;                 // --mesh-weld TOL, --mesh-trim MIN_VIEWS[,MIN_PIXELS[,TOL]], --mesh-depth-maps, --mesh-min-component FACES, --mesh-smooth ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]], --mesh-simplify CELL[,mean|quadric], --mesh-normals, --mesh-recolour [TOL[,MIN_COS]]: what becomes of that mesh before it is written; --mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]: its score
    bool fusion_thresholds_set = false;   // one of the five threshold flags was given: the ETH loop only
    bool copy_images = false;         // --copy-images: handles copy and pack their images per (view, pass) instead of sharing the level images (A/B)
    bool clean_exit = false;          // --clean-exit: return from main() instead of _Exit (exit handlers run: profilers)
    double scheduler_free_gb = 0;     // --scheduler-free-gb X: RunMultiDevice's own fit test counts at most X GB of free device memory (main()'s
                                      // choice of scheduler still uses the device's figure: this is how a test reaches the fall-back to files)
    std::string masks_dir;            // --masks [DIR]: per-view pixel masks <dense_folder>/DIR/<%08d>.jpg|pgm (default DIR: masks); empty: none
    bool late_fusion_inputs = false;  // --late-fusion-inputs: colour decode + upload after the passes instead of behind them (A/B measurements)
};

// true when a run over this device list sets RCCL up (several physical devices, or --rccl); the set-up blocks before the first pass
// (round 5's --async-rccl measured slower and is gone: profiles/r05/ab_rccl_async_tt24.txt)
inline bool WantsRccl(const Options &opt)
{
    bool several = false;
    for (size_t i = 1; i < opt.devices.size(); ++i) {
        several = several || opt.devices[i] != opt.devices[0];
    }
    return opt.use_rccl && (several || opt.force_rccl);
}

// One pass over all views.  round_num pyramid levels, coarse to fine; per level one photometric pass and three
// geometric ones (main.cpp:168-215).
struct Pass {
    int level = 0;             // i of main.cpp:168
    int iteration = 0;         // Problem::iteration, counts passes
    int scale_size = 1;        // 2^(round_num - 1 - level)
    RunState state = FIRST_INIT;
    bool geom_consistency = false, use_APD = false;
    int weak_peak_radius = 6;
    float ransac_threshold = 0.005f;  // only read when use_APD (the struct default otherwise, main.h:92)
    int rotate_time = 4;
};

inline int RoundNum(int width, int height)  // main.cpp:72-88: halve until the longer side is <= 1000
{
    int rounds = 1;
    for (int longest = std::max(width, height); longest > 1000; longest /= 2) {
        ++rounds;
    }
    return rounds;
}

inline std::vector<Pass> BuildSchedule(int round_num, bool single_level)
{
    std::vector<Pass> plan;
    for (int level = 0; level < round_num; ++level) {
        for (int k = 0; k < 4; ++k) {  // k = 0: photometric, k = 1..3: geometric with j = k - 1
            Pass p;
            p.level = level;
            p.iteration = (int)plan.size();
            p.scale_size = single_level ? 1 : 1 << (round_num - 1 - level);
            p.state = k > 0 ? REFINE_ITER : (level == 0 ? FIRST_INIT : REFINE_INIT);
            p.geom_consistency = k > 0;
            p.weak_peak_radius = k == 0 ? 6 : std::max(4 - 2 * (k - 1), 2);
            p.use_APD = level > 0;
            if (p.use_APD) {
                p.ransac_threshold = (float)(0.01 - level * 0.00125);  // double arithmetic, then float, as main.cpp:180
                p.rotate_time = std::min(1 << level, 4);
            }
            plan.push_back(p);
        }
    }
    return plan;
}

// The reference keeps one PatchMatchParams per problem alive across passes and only overwrites some fields, so
// ransac_threshold / rotate_time of level 0 are the struct defaults: same here.
inline void Configure(Problem &problem, const Pass &pass, const Options &o)
{
    PatchMatchParams &q = problem.params;
    q.state = pass.state;
    q.use_APD = pass.use_APD;
    if (pass.use_APD) {
        q.ransac_threshold = pass.ransac_threshold;
        q.rotate_time = pass.rotate_time;
    }
    q.geom_consistency = pass.geom_consistency;
    q.max_iterations = o.iters;
    q.weak_peak_radius = pass.weak_peak_radius;
    q.seed = o.seed + (uint64_t)pass.iteration * 7919u + (uint64_t)problem.index;  // the reference seeds with clock64()
    problem.iteration = pass.iteration;
    problem.show_medium_result = true;
    problem.scale_size = pass.scale_size;
}

static const char *const kStateFiles[4] = {"depths.dmb", "normals.dmb", "weak.bin", "selected_views.bin"};

// The four state files of a view (main.cpp:117-124) into its result folder.  Returns an empty string, or the file that could not be written.
inline std::string WriteStateFiles(const path &result_folder, const Mat &depth, const Mat &normal, const Mat &weak, const Mat &views)
{
    const Mat *maps[4] = {&depth, &normal, &weak, &views};
    for (int k = 0; k < 4; ++k) {
        if (!WriteBinMat(result_folder / kStateFiles[k], *maps[k])) {
            return (result_folder / kStateFiles[k]).string();
        }
    }
    return std::string();
}

// host/multi_device.cpp: every pass on all listed devices (views round-robin), state resident on the devices, depth maps
// all-gathered after every pass.  Returns the process exit code.
int RunMultiDevice(const Options &opt, std::vector<Problem> &problems);

// Views in flight per device by frame size, and the device bytes per pixel (finest level) the in-memory scheduler keeps resident
// on its busiest device (host/multi_device.cpp).
int DefaultLanes(size_t pixels);
int InMemoryLanes(const Options &opt, int width, int height, int num_views, int num_ranks, bool distinct_devices);
double InMemoryBytesPerPixel(int num_images, int num_views, int num_ranks, int lanes, int max_sources, double *passes_out = nullptr,
                             double *final_out = nullptr, bool fusion_prefetch = false, bool masks = false);
// The scheduler's fit test, ONE function for main()'s choice of scheduler and for RunMultiDevice's own check: bytes the run keeps resident on
// `device` (its busiest one) against 90 % of the free device memory, the latter capped by --scheduler-free-gb.
struct InMemoryFit {
    bool have_memory = false;            // hipMemGetInfo answered
    bool fits = true;                    // need <= 0.9 * free (true when the device did not answer: the allocations will tell)
    bool release_before_fusion = true;   // no room for the passes' buffers and the final maps at once
    double need_bytes = 0, free_bytes = 0;
};
InMemoryFit TestInMemoryFit(const Options &opt, int device, int width, int height, int num_images, int num_views, int num_ranks, int lanes, int max_sources);
constexpr int kExitDoesNotFit = 75;  // RunMultiDevice: the folder does not fit the in-memory scheduler (nothing has been run or written)

// APD.h:34 with the maps already in memory (index = problem index); RunFusion reads them from the result folders instead
struct FinalMaps {
    Mat depth, normal, weak;
};
void RunFusionWithMaps(const path &dense_folder, const std::vector<Problem> &problems, const std::vector<FinalMaps> *maps);
// ... and with the final maps resident on `device` (cols x rows each; depth, normal = 3 floats per pixel, weak): nothing is
// downloaded.  StartFusionInputs decodes the colour images, reads cameras and masks and uploads them on a background thread
// (call it before the passes); RunFusionOnDevice joins it and fuses; CancelFusionInputs joins and frees without fusing.
struct FusionPrefetch;
FusionPrefetch *StartFusionInputs(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows, unsigned threads);
void RunFusionOnDevice(FusionPrefetch *inputs, const std::vector<const float *> &depths, const std::vector<const float *> &normals,
                       const std::vector<const uint8_t *> &weaks);
void CancelFusionInputs(FusionPrefetch *inputs);
bool FusionInputsFailed(const FusionPrefetch *inputs, std::string *why);

// --filtered-maps: the geometric filter (apd_filter_views) with the rule of SetFusionOptions on every view's final maps, read from
// the result folders (RunFilter) or resident on `device` (RunFilterOnDevice: only the outputs come down); writes
// depths_filtered.dmb and consistency.dmb (as depths.dmb) and votes.bin (as weak.bin) into every result folder.  Honours
// <dense>/blocks like the fusion.
void RunFilter(const path &dense_folder, const std::vector<Problem> &problems);
void RunFilterOnDevice(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows,
                       const std::vector<const float *> &depths, const std::vector<const float *> &normals, const std::vector<const uint8_t *> &weaks);

// --mesh VOXEL[,TRUNC], after the fusion has written APD/APD.ply: the filter above on every view's final maps (read from the result
// folders, or resident on `device`), apd_volume_create over the box of the finite points of APD.ply grown by `trunc`,
// apd_volume_integrate of the filtered maps with the views' colour images, every view weighing 1, apd_volume_extract_mesh, and
// the steps of `clean` on the mesh, one printed line each with the counts before and after, and apd_mesh_write_ply into
// APD/APD.ply.mesh.  Honours <dense>/blocks and the --fusion-* rule like the filter.
void RunMesh(const path &dense_folder, const std::vector<Problem> &problems, float voxel, float trunc, const MeshClean &clean);
void RunMeshOnDevice(const path &dense_folder, const std::vector<Problem> &problems, int device, int cols, int rows,
                     const std::vector<const float *> &depths, const std::vector<const float *> &normals, const std::vector<const uint8_t *> &weaks,
                     float voxel, float trunc, const MeshClean &clean);

#endif  // APD_MI355X_HOST_SCHEDULE_H_
