/*
 * apd_mi355x.h -- C ABI of the MI355X-native PatchMatch path of APD-MVS.
 *
 * The reference (whoiszzj/APD-MVS) has no C ABI / FFI layer: its boundary for this path is the C++
 * class `APD` (APD.h:67-145) driven by `ProcessProblem` (main.cpp:91-138).  This header is the
 * flat `extern "C"` equivalent of that class: one handle == one `APD` object == one
 * (reference view, pass).  Every entry point cites the reference member it replaces.  The C++
 * drop-in class (apd-mvs_amd/host/APD.h) and the Python host mirror (apd-mvs_amd/__init__.py)
 * are thin layers over exactly these symbols.
 *
 * Conventions: all functions return 0 on success and a negative apd_status otherwise (the
 * reference calls exit(); a library must not).  apd_last_error() gives the message of the last
 * failure on the calling thread.  Caller owns every buffer it passes.  A handle is bound to one
 * device and is not thread-safe; distinct handles on distinct devices may run concurrently.
 * Pointers passed to upload/download may be host or device pointers (hipMemcpyDefault).
 */
#ifndef APD_MI355X_H_
#define APD_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APD_MAX_IMAGES 32        /* main.h:37 MAX_IMAGES */
#define APD_NEIGHBOUR_NUM 9      /* main.h:38 NEIGHBOUR_NUM */
#define APD_MAX_SEARCH_RADIUS 4096 /* main.h:39 */

typedef enum { APD_FIRST_INIT = 0, APD_REFINE_INIT = 1, APD_REFINE_ITER = 2 } apd_run_state; /* main.h:63-67 */
typedef enum { APD_WEAK = 0, APD_STRONG = 1, APD_UNKNOWN = 2 } apd_pixel_state;              /* main.h:69-73 */

typedef enum {
    APD_OK = 0,
    APD_ERR_INVALID = -1,   /* bad argument */
    APD_ERR_HIP = -2,       /* HIP runtime error (reference: CudaSafeCall -> exit, APD.cpp:315-323) */
    APD_ERR_TOO_MANY = -3,  /* > APD_MAX_IMAGES images (reference: exit, APD.cpp:428-431) */
    APD_ERR_STATE = -4,     /* call order violated (e.g. run before upload) */
    APD_ERR_UNSUPPORTED = -5,
    APD_ERR_IO = -6         /* a file could not be written */
} apd_status;

/* Byte-compatible with the reference `Camera` (main.h:47-56, 112 bytes). */
typedef struct apd_camera {
    float K[9];
    float R[9];
    float t[3];
    float c[3];
    int height;
    int width;
    float depth_min;
    float depth_max;
} apd_camera;

/* Fields of `PatchMatchParams` (main.h:75-94) in the reference's order, then the additive knobs. */
typedef struct apd_params {
    int max_iterations;     /* 3 */
    int num_images;         /* set by apd_upload_views */
    float sigma_spatial;    /* 5.0  (dead in the reference: weight == 1, APD.cu:473,575) */
    float sigma_color;      /* 3.0  (dead) */
    int top_k;              /* 4 */
    float depth_min;        /* 0.6 * ref camera depth_min (APD.cpp:454) */
    float depth_max;        /* 1.2 * ref camera depth_max (APD.cpp:455) */
    int geom_consistency;   /* bool */
    int strong_radius;      /* 5 */
    int strong_increment;   /* 2 */
    int weak_radius;        /* 5 */
    int weak_increment;     /* 5 */
    int use_APD;            /* bool */
    int weak_peak_radius;   /* 2 */
    int rotate_time;        /* 4; 1..4 only (K3 keeps 8 x 4 ray slots): apd_create / apd_reset refuse any other value
                               with APD_ERR_UNSUPPORTED */
    float ransac_threshold; /* 0.005 */
    float geom_factor;      /* 0.2 */
    int state;              /* apd_run_state */
    /* ---- additive knobs (absent in the reference; defaults keep reference behaviour) ---- */
    uint64_t seed;          /* replaces clock64() in curand_init, APD.cu:803 */
} apd_params;

typedef struct apd_context *apd_handle;

/* Kernel ids for apd_run_kernel / apd_profile_get. */
enum {
    APD_K1_INIT_RANDOM_STATES = 1,   /* APD.cu:791  */
    APD_K2_FIND_NEAREST_STRONG = 2,  /* APD.cu:2234 */
    APD_K3_GEN_NEIGHBOURS = 3,       /* APD.cu:1750 */
    APD_K4_NEIGHBOUR_UPDATE = 4,     /* APD.cu:1971 */
    APD_K5_RANDOM_INITIALIZATION = 5,/* APD.cu:806  */
    APD_K6_BLACK_UPDATE_STRONG = 6,  /* APD.cu:1547 */
    APD_K7_RED_UPDATE_STRONG = 7,    /* APD.cu:1567 */
    APD_K8_RANSAC_FIT_PLANE = 8,     /* APD.cu:2272 */
    APD_K9_BLACK_UPDATE_WEAK = 9,    /* APD.cu:1510 */
    APD_K10_RED_UPDATE_WEAK = 10,    /* APD.cu:1529 */
    APD_K11_GET_DEPTH_NORMAL = 11,   /* APD.cu:1587 */
    APD_K12_BLACK_FILTER = 12,       /* APD.cu:1716 */
    APD_K13_RED_FILTER = 13,         /* APD.cu:1733 */
    APD_K14_DEPTH_TO_WEAK = 14,      /* APD.cu:1990 */
    APD_K15_LOCAL_REFINE = 15,       /* APD.cu:2146 */
    APD_KERNEL_COUNT = 16
};

/* State arrays readable with apd_download_state (tests / snapshots). */
enum {
    APD_STATE_PLANES = 0,        /* float4  [H*W]      plane_hypotheses_cuda      */
    APD_STATE_FIT_PLANES = 1,    /* float4  [H*W]      fit_plane_hypotheses_cuda  */
    APD_STATE_COSTS = 2,         /* float   [H*W]      costs_cuda                 */
    APD_STATE_RNG = 3,           /* uint32  [H*W*6]    rand_states_cuda (x0..x4,d)*/
    APD_STATE_SELECTED_VIEWS = 4,/* uint32  [H*W]      selected_views_cuda        */
    APD_STATE_VIEW_WEIGHT = 5,   /* uint8   [H*W*32]   view_weight_cuda           */
    APD_STATE_WEAK_INFO = 6,     /* uint8   [H*W]      weak_info_cuda             */
    APD_STATE_WEAK_RELIABLE = 7, /* uint8   [H*W]      weak_reliable_cuda         */
    APD_STATE_NEAREST_STRONG = 8,/* short2  [H*W]      weak_nearest_strong        */
    APD_STATE_NEIGHBOURS_MAP = 9,/* int32   [H*W]      neighbours_map_cuda        */
    APD_STATE_NEIGHBOURS = 10    /* short2  [weak*9]   neighbours_cuda            */
};

/* Defaults of PatchMatchParams (main.h:75-94), seed = 12345. */
void apd_default_params(apd_params *p);

/* APD::APD(const Problem&) (APD.cpp:356-359) + the allocations of CudaSpaceInitialization
 * (APD.cpp:636-666).  `device` < 0 keeps the current device (reference: cudaSetDevice, main.cpp:153).
 * Limits (APD_ERR_UNSUPPORTED otherwise): width, height <= 16384 (16-bit neighbour coordinates, 24-bit index
 * arithmetic) and (width + 1) * (height + 1) * 16 < 2^32 (32-bit byte offsets into the float texel-quad copy of a source:
 * 16384 x 16382 is the largest frame with a 16384-px axis); patch geometry strong 5/2, weak 5/5; rotate_time 1..4.  These
 * are answered before any device call.  Non-positive sizes are APD_ERR_INVALID.  No handle is returned on failure. */
int apd_create(apd_handle *out, int device, int width, int height, const apd_params *params);

/* ~APD (APD.cpp:361-397). */
int apd_destroy(apd_handle h);

/* Re-arms a handle for another (view, pass) of the same width x height with new parameters: the state arrays return to
 * what apd_create leaves (so a recycled handle gives the same bits as a new one), uploads are forgotten, device buffers
 * are kept.  Saves the ~25 hipMalloc/hipFree pairs per (view, pass) of the construct-run-destroy cycle of
 * ProcessProblem (main.cpp:91-138).  Parameters apd_create would refuse (patch geometry, rotate_time) are refused here
 * too, with APD_ERR_UNSUPPORTED, and leave the handle as it was: armed for the pass it was armed for. */
int apd_reset(apd_handle h, const apd_params *params);

/* Image / depth / camera upload of CudaSpaceInitialization (APD.cpp:588-634).  images[0] is the
 * reference view; `depths` may be NULL unless params.geom_consistency.  All images are W*H floats,
 * row-major, no padding.  Sets params.num_images.
 * The pixel domain: every pixel finite and in [-2^20, 2^20] (8- and 16-bit images at any scale up to that, [0, 1] images, images
 * centred on zero).  Inside it every NCC has the reference's bits; outside it the variance products leave the range the NCC tail is
 * exact in.  apd_upload_views, apd_upload_views_split and apd_image_create test every pixel on the device and answer
 * APD_ERR_UNSUPPORTED with the first offending view in apd_last_error; no kernel of a pass runs, and a handle whose upload was
 * refused holds no views until the next accepted upload.  Depth maps may hold any float (0 and -0 mean "no depth"). */
int apd_upload_views(apd_handle h, int num_images, const apd_camera *cameras, const float *const *images,
                     const float *const *depths);

/* A geometric pass in two halves, for a scheduler that keeps several views in flight: the sources' depth maps are the only
 * input of a (view, pass) that other views of the same pass produce (the reference reads depths.dmb as the files are at that
 * moment, APD.cpp:497-500), and only the weak update (K9/K10), K14 and K15 read them (ComputeGeomConsistencyCost, APD.cu:752).
 *   apd_upload_views_split   = apd_upload_views without depth maps (their buffers are allocated);
 *   apd_run_before_depths    = the longest prefix of the schedule that reads no depth map: K1..K5, iteration 0 of K6..K8 and --
 *                              while no WEAK pixel exists -- the other iterations and K11..K13; without the geometric term the
 *                              whole pass;
 *   apd_upload_depths        = the num_images depth maps (index 0: the view's own), copied on the handle's stream, i.e. after the
 *                              kernels already launched; returns when the copies are done;
 *   apd_run_after_depths     = the rest of the schedule.
 * before + after launch exactly the kernels of apd_run, in its order: same bits.  K9, K10, K14 and K15 return APD_ERR_STATE
 * while the depth maps of a split upload are outstanding. */
int apd_upload_views_split(apd_handle h, int num_images, const apd_camera *cameras, const float *const *images);
int apd_upload_depths(apd_handle h, int num_images, const float *const *depths);
int apd_run_before_depths(apd_handle h);
int apd_run_after_depths(apd_handle h);

/* Shared images.  A pyramid-level image of a view is the reference image of one (view, pass) and a source of ten others, pass after
 * pass; apd_upload_views copies it into the handle, tests it for 8-bit content and packs it again every time.  A scheduler that
 * keeps the level images on the device creates each one ONCE (pixels: width x height floats, host or device; the float plane, the
 * 8-bit test, the packed copy the kernels gather from -- further copies on first demand) and uploads views by reference:
 * apd_upload_views_shared == apd_upload_views_split without the copies (images[0] the reference view; every image of the handle's
 * size and on its device; in a geometric pass the depth maps follow with apd_upload_depths).  An image may serve any number of
 * handles on any threads at once and must outlive the passes that use it.  Same bits as the copying uploads. */
/* apd_image_create returns APD_ERR_INVALID for every size no handle can have (non-positive, or outside apd_create's limits). */
typedef struct apd_image *apd_image_t;
int apd_image_create(apd_image_t *out, int device, int width, int height, const float *pixels);
int apd_image_destroy(apd_image_t image);
const float *apd_image_pixels(apd_image_t image);   /* the float plane on the device (e.g. for a copying apd_upload_views of the same image) */
int apd_upload_views_shared(apd_handle h, int num_images, const apd_camera *cameras, const apd_image_t *images);

/* Prior state of a previous pass (APD.cpp:552-581, 643-661): planes = (world normal xyz, depth w),
 * selected-view bitmasks and weak map.  Any pointer may be NULL: planes/views zero, weak = all STRONG
 * (APD.cpp:541-547).  Builds the weak index map of APD.cpp:526-537. */
int apd_upload_prior(apd_handle h, const float *planes4, const uint32_t *selected_views, const uint8_t *weak_info);

/* Per-view pixel mask of this (view, pass): W*H bytes, host or device pointer, non-zero = process, zero = masked out; NULL
 * clears it.  The reference knows one mask, `blocks/mask_<id>.jpg`, and only its fusion reads it (APD.cpp:849-853): PatchMatch
 * has by then spent its time on those pixels and used their depths as geometric partners of other views.  Here the mask
 * reaches the kernels:
 *   - before the first kernel of the pass the masked pixels of the weak map (apd_upload_prior's, or the all-STRONG default)
 *     become APD_UNKNOWN: never WEAK, so in no WEAK list and without neighbours (K2..K4), never an anchor of K3 or a tap of
 *     K12/K13; the weak index map and apd_weak_count are those of that map;
 *   - K1..K5 run on masked pixels as on any other; K6..K15 write no state array at a masked pixel (a wave whose pixels are
 *     all masked leaves at its first ballot), and live pixels read masked neighbours like any neighbour;
 *   - apd_download, apd_export_state_device and apd_export_depth_normal_device give a masked pixel depth 0, normal (0,0,0),
 *     plane (0,0,0,0), APD_UNKNOWN, selected views 0 -- "no estimate" for the geometric term and for every fusion loop
 *     (apd_download_state stays a raw copy).
 * Without a mask, or with one that is non-zero everywhere, every bit is what an unmasked handle computes.  Valid after
 * apd_create / apd_reset and before the first kernel of the pass (APD_ERR_STATE afterwards), before or after
 * apd_upload_prior and the view uploads; forgotten by apd_reset like them.  Copied on the handle's stream; returns when the
 * copy is done.  apd_masked_count: zero bytes of the current mask (0 without one). */
int apd_upload_mask(apd_handle h, const uint8_t *mask);
int apd_masked_count(apd_handle h);

/* APD::RunPatchMatch (APD.cu:2386-2495), without the final device->host copies.  One handle is one (view, pass), like one
 * APD object: K14 rewrites the weak map the WEAK lists, the neighbour table and its index map were sized for, so a second
 * apd_run -- or K3 / K8 / K9 / K10 through apd_run_kernel after K14 or after apd_upload_state(APD_STATE_WEAK_INFO) -- returns
 * APD_ERR_STATE until apd_upload_prior or apd_reset re-arms the handle. */
int apd_run(apd_handle h);

/* One kernel of the schedule (single stepping for snapshot tests). */
int apd_run_kernel(apd_handle h, int kernel_id, int iter);

/* The metric's timed region: loop body APD.cu:2443-2457 (K6,K7,K8,K9,K10) for
 * iter = first_iter .. first_iter+iters-1.  Asynchronous; pair with apd_synchronize. */
int apd_run_sweeps(apd_handle h, int first_iter, int iters);

int apd_synchronize(apd_handle h);

/* The three copies at the end of RunPatchMatch (APD.cu:2490-2492) == GetPlaneHypothesis /
 * GetPixelStates / GetSelectedViews (APD.cpp:701-711).  Any pointer may be NULL. */
int apd_download(apd_handle h, float *planes4, uint8_t *weak_info, uint32_t *selected_views);

/* Raw copy of one state array (see APD_STATE_*).  `bytes` must not exceed the array size. */
int apd_download_state(apd_handle h, int which, void *dst, size_t bytes);
int apd_upload_state(apd_handle h, int which, const void *src, size_t bytes);
size_t apd_state_bytes(apd_handle h, int which);

/* Post-processing of ProcessProblem (main.cpp:105-115) done on the device: depth = plane.w with
 * out-of-range -> 0, normal = plane.xyz.  `depth_dev` (W*H floats) and `normal_dev` (3*W*H floats)
 * are DEVICE pointers (e.g. torch tensors handed to an RCCL all-gather). */
int apd_export_depth_normal_device(apd_handle h, float *depth_dev, float *normal_dev);

/* The same post-processing in the layout apd_upload_prior takes, left on the device (a scheduler that keeps state resident
 * between passes): planes4 = (world normal xyz, depth w) with an out-of-range depth -> 0 and its pixel UNKNOWN in `weak`
 * (main.cpp:109-112), selected views, and the depth map alone (what the geometric term of the next pass reads,
 * APD.cpp:492-509).  DEVICE pointers, W*H elements each; any may be NULL. */
int apd_export_state_device(apd_handle h, float *planes4_dev, uint8_t *weak_dev, uint32_t *views_dev, float *depth_dev);
/* The HIP event (hipEvent_t) the handle records on its stream behind the kernel of its last apd_export_state_device /
 * apd_export_depth_normal_device (NULL before the first export): what a consumer on another stream waits for
 * (apd_exchange_allgather_after).  Owned by the handle, re-recorded by every export. */
int apd_export_event(apd_handle h, void **hip_event);

/* ---- several devices in one process (one host thread + one stream per device) ----------------------------
 * The reference takes one device index (main.cpp:149-153).  A multi-device host shards the reference views over devices
 * and needs, besides the handles above (one per device, each used from its own thread): device memory without a HIP
 * toolchain, the nearest-neighbour resampling of prior state between pyramid levels (RescaleMatToTargetSize,
 * APD.cpp:752-774, swapped factors included) on the device, and the all-gather of per-view maps after every pass -- the
 * exchange the reference does through depths.dmb files (APD.cpp:497-500). */
int apd_device_malloc(int device, size_t bytes, void **out);
int apd_device_free(int device, void *p);
int apd_device_memcpy(int device, void *dst, const void *src, size_t bytes);   /* host or device pointers on either side */
int apd_device_memset(int device, void *dst, int value, size_t bytes);
int apd_device_memory(int device, size_t *free_bytes, size_t *total_bytes);   /* hipMemGetInfo: does an in-memory run fit? */
int apd_rescale_nearest_device(int device, const void *src, int src_w, int src_h, void *dst, int dst_w, int dst_h, int elem_bytes /* 1, 4, 16 */);
/* The same helpers on a HIP stream (hipStream_t, e.g. apd_get_stream of the handle whose kernels produce or consume the data):
 * asynchronous, ordered with that stream's work and with nothing else -- the device-wide forms above wait for the whole device,
 * which stalls every other view in flight on it.  apd_stream_synchronize waits for that stream alone. */
int apd_device_memcpy_async(int device, void *hip_stream, void *dst, const void *src, size_t bytes);
int apd_rescale_nearest_async(int device, void *hip_stream, const void *src, int src_w, int src_h, void *dst, int dst_w, int dst_h, int elem_bytes);
int apd_stream_synchronize(int device, void *hip_stream);
int apd_stream_create(int device, void **hip_stream);    /* a non-blocking stream of its own (not ordered with the null stream) */
int apd_stream_destroy(int device, void *hip_stream);
/* (float4 plane = world normal xyz + depth w) -> the depth map and the 3-float normal map apd_fuse_views takes; device pointers. */
int apd_split_planes_async(int device, void *hip_stream, const float *planes4, size_t pixels, float *depth, float *normal3);
/* Page-locks / releases a host buffer (hipHostRegister): uploads from it run at the link's rate and asynchronously.
 * apd_host_alloc / apd_host_free: a page-locked buffer of its own (hipHostMalloc) -- a staging buffer that is mapped ONCE: every
 * map / unmap of host pages (hipHostRegister, and the on-the-fly pinning a plain hipMemcpy of pageable memory does) holds up the
 * kernels running on the device for milliseconds. */
int apd_host_register(void *p, size_t bytes);
int apd_host_unregister(void *p);
int apd_host_alloc(size_t bytes, void **out);
int apd_host_free(void *p);

/* All-gather across `num_ranks` ranks of this process, rank r on devices[r]: after apd_exchange_allgather every recv[r]
 * holds send[0] | send[1] | ... (bytes_per_rank each).  prefer_rccl != 0: RCCL (ncclCommInitAll, grouped ncclAllGather,
 * one stream per rank; librccl is opened at run time); direct hipMemcpyPeerAsync copies when librccl is missing, when its
 * initialisation fails or when there is a single rank.  A list that names devices more than once (several scheduler ranks
 * per device, e.g. 0,1,0,1) runs RCCL between one leader rank per device and copies inside the devices; 0,0,0 (one device)
 * uses copies unless RCCL is forced.  Blocking; not thread-safe per exchange object. */
typedef struct apd_exchange *apd_exchange_t;
/* prefer_rccl != 0: RCCL, set up before the call returns.  That takes seconds on a fresh box (5.0 s to dlopen librccl from a cold page
 * cache, 1.0 s warm; ncclCommInitAll 0.65 s for one device: profiles/r05/rccl_init_time.txt); a caller with a single rank should pass 0.
 * (Round 5's asynchronous set-up -- preload thread, communicators initialised behind the first passes -- measured slower and was removed
 * in round 6: profiles/r05/ab_rccl_async_tt24.txt.)  apd_exchange_setup_times: what the dlopen and the initialisation took. */
int apd_exchange_create(apd_exchange_t *out, int num_ranks, const int *devices, int prefer_rccl);
int apd_exchange_setup_times(apd_exchange_t x, double *dlopen_ms, double *init_ms);
int apd_exchange_allgather(apd_exchange_t x, const void *const *send, void *const *recv, size_t bytes_per_rank);
/* ... without the device-wide synchronisation: the exchange's streams wait for the `num_events` HIP events (hipEvent_t; NULL entries are
 * skipped) that mark the send buffers complete -- apd_export_event of every handle that exported a block -- and for nothing else, so
 * kernels queued by other host threads (the next pass's first halves) keep running beside the exchange.  The caller knows the recv
 * buffers to be idle. */
int apd_exchange_allgather_after(apd_exchange_t x, const void *const *send, void *const *recv, size_t bytes_per_rank, int num_events,
                                 void *const *hip_events);
const char *apd_exchange_backend(apd_exchange_t x);   /* "rccl" or "peer-copy" */
int apd_exchange_counts(apd_exchange_t x, int *with_rccl, int *with_copies);   /* exchanges served by either backend so far */
int apd_exchange_destroy(apd_exchange_t x);
const char *apd_exchange_last_error(void);

/* Getters of APD.h:76-81. */
int apd_width(apd_handle h);
int apd_height(apd_handle h);
float apd_depth_min(apd_handle h);
float apd_depth_max(apd_handle h);
int apd_weak_count(apd_handle h);

/* Per-kernel timing with HIP events on the handle's stream. */
int apd_profile_enable(apd_handle h, int on);
int apd_profile_reset(apd_handle h);
int apd_profile_get(apd_handle h, int kernel_id, double *total_ms, int *launches);

/* Options of one handle.  The library reads NOTHING from the process environment: every switch is set here, explicitly,
 * and can be read back.  All options but APD_OPT_FAST_RCP leave every result bit unchanged (they select between
 * implementations that the test-suite compares bit for bit); APD_OPT_FAST_RCP is a tolerance mode and is off by default.
 * Options marked (upload) are latched by the next apd_upload_views. */
enum {
    APD_OPT_FAST_RCP = 0,       /* 0 (default) exact reciprocals: results are the arithmetic contract's bits.  1: the K6/K7 sample
                                 * loops stop at v_rcp_f32 (<= 1 ulp), what the reference's --use_fast_math build does
                                 * (CMakeLists.txt:20); NOT bit-identical, see tests/test_gpu_fast_rcp.py */
    APD_OPT_EARLY_OUT = 1,      /* 1 (default) exact early-outs of the refinement loops, K14 and K15; 0: every NCC the reference evaluates */
    APD_OPT_SOURCE_QUADS = 2,   /* (upload) 1 (default) 8-bit inputs are also kept as packed texel pairs; 0: float texel quads for every input */
    APD_OPT_TILED_COPY = 3,     /* (upload) second, tiled copy of 8-bit sources for random gathers: 0 never, 1 (default) built for FIRST_INIT
                                 * passes and used while the planes are random (first iteration), 2 built always, used by every global gather */
    APD_OPT_K67_WINDOWS = 4,    /* 1 (default) K6/K7 with LDS source windows; 0: every sample from HBM */
    APD_OPT_K1415_WINDOWS = 5,  /* 1 (default) K14/K15 with LDS source windows */
    APD_OPT_COUNT = 6
};
int apd_set_option(apd_handle h, int option, int value);
int apd_get_option(apd_handle h, int option, int *value);

/* Use an existing HIP stream (hipStream_t) instead of the handle's own. */
int apd_set_stream(apd_handle h, void *hip_stream);
/* The stream the handle launches on (hipStream_t), for the stream forms of the device helpers. */
int apd_get_stream(apd_handle h, void **hip_stream);

/* Depth-map fusion on the device: what RunFusion (APD.cpp:826-977, ETH variant) + ExportPointCloud (APD.cpp:214-254)
 * produce, i.e. <dense>/APD/APD.ply, from the final maps of every view (after the all-gather in a multi-GPU run).
 * View i has cameras[i] (K already scaled to the map size, APD.cpp:729-750), image images[i] (floats 0..255,
 * image_channels = 1: grey, 3: blue, green, red interleaved as cv::imread(IMREAD_COLOR) gives them, APD.cpp:859),
 * depths[i] (<= 0: no estimate), normals[i] (3 floats per pixel, world frame), weaks[i] (PixelState), optionally
 * blocks[i] (the `blocks/mask_<id>.jpg` of APD.cpp:849-853: reference pixels below 128 are skipped; `blocks` or any
 * blocks[i] may be NULL), all
 * rows[i] x cols[i]; its sources are pair_indices[pair_offsets[i] .. pair_offsets[i+1]) (indices of views, in
 * pair.txt order).  maps_on_device != 0: the four map arrays hold DEVICE pointers (e.g. the gathered torch tensors).
 * Views are fused in order, and inside a view the raster-order consumption of source pixels (`masks`) is resolved
 * exactly, so the point list is the one the sequential host loop writes.  A view that lists itself as a source is
 * refused (APD_ERR_INVALID), and so is a view whose rows[i] * cols[i] is negative or above 0x7fffff00: a pixel index is
 * an int on the device. */
int apd_fuse_views(int device, int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                   const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                   const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, int maps_on_device, const char *ply_path,
                   long long *num_points);
const char *apd_fusion_last_error(void);
/* Where the last apd_fuse_views of this thread spent its time (ms): set-up (allocations, uploads of host maps), the views (kernels,
 * consumption rounds, download of the points), the PLY file (release of the buffers + write). */
int apd_fusion_last_timing(double *setup_ms, double *views_ms, double *file_ms);

/* The reference's three fusion loops: RunFusion (ETH, APD.cpp:826-977), RunFusion_TAT_Intermediate (APD.cpp:979-1147) and
 * RunFusion_TAT_advanced (APD.cpp:1149-1296, Tanks and Temples). */
enum { APD_FUSION_ETH = 0, APD_FUSION_TAT_INTERMEDIATE = 1, APD_FUSION_TAT_ADVANCED = 2 };
/* apd_fuse_views with a choice of loop.  APD_FUSION_ETH is apd_fuse_views itself.  The two T&T variants read no weak maps
 * (`weaks` may be NULL), never consume source pixels (they mark only the reference pixels they emit), and keep the reference's
 * per-view `diff` entries: a source that is not valid at a pixel keeps the values of the last earlier pixel of the view, in
 * raster order, at which it was.  The point list is the one the sequential host loop writes.  An unknown variant or a view
 * that lists itself as a source is refused (APD_ERR_INVALID) and nothing is written.  apd_fusion_last_error /
 * apd_fusion_last_timing report on it like on apd_fuse_views. */
int apd_fuse_views_variant(int variant, int device, int num_views, const apd_camera *cameras, const float *const *images,
                           int image_channels, const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                           const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets,
                           const int *pair_indices, int maps_on_device, const char *ply_path, long long *num_points);

/* Options of one fusion call.  The acceptance rule of the ETH loop (APD.cpp:941-951) as values instead of literals, and the
 * form of the result.  apd_fusion_default_options sets struct_size and today's behaviour: with it, apd_fuse_views_opt writes
 * the bytes apd_fuse_views_variant writes.  A vote needs reprojection error < max_reproj_error (pixels), relative depth
 * difference < max_relative_depth and normal angle < max_angle (radians); it adds exp(-(reproj + depth_weight * depth +
 * angle_weight * angle)) to the consistency; a pixel becomes a point with at least min_consistent votes and consistency >
 * factor * votes, factor_strong for a STRONG / UNKNOWN pixel and factor_weak for a WEAK one.  The eight values apply to
 * APD_FUSION_ETH only: the Tanks and Temples loops keep their own ladder of thresholds that grow with the round k, and a T&T
 * variant with any of the eight off its default is refused (APD_ERR_UNSUPPORTED).  The output options apply to all three. */
typedef struct apd_fusion_options {
    size_t struct_size;           /* sizeof(apd_fusion_options) of the caller's header: first, so that the struct can grow */
    int    variant;               /* APD_FUSION_ETH | _TAT_INTERMEDIATE | _TAT_ADVANCED */
    float  max_reproj_error;      /* 2.0      */
    float  max_relative_depth;    /* 0.01     */
    float  max_angle;             /* 0.174533 */
    float  depth_weight;          /* 200      */
    float  angle_weight;          /* 10       */
    int    min_consistent;        /* 1; 1 .. APD_MAX_IMAGES */
    float  factor_strong;         /* 0.3      */
    float  factor_weak;           /* 0.45     */
    int    ply_normals;           /* 0: 15-byte records x y z + colour; 1: x y z nx ny nz + colour, 27 bytes */
    int    result_on_device;      /* where the arrays of an apd_points_t live: 0 host memory, 1 device memory on `device` */
} apd_fusion_options;
void apd_fusion_default_options(apd_fusion_options *o);

/* The points of one fusion as a structure of arrays, in the order of the PLY file: views in order, pixels of a view in raster
 * order.  Point k has
 *   xyz      3 floats: the reference pixel's lifted point (the reference averages only colour; apd_points_average gives the mean);
 *   normal   3 floats: the reference pixel's normal as given in normals[view], copied, not renormalised;
 *   bgr      3 bytes: the colour of the PLY record;
 *   support  1 byte: the votes the point was accepted with (ETH: num_consistent >= min_consistent; T&T: `count` of the round
 *            that emitted it);
 *   view, pixel   int32 each: the index of the reference view and the raster index row * cols + col in it;
 *   sources  uint32: which sources those votes are.  Bit j is set when the j-th source of the point's view, in pair.txt order
 *            (view pair_indices[pair_offsets[view] + j] of the call), is one of them -- the convention of the selected views of
 *            apd_download.  ETH: the votes that survived the consumption of source pixels, the ones support counts and the
 *            colour is averaged over; T&T: the sources counted in `count` of the emitting round.  popcount(sources) == support.
 * The arrays are host memory, or device memory on the call's device when options.result_on_device was set (then nothing is
 * downloaded unless a PLY file is asked for as well).  They belong to the object and live until apd_points_destroy; an accessor
 * of an object without points may return NULL. */
typedef struct apd_points *apd_points_t;
long long apd_points_count(apd_points_t p);
int apd_points_on_device(apd_points_t p);
const float *apd_points_xyz(apd_points_t p);
const float *apd_points_normal(apd_points_t p);
const uint8_t *apd_points_bgr(apd_points_t p);
const uint8_t *apd_points_support(apd_points_t p);
const int32_t *apd_points_view(apd_points_t p);
const int32_t *apd_points_pixel(apd_points_t p);
const uint32_t *apd_points_sources(apd_points_t p);
/* The views that see each point, as lists in compressed form: *offsets has count + 1 entries, point k has
 * (*views)[(*offsets)[k] .. (*offsets)[k + 1]): first its own reference view view[k], then its agreeing sources as indices of views
 * of the fusion call, in ascending bit order of sources[k] -- support[k] + 1 entries.  The object keeps a copy of the call's
 * pair_offsets / pair_indices for this.  The two arrays are built on the first call and kept; they live where the points live
 * (device-resident points: built on the device, offsets by a 64-bit scan over all points, since a large run has more than 2^31
 * entries) and belong to the object.  An object without points gives *offsets = {0}.  NULL for any argument: APD_ERR_INVALID;
 * the message is apd_fusion_last_error's. */
int apd_points_visibility(apd_points_t p, const long long **offsets, const int32_t **views);
/* Writes the lists as COLMAP's fused.ply.vis (what its Delaunay mesher and Poisson trimming read beside fused.ply), little
 * endian: uint64 number of points, then per point uint32 n and n x uint32 view index -- the entries of apd_points_visibility,
 * i.e. positions of views in the fusion call.  Host- or device-resident points.  NULL p or path: APD_ERR_INVALID; a file that
 * cannot be written: APD_ERR_IO. */
int apd_points_write_vis(apd_points_t p, const char *path);
/* Mean geometry: a new points object with p's points in p's order, each with the mean of the points and of the normals of the views
 * that agree on it -- what fusibile, ACMM's RunFusion and COLMAP's stereo fusion emit; p itself, like every fusion call, keeps the
 * reference pixel's.  cameras, depths, normals, rows, cols, maps_on_device: as in the fusion call that made p (the same maps, or
 * others of the same sizes, e.g. filtered ones); the images, weak maps and block masks are not needed.  Point k with position P =
 * xyz[k], normal n, view v and mask m = sources[k]: for every set bit j of m in ascending order, s = pair_indices[pair_offsets[v]
 * + j]; P is projected into view s exactly as the fusion projected it (APD.cpp:896-899); a source whose pixel lies outside the
 * view or has depth <= 0 there is skipped; otherwise the pixel's lifted point (Get3DPointonWorld) and its normal are added to
 * sums that start from P and n.  The result has xyz = sum / (used + 1), normal = the mean normal renormalised ((0, 0, 0) when its
 * length is 0 or NaN), sources = the bits that were not skipped, support = their number `used`; bgr, view and pixel are copied.
 * binary32 in that fixed order (contract C9).  With the maps of the ETH fusion that made p nothing is skipped and sources and
 * support come back unchanged; a Tanks and Temples point may name a source through a stale `diff` entry that its own projection
 * does not reach: that source is skipped by the rule above.  The object lives where p lives (host memory, or device memory on
 * p's device), carries p's source lists on (apd_points_visibility and apd_points_write_vis work on it and list the views that were
 * kept) and is released with apd_points_destroy.  The mean is computed on p's device, whatever memory p and the maps are in
 * (host-resident points and host maps are uploaded, the result is downloaded); an object without points gives an object without
 * points.  Refused with APD_ERR_INVALID before any device is touched, message "apd_points_average: ..." (apd_fusion_last_error):
 * a NULL argument, num_views, rows[i] or cols[i] other than the fusion call's, a NULL depths[s] or normals[s] for a view s that
 * some source list names.  *out is untouched when the call fails. */
int apd_points_average(apd_points_t p, int num_views, const apd_camera *cameras, const float *const *depths,
                       const float *const *normals, const int *rows, const int *cols, int maps_on_device, apd_points_t *out);
/* The PLY file of any points object, a fusion's or an averaged one: the header and the records of ExportPointCloud (APD.cpp:214-254)
 * as the fusion writes them, x y z + colour (15 bytes) or with_normals != 0: x y z nx ny nz + colour (27 bytes).  For the points
 * of a fusion call these are the bytes that call writes to its ply_path with the same ply_normals.  Host- or device-resident
 * points.  `element vertex` is printed from the 64-bit count.  NULL p or path: APD_ERR_INVALID; a file that cannot be written:
 * APD_ERR_IO. */
int apd_points_write_ply(apd_points_t p, const char *path, int with_normals);
/* A points object from a PLY file: the way back from apd_points_write_ply, and the way in of a cloud made elsewhere -- the ground
 * truth ETH3D and Tanks and Temples ship -- so that it can be searched, filtered and scored like one that was fused here.  Host
 * code.  Read: a `format binary_little_endian 1.0` file whose `element vertex` has float (float32) properties x, y and z; float nx,
 * ny, nz when all three are there (otherwise every normal is 0, 0, 0); uchar (uint8) red, green, blue or diffuse_red,
 * diffuse_green, diffuse_blue when all three are there (otherwise every colour is 0, 0, 0).  Any other scalar property of a
 * vertex is skipped by the size of its type, the properties may stand in any order, `comment` and `obj_info` lines and every
 * element after `vertex` (the faces of a mesh) are ignored.  The object names one view of 1 x 1 pixels without sources: support,
 * view, pixel and sources are 0 for every point, which are apd_points_create's rules.  on_device != 0: device memory on `device`;
 * otherwise host memory, no device is touched and the call works on a machine without a GPU.
 * Refused with a message "apd_points_read_ply: <path>: <reason>" (apd_fusion_last_error).  APD_ERR_INVALID: a NULL argument (no
 * path in the message), a file that does not start with `ply`, a format other than binary_little_endian 1.0 (ascii, big endian), a
 * list property in `element vertex`, a missing or non-float coordinate, an element before `vertex`, no `element vertex`, an unknown
 * header line or type.  APD_ERR_IO: a file that cannot be read, that ends inside its header or before its vertices do.  *out is
 * untouched when the call fails. */
int apd_points_read_ply(const char *path, int device, int on_device, apd_points_t *out);
/* A points object from caller arrays: a cloud that was not fused in this call, to be merged, listed or written like one that
 * was.  The arrays are HOST pointers with the layout of the accessors above (xyz and normal 3 floats, bgr 3 bytes per point) and
 * are copied; rows, cols, pair_offsets (num_views + 1 entries) and pair_indices are those of a fusion call and say what view,
 * pixel and the bits of sources mean.  on_device != 0: the copy is device memory on `device`; otherwise it is host memory and no
 * device is touched -- with the host paths of apd_points_visibility, apd_points_write_vis and apd_points_write_ply such an object
 * works on a machine without a GPU.  Refused with APD_ERR_INVALID before anything is allocated, message "apd_points_create: ..."
 * (apd_fusion_last_error): a NULL argument (count == 0 may pass NULL arrays, and pair_indices may be NULL when no view has a
 * source), a negative count, num_views < 1, a rows or cols entry that is not positive, pair_offsets not ascending from 0, a
 * pair_indices entry outside 0 .. num_views - 1 or equal to its own view, a source list longer than APD_MAX_IMAGES, a view[k]
 * outside the views, a pixel[k] outside its view, a bit of sources[k] at or above the length of its view's source list,
 * popcount(sources[k]) != support[k].  *out is untouched when the call fails. */
int apd_points_create(int device, int on_device, long long count, const float *xyz, const float *normal, const uint8_t *bgr,
                      const uint8_t *support, const int32_t *view, const int32_t *pixel, const uint32_t *sources, int num_views,
                      const int *rows, const int *cols, const int *pair_offsets, const int *pair_indices, apd_points_t *out);
/* One point per occupied cell of a cubic grid, with the union of the members' visibility lists: the form COLMAP's fusion gives
 * (one point per surface element with all the views that see it) and its Delaunay mesher reads.  binary32, IEEE operations in
 * the order given (contract C10; csrc/apd_voxel_math.h).
 *   Cell and key.  Per axis c: t = (xyz[c] - origin[c]) / voxel_size (a subtraction, then a division), f = floorf(t).  A point is
 *   DROPPED when for any axis f is not in [-1048576, 1048576) -- NaN fails the test, so points with a non-finite coordinate are
 *   dropped; *dropped (may be NULL) receives their number.  Otherwise i_c = (int)f and the key is
 *   ((iz + 2^20) << 42) | ((iy + 2^20) << 21) | (ix + 2^20).
 *   Output.  One point per distinct key, in ascending key order.  The members of a cell are taken in ascending input index; a
 *   merged point with m members and representative r (the first member) has
 *     xyz      per component the binary32 sum of the members' values in member order, starting from r's, divided by (float)m;
 *     normal   the same sum and division, then renormalised by the rule of apd_points_average (left-to-right sum of squares,
 *              sqrtf, (0, 0, 0) when the length is 0 or NaN);
 *     bgr      per channel (sum + m / 2) / m in unsigned 64-bit integers;
 *     view, pixel, sources   those of r, copied.  They describe r ALONE: sources does not name the views of the list below;
 *     support  min(255, L - 1), L the length of the list below.
 *   Visibility.  The list of a merged point holds the distinct views of the union of its members' lists, ascending; the
 *   members' lists are the input's apd_points_visibility lists (not its sources bits, so a merged object can be merged again on
 *   a coarser grid).  The result carries these lists as its own: apd_points_visibility and apd_points_write_vis return them,
 *   apd_points_write_ply writes the merged points.
 * The means are unweighted: merging a merged object again weighs every earlier cell as one point, whatever it had absorbed.
 * apd_points_average refuses a merged object (APD_ERR_INVALID, "merged points name no sources").
 * The result lives where p lives and is released with apd_points_destroy.  The merge is computed on p's device whatever memory p
 * is in (host-resident points and lists are uploaded, the result is downloaded); there is no host implementation.  An object
 * without points gives an object without points, with no device touched.  Refused, message "apd_points_merge_voxels: ...":
 * APD_ERR_INVALID for a NULL p or out, a voxel_size that is not finite or not above 0, a non-finite origin component (origin3
 * NULL: 0, 0, 0); APD_ERR_UNSUPPORTED for 2^31 or more points (the sort carries a 32-bit index) or 2^32 or more list entries in
 * total.  All of these before any device is touched, but for the entry total of device-resident points, which is known once
 * their lists are built on their device.  *out and *dropped are untouched when the call fails.  apd_fusion_last_timing reports
 * the call: set-up (uploads, allocations), the kernels (and the download of a host result) as "views", file 0. */
int apd_points_merge_voxels(apd_points_t p, float voxel_size, const float *origin3, apd_points_t *out, long long *dropped);
int apd_points_merged(apd_points_t p);   /* 1 for a result of apd_points_merge_voxels (or of a removal from one), else 0 */
/* Neighbours within a radius, and the removal of points that have too few of them: the radius outlier filter that is run between
 * fusion and meshing, here on the points object, so that sources, support, view / pixel and the visibility lists survive it.
 * binary32, IEEE operations in the order given (contract C11; csrc/apd_radius_math.h).
 *   Grid.  Cubic, cell size `radius`, origin origin3 (NULL: 0, 0, 0); the cell of a point on each axis is that of
 *   apd_points_merge_voxels.  A point that the merge would drop (a non-finite coordinate, a cell outside [-2^20, 2^20)) is outside
 *   the grid: it has no neighbours and is nobody's neighbour.
 *   Neighbour.  Point j is a neighbour of point i when j != i as indices (coincident points are each other's neighbours), both
 *   are inside the grid, their cells differ by at most 1 on every axis, and (dx * dx + dy * dy) + dz * dz <= radius * radius
 *   with dx = x_i - x_j and so on.  The cell condition is part of the definition: the search of the 27 cells around a point is
 *   exact, not an approximation; in real arithmetic it follows from the distance test, in binary32 it can only turn away a pair
 *   within the rounding of the cell quotient (2^-24 of a cell near the origin, about 1/8 at cell 2^20) of exactly one radius apart.
 *   counts[i] = min(neighbours of i, cap); cap == 0: no cap.  Kept by apd_points_remove_sparse: the points with at least
 *   min_neighbours neighbours; min_neighbours == 0 keeps every point, those outside the grid too.
 * apd_points_neighbour_counts: `counts` has apd_points_count(p) entries, host memory for host-resident points, device memory on
 * p's device for device-resident ones.
 * apd_points_remove_sparse: *out is a new object with the kept points in p's order, every array copied; *removed (may be NULL)
 * the number of points left out.  The result of a fusion's or an averaged object carries its source lists and view sizes on:
 * apd_points_visibility, apd_points_write_vis and apd_points_average work on it as on p.  The result of a merged object is a merged
 * object (apd_points_merged) with the kept points' lists.  It lives where p lives and is released with apd_points_destroy.
 * Both are computed on p's device, on its null stream, whatever memory p is in (host-resident points are uploaded, the result is
 * downloaded); there is no host implementation.  An object without points gives no counts, or an object without points, with no
 * device touched.  The work is the number of (point, candidate in the 27 cells around it) pairs: with cap == 0 a cell of m
 * members costs m * m distance tests, one lane per point; the removal runs with cap = min_neighbours and leaves a dense
 * neighbourhood after that many hits.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_neighbour_counts: ..." or
 * "apd_points_remove_sparse: ..." (apd_fusion_last_error): a NULL p, a NULL counts or out, a radius that is not finite or not
 * above 0, a radius whose square is not finite or is zero, a non-finite origin component; APD_ERR_UNSUPPORTED for 2^31 or more
 * points (the sort carries a 32-bit index).  *out and *removed are untouched when the call fails. */
int apd_points_neighbour_counts(apd_points_t p, float radius, const float *origin3, unsigned cap, uint32_t *counts);
int apd_points_remove_sparse(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, apd_points_t *out,
                             long long *removed);
/* The mean distance to the k nearest neighbours, and the removal of the points whose value is an outlier of the cloud's own
 * distribution of it: the statistical outlier filter that is run between fusion and meshing (PCL's StatisticalOutlierRemoval,
 * Open3D's remove_statistical_outlier), here on the points object, so that sources, support, view / pixel and the visibility lists
 * survive it.  IEEE operations in the order given (contract C12; csrc/apd_knn_math.h).
 *   Neighbours.  Those of apd_points_neighbour_counts, on the grid of cell size `radius` at origin3 (NULL: 0, 0, 0): the search is
 *   bounded by the radius, which keeps it exact and bounds the work of an isolated point.
 *   Score.  mean[i] of a point with at least k neighbours: the k smallest (dx * dx + dy * dy) + dz * dz over its neighbours,
 *   sqrtf of each, summed in ascending order in binary32 from 0, divided by (float)k.  With fewer than k neighbours -- an isolated
 *   point, a point outside the grid --: +inf.  k is 1 .. 64.
 *   Threshold.  Over the points with a finite score, in input order, in binary64: n_f their number, S1 the sum of the scores and
 *   S2 of their squares, each summed in chunks of 256 consecutive input indices (a chunk sequentially from 0, then the chunk
 *   sums sequentially); mu = S1 / n_f, var = (S2 - S1 * S1 / n_f) / (n_f - 1) clamped below at 0 (0 for n_f < 2),
 *   T = mu + (double)std_ratio * sqrt(var); n_f == 0: T = 0.
 *   Kept by apd_points_remove_statistical: the points with a finite score and (double)score <= T, in p's order.
 * apd_points_knn_mean_distances: `mean` has apd_points_count(p) entries, host memory for host-resident points, device memory on
 * p's device for device-resident ones.
 * apd_points_remove_statistical: *out is a new object with the kept points, every array copied, and carries what the result of
 * apd_points_remove_sparse carries (source lists and view sizes; a merged object gives a merged object with the kept points'
 * lists); *removed (may be NULL) the number of points left out, *threshold (may be NULL) T.  std_ratio may be zero or negative.
 * Both are computed on p's device, on its null stream, whatever memory p is in; there is no host implementation.  The scores of
 * device-resident points never leave the device for the removal: n / 256 chunk sums do.  An object without points gives no
 * scores, or an object without points and T = 0, with no device touched.  The work is that of apd_points_neighbour_counts
 * without a cap plus the selection: k LDS reads for every candidate that displaces one of the k held.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_knn_mean_distances: ..." or
 * "apd_points_remove_statistical: ..." (apd_fusion_last_error): what apd_points_neighbour_counts refuses, a k outside 1 .. 64, a
 * std_ratio that is not finite; APD_ERR_UNSUPPORTED for 2^31 or more points.  *out, *removed and *threshold are untouched when
 * the call fails. */
int apd_points_knn_mean_distances(apd_points_t p, float radius, const float *origin3, unsigned k, float *mean);
int apd_points_remove_statistical(apd_points_t p, float radius, const float *origin3, unsigned k, float std_ratio,
                                  apd_points_t *out, long long *removed, double *threshold);
/* The connected components of the points within a radius of each other, and the removal of the small ones: the filter that is run
 * after the radius and the statistical filter (PCL's EuclideanClusterExtraction, Open3D's cluster_dbscan and a size cut, MeshLab's
 * "remove isolated pieces"), here on the points object, so that sources, support, view / pixel and the visibility lists survive it.
 * A detached clump of 200 points passes both other filters, which judge a point by its own neighbourhood; this one judges the clump.
 * Integers only (contract C13; csrc/apd_points_clusters.hip).
 *   Graph.  The vertices are the points of p.  Points i and j share an edge exactly when they are neighbours by the relation of
 *   apd_points_neighbour_counts, on the grid of cell size `radius` at origin3 (NULL: 0, 0, 0); the relation is symmetric.  A point
 *   outside the grid has no edges.
 *   Component.  A connected component of that graph; a point outside the grid is a component of its own.
 *   label[i] is the smallest index among the points of i's component, size[i] their number (below 2^31).  Both are functions of
 *   the input alone: no visiting order, launch shape or race outcome shows in them.
 *   Kept by apd_points_remove_small_components: the points with size[i] >= min_size, in p's order.  min_size 0 and 1 keep every
 *   point, those outside the grid too; from 2 on a point outside the grid goes.
 * apd_points_components: `label` and `size` have apd_points_count(p) entries each, host memory for host-resident points, device
 * memory on p's device for device-resident ones; `size` may be NULL, `label` may not.  *components (may be NULL) receives the
 * number of components, which is the number of i with label[i] == i.
 * apd_points_remove_small_components: *out is a new object with the kept points, every array copied, and carries what the result
 * of apd_points_remove_sparse carries (source lists and view sizes; a merged object gives a merged object with the kept points'
 * lists); *removed (may be NULL) the number of points left out, *components (may be NULL) the number of components of p.  With
 * min_size <= 1 and components == NULL nothing is labelled.
 * Both are computed on p's device, on its null stream, whatever memory p is in; there is no host implementation.  An object
 * without points gives no labels, or an object without points, and *components = 0, with no device touched.  The work is half
 * the distance tests of apd_points_neighbour_counts without a cap, plus a concurrent union-find over the edges found.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_components: ..." or
 * "apd_points_remove_small_components: ..." (apd_fusion_last_error): what apd_points_neighbour_counts refuses;
 * APD_ERR_UNSUPPORTED for 2^31 or more points.  *out, *removed and *components are untouched when the call fails. */
int apd_points_components(apd_points_t p, float radius, const float *origin3, uint32_t *label, uint32_t *size, long long *components);
int apd_points_remove_small_components(apd_points_t p, float radius, const float *origin3, unsigned min_size, apd_points_t *out,
                                       long long *removed, long long *components);
/* Normals and surface variation from each point's neighbourhood: the step a Poisson mesher depends on (PCL's NormalEstimation,
 * Open3D's estimate_normals), here on the points object, so that sources, support, view / pixel and the visibility lists survive
 * it.  The stored normal -- the PatchMatch normal of one pixel, or a mean of such -- only chooses the sign.  IEEE operations in
 * the order given (contract C14; csrc/apd_normal_math.h).
 *   Neighbours.  Those of apd_points_neighbour_counts, on the grid of cell size `radius` at origin3 (NULL: 0, 0, 0).
 *   Estimate.  A point with at least min_neighbours neighbours (itself not counted; min_neighbours is 2 .. 2^31 - 1): over the
 *   point and its neighbours in ascending (cell, index) order, with d = Q - P in binary32, the binary64 sums n, of d and of the
 *   six products d_a * d_b; the covariance C_ab = S_ab / n - (S_a / n) * (S_b / n); its eigenvalues l0 <= l1 <= l2 (clamped
 *   below at 0) and vectors by cyclic Jacobi rotations in binary64, in the order (0,1), (0,2), (1,2), at most 5 sweeps.  The
 *   normal is the eigenvector of l0 (the lowest column among equal eigenvalues), renormalised, flipped when its binary64 dot
 *   product with the stored normal is < 0; when that product is neither < 0 nor > 0 (a zero, NaN or orthogonal stored normal)
 *   its first non-zero component is made positive; converted to binary32 last.  variation = (float)(l0 / (l0 + l1 + l2)), the
 *   "surface variation", between 0 (a plane) and 1/3; 0 when the sum is 0 (coincident points).
 *   No estimate.  A point with fewer neighbours and a point outside the grid: its normal is the stored normal, copied, and its
 *   variation +inf.  A result is never NaN unless the stored normal was.
 * apd_points_estimate_normals: normal3 takes 3 * apd_points_count(p) floats and variation apd_points_count(p), host memory for
 * host-resident points, device memory on p's device for device-resident ones; either may be NULL, not both.
 * apd_points_with_estimated_normals: *out is a new object with p's points in p's order, every array copied and `normal`
 * replaced; it lives where p lives, is merged when p is and then carries p's lists; *estimated (may be NULL) is the number of
 * points that got an estimate.  p is left as it is.
 * Both are computed on p's device, on its null stream, whatever memory p is in; there is no host implementation.  An object
 * without points gives no results, or an object without points and *estimated = 0, with no device touched.  The work is that of
 * apd_points_neighbour_counts without a cap, with sixteen binary64 operations per neighbour, plus one eigen-solve per point.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_estimate_normals: ..." or
 * "apd_points_with_estimated_normals: ..." (apd_fusion_last_error): what apd_points_neighbour_counts refuses, both of normal3
 * and variation NULL, a min_neighbours outside 2 .. 2^31 - 1; APD_ERR_UNSUPPORTED for 2^31 or more points.  *out and *estimated
 * are untouched when the call fails. */
int apd_points_estimate_normals(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *normal3,
                                float *variation);
int apd_points_with_estimated_normals(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, apd_points_t *out,
                                      long long *estimated);
/* Smoothed positions: every point projected on the weighted least-squares plane of its neighbourhood, the step that takes the
 * depth noise along the viewing ray out of a cloud before a Poisson or Delaunay mesher (PCL's MovingLeastSquares, CloudCompare,
 * MeshLab), here on the points object, so that sources, support, view / pixel and the visibility lists survive it.  The only step
 * that moves a point.  IEEE operations in the order given (contract C16; csrc/apd_smooth_math.h).
 *   Neighbours.  Those of apd_points_neighbour_counts, on the grid of cell size `radius` at origin3 (NULL: 0, 0, 0).
 *   Estimate.  A point at P with at least min_neighbours neighbours (itself not counted; min_neighbours is 2 .. 2^31 - 1): over
 *   the point and its neighbours in ascending (cell, index) order, a term at Q has the weight w = t * t with t = 1 - d2 / r2 in
 *   binary64, d2 the binary32 squared distance and r2 = radius * radius in binary32 -- 1 for the point itself, 0 at exactly the
 *   radius -- and, with d = Q - P in binary32, the binary64 sums W of w, s of w * d and S of the six (w * d_a) * d_b.  The plane's
 *   normal is that of apd_points_estimate_normals on these sums with n = W (the same solve, the same cap of 5 sweeps, signed like
 *   the stored normal), as binary32.  With m = s / W and that normal n: h = (m_0 n_0 + m_1 n_1) + m_2 n_2; the new position is
 *   (float)(P_a + h * n_a) and the offset (float)h, the signed distance moved along the returned normal.  |h| <= radius.
 *   No estimate.  A point with fewer neighbours and a point outside the grid: its position is copied bit for bit and its offset
 *   is +inf.
 *   Iterations.  Simultaneous: iteration k takes every position from iteration k - 1, with the grid and the cell order rebuilt
 *   from them; the stored normal stays p's own.  A point that moves out of the grid stays where it then is.
 * apd_points_smoothed_positions: one iteration.  xyz3 takes 3 * apd_points_count(p) floats and offset apd_points_count(p), host
 * memory for host-resident points, device memory on p's device for device-resident ones; either may be NULL, not both.
 * apd_points_with_smoothed_positions: `iterations` is 1 .. 16.  *out is a new object with p's points in p's order, every array
 * copied and `xyz` replaced by the positions after the last iteration; it lives where p lives, is merged when p is and then
 * carries p's lists; *moved (may be NULL) is the number of points that had an estimate in at least one iteration.  p is left as
 * it is.  Host-resident points go up once and the result comes down once.
 * Both are computed on p's device, on its null stream, whatever memory p is in; there is no host implementation.  An object
 * without points gives no results, or an object without points and *moved = 0, with no device touched.  The work per iteration
 * is that of apd_points_estimate_normals at the same radius, with one binary64 division and a few multiplications more per
 * neighbour.  Plane projection shrinks a curved surface towards its centre of curvature by about the sagitta of the
 * neighbourhood, radius^2 / (2 R) and less, per iteration: choose the radius and the iterations with that in mind.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_smoothed_positions: ..." or
 * "apd_points_with_smoothed_positions: ..." (apd_fusion_last_error): what apd_points_neighbour_counts refuses, both of xyz3 and
 * offset NULL, a min_neighbours outside 2 .. 2^31 - 1, iterations outside 1 .. 16; APD_ERR_UNSUPPORTED for 2^31 or more points.
 * *out and *moved are untouched when the call fails. */
int apd_points_smoothed_positions(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *xyz3, float *offset);
int apd_points_with_smoothed_positions(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, unsigned iterations,
                                       apd_points_t *out, long long *moved);
/* The nearest point of another cloud, and from it precision, recall and F-score: the first query that relates two points objects.
 * How close a fused cloud is to a ground truth and how much of the ground truth it covers is what accuracy, completeness and
 * F-score of Tanks and Temples measure, and what the radii and thresholds of every filter above can be chosen by.  IEEE operations
 * in the order given (contract C17; csrc/apd_nearest_math.h).
 *   Grid.  That of apd_points_neighbour_counts, cell size `radius` at origin3 (NULL: 0, 0, 0), for both clouds.  A point outside it
 *   (a non-finite coordinate, a cell beyond +-2^20) has no nearest point and is nobody's nearest point.
 *   Candidates.  Those of point i of p are the points j of q inside the grid whose cell differs from i's by at most 1 on every axis
 *   and whose binary32 squared distance d2 = (dx * dx + dy * dy) + dz * dz is <= radius * radius.  As for the neighbour counts the
 *   cell condition is part of the definition.  p and q may be the same object: a point is then its own candidate.
 *   Nearest.  The candidate with the least d2, among equal d2 the smallest index j.  distance[i] = sqrtf(d2), index[i] = j; without
 *   a candidate +inf and -1.  A distance is finite exactly when some point of q is within the radius.
 * apd_points_nearest: distance and index take apd_points_count(p) entries each, host memory for a host-resident p, device memory
 * on p's device for a device-resident one; either may be NULL, not both.  Computed on p's device, on its null stream, whatever
 * memory p is in; there is no host implementation.  A host-resident q goes up for the call; a device-resident q must live on
 * that device (APD_ERR_UNSUPPORTED otherwise, before any device is touched).  A p without points gives no results with no device
 * touched; a q without points, or without a point inside the grid, gives +inf and -1 throughout.  The work is the number of
 * (point of p, point of q in the 27 cells around it) pairs, plus one sort of each cloud.
 * apd_points_score: p against `truth` at radius = threshold, so that "finite" is "within the threshold".  With a the number of
 * finite distances from p to truth and b that from truth to p, both searches from one pair of sorts:
 *   n_p, n_q       the points of p and of truth, those outside the grid too
 *   p_within, q_within   a and b
 *   precision      (double)a / (double)n_p, 0 when n_p is 0: the share of p that has truth within the threshold (accuracy)
 *   recall         (double)b / (double)n_q, 0 when n_q is 0: the share of truth that has p within the threshold (completeness)
 *   fscore         2 * precision * recall / (precision + recall), 0 when the sum is 0
 *   mean_p, mean_q the mean finite distance from p to truth and from truth to p: binary64 sums over chunks of 256 consecutive
 *                  indices as in apd_points_remove_statistical, divided by a and by b; 0 when there is none
 * Of the distances only the chunk sums leave the device.  When either object has no points the counts are set, the rest is 0 and
 * no device is touched.  This is nearest-neighbour precision / recall at one threshold as Tanks and Temples defines them, without
 * its registration and cropping and without ETH3D's occlusion-aware evaluation: scores of two runs compare with each other.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_nearest: ..." or "apd_points_score: ..."
 * (apd_fusion_last_error): what apd_points_neighbour_counts refuses, for either object (the threshold is the radius), a NULL q or
 * truth, both of distance and index NULL, a NULL out; APD_ERR_UNSUPPORTED for 2^31 or more points in either.  *out is untouched
 * when the call fails. */
typedef struct {
    long long n_p, n_q, p_within, q_within;
    double precision, recall, fscore, mean_p, mean_q;
} apd_points_score_t;
int apd_points_nearest(apd_points_t p, apd_points_t q, float radius, const float *origin3, float *distance, int32_t *index);
int apd_points_score(apd_points_t p, apd_points_t truth, float threshold, const float *origin3, apd_points_score_t *out);
/* Alignment to another cloud, and the points moved by a transform.  A reconstruction stands in the arbitrary frame and scale of
 * its structure-from-motion model and a ground truth in its scanner's; the Tanks and Temples protocol registers the two, refines
 * with ICP and then computes the precision / recall of apd_points_score.  apd_points_align is that refinement: point-to-point ICP,
 * rigid or with a scale, bounded by a radius; apd_points_transformed applies its answer, or any similarity transform, to the
 * points object, so that sources, support, view / pixel and the visibility lists survive.  IEEE operations in the order given
 * (contract C18; csrc/apd_align_math.h), binary64 with + - * / and sqrt alone.
 *   Step k = 0, 1, .. on the positions X_k of p; X_0 is p's own.
 *   Matches.  apd_points_nearest of X_k in q at `radius` and origin3, as it stands: a point without a candidate has no match.
 *   Sums.  Over the matched points, p a point of X_k and q its match, coordinates converted to binary64: their number m, the sums
 *   of p and of q, and of |p - q|^2; then, about the means pm and qm, the nine sums of (p - pm)_a (q - qm)_b and that of |p - pm|^2.
 *   Each is taken per chunk of 256 consecutive indices of p by a fixed pairwise tree (csrc/apd_align_math.h) and the chunk sums are
 *   added in ascending order.  rms_k = sqrt(sum |p - q|^2 / m).
 *   Solve.  Horn's closed form: the 4 x 4 symmetric matrix of the nine sums, diagonalised by cyclic Jacobi (at most 16 sweeps); the
 *   eigenvector of the largest eigenvalue is the rotation's quaternion, taken with w >= 0 and normalised: always a proper
 *   rotation.  The step's scale is 1, or with_scale sum (q - qm) . R (p - pm) / sum |p - pm|^2; its translation qm - scale R pm.
 *   Total.  The step is applied after the total of the steps before it, in binary64 on the host; X_{k+1} is X_0 moved by the
 *   total, x' = (float)(((m_0 x + m_1 y) + m_2 z) + t) per component with m = scale * R, so that no rounding accumulates.
 *   Stop.  After opt->iterations steps (1 .. 64; APD_ALIGN_ITERATIONS), or before step k when m < 3 or sum |p - pm|^2 == 0
 *   (APD_ALIGN_TOO_FEW), or when k > 0 and |rms_k - rms_(k-1)| <= opt->tolerance * rms_(k-1) (APD_ALIGN_CONVERGED).
 * apd_points_align: *out is the total (x' = scale * rotation x + translation, rotation row-major, takes p onto q), the number of
 * matched points and their rms distance before any step and under the returned transform, the steps taken and why they ended.
 * It moves nothing.  opt NULL: 16 iterations, tolerance 1e-6, no scale.  K steps take K + 1 searches, each with one sort of p's
 * positions; q is sorted once.  Computed on p's device, on its null stream, whatever memory p is in; a host-resident q goes up
 * for the call, a device-resident q must live on that device.  Of the points only chunk sums leave the device.  p and q may be the
 * same object: the identity and rms 0.  When either has no points the answer is the identity, APD_ALIGN_TOO_FEW and 0 steps and
 * no device is touched.  ICP within a radius needs a start within about that radius of the answer: apd_points_register (below)
 * gives one from any start.
 * apd_points_transformed: *out is a new object with p's points in p's order, xyz replaced by scale * R x + t (the expression
 * above) and normal by R n, unscaled, in the same expression with t = +0.0, not renormalised; every other array is copied; it
 * lives where p lives, is merged when p is and then carries p's lists.  p is left as it is.  An object without points gives an
 * object without points with no device touched.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_align: ..." or "apd_points_transformed: ..."
 * (apd_fusion_last_error): what apd_points_nearest refuses; iterations outside 1 .. 64, a tolerance that is negative or not
 * finite; a NULL p, rotation9, translation3 or out, a number that is not finite, a scale <= 0, a rotation9 for which an entry of
 * R^T R, in binary64, differs from the identity's by more than 1e-6; APD_ERR_UNSUPPORTED for 2^31 or more points.  *out is
 * untouched when a call fails. */
enum { APD_ALIGN_ITERATIONS = 0, APD_ALIGN_CONVERGED = 1, APD_ALIGN_TOO_FEW = 2 };
typedef struct {
    unsigned iterations;
    double tolerance;
    int with_scale;
} apd_points_align_options;
typedef struct {
    double scale, rotation[9], translation[3];
    long long matched_before, matched_after;
    double rms_before, rms_after;
    int steps, stopped;
} apd_points_alignment_t;
int apd_points_align(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_align_options *opt,
                     apd_points_alignment_t *out);
int apd_points_transformed(apd_points_t p, double scale, const double *rotation9, const double *translation3, apd_points_t *out);
/* Alignment to another cloud's tangent planes: point-to-plane ICP, the refinement to prefer over apd_points_align once a start
 * within about a radius exists and q carries normals.  A fused cloud and a laser scan sample the same surfaces at different
 * points: point-to-point ICP pulls every point towards the nearest SAMPLE, converges slowly along the surface and settles with
 * the sampling offset as its residual; this call minimises the distances to the planes through the matched points of q
 * perpendicular to q's STORED normals, which lets p slide along the surface.  A q without normals gets them from
 * apd_points_with_estimated_normals first.  Rigid only.  IEEE operations in the order given (contract C20, DESIGN.md;
 * csrc/apd_align_plane_math.h), binary64 with + - * / and sqrt alone.
 *   Step k, matches, the total and the move: those of apd_points_align.  Its sums of pass 1 give m, the mean qm of the matches
 *   and the point rms, as there.
 *   Sums.  A matched point is usable when its match's normal n has a squared length, in binary64, that is finite and > 0; u is n
 *   over its length, and its sign plays no part.  With c = qm, x = p - c, y = q - c, a = x cross u, g = (a, u) and
 *   r = (x - y) . u: the 21 sums of g_i g_j (i <= j), the 6 of g_i r, those of r^2, of 1 (m_plane) and of |x|^2, through the same
 *   tree over chunks of 256.  The plane rms is sqrt(sum r^2 / m_plane).
 *   Solve.  (sum g g^T) z = -(sum g r) for z = (omega, tau) by LDL^T without pivoting, in binary64 on the host.  The geometry is
 *   degenerate when a pivot d_j fails d_j > 2^-20 * bound_j, bound_j = sum |x|^2 for the three rotations and m_plane for the
 *   three translations -- the largest value the entry can have: a plane, a cylinder along its axis, a sphere about its centre
 *   do not constrain every motion, and no step is invented for them.  The rotation is that of the quaternion
 *   (1, omega / 2) normalised, about c; the translation c + tau - R c.
 *   Stop.  After opt->iterations steps (APD_ALIGN_ITERATIONS); before step k when m < 3 or m_plane < 6 (APD_ALIGN_TOO_FEW); when
 *   k > 0 and |rms_k - rms_(k-1)| <= opt->tolerance * rms_(k-1), rms the point rms (APD_ALIGN_CONVERGED); when the solve is
 *   degenerate or a component of z not finite (APD_ALIGN_DEGENERATE): the total of the steps before it is returned.
 * *out begins with the fields of apd_points_alignment_t in their order and layout (scale is 1.0; rms_* are the point rms); then the
 * usable matches and the plane rms before any step and under the returned transform (0 and 0.0 when nothing is matched).  It
 * moves nothing: apd_points_transformed applies the answer.  opt NULL: 16 iterations, tolerance 1e-6.  Computed on p's device, on
 * its null stream, whatever memory p is in; a host-resident q goes up for the call, positions and normals; a device-resident q must
 * live on that device.  There is no host path.  p and q may be the same object.  When either has no points the answer is the
 * identity, APD_ALIGN_TOO_FEW and 0 steps and no device is touched.  Not here: a cropping volume, ETH3D's occlusion-aware
 * evaluation, robust kernels (every usable match weighs the same), the normals of p (only q's are read).
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_align_planes: ..." (apd_fusion_last_error): what
 * apd_points_align refuses.  *out is untouched when the call fails. */
enum { APD_ALIGN_DEGENERATE = 3 };
typedef struct {
    unsigned iterations;
    double tolerance;
} apd_points_align_planes_options;
typedef struct {
    double scale, rotation[9], translation[3];
    long long matched_before, matched_after;
    double rms_before, rms_after;
    int steps, stopped;
    long long planes_before, planes_after;
    double plane_rms_before, plane_rms_after;
} apd_points_plane_alignment_t;
int apd_points_align_planes(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_align_planes_options *opt,
                            apd_points_plane_alignment_t *out);
/* Global registration to another cloud: the first step of "register, refine with ICP, score" for a cloud that stands in an
 * arbitrary frame relative to the other, at a scale that is already about right.  FPFH descriptors from the STORED normals
 * (apd_points_with_estimated_normals gives a cloud that has none its normals), the nearest descriptor of the other cloud for
 * every point, RANSAC over those matches and a refit of the winning transform on its inliers by the solve of apd_points_align.
 * IEEE operations in the order given (contract C19; csrc/apd_register_math.h): + - * / and sqrt alone, no trigonometric
 * function anywhere.
 *   Descriptors.  A point has a frame when its normal's length is finite and > 0 and it lies inside the grid (cell size `radius`,
 *   origin3); its neighbours are those of apd_points_neighbour_counts at `radius` that have a frame.  Per (centre, neighbour) the
 *   Darboux frame and the three features of PCL's computePairFeatures, in binary64; a neighbour at the same position, or with
 *   the connecting line parallel to the source normal, is skipped.  Each feature falls into one of 11 bins: the two cosines
 *   linearly over [-1, 1], the angle over [-pi, pi) by comparing its (sine, cosine) pair with the ten edge directions.  SPFH: the
 *   three histograms over the k admitted neighbours divided by k; a point with k < min_neighbours (>= 3) has no descriptor.
 *   FPFH = SPFH + (1 / k) sum SPFH(neighbour) / d^2 over the admitted neighbours that have an SPFH, in the search's ascending
 *   order, each block of 11 divided by its own sum: 33 floats per point, 33 zeros and has = 0 for a point without a descriptor.
 *   Matches.  For a point of p with a descriptor the point of q with a descriptor at the least squared distance in the 33
 *   dimensions (binary32, ascending bins), the smallest index among equals; `mutual`: kept only when the match's match is the
 *   point itself.  index is the match's index in q (-1: none), distance the distance in the 33 dimensions (+inf: none).
 *   Trials.  Trial t = 0 .. trials - 1 draws three distinct matches from a counter-based generator keyed by (seed, t); it is
 *   admitted when each edge of the triangle has squared lengths on the two sides within edge_ratio^2 of each other and neither
 *   triangle is degenerate; its rigid transform is the solve of apd_points_align on the three pairs.  A match is an inlier of a
 *   transform when p's point, moved, lies within inlier_distance of q's.  The best trial has the most inliers, the lowest t among
 *   equals.
 *   Refit.  One solve of apd_points_align over the best trial's inlier pairs, with_scale the caller's choice (the scale is only
 *   refined: the trials are rigid); the inliers are counted once more under it, with their rms distance.
 * apd_points_features: features (33 per point) and has (may be NULL) in host or device memory by p's residence.
 * apd_points_match_features: index and distance (either may be NULL, not both), likewise.
 * apd_points_register: *out is the transform (x' = scale * rotation x + translation, takes p onto q; apd_points_transformed
 * applies it), the number of points with a descriptor on either side, of matches, of admitted trials, the best trial (-1: none)
 * and its inliers, the inliers and their rms distance under the returned transform, and how it ended: APD_REGISTER_OK;
 * APD_REGISTER_TOO_FEW_MATCHES with fewer than 3 matches; APD_REGISTER_NO_TRIAL when no trial is admitted or the best has fewer
 * than 3 inliers; both failures return the identity.  opt NULL: 4096 trials, seed 0, inlier_distance radius / 2, edge_ratio 0.9,
 * min_neighbours 5, mutual, no scale.  The same call gives the same bits.  Computed on p's device, on its null stream; a
 * host-resident q goes up for the call, a device-resident q must live on that device.  The index array and the positions come to
 * the host for the trials; of the trials only the admitted transforms go up and the counts come down.  When either object has no
 * points the answer is the identity and APD_REGISTER_TOO_FEW_MATCHES and no device is touched.
 * The cost of matching is the product of the two numbers of descriptors: registration is done on a thinned cloud
 * (apd_points_merge_voxels).  Not here: a cropping volume, ETH3D's occlusion-aware evaluation.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_features: ...", "apd_points_match_features:
 * ..." or "apd_points_register: ..." (apd_fusion_last_error): what apd_points_neighbour_counts refuses for either object, a
 * min_neighbours < 3, trials outside 1 .. 65536, an inlier_distance that is not positive and finite with such a square, an
 * edge_ratio outside (0, 1]; APD_ERR_UNSUPPORTED for more than 262144 points on either side of a match.  The outputs are
 * untouched when a call fails. */
enum { APD_REGISTER_OK = 0, APD_REGISTER_TOO_FEW_MATCHES = 1, APD_REGISTER_NO_TRIAL = 2 };
int apd_points_features(apd_points_t p, float radius, const float *origin3, unsigned min_neighbours, float *features, unsigned char *has);
int apd_points_match_features(apd_points_t p, apd_points_t q, float radius, const float *origin3, unsigned min_neighbours, int mutual,
                              int32_t *index, float *distance);
typedef struct {
    unsigned trials;
    unsigned long long seed;
    float inlier_distance;
    float edge_ratio;
    unsigned min_neighbours;
    int mutual;
    int with_scale;
} apd_points_register_options;
typedef struct {
    double scale, rotation[9], translation[3];
    long long features_p, features_q, matches, trials_admitted, best_trial, inliers, inliers_after;
    double rms_after;
    int stopped;
} apd_points_registration_t;
int apd_points_register(apd_points_t p, apd_points_t q, float radius, const float *origin3, const apd_points_register_options *options,
                        apd_points_registration_t *out);
/* The cloud drawn into a camera with a z-buffer, and from such maps the views that see each point, occlusion included: what the
 * cleaned cloud looks like from a camera (a depth map and a point-index map, to inspect holes, to derive a mask, to compare with a
 * view's own depth map), and the visibility lists COLMAP's Delaunay mesher and Poisson trimming read, rebuilt for the cloud as it
 * is now.  The lists of a fusion only record which sources agreed with one reference pixel; these name every camera of the call
 * that sees the point.  binary32, IEEE operations in the order given (contract C15; csrc/apd_render_math.h).
 *   Draw.  Point k at P and a camera (K, R, t, width, height; the other fields are not read): u, w and the depth d by the fusion's
 *   projection (ProjectCamera, APD.cpp:805-815), c = int(u + 0.5f) and r = int(w + 0.5f) where that conversion is defined.  The
 *   point is drawn when d > 0 and finite, both conversions are defined, and 0 <= c < width, 0 <= r < height.  A point whose centre
 *   pixel is outside the image is not drawn at all.
 *   Footprint.  The pixels (c + dc, r + dr) with |dc|, |dr| <= splat (0 .. 8), clipped to the image.
 *   Maps.  Per pixel over the points whose footprint covers it: the smallest key ((uint64)bits(d) << 32) | k, i.e. the nearest
 *   point, and among equal depths the lowest index.  depth is that point's d, or 0.0f where no footprint reaches; index is its
 *   k, or 0xFFFFFFFF.  Both are functions of the input alone: no launch shape, order of arrival or race outcome shows in them.
 *   Seen.  Point k is seen by a camera when it is drawn and d - z <= rel_tolerance * z, z the depth of the map (rendered with the
 *   call's splat) at the point's own centre pixel: one subtraction, one multiplication, one comparison.  With rel_tolerance 0 only
 *   the winner of the pixel and exact ties are seen.
 * apd_points_render: depth and index have camera->width * camera->height entries in row-major order, host memory for
 * host-resident points, device memory on p's device for device-resident ones; either may be NULL, not both.  Host-resident points
 * without any give all-empty maps with no device touched; device-resident ones have their maps filled on their device.
 * apd_points_rendered_visibility: *out is a new object with p's points in p's order, every array copied, and it is a merged
 * object (apd_points_merged): it carries explicit lists, the rendered ones.  The list of point k holds the cameras of the call
 * that see it, as indices 0 .. num_views - 1, ascending, and may be empty; support[k] is 0 for an empty list, else
 * min(255, L - 1); view, pixel and sources are copied and describe the original point alone, as after a merge.  num_views is the
 * call's own and need not be the fusion's; the result names max(num_views, the views of p) views, a view past p's own with the size
 * of its camera.  apd_points_visibility, apd_points_write_vis, apd_points_write_ply, the filters and apd_points_merge_voxels work
 * on it as on any merged object, and apd_points_average refuses it.  *unseen (may be NULL) is the number of points with an empty
 * list.  The result lives where p lives.  An object without points gives an object without points and *unseen = 0, with no device
 * touched.  p may itself be a merged object: its lists are not read.
 * Both are computed on p's device, on its null stream, whatever memory p is in; there is no host implementation.  One image of
 * 64-bit keys is alive at a time, allocated once at the largest camera of the call.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_points_render: ..." or
 * "apd_points_rendered_visibility: ..." (apd_fusion_last_error): a NULL p, camera, cameras or out, both maps NULL, a splat outside
 * 0 .. 8, a width or height that is not positive or whose product is 2^31 or more, num_views < 1, a rel_tolerance that is negative
 * or not finite; APD_ERR_UNSUPPORTED for 2^31 or more points and for 2^32 or more list entries (known once the lists are counted
 * on the device).  *out and *unseen are untouched when the call fails.  apd_fusion_last_timing reports the call like the merge:
 * set-up, the kernels (and the download of a host result) as "views", file 0. */
int apd_points_render(apd_points_t p, const apd_camera *camera, int splat, float *depth, uint32_t *index);
int apd_points_rendered_visibility(apd_points_t p, int num_views, const apd_camera *cameras, int splat, float rel_tolerance,
                                   apd_points_t *out, long long *unseen);
/* The tile sizes of the device sort under apd_points_merge_voxels (csrc/apd_sort.h): elements per workgroup of a sort pass and
 * entries per workgroup of its scan.  For tests that choose sizes around them. */
void apd_sort_tile_sizes(int *sort_tile, int *scan_tile);
int apd_points_destroy(apd_points_t p);

/* A surface: a truncated signed distance volume integrated from depth maps -- the filtered maps of apd_filter_views, left on the
 * device, are the intended input -- and the indexed triangle mesh that marching tetrahedra takes from it.  Every cell is split into
 * the same six tetrahedra (Kuhn), so neighbouring cells agree on every shared face, no case is ambiguous, and the mesh is
 * watertight wherever the volume is known.  binary32, IEEE operations in the order given (contract C21, DESIGN.md;
 * csrc/apd_volume_math.h).
 *   Grid.  nx x ny x nz samples; sample (i, j, k) has the linear index i + nx * (j + ny * k) and the position
 *   origin[a] + (float)index_a * voxel: one multiplication, one addition.  Per sample a distance D (initially 1.0f) and a weight W
 *   (initially 0); with colour also blue, green, red and a colour weight CW (all initially 0).
 *   Integrate.  A view is a camera (K, R, t, width, height; the other fields are not read), a depth map of height x width floats,
 *   optionally an image of the same size with 1 or 3 interleaved float channels (blue, green, red, as apd_fuse_views takes them;
 *   one channel feeds all three) and a weight w > 0.  The sample at P is observed when it is drawn into the camera as
 *   apd_points_render draws a point (depth d > 0 and finite, c = int(u + 0.5f) and r = int(v + 0.5f) defined and inside the map),
 *   z = depth[r * width + c] is > 0 and finite, and sdf = z - d >= -trunc.  Then v = sdf / trunc, 1.0f where v > 1.0f;
 *   a = D * W; b = v * w; s = W + w; D = (a + b) / s; W = s > max_weight ? max_weight : s.  Where also sdf <= trunc each colour
 *   channel becomes (C * CW + colour * w) / (CW + w) in that operation order, and then CW as W.  The views of a call are applied
 *   to a sample in the call's order: two calls of k views equal one call of the 2k.  There is no culling.
 *   Vertices.  A sample is known when W > 0 and inside when known and D < 0 (zero and -0 are outside).  From a sample seven edges
 *   run, in the directions (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), numbered 0 .. 6, where the upper end exists.
 *   An edge carries a vertex when both ends are known and exactly one is inside: with fa, pa at the lower end, t = fa / (fa - fb)
 *   and per component pa + t * (pb - pa); per colour channel ca + t * (cb - ca) where both ends have CW > 0, the colour of the one
 *   end that has, else 0; clamped to 0 .. 255 (a NaN is 0) and converted by (int)(x + 0.5f).  Vertex ids ascend with
 *   (linear index * 7 + direction).  No two edges share a vertex: t = 0 gives coincident vertices and triangles without area,
 *   which are kept.
 *   Faces.  The cell with lower sample (i, j, k) has the tetrahedra q = 0 .. 5 along the axis permutations xyz, xzy, yxz, yzx,
 *   zxy, zyx: corners v0 = (0,0,0), v1 = v0 + e_p1, v2 = v1 + e_p2, v3 = (1,1,1).  A tetrahedron with a corner that is not known
 *   has no faces.  One corner a apart from the others b < c < d: the triangle (e_ab, e_ac, e_ad); two inside a < b and two outside
 *   c < d: (e_ac, e_ad, e_bd) and (e_ac, e_bd, e_bc); each turned to (first, third, second) where that makes its right-hand normal
 *   point from inside to outside, which a table fixed at compile time says.  Faces are ordered by cell index
 *   i + (nx - 1) * (j + (ny - 1) * k), then q, then as above.
 * apd_volume_create checks its arguments and touches no device: the volume's memory -- 8 bytes a sample, 24 with colour -- is
 * allocated on `device` by the first call that needs it.  apd_volume_integrate: depths and images (may be NULL: no colour is
 * updated) are num_views pointers each, host memory, or device memory on the volume's device with maps_on_device; weights NULL:
 * all 1.  apd_volume_download / apd_volume_upload copy D (tsdf), W (weight) and the four colour floats of every sample
 * (colour4) to or from host arrays in linear order; any may be NULL, not all: the way to save a volume, and to extract from any
 * field.  apd_volume_extract_mesh: *mesh is a new mesh on the volume's device, released with apd_mesh_destroy; a volume without a
 * crossing edge gives a mesh of 0 vertices and 0 faces.  Extraction takes 26 bytes a sample of scratch memory for the length of
 * the call.  apd_mesh_download: xyz takes 3 floats and bgr (a mesh with colour only) 3 bytes per vertex, faces 3 ints per face, host
 * memory; any may be NULL, not all.  apd_mesh_write_ply: binary little-endian, `vertex` with x y z float and, with colour, red green
 * blue uchar, then `face` with `property list uchar int vertex_indices`; apd_points_read_ply reads such a file back as its
 * vertices.  apd_volume_view_chunk: the views one kernel launch of apd_volume_integrate takes, for tests that go past it.
 * Everything is computed on the volume's device, on its null stream; there is no host implementation.
 * Refused with APD_ERR_INVALID before any device is touched, message "<function>: ..." (apd_fusion_last_error): a NULL volume,
 * mesh, origin3, cameras, depths, path or output pointer, a NULL map, all arrays NULL; a dimension below 2 or 2^31 or more
 * samples; a voxel, trunc or max_weight that is not positive and finite, max_weight < 1, an origin that is not finite, a negative
 * device; num_views < 1; a weight that is not positive and finite; images or a colour array for a volume or mesh without colour;
 * image_channels other than 1 or 3; a camera whose width or height is not positive or whose product is 2^31 or more.
 * APD_ERR_UNSUPPORTED for 2^31 or more vertices or faces (known once they are counted on the device).  Outputs are untouched when
 * a call fails.  apd_fusion_last_timing reports a call like the other points calls: set-up, the kernels and copies as "views",
 * and for apd_mesh_write_ply the file. */
typedef struct apd_volume *apd_volume_t;
typedef struct apd_mesh *apd_mesh_t;
int apd_volume_create(int device, int nx, int ny, int nz, const float *origin3, float voxel, float trunc, float max_weight, int with_colour,
                      apd_volume_t *volume);
int apd_volume_destroy(apd_volume_t volume);
int apd_volume_integrate(apd_volume_t volume, int num_views, const apd_camera *cameras, const float *const *depths, const float *const *images,
                         int image_channels, const float *weights, int maps_on_device);
int apd_volume_download(apd_volume_t volume, float *tsdf, float *weight, float *colour4);
int apd_volume_upload(apd_volume_t volume, const float *tsdf, const float *weight, const float *colour4);
int apd_volume_extract_mesh(apd_volume_t volume, apd_mesh_t *mesh);
int apd_volume_view_chunk(void);
int apd_mesh_counts(apd_mesh_t mesh, long long *vertices, long long *faces);
int apd_mesh_has_colour(apd_mesh_t mesh);
int apd_mesh_download(apd_mesh_t mesh, float *xyz, uint8_t *bgr, int32_t *faces);
int apd_mesh_write_ply(apd_mesh_t mesh, const char *path);
int apd_mesh_destroy(apd_mesh_t mesh);
/* Cleaning a mesh: what every pipeline that builds a distance volume runs after extraction -- merge close vertices, drop small
 * connected components, compute vertex normals (Open3D's merge_close_vertices, remove small clusters of connected triangles and
 * compute_vertex_normals; MeshLab's filters of the same names) -- here on the mesh object, on its device.  Every call leaves its
 * input as it is, gives a new mesh that shares nothing with it (released with apd_mesh_destroy), and its result is a function of
 * the input alone: two runs write the same bytes (contract C22; csrc/apd_mesh_math.h, csrc/apd_mesh.hip).
 *   apd_mesh_create.  A mesh on `device` from the caller's arrays: xyz 3 floats per vertex, bgr (may be NULL: a mesh without
 *   colour) 3 bytes per vertex, index 3 ints per face, each in [0, vertices); host memory, or with on_device device memory on
 *   `device`; the arrays are copied.  A face may repeat an index.  A mesh of 0 vertices and 0 faces is allowed and touches no device.
 *   Weld.  apd_mesh_weld joins vertices that are connected by a chain of pairs within `tolerance` of each other: the components of
 *   apd_points_components over the vertex positions with radius = tolerance, on the grid of cell size `tolerance` at origin3 (NULL:
 *   0, 0, 0), with that call's neighbour relation and grid limits; a vertex outside the grid (a coordinate that is not finite, 2^20
 *   cells from the origin) is joined to nothing.  The representative of a group is its smallest index; it keeps its own position,
 *   colour and normal, nothing is averaged.  Every face index is replaced by its representative; a face with two equal indices
 *   after that is dropped; a vertex that is no representative, or that no surviving face names, is dropped; surviving vertices and
 *   faces keep their order and the faces are renumbered.  -0.0 and +0.0 are one position.  A tolerance far below the voxel size,
 *   such as voxel * 1e-4, welds only the coincident vertices that t = 0 gives (see Vertices above) and drops their triangles
 *   without area; a tolerance near the voxel size collapses the surface.  *removed_vertices and *removed_faces (may be NULL): how
 *   many fewer the result has.
 *   Components.  Two faces are adjacent when they name a common vertex index; a component is the closure of that.  label[f] is the
 *   smallest face index of f's component, size[f] its number of faces; host memory, one entry per face, `size` may be NULL;
 *   *components (may be NULL) their number.  apd_mesh_remove_small_components keeps the faces with size[f] >= min_faces in their
 *   order (0 and 1 keep every face), drops the vertices no kept face names -- an unreferenced vertex goes whatever min_faces is --
 *   and renumbers; *removed_faces and *components (of the input) may be NULL.
 *   Vertex normals, area-weighted.  Face f with corners a, b, c at positions widened to binary64: u = b - a, w = c - a,
 *   g = (u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x), every product and difference one binary64
 *   operation.  The sum s of vertex v is that of g over the corners (f, c) with index[3 f + c] == v in ascending 3 f + c, in
 *   binary64 from +0.0.  len = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z); the normal is (float)(s / len) per component where len
 *   is finite and > 0, else (0, 0, 0): a vertex no face names, a vertex whose faces cancel, a face with a position that is not
 *   finite.  The sums are gathered through a stable sort of the corners by vertex and never added atomically, so their order, and
 *   with it every bit, is fixed.  apd_mesh_with_vertex_normals gives the mesh with these normals (replacing any it had);
 *   apd_mesh_has_normals tells; apd_mesh_download_normals takes 3 floats per vertex, host memory.  Weld and removal carry the
 *   normals of the vertices they keep along, unchanged.
 * apd_mesh_write_ply of a mesh with normals writes `property float nx`, ny, nz after z and before the colours, as the points'
 * file orders them; a mesh without writes the bytes it always wrote.  apd_points_read_ply reads either back as its vertices.
 * Everything is computed on the mesh's device, on its null stream; there is no host implementation.  A mesh without vertices
 * gives a mesh without, and no labels, with no device touched.
 * Refused with APD_ERR_INVALID before any device is touched, message "<function>: ...": a NULL mesh or output pointer (label for
 * apd_mesh_components); for apd_mesh_create a negative count, 2^31 or more of either, a NULL array with a count that is not 0, a
 * negative device and, for host arrays, an index outside [0, vertices) -- for device arrays a kernel checks the range and a
 * failure returns the same code; for apd_mesh_weld a tolerance that is not positive and finite or whose square is not, an origin
 * that is not finite; apd_mesh_download_normals of a mesh without normals.  APD_ERR_UNSUPPORTED from
 * apd_mesh_with_vertex_normals for a mesh whose 3 * faces reach 2^32 (the sort carries a 32-bit corner id).  Outputs are untouched
 * when a call fails.  apd_fusion_last_timing reports each call like the other mesh calls: set-up, the kernels and copies as
 * "views", file 0. */
int apd_mesh_create(int device, long long vertices, const float *xyz, const uint8_t *bgr, long long faces, const int32_t *index, int on_device,
                    apd_mesh_t *mesh);
int apd_mesh_weld(apd_mesh_t mesh, float tolerance, const float *origin3, apd_mesh_t *out, long long *removed_vertices, long long *removed_faces);
int apd_mesh_components(apd_mesh_t mesh, uint32_t *label, uint32_t *size, long long *components);
int apd_mesh_remove_small_components(apd_mesh_t mesh, unsigned min_faces, apd_mesh_t *out, long long *removed_faces, long long *components);
int apd_mesh_with_vertex_normals(apd_mesh_t mesh, apd_mesh_t *out);
int apd_mesh_has_normals(apd_mesh_t mesh);
int apd_mesh_download_normals(apd_mesh_t mesh, float *nxyz);

/* apd_mesh_simplify: the mesh thinned by vertex clustering on the cubic grid of cell size `cell` at origin3 (NULL: 0, 0, 0), each
 * cluster's vertex placed at its members' mean (APD_SIMPLIFY_MEAN) or on the surface, on creases and on corners by the quadric of
 * the faces around its members (APD_SIMPLIFY_QUADRIC) -- arithmetic contract C23, the rules written once in
 * csrc/apd_simplify_math.h.  Like the other mesh calls it leaves its input as it is, gives a new mesh on the input's device that
 * shares nothing with it, is a function of the input alone (stable sorts and scans, every sum walked in a fixed order, no
 * floating-point atomic) and has no host implementation.
 *   Clusters.  Vertex v is inside the grid when the voxel key of contract C10 exists for (P_v, origin, cell).  A cluster is the set
 *   of inside vertices with one key, its members in ascending vertex index; clusters are ordered by ascending key.  A vertex
 *   outside the grid (a non-finite coordinate, a cell beyond +-2^20) belongs to no cluster.
 *   Faces.  A face that names an outside vertex is dropped.  Every other face has each index replaced by its cluster; a face that
 *   then names a cluster twice is dropped.  Of the rest two are duplicates when their triples are equal after each is rotated (not
 *   reflected) so that its smallest cluster comes first -- reflected triples are different faces and both stay --, and of a set of
 *   duplicates the face with the smallest input index survives.  Surviving faces keep the input order and their corner order.  A
 *   cluster survives when a surviving face names it; surviving clusters are numbered in key order and the faces renumbered.
 *   Colour, both placements: per channel (sum + m / 2) / m over the m members in unsigned 64-bit, the rule of the voxel merge.
 *   Normals: the result has none, whatever the input had.  The normal of a simplified surface is that of its new faces:
 *   apd_mesh_with_vertex_normals is the step to run after.
 *   MEAN: per component the binary32 sum of the members' positions in member order, from the first member's value, divided by
 *   (float)m -- the position rule of the voxel merge.
 *   QUADRIC, all in binary64, every product and sum one IEEE operation in the order written.  (1) c_a = (double)origin_a +
 *   ((double)i_a + 0.5) * (double)cell, the centre of the cluster's cell (i signed).  (2) mu_a = (sum over the members of
 *   ((double)P_a - c_a), from +0.0) / (double)m.  (3) Over the corners (f, k) of the input faces whose three vertices are all
 *   inside the grid -- whether or not the face survives -- with index[3 f + k] a member, in ascending 3 f + k (a face with two
 *   corners in the cluster adds twice): g = the binary64 cross product of face f as for the vertex normals, a_a = (double)A_a - c_a
 *   with A the face's first corner, d = -((g0 * a0 + g1 * a1) + g2 * a2); S_ij += g_i * g_j for the six i <= j and t_a += g_a * d,
 *   from +0.0.  (4) q_a = (S_a0 * mu0 + S_a1 * mu1) + S_a2 * mu2, r_a = (-t_a) - q_a.  (5) The cyclic Jacobi of contract C14 on S:
 *   eigenvalues lambda_k (unclamped) with vectors e_k, lmax the largest.  (6) x = mu; for k = 0, 1, 2 where lambda_k > 0 and
 *   lambda_k > 1e-3 * lmax: p = ((e_0k * r0 + e_1k * r1) + e_2k * r2) / lambda_k, x_a = x_a + e_ak * p: the vertex moves only along
 *   the directions the faces constrain.  (7) x is accepted when every |x_a| <= (double)cell (a NaN fails); otherwise, or when a
 *   sum is not finite or lmax is not > 0, x = mu.  (8) The position is (float)(c_a + x_a).
 * *removed_vertices and *removed_faces (may be NULL): how many fewer the result has.  A mesh without vertices gives a mesh
 * without, with no device touched.  Refused with APD_ERR_INVALID before any device is touched, message "apd_mesh_simplify: ...":
 * a NULL mesh or out, a cell that is not positive and finite, an origin that is not finite, a placement other than the two.
 * APD_ERR_UNSUPPORTED where 3 * faces reaches 2^32, as for the normals.  Outputs are untouched on failure.
 * apd_fusion_last_timing reports the call like the other mesh calls. */
enum { APD_SIMPLIFY_MEAN = 0, APD_SIMPLIFY_QUADRIC = 1 };
int apd_mesh_simplify(apd_mesh_t mesh, float cell, const float *origin3 /* NULL: 0,0,0 */, int placement, apd_mesh_t *out,
                      long long *removed_vertices, long long *removed_faces);

/* apd_mesh_adjacency and apd_mesh_smooth: the vertex-to-vertex adjacency of a mesh with its edge multiplicities, and Laplacian or
 * Taubin lambda|mu smoothing of the vertex positions over it -- arithmetic contract C24, the rules written once in
 * csrc/apd_mesh_smooth_math.h.  Like the other mesh calls they leave their input as it is, are functions of the input alone (a
 * stable sort and scans, every sum walked by one lane in a fixed order, no atomic) and have no host implementation.
 *   Adjacency (integers only).  Every face (a, b, c) gives the six directed pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c); a pair
 *   with equal ends is dropped (a face may repeat an index).  The neighbours of v are the distinct w of its pairs, ascending.  The
 *   multiplicity of the edge {v, w} is the number of times the pair (v, w) occurs: the number of face sides on the edge.
 *   Multiplicity 1 is a boundary edge, 3 or more a non-manifold edge; a vertex is a boundary vertex when one of its edges is a
 *   boundary edge.  A vertex no face names has no neighbours and is not a boundary vertex.  Two equal faces give their edges
 *   multiplicity 2.
 *   One step with a factor k (a float, widened to binary64), positions p to p'.  Neighbour w of v contributes when the three
 *   coordinates of p[w] are finite; under APD_SMOOTH_BOUNDARY_ALONG a boundary vertex takes only the neighbours across its boundary
 *   edges, under _FIXED a boundary vertex does not move, under _FREE it is treated as any other.  A vertex moves when it is not held
 *   fixed, its own position is finite and at least one neighbour contributes; then per coordinate s = the binary64 sum of
 *   (double)p[w] over the contributing neighbours in ascending w from +0.0, m = s / (double)count, p'[v] = (float)((double)p[v] +
 *   k * (m - (double)p[v])), every operation one IEEE operation.  For every other vertex p'[v] = p[v], the same bits.
 *   An iteration is a step with lambda, followed, when mu != 0, by a step with mu: mu = 0 is plain Laplacian smoothing, lambda =
 *   0.5 with mu = -0.53 is Taubin's pair, which does not shrink.  Every step reads only the positions of the step before it; the
 *   adjacency is built once per call and the boundary flags, which come from the connectivity, stay.
 * apd_mesh_adjacency: valence[v] = the number of neighbours of v and boundary[v] = 1 for a boundary vertex, 0 otherwise (host
 * arrays, one entry per vertex); *edges = the undirected edges, *boundary_edges and *nonmanifold_edges those of multiplicity 1 and
 * of 3 or more: a mesh is closed when it has no boundary edge and manifold along its edges when it has no non-manifold one.  Every
 * output may be NULL, not all of them.
 * apd_mesh_smooth: `iterations` iterations into *out, a new mesh on the input's device with the same faces, colours and vertex
 * count, and no normals, whatever the input had: they would be stale, apd_mesh_with_vertex_normals is the step to run after.
 * *moved (may be NULL): the vertices that move in the first step.  A mesh without faces or without vertices gives a copy without
 * normals and *moved = 0.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_mesh_adjacency: ..." or "apd_mesh_smooth: ...": a NULL
 * mesh or out, outputs all NULL, iterations outside 1 .. 1000, lambda not in (0, 1], mu not in [-2, 0] or not finite, a boundary
 * mode other than the three.  APD_ERR_UNSUPPORTED where 6 * faces reaches 2^32: the positions of the neighbour lists are 32-bit, as
 * the corners of the vertex normals are.  Outputs are untouched on failure.  apd_fusion_last_timing reports the calls like the
 * other mesh calls. */
enum { APD_SMOOTH_BOUNDARY_FIXED = 0, APD_SMOOTH_BOUNDARY_ALONG = 1, APD_SMOOTH_BOUNDARY_FREE = 2 };
int apd_mesh_adjacency(apd_mesh_t mesh, uint32_t *valence, uint8_t *boundary, long long *edges, long long *boundary_edges,
                       long long *nonmanifold_edges);
int apd_mesh_smooth(apd_mesh_t mesh, int iterations, float lambda, float mu, int boundary, apd_mesh_t *out, long long *moved);

/* apd_mesh_render, apd_mesh_face_visibility and apd_mesh_remove_unseen: the mesh rasterised into a camera with a z-buffer, the number
 * of cameras that see each face, and the mesh without the faces too few cameras see -- arithmetic contract C25, the rules
 * written once in csrc/apd_mesh_render_math.h.  Like the other mesh calls they leave their input as it is, are functions of the input
 * alone (integer coverage, one IEEE operation per step of the depth, a 64-bit integer atomic min per pixel and integer atomic adds:
 * none depends on the order of arrival, and there is no floating-point atomic) and have no host implementation.
 *   Vertex.  The fusion's projection (ProjectCamera) gives u, w, d in binary32.  A vertex is usable when d > 0 and finite and
 *   su = u * 256.0f + 0.5f, sw = w * 256.0f + 0.5f are finite with |floorf(.)| <= 2^27 (the guard band: 2^19 pixels either side of
 *   the origin); X = (int)floorf(su), Y = (int)floorf(sw) are its position in 1/256 pixel.  Pixel (c, r) has its centre at
 *   (256 c, 256 r): integer coordinates are pixel centres, as everywhere in the fusion.
 *   Face.  Drawn when its three vertices are usable and A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) is not 0.  Two stated limits:
 *   there is NO NEAR-PLANE CLIPPING -- a face with a corner behind the camera is not drawn at all, rather than cut --, and a face
 *   with a corner BEYOND THE GUARD BAND is not drawn at all.  A face is front-facing, its right-hand normal (the one
 *   apd_mesh_with_vertex_normals sums) towards the camera, when A2 < 0; APD_RENDER_CULL_BACK draws front faces only,
 *   APD_RENDER_CULL_NONE both sides.  With A2 < 0 corners 1 and 2 are exchanged for what follows.
 *   Coverage (integers only).  Edge a -> b: dx = Xb - Xa, dy = Yb - Ya, E(p) = dx (py - Ya) - dy (px - Xa) in 64 bits.  A pixel
 *   centre of the face's bounding box clipped to the image is covered when for all three edges E > 0, or E == 0 with dy < 0, or
 *   E == 0 with dy == 0 and dx > 0 (the top-left rule): a centre on an edge two faces share belongs to exactly one of them.
 *   Depth (binary64, one IEEE operation per step).  w_i: the edge function opposite corner i, S = w0 + w1 + w2,
 *   q = (w0 / d0 + w1 / d1) + w2 / d2, z = (float)(S / q): perspective-correct.  The pixel takes the face only when z > 0 and finite.
 *   Maps.  Per pixel the nearest face, among equal depth bits the lowest index: depth z or 0.0f, face f or 0xFFFFFFFF.
 *   Seen.  A camera sees face f when f is drawn (and not culled) and (a) owns at least min_pixels pixels of the camera's face map
 *   or (b) each of its corners passes the points' test (apd_points_rendered_visibility): the corner's own pixel is inside the image,
 *   the map depth z there is > 0 and d - z <= rel_tolerance * z.  (a) alone loses faces smaller than a pixel, (b) alone large faces
 *   whose corners are hidden or outside the frame.
 * apd_mesh_render: depth and face take width * height entries each, host memory; either may be NULL, not both.
 * apd_mesh_face_visibility: views[f] = the cameras that see face f, pixels[f] = the pixels f owns over all cameras (host arrays, one
 * entry per face), *unseen = the faces no camera sees; each may be NULL, not all.
 * apd_mesh_remove_unseen: *out is a new mesh on the input's device of the faces with views[f] >= min_views, in their order, and of
 * the vertices they name, renumbered, with their colours and normals unchanged, as apd_mesh_remove_small_components gives its
 * result; min_views 0 keeps every face (and draws nothing).  *removed_faces, *removed_vertices (may be NULL): what went.
 * A mesh without faces gives empty maps, nothing to count and *unseen = 0, or a mesh without faces or vertices, with no device
 * touched.  One image of keys is alive at a time, allocated once per call at the largest camera.
 * apd_mesh_render_split: faces whose clipped bounding box has more than box_pixels pixels are drawn by a wave instead of a lane;
 * 0 restores the built-in value.  The results do not depend on it: it exists for the timing tool and a same-bytes test.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_mesh_render: ...", "apd_mesh_face_visibility: ..." or
 * "apd_mesh_remove_unseen: ...": a NULL mesh, camera, cameras or out, outputs all NULL, a cull other than the two, min_pixels < 1, a
 * rel_tolerance that is negative or not finite, num_views < 1, a camera whose width or height is not positive or whose product is
 * 2^31 or more.  APD_ERR_UNSUPPORTED where the faces drawn by waves need more waves than one launch holds (2^33 - 3 or more: every
 * such face takes 1 to 64, one per 256 tiles of 8 x 8 pixels of its clipped bounding box).  Outputs are untouched on failure.
 * apd_fusion_last_timing reports the calls like the other mesh calls: set-up (allocations), work, and 0 for the file. */
enum { APD_RENDER_CULL_NONE = 0, APD_RENDER_CULL_BACK = 1 };
int apd_mesh_render(apd_mesh_t mesh, const apd_camera *camera, int cull, float *depth, uint32_t *face);
int apd_mesh_face_visibility(apd_mesh_t mesh, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance,
                             uint32_t *views, uint64_t *pixels, long long *unseen);
int apd_mesh_remove_unseen(apd_mesh_t mesh, int num_views, const apd_camera *cameras, int cull, unsigned min_pixels, float rel_tolerance,
                           unsigned min_views, apd_mesh_t *out, long long *removed_faces, long long *removed_vertices);
void apd_mesh_render_split(int box_pixels);

/* apd_mesh_colour_from_views: the mesh with every vertex coloured from the images of the cameras that see it, through the mesh's own
 * z-buffer -- arithmetic contract C26, the rules written once in csrc/apd_mesh_colour_math.h.  Like the other mesh calls it
 * leaves its input as it is, is a function of the input alone (one writer per vertex, the views in the call's order, no floating-point
 * atomic) and has no host implementation.
 *   Inputs.  num_views cameras and one image per view of the camera's height x width, of 1 or 3 interleaved float channels, blue
 *   green red, as apd_volume_integrate takes them (one channel feeds all three); host memory, or with maps_on_device device memory on
 *   the mesh's device.  The vertex normals are the mesh's own, or where it has none those apd_mesh_with_vertex_normals would give it.
 *   Per view, in the call's order, Z = the depth map of apd_mesh_render(mesh, camera, APD_RENDER_CULL_NONE): both sides occlude.
 *   Sample.  The vertex at P with normal n takes a sample from a view when (1) n is not (0, 0, 0); (2) the fusion's projection gives
 *   d > 0 and finite; (3) the bilinear footprint is inside the image: c0 = (int)floorf(u), r0 = (int)floorf(w), 0 <= c0,
 *   c0 + 1 <= width - 1, 0 <= r0, r0 + 1 <= height - 1 (so u == width - 1 takes none); (4) it is not occluded at any of the four
 *   pixels (c0 | c0 + 1, r0 | r0 + 1): z = Z there is > 0 and d - z <= rel_tolerance * z, the points' test
 *   (apd_points_rendered_visibility) on the whole footprint, which keeps a nearer surface's colour out of a vertex just behind its
 *   silhouette and costs a mesh's border vertices some views; (5) it faces the camera: in binary64 e = centre - P,
 *   c = (n . e) / sqrt(e . e), c > min_cos.  The weight of the sample is c.
 *   Colour of a sample (binary32, one operation per step): fu = u - floorf(u), fw = w - floorf(w), per channel
 *   top = a + fu * (b - a), bot = a' + fu * (b' - a'), value = top + fw * (bot - top).
 *   Sums (binary64, in view order): S_k += c * value_k per channel, W += c, count += 1.
 *   Result.  count > 0: per channel x = (float)(S_k / W) clamped to 0 .. 255 (a NaN is 0), (int)(x + 0.5f), the conversion of the
 *   volume's vertex colours.  count == 0: the input's colour, (0, 0, 0) for a mesh without.
 * *out is a new mesh on the input's device that always has colour, with the input's vertices, faces and normals bit for bit.
 * views[v] (host, one entry per vertex, may be NULL) = the views vertex v took a sample from, *uncoloured (may be NULL) = the
 * vertices with none.  rel_tolerance: 0.01 is apd_mesh_face_visibility's; min_cos: 0.1 drops the views that see a vertex at more
 * than about 84 degrees, which contribute smear -- a design choice, not a measurement.  C25's two limits carry over: a face that is
 * not drawn occludes nothing.
 * A mesh without vertices gives an empty coloured mesh and *uncoloured = 0 with no device touched; a mesh with vertices and no
 * faces renders nothing, so every vertex is uncoloured.  Alive on the device at a time: one image of keys, one depth map and (for
 * host images, which go up one view at a time) one image buffer, each allocated once per call at the largest camera, and 36 bytes
 * a vertex; for a mesh without normals also the mesh with them.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_mesh_colour_from_views: ...": a NULL mesh, cameras, images,
 * image or out, num_views < 1, image_channels other than 1 or 3, a rel_tolerance that is negative or not finite, a min_cos outside
 * [0, 1) or not finite, a camera whose width or height is not positive or whose product is 2^31 or more.  APD_ERR_UNSUPPORTED as
 * apd_mesh_render and, for a mesh without normals, as apd_mesh_with_vertex_normals.  Outputs are untouched on failure.
 * apd_fusion_last_timing reports the call like the other mesh calls: set-up (allocations), work, and 0 for the file. */
int apd_mesh_colour_from_views(apd_mesh_t mesh, int num_views, const apd_camera *cameras, const float *const *images, int image_channels,
                               int maps_on_device, float rel_tolerance, float min_cos, apd_mesh_t *out, uint32_t *views, long long *uncoloured);

/* apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score: a mesh related to a cloud -- the closest point of the surface for
 * every point of a points object, points drawn on the surface uniformly by area, and from the two the precision, recall and F-score
 * of the surface against a ground-truth cloud, as Tanks and Temples and ETH3D evaluate a surface against a scan.  IEEE operations in
 * the order given (contract C27; csrc/apd_mesh_nearest_math.h).  Like the other mesh calls they leave their inputs as they
 * are, are functions of the inputs alone (two runs write the same bytes) and have no host implementation; they run on the mesh's
 * device, on its null stream.  A host-resident points object goes up for the call; a device-resident one must live on the mesh's
 * device (APD_ERR_UNSUPPORTED otherwise, before any device is touched).
 *   apd_mesh_nearest.  Grid: that of apd_points_neighbour_counts, cell size `radius` at origin3 (NULL: 0, 0, 0).  Face f is a
 *   candidate of point i of p when its three indices are distinct, its nine coordinates are finite and inside the grid, the binary64
 *   squared length of (b - a) x (c - a) is > 0, the point is inside the grid, and the binary64 squared distance d2 from the point to
 *   its closest point X on the face is <= (double)radius * (double)radius.  X is the Voronoi-region method of Ericson, Real-Time
 *   Collision Detection 5.1.5 -- the vertex regions a, b, c, the edge regions ab, ac, bc and the interior, in that order -- in binary64
 *   on the binary32 inputs widened, every dot product (x * x' + y * y') + z * z', and X held inside the face's bounding box.  The nearest face is the candidate of least d2,
 *   among equal d2 the one of smallest index: a point over a shared edge or vertex has one answer.  distance[i] = (float)sqrt(d2),
 *   face[i] = that face, closest3[3 i ..] = X rounded to binary32; without a candidate +inf, -1 and three NaNs.  The definition does
 *   not depend on how the search is organised: a loop over all faces gives the same bits.  Each output takes apd_points_count(p)
 *   entries (closest3 three times as many), host memory for a host-resident p, device memory on its device otherwise; any may be
 *   NULL, not all.  A p without points gives nothing with no device touched; a mesh without faces gives +inf, -1 and NaN throughout.
 *   The search puts every face into each cell of the grid that its bounding box overlaps and walks, per point, the 27 cells around
 *   it; a side of the box whose corner stands within binary32 rounding of a cell boundary takes one cell more, so that the cells,
 *   which are binary32 quotients, cannot hide a face that is within the radius (csrc/apd_mesh_nearest_math.h has the bound).  The work
 *   is the number of (cell, face) pairs, one sort of them, and the pairs in the 27 cells of every point.  A radius far
 *   below the size of the faces makes the pairs many: when they reach 2^31 the call is refused with APD_ERR_UNSUPPORTED after the
 *   counting pass, the message names their number (a lower bound: one face counts for at most 2^31), the radius and the remedy --
 *   a larger radius, or apd_mesh_simplify / a subdivision elsewhere.  apd_mesh_nearest_pair_limit sets another limit (at most 2^31;
 *   0 restores it): it exists for a test of that refusal.  apd_fusion_last_timing reports the pair build, the two sorts and the search.
 *   apd_mesh_sample_points.  *out is a new points object (released with apd_points_destroy) in device memory on the mesh's device
 *   (on_device != 0) or in host memory, with apd_points_read_ply's convention: one view of 1 x 1 pixels without sources; support,
 *   view, pixel and sources are 0.  A face with a repeated index, a non-finite coordinate or a cross product of squared length not
 *   > 0 gets no sample; any other face f gets n_f = floor(area_f * density + u(seed, f)) of them, area_f = 0.5 * sqrt(|(b - a) x
 *   (c - a)|^2) in binary64 and u in [0, 1): stochastic rounding, so that the expected total is density * area and a mesh of faces
 *   far smaller than 1 / density is still sampled.  u and the two numbers r1, r2 of sample k of face f come from a counter-based
 *   generator, two splitmix64 finalisers on (seed, f) and (k, c), the top 53 bits scaled by 2^-53; r1 + r2 > 1 folds them to 1 - r1
 *   and 1 - r2.  Position a + r1 (b - a) + r2 (c - a) in binary64 rounded to binary32; normal the unit face normal (not the
 *   vertex normals); colour the barycentric mix of the corners' colours rounded half up per channel, 0 for a mesh without colours.
 *   Order: faces ascending, k ascending within a face.  face (host, may be NULL): one entry per sample, the face it lies on.  A
 *   function of (mesh, density, seed) alone; no floating-point sum decides a position.
 *   apd_mesh_score.  Fills the struct of apd_points_score at radius = threshold.  Precision side: the samples of
 *   apd_mesh_sample_points(mesh, density, seed) against `truth` by apd_points_nearest's search (n_p = the samples, p_within those with a
 *   point of truth within the threshold, mean_p their mean distance).  Recall side: `truth` against the surface by apd_mesh_nearest
 *   (n_q, q_within, mean_q): exact, it does not depend on the sampling.  density <= 0: 4 / (threshold * threshold) in binary64, about four
 *   samples per threshold-sized square.  Of the distances only the binary64 chunk sums leave the device.  As for apd_points_score there
 *   is no cropping volume and no occlusion-aware evaluation: scores of two runs compare with each other.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_mesh_nearest: ...", "apd_mesh_sample_points: ..." or
 * "apd_mesh_score: ..." (apd_fusion_last_error): a NULL mesh, p, truth or out, all three outputs NULL, what apd_points_nearest refuses
 * for the radius (the threshold) and origin3, a density that is not positive and finite (apd_mesh_score: not finite).
 * APD_ERR_UNSUPPORTED: 2^31 or more points, the pair limit, and samples that would reach 2^31 (known after the scan of the counts,
 * before they are allocated).  A refused call has written no output: the pair limit is held before the first of them is filled.  A
 * HIP error in the middle of apd_mesh_nearest (APD_ERR_HIP) may leave device-resident outputs holding the fill values +inf, -1 and NaN.
 * apd_mesh_device: the device the mesh lives on, where these calls compute and device-resident samples live; -1 for a NULL mesh. */
int apd_mesh_device(apd_mesh_t mesh);
int apd_mesh_nearest(apd_mesh_t mesh, apd_points_t p, float radius, const float *origin3, float *distance, int32_t *face, float *closest3);
void apd_mesh_nearest_pair_limit(long long pairs);
int apd_mesh_sample_points(apd_mesh_t mesh, double density, unsigned long long seed, int on_device, apd_points_t *out,
                           int32_t *face /* may be NULL; host, one per sample */);
int apd_mesh_score(apd_mesh_t mesh, apd_points_t truth, float threshold, const float *origin3,
                   double density /* <= 0: 4 / (threshold * threshold) in binary64 */, unsigned long long seed, apd_points_score_t *out);

/* apd_fuse_views_variant(options->variant, ...) with options.  ply_path and points may each be NULL, not both: a file, the
 * points in memory (*points, released with apd_points_destroy; untouched when the call fails), or both from one fusion.  With
 * ply_normals the file has the properties x y z nx ny nz (float) before the three colour bytes.  Refused with APD_ERR_INVALID
 * before any device is touched, message "apd_fuse_views_opt: ...": struct_size other than sizeof(apd_fusion_options), an
 * unknown variant, a threshold, weight or factor that is negative or not finite, min_consistent outside 1 .. APD_MAX_IMAGES,
 * ply_path and points both NULL, and everything apd_fuse_views refuses. */
int apd_fuse_views_opt(const apd_fusion_options *options, int device, int num_views, const apd_camera *cameras,
                       const float *const *images, int image_channels, const float *const *depths, const float *const *normals,
                       const uint8_t *const *weaks, const uint8_t *const *blocks, const int *rows, const int *cols,
                       const int *pair_offsets, const int *pair_indices, int maps_on_device, const char *ply_path,
                       long long *num_points, apd_points_t *points);

/* The geometric filter: per view what the vote test of RunFusion (APD.cpp:896-951) says about its own pixels -- a filtered depth
 * map, the number of agreeing sources and the consistency score -- without the loop's consumption of source pixels (`masks`,
 * APD.cpp:928, :959), which makes a view's result depend on the views fused before it.  Inputs as apd_fuse_views_opt, minus the
 * images; of `options` only struct_size, variant (APD_FUSION_ETH) and the eight values of the rule are read.  Pixel p of view i:
 * where blocks[i][p] < 128 or depths[i][p] <= 0, votes = 0, consistency = 0 and depth_out = 0.  Otherwise the pixel is lifted
 * (Get3DPointonWorld) and, for each source in pair.txt order, projected into it (APD.cpp:896-899); a source pixel with depth > 0
 * that passes the three thresholds (APD.cpp:941) adds 1 to votes and exp(-(reproj + depth_weight * depth + angle_weight * angle))
 * to consistency (a float sum in source order from 0, APD.cpp:944-947); depth_out = depths[i][p] if votes >= min_consistent and
 * consistency > factor * votes (APD.cpp:950-951), else 0.  votes and consistency are written for every pixel, accepted or not.
 * Every view is judged against the unfiltered maps of its sources: the result of a view depends on no other view's.
 * depth_out, votes_out, consistency_out: per-view caller-owned buffers of rows[i] * cols[i] elements, device pointers on
 * `device` with outputs_on_device != 0, host pointers otherwise; a table or any entry may be NULL and is then not written.
 * Refused with APD_ERR_INVALID before any device is touched, message "apd_filter_views: ...": what apd_fuse_views_opt refuses in
 * its options, a variant other than APD_FUSION_ETH, no output pointer at all, an output pointer equal to an input map, and
 * everything apd_fuse_views refuses of its views.  apd_fusion_last_error / apd_fusion_last_timing report on it (set-up, views; the
 * file time is 0). */
int apd_filter_views(const apd_fusion_options *options, int device, int num_views, const apd_camera *cameras,
                     const float *const *depths, const float *const *normals, const uint8_t *const *weaks,
                     const uint8_t *const *blocks, const int *rows, const int *cols, const int *pair_offsets,
                     const int *pair_indices, int maps_on_device, float *const *depth_out, uint8_t *const *votes_out,
                     float *const *consistency_out, int outputs_on_device);

/* Host-side constant of K3 (GenNeighbours, APD.cu:1911 / :1946): its inlier test `dist / (depth_max - depth_min) <
 * ransac_threshold` (dist >= 0) is evaluated on the device as `dist < cut`, the same predicate for every binary32 dist because
 * x -> RN(x / d) is monotone.  Returns 1 and the cut, or 0 when the parameters admit none (the kernel then divides).  Needs
 * no device; exported so that the equivalence can be tested on any machine (tests/test_host_constants.py). */
int apd_ransac_distance_cut(float depth_min, float depth_max, float ransac_threshold, float *cut);

const char *apd_last_error(void);
int apd_version(void);
/* Digest (16 hex digits) of the HIP sources, headers and compiler flags the library was built from: equals
 * apd-mvs_amd/build.py:expected_build_id() of the same tree; anything else is a stale binary. */
const char *apd_build_id(void);
int apd_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* APD_MI355X_H_ */
