"""apd_mvs_amd -- thin ctypes layer over the C ABI (include/apd_mi355x.h) of the MI355X PatchMatch path.

This is plumbing for tests and bench.py only; the product is the HIP library
(`_build/libapd_mi355x.so`) and the C++ drop-in host in `host/`.  There is no CPU fallback: if the
library is missing or a GPU call fails, this module raises.

The directory is called `apd-mvs_amd` (not importable by name); `__graft_entry__.load_package()`
registers it as the module `apd_mvs_amd`.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libapd_mi355x.so")

FIRST_INIT, REFINE_INIT, REFINE_ITER = 0, 1, 2
WEAK, STRONG, UNKNOWN = 0, 1, 2
MAX_IMAGES = 32

(K1, K2, K3, K4, K5, K6, K7, K8, K9, K10, K11, K12, K13, K14, K15) = range(1, 16)
KERNEL_NAMES = {
    1: "InitRandomStates", 2: "FindNearestStrongPoint", 3: "GenNeighbours", 4: "NeigbourUpdate",
    5: "RandomInitialization", 6: "BlackPixelUpdateStrong", 7: "RedPixelUpdateStrong",
    8: "RANSACToGetFitPlane", 9: "BlackPixelUpdateWeak", 10: "RedPixelUpdateWeak",
    11: "GetDepthandNormal", 12: "BlackPixelFilterStrong", 13: "RedPixelFilterStrong",
    14: "DepthToWeak", 15: "LocalRefine",
}

# apd_set_option / apd_get_option (include/apd_mi355x.h): the library reads nothing from the environment
(OPT_FAST_RCP, OPT_EARLY_OUT, OPT_SOURCE_QUADS, OPT_TILED_COPY, OPT_K67_WINDOWS, OPT_K1415_WINDOWS) = range(6)
OPTION_NAMES = {"fast_rcp": OPT_FAST_RCP, "early_out": OPT_EARLY_OUT, "source_quads": OPT_SOURCE_QUADS, "tiled_copy": OPT_TILED_COPY,
                "k67_windows": OPT_K67_WINDOWS, "k1415_windows": OPT_K1415_WINDOWS}

(STATE_PLANES, STATE_FIT_PLANES, STATE_COSTS, STATE_RNG, STATE_SELECTED_VIEWS, STATE_VIEW_WEIGHT,
 STATE_WEAK_INFO, STATE_WEAK_RELIABLE, STATE_NEAREST_STRONG, STATE_NEIGHBOURS_MAP, STATE_NEIGHBOURS) = range(11)


class Camera(C.Structure):
    """apd_camera == reference Camera (main.h:47-56)."""

    _fields_ = [("K", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3), ("c", C.c_float * 3),
                ("height", C.c_int), ("width", C.c_int), ("depth_min", C.c_float), ("depth_max", C.c_float)]


class Params(C.Structure):
    """apd_params == reference PatchMatchParams (main.h:75-94) + seed."""

    _fields_ = [
        ("max_iterations", C.c_int), ("num_images", C.c_int), ("sigma_spatial", C.c_float),
        ("sigma_color", C.c_float), ("top_k", C.c_int), ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("geom_consistency", C.c_int), ("strong_radius", C.c_int), ("strong_increment", C.c_int),
        ("weak_radius", C.c_int), ("weak_increment", C.c_int), ("use_APD", C.c_int),
        ("weak_peak_radius", C.c_int), ("rotate_time", C.c_int), ("ransac_threshold", C.c_float),
        ("geom_factor", C.c_float), ("state", C.c_int), ("seed", C.c_uint64),
    ]


class FusionOptions(C.Structure):
    """apd_fusion_options (include/apd_mi355x.h): the ETH fusion's acceptance rule as values, and the form of the result."""

    _fields_ = [
        ("struct_size", C.c_size_t), ("variant", C.c_int), ("max_reproj_error", C.c_float), ("max_relative_depth", C.c_float),
        ("max_angle", C.c_float), ("depth_weight", C.c_float), ("angle_weight", C.c_float), ("min_consistent", C.c_int),
        ("factor_strong", C.c_float), ("factor_weak", C.c_float), ("ply_normals", C.c_int), ("result_on_device", C.c_int),
    ]


class ApdError(RuntimeError):
    pass


_lib = None


def library_path():
    return LIB_PATH


def expected_build_id():
    """Digest of csrc/*, the headers and the compiler flags of THIS tree (build.py: expected_build_id)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("apd_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.expected_build_id()


def build_id(L=None):
    """apd_build_id() of the loaded library: the digest of the sources it was compiled from."""
    L = L or lib()
    L.apd_build_id.restype = C.c_char_p
    return L.apd_build_id().decode()


def check_build_id(L):
    """A library built from other sources than the tree's is refused (an mtime test cannot tell a stale binary on a box
    whose push preserved the times).  APD_ALLOW_STALE_LIBRARY=1 skips the test (lab builds with ad-hoc flags)."""
    if os.environ.get("APD_ALLOW_STALE_LIBRARY") == "1":
        return
    if not hasattr(L, "apd_build_id"):
        raise ApdError("%s has no apd_build_id(): a binary of an earlier round; run __graft_entry__.build()" % LIB_PATH)
    have, want = build_id(L), expected_build_id()
    if have != want:
        raise ApdError("stale HIP library: %s was built from sources with digest %s, the tree's csrc/ + flags give %s; "
                       "run __graft_entry__.build() (a lab build with APD_EXTRA_FLAGS: set APD_ALLOW_STALE_LIBRARY=1)" % (LIB_PATH, have, want))


def lib():
    """Loads the HIP library; raises if it has not been built or was built from other sources (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ApdError("HIP library %s is missing: run __graft_entry__.build() first" % LIB_PATH)
    try:
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7; if it is going to
        # be used (streams, device tensors, RCCL) it must be the copy that gets loaded, so import it first.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    check_build_id(L)
    H = C.c_void_p
    fpp = C.POINTER(C.c_void_p)
    L.apd_default_params.argtypes = [C.POINTER(Params)]
    L.apd_default_params.restype = None
    L.apd_create.argtypes = [C.POINTER(H), C.c_int, C.c_int, C.c_int, C.POINTER(Params)]
    L.apd_destroy.argtypes = [H]
    L.apd_reset.argtypes = [H, C.POINTER(Params)]
    L.apd_upload_views.argtypes = [H, C.c_int, C.POINTER(Camera), fpp, fpp]
    L.apd_upload_views_split.argtypes = [H, C.c_int, C.POINTER(Camera), fpp]
    L.apd_image_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.apd_image_destroy.argtypes = [C.c_void_p]
    L.apd_upload_views_shared.argtypes = [H, C.c_int, C.POINTER(Camera), fpp]
    L.apd_upload_depths.argtypes = [H, C.c_int, fpp]
    L.apd_run_before_depths.argtypes = [H]
    L.apd_run_after_depths.argtypes = [H]
    L.apd_upload_prior.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_upload_mask.argtypes = [H, C.c_void_p]
    L.apd_masked_count.argtypes = [H]
    L.apd_run.argtypes = [H]
    L.apd_run_kernel.argtypes = [H, C.c_int, C.c_int]
    L.apd_run_sweeps.argtypes = [H, C.c_int, C.c_int]
    L.apd_synchronize.argtypes = [H]
    L.apd_download.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_download_state.argtypes = [H, C.c_int, C.c_void_p, C.c_size_t]
    L.apd_upload_state.argtypes = [H, C.c_int, C.c_void_p, C.c_size_t]
    L.apd_state_bytes.argtypes = [H, C.c_int]
    L.apd_state_bytes.restype = C.c_size_t
    L.apd_export_depth_normal_device.argtypes = [H, C.c_void_p, C.c_void_p]
    L.apd_export_state_device.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for n in ("apd_width", "apd_height", "apd_weak_count"):
        getattr(L, n).argtypes = [H]
    for n in ("apd_depth_min", "apd_depth_max"):
        getattr(L, n).argtypes = [H]
        getattr(L, n).restype = C.c_float
    L.apd_profile_enable.argtypes = [H, C.c_int]
    L.apd_profile_reset.argtypes = [H]
    L.apd_profile_get.argtypes = [H, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.apd_set_stream.argtypes = [H, C.c_void_p]
    L.apd_set_option.argtypes = [H, C.c_int, C.c_int]
    L.apd_get_option.argtypes = [H, C.c_int, C.POINTER(C.c_int)]
    L.apd_last_error.restype = C.c_char_p
    L.apd_device_count.restype = C.c_int
    L.apd_exchange_last_error.restype = C.c_char_p
    L.apd_fusion_last_error.restype = C.c_char_p
    L.apd_fusion_default_options.argtypes = [C.POINTER(FusionOptions)]
    L.apd_fusion_default_options.restype = None
    ipp = C.POINTER(C.c_int)
    L.apd_fuse_views_opt.argtypes = [C.POINTER(FusionOptions), C.c_int, C.c_int, C.c_void_p, fpp, C.c_int, fpp, fpp, fpp, fpp, ipp, ipp, ipp, ipp,
                                     C.c_int, C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_void_p)]
    L.apd_filter_views.argtypes = [C.POINTER(FusionOptions), C.c_int, C.c_int, C.c_void_p, fpp, fpp, fpp, fpp, ipp, ipp, ipp, ipp, C.c_int,
                                   fpp, fpp, fpp, C.c_int]
    L.apd_points_count.argtypes = [C.c_void_p]
    L.apd_points_count.restype = C.c_longlong
    L.apd_points_on_device.argtypes = [C.c_void_p]
    for n in ("xyz", "normal", "bgr", "support", "view", "pixel", "sources"):
        getattr(L, "apd_points_" + n).argtypes = [C.c_void_p]
        getattr(L, "apd_points_" + n).restype = C.c_void_p
    L.apd_points_visibility.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.apd_points_write_vis.argtypes = [C.c_void_p, C.c_char_p]
    L.apd_points_average.argtypes = [C.c_void_p, C.c_int, C.c_void_p, fpp, fpp, ipp, ipp, C.c_int, C.POINTER(C.c_void_p)]
    L.apd_points_write_ply.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.apd_points_create.argtypes = [C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 7 + [C.c_int, ipp, ipp, ipp, ipp, C.POINTER(C.c_void_p)]
    L.apd_points_merge_voxels.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
    L.apd_points_merged.argtypes = [C.c_void_p]
    L.apd_points_neighbour_counts.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p]
    L.apd_points_remove_sparse.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
    L.apd_points_knn_mean_distances.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p]
    L.apd_points_remove_statistical.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_float, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.apd_points_components.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    L.apd_points_remove_small_components.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_points_estimate_normals.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p, C.c_void_p]
    L.apd_points_with_estimated_normals.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_longlong)]
    L.apd_points_smoothed_positions.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p, C.c_void_p]
    L.apd_points_with_smoothed_positions.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_uint, C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_longlong)]
    L.apd_points_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    L.apd_points_score.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(PointsScore)]
    L.apd_points_align.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(PointsAlignOptions), C.POINTER(PointsAlignment)]
    L.apd_points_align_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(PointsAlignPlanesOptions),
                                          C.POINTER(PointsPlaneAlignment)]
    L.apd_points_transformed.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_void_p)]
    L.apd_points_features.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p, C.c_void_p]
    L.apd_points_match_features.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    L.apd_points_match_features_bounded.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_int, C.c_ulonglong,
                                                    C.c_void_p, C.c_void_p]
    L.apd_points_register.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(PointsRegisterOptions),
                                      C.POINTER(PointsRegistration)]
    L.apd_points_read_ply.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.apd_points_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_void_p, C.c_void_p]
    L.apd_points_rendered_visibility.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
    L.apd_sort_tile_sizes.argtypes = [ipp, ipp]
    L.apd_sort_tile_sizes.restype = None
    L.apd_points_destroy.argtypes = [C.c_void_p]
    L.apd_volume_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_int,
                                    C.POINTER(C.c_void_p)]
    L.apd_volume_destroy.argtypes = [C.c_void_p]
    L.apd_volume_integrate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, fpp, fpp, C.c_int, C.POINTER(C.c_float), C.c_int]
    L.apd_volume_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_volume_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_volume_extract_mesh.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.apd_volume_view_chunk.argtypes = []
    L.apd_mesh_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_mesh_has_colour.argtypes = [C.c_void_p]
    L.apd_mesh_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_mesh_write_ply.argtypes = [C.c_void_p, C.c_char_p]
    L.apd_mesh_destroy.argtypes = [C.c_void_p]
    L.apd_mesh_create.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.apd_mesh_weld.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_mesh_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    L.apd_mesh_remove_small_components.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_mesh_with_vertex_normals.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.apd_mesh_simplify.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                    C.POINTER(C.c_longlong)]
    L.apd_mesh_adjacency.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_mesh_smooth.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
    L.apd_mesh_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_void_p, C.c_void_p]
    L.apd_mesh_face_visibility.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    L.apd_mesh_remove_unseen.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_uint, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.apd_mesh_colour_from_views.argtypes = [C.c_void_p, C.c_int, C.c_void_p, fpp, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_void_p), C.c_void_p,
                                             C.POINTER(C.c_longlong)]
    L.apd_mesh_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
    L.apd_mesh_device.argtypes = [C.c_void_p]
    L.apd_mesh_nearest_pair_limit.argtypes = [C.c_longlong]
    L.apd_mesh_nearest_pair_limit.restype = None
    L.apd_mesh_sample_points.argtypes = [C.c_void_p, C.c_double, C.c_ulonglong, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    L.apd_mesh_score.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_double, C.c_ulonglong, C.POINTER(PointsScore)]
    L.apd_mesh_render_split.argtypes = [C.c_int]
    L.apd_mesh_render_split.restype = None
    L.apd_mesh_has_normals.argtypes = [C.c_void_p]
    L.apd_mesh_download_normals.argtypes = [C.c_void_p, C.c_void_p]
    L.apd_device_memcpy.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise ApdError("apd error %d: %s" % (rc, lib().apd_last_error().decode()))


def default_params(**kw):
    p = Params()
    lib().apd_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_fusion_options(**kw):
    """apd_fusion_default_options (the reference's literals, 15-byte PLY records, host results) with the given fields replaced."""
    o = FusionOptions()
    lib().apd_fusion_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(FusionOptions._fields_):
            raise TypeError("apd_fusion_options has no field %r" % k)
        setattr(o, k, v)
    return o


class PointsScore(C.Structure):
    """apd_points_score_t."""
    _fields_ = [(n, C.c_longlong) for n in ("n_p", "n_q", "p_within", "q_within")] + \
               [(n, C.c_double) for n in ("precision", "recall", "fscore", "mean_p", "mean_q")]


# What Points.score returns: the nine fields of apd_points_score_t
Score = collections.namedtuple("Score", [n for n, _ in PointsScore._fields_])


class PointsAlignOptions(C.Structure):
    """apd_points_align_options."""
    _fields_ = [("iterations", C.c_uint), ("tolerance", C.c_double), ("with_scale", C.c_int)]


class PointsAlignment(C.Structure):
    """apd_points_alignment_t."""
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("matched_before", C.c_longlong),
                ("matched_after", C.c_longlong), ("rms_before", C.c_double), ("rms_after", C.c_double), ("steps", C.c_int), ("stopped", C.c_int)]


# What Points.align returns: the fields of apd_points_alignment_t, rotation as a float64 [3, 3] array and translation as a float64
# [3] array; `stopped` is one of these
Alignment = collections.namedtuple("Alignment", [n for n, _ in PointsAlignment._fields_])
ALIGN_ITERATIONS, ALIGN_CONVERGED, ALIGN_TOO_FEW = 0, 1, 2


class PointsAlignPlanesOptions(C.Structure):
    """apd_points_align_planes_options."""
    _fields_ = [("iterations", C.c_uint), ("tolerance", C.c_double)]


class PointsPlaneAlignment(C.Structure):
    """apd_points_plane_alignment_t: the fields of apd_points_alignment_t, then the plane figures."""
    _fields_ = PointsAlignment._fields_ + [("planes_before", C.c_longlong), ("planes_after", C.c_longlong), ("plane_rms_before", C.c_double),
                                           ("plane_rms_after", C.c_double)]


# What Points.align_planes returns: the fields of Alignment, in its shapes, then the usable matches and the plane rms before and
# after; `stopped` may also be ALIGN_DEGENERATE
PlaneAlignment = collections.namedtuple("PlaneAlignment", [n for n, _ in PointsPlaneAlignment._fields_])
ALIGN_DEGENERATE = 3


class PointsRegisterOptions(C.Structure):
    """apd_points_register_options."""
    _fields_ = [("trials", C.c_uint), ("seed", C.c_ulonglong), ("inlier_distance", C.c_float), ("edge_ratio", C.c_float), ("min_neighbours", C.c_uint),
                ("mutual", C.c_int), ("with_scale", C.c_int)]


class PointsRegistration(C.Structure):
    """apd_points_registration_t."""
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3)] + \
               [(n, C.c_longlong) for n in ("features_p", "features_q", "matches", "trials_admitted", "best_trial", "inliers", "inliers_after")] + \
               [("rms_after", C.c_double), ("stopped", C.c_int)]


# What Points.register returns: the fields of apd_points_registration_t, rotation as a float64 [3, 3] array and translation as a
# float64 [3] array; `stopped` is one of these
Registration = collections.namedtuple("Registration", [n for n, _ in PointsRegistration._fields_])
REGISTER_OK, REGISTER_TOO_FEW_MATCHES, REGISTER_NO_TRIAL = 0, 1, 2
FEATURE_WIDTH = 33


class _Borrowed:
    """Memory of a Points object as an array interface; keeps its owner alive."""

    def __init__(self, owner, address, shape, typestr):
        self.owner = owner
        self.__array_interface__ = {"data": (address, True), "shape": shape, "typestr": typestr, "version": 3}


class Points:
    """One fusion's points (apd_points_t) in PLY order as arrays: xyz float32 [N, 3] (the reference pixel's lifted point),
    normal float32 [N, 3] (its normal as given, not renormalised), bgr uint8 [N, 3], support uint8 [N] (the votes the point was
    accepted with), view and pixel int32 [N] (reference view and raster index in it), sources uint32 [N] (bit j: the j-th source
    of the point's view is one of those votes; a device result holds the same bit patterns as int32).  A host result gives
    read-only numpy views of the library's memory, valid while an array or this object lives; a device result gives torch tensors
    on its device, filled by device-to-device copies (no host round trip) and independent of this object.  visibility() and
    write_vis() are the library's (apd_points_visibility, apd_points_write_vis), and so are average() (apd_points_average: a new
    Points with positions and normals averaged over the agreeing views) and write_ply() (apd_points_write_ply); the object keeps
    the library's points for them until close().  from_arrays() makes a Points of a caller's arrays (apd_points_create);
    merge_voxels() gives one point per cell of a cubic grid with the union of the members' lists (apd_points_merge_voxels), and
    `merged` says whether an object is such a result: its view, pixel and sources are its representative's alone, its lists are
    those of visibility(), and average() refuses it.  neighbour_counts() counts every point's neighbours within a radius
    (apd_points_neighbour_counts) and remove_sparse() gives the points that have enough of them (apd_points_remove_sparse), with
    everything else an object carries.  knn_mean_distances() gives every point's mean distance to its k nearest neighbours within
    a radius (apd_points_knn_mean_distances) and remove_statistical() the points whose value is no outlier of the cloud's own
    distribution of it (apd_points_remove_statistical), likewise.  components() labels the connected components of the points within
    a radius of each other (apd_points_components) and remove_small_components() gives the points of the components that are large
    enough (apd_points_remove_small_components), likewise.  estimate_normals() gives every point's normal and surface variation
    from its neighbourhood within a radius (apd_points_estimate_normals) and with_estimated_normals() these points with those
    normals in place of the stored ones (apd_points_with_estimated_normals), likewise.  smoothed_positions() gives every point's
    position projected on the weighted least-squares plane of its neighbourhood within a radius and the signed distance it moved
    (apd_points_smoothed_positions) and with_smoothed_positions() these points with those positions, iterated, in place of the
    stored ones (apd_points_with_smoothed_positions), likewise: the one step that moves a point.  nearest() gives for every point
    the nearest point of another Points within a radius (apd_points_nearest), score() the precision, recall and F-score of these
    points against another Points at a threshold (apd_points_score), align() the rigid or similarity transform that brings these
    points onto another Points by ICP within a radius (apd_points_align), align_planes() the rigid one onto the other's tangent
    planes (apd_points_align_planes), transformed() these points moved by such a transform
    (apd_points_transformed), features() every point's FPFH descriptor from the stored normals (apd_points_features),
    match_features() the point of another Points with the nearest descriptor (apd_points_match_features), register() the transform
    that brings these points onto another Points from any start, by RANSAC over those matches (apd_points_register), and read_ply() makes a Points of a PLY file, a ground truth for instance (apd_points_read_ply).
    render() draws the points into a camera with a z-buffer: the depth and the index of the nearest point per pixel
    (apd_points_render); with_rendered_visibility() gives these points as a merged object whose lists name the cameras that see
    each point, occlusion included (apd_points_rendered_visibility)."""

    _FIELDS = (("xyz", 3, "<f4", 4), ("normal", 3, "<f4", 4), ("bgr", 3, "|u1", 1), ("support", 1, "|u1", 1), ("view", 1, "<i4", 4),
               ("pixel", 1, "<i4", 4), ("sources", 1, "<u4", 4))
    _TORCH = {"<f4": "float32", "|u1": "uint8", "<i4": "int32", "<u4": "int32", "<i8": "int64"}

    def __init__(self, handle, device=0):
        L = lib()
        self._p = handle
        self.device = int(device)
        self.count = int(L.apd_points_count(handle))
        self.on_device = bool(L.apd_points_on_device(handle))
        self.merged = bool(L.apd_points_merged(handle))
        self._lists = None
        for name, width, typestr, size in self._FIELDS:
            address = getattr(L, "apd_points_" + name)(handle)
            setattr(self, name, self._array(address, (self.count, width) if width > 1 else (self.count,), typestr, size))

    def _array(self, address, shape, typestr, size):
        """`shape` elements at `address` of the library's memory: a torch tensor (a device-to-device copy) or a numpy view."""
        count = int(np.prod(shape))
        if self.on_device:
            import torch
            t = torch.empty(shape, dtype=getattr(torch, self._TORCH[typestr]), device=torch.device("cuda", self.device))
            if count:
                rc = lib().apd_device_memcpy(self.device, t.data_ptr(), address, count * size)
                if rc != 0:
                    raise ApdError("apd error %d copying the points: %s" % (rc, lib().apd_exchange_last_error()))
            return t
        if count:
            return np.asarray(_Borrowed(self, address, shape, typestr))
        return np.empty(shape, np.dtype(typestr))

    @classmethod
    def from_arrays(cls, xyz, normal, bgr, support, view, pixel, sources, rows, cols, pairs, device=0, on_device=False):
        """apd_points_create: a Points of the caller's arrays (numpy or anything numpy converts; copied), as if fused over views of
        rows[i] x cols[i] pixels with the source lists pairs[i] (view indices).  on_device: the copy lives on GPU `device`;
        otherwise it is host memory and no device is touched.  The library checks the arrays against the views and the lists and
        raises ApdError with its message."""
        L = lib()
        arrays = [np.ascontiguousarray(a, t) for a, t in zip((xyz, normal, bgr, support, view, pixel, sources),
                                                            (np.float32, np.float32, np.uint8, np.uint8, np.int32, np.int32, np.uint32))]
        count = len(arrays[4])
        for a, width in zip(arrays, (3, 3, 3, 1, 1, 1, 1)):
            if a.size != count * width:
                raise ValueError("Points.from_arrays: %d views (one per point) and an array of %d elements, not %d" % (count, a.size, count * width))
        V = len(rows)
        if len(cols) != V or len(pairs) != V:
            raise ValueError("Points.from_arrays: %d rows, %d cols, %d source lists" % (V, len(cols), len(pairs)))
        flat = [int(s) for p in pairs for s in p]
        offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
        idx = (C.c_int * max(len(flat), 1))(*flat)
        out = C.c_void_p()
        rc = L.apd_points_create(int(device), int(bool(on_device)), count, *[C.c_void_p(a.ctypes.data) for a in arrays], V,
                                 (C.c_int * max(V, 1))(*[int(r) for r in rows]), (C.c_int * max(V, 1))(*[int(c) for c in cols]), offs, idx, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return cls(out, device)

    def merge_voxels(self, size, origin=None):
        """apd_points_merge_voxels: (Points, dropped) -- one point per occupied cell of the cubic grid of cell size `size` with a
        corner at `origin` (0, 0, 0 by default), in ascending cell order (z-major), each the mean of its members in input order,
        with the distinct views of its members' lists as its visibility() list; `dropped` points had a non-finite coordinate or
        lie more than 2^20 cells from the origin.  Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.merge_voxels: the points are closed")
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, dropped = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_points_merge_voxels(self._p, float(size), org, C.byref(out), C.byref(dropped))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(dropped.value)

    def neighbour_counts(self, radius, cap=0, origin=None):
        """apd_points_neighbour_counts: per point the number of other points within `radius` of it (contract C11: on the grid of cell
        size `radius` with a corner at `origin`, 0, 0, 0 by default), at most `cap` (0: no cap); a point with a non-finite
        coordinate or more than 2^20 cells from the origin counts 0 and is counted by nobody.  uint32 [N]: a numpy array for host
        points; for device points a torch tensor on their device holding the same bit patterns as int32, like `sources`.
        Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.neighbour_counts: the points are closed")
        if not 0 <= int(cap) <= 0xFFFFFFFF:
            raise ValueError("Points.neighbour_counts: a cap of %r, not in 0 .. 2^32 - 1" % (cap,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_uint32 * 1)()   # where an object without points gets its no counts: the library refuses NULL
        if self.on_device:
            import torch
            counts = torch.empty((self.count,), dtype=torch.int32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(counts.device)
            address = counts.data_ptr() if self.count else C.addressof(nothing)
        else:
            counts = np.zeros(self.count, np.uint32)
            address = counts.ctypes.data if self.count else C.addressof(nothing)
        rc = L.apd_points_neighbour_counts(self._p, float(radius), org, int(cap), C.c_void_p(address))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return counts

    def remove_sparse(self, radius, min_neighbours, origin=None):
        """apd_points_remove_sparse: (Points, removed) -- the points with at least `min_neighbours` other points within `radius`
        (the relation of neighbour_counts), in their order, with all seven arrays; `removed` is the number left out.
        min_neighbours = 0 keeps every point.  The result lists, writes and averages itself like these points; the result of a
        merged object is a merged object with the kept points' lists.  Computed on these points' device; the result lives where
        they live."""
        if not self._p:
            raise ApdError("Points.remove_sparse: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.remove_sparse: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, removed = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_points_remove_sparse(self._p, float(radius), org, int(min_neighbours), C.byref(out), C.byref(removed))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(removed.value)

    def knn_mean_distances(self, radius, k, origin=None):
        """apd_points_knn_mean_distances: per point the mean distance to its `k` (1 .. 64) nearest neighbours among the other points
        within `radius` of it (contract C12: the neighbours of neighbour_counts, the k smallest squared distances, their square
        roots summed in ascending order and divided by k, in binary32); +inf for a point with fewer than k neighbours, an isolated
        point and a point outside the grid among them.  float32 [N]: a numpy array for host points, a torch tensor on their device
        for device points.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.knn_mean_distances: the points are closed")
        if not 0 <= int(k) <= 0xFFFFFFFF:
            raise ValueError("Points.knn_mean_distances: k = %r, not in 0 .. 2^32 - 1" % (k,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_float * 1)()   # where an object without points gets its no scores: the library refuses NULL
        if self.on_device:
            import torch
            mean = torch.empty((self.count,), dtype=torch.float32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(mean.device)
            address = mean.data_ptr() if self.count else C.addressof(nothing)
        else:
            mean = np.zeros(self.count, np.float32)
            address = mean.ctypes.data if self.count else C.addressof(nothing)
        rc = L.apd_points_knn_mean_distances(self._p, float(radius), org, int(k), C.c_void_p(address))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return mean

    def remove_statistical(self, radius, k, std_ratio, origin=None):
        """apd_points_remove_statistical: (Points, removed, threshold) -- the points whose knn_mean_distances(radius, k) value is
        finite and at most threshold = mu + std_ratio * sigma, mu and sigma the mean and the sample standard deviation of the
        finite values (binary64, summed in a fixed order: contract C12), in their order, with all seven arrays; `removed` is the
        number left out.  std_ratio may be zero or negative.  The result carries what the result of remove_sparse carries.
        Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.remove_statistical: the points are closed")
        if not 0 <= int(k) <= 0xFFFFFFFF:
            raise ValueError("Points.remove_statistical: k = %r, not in 0 .. 2^32 - 1" % (k,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, removed, threshold = C.c_void_p(), C.c_longlong(0), C.c_double(0.0)
        rc = L.apd_points_remove_statistical(self._p, float(radius), org, int(k), float(std_ratio), C.byref(out), C.byref(removed), C.byref(threshold))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(removed.value), float(threshold.value)

    def components(self, radius, origin=None):
        """apd_points_components: (label, size, components) -- the connected components of the graph in which two points share an edge
        when they are neighbours within `radius` (contract C13: the relation of neighbour_counts, on the grid of cell size `radius`
        with a corner at `origin`, 0, 0, 0 by default).  label[i] is the smallest index among the points of i's component, size[i]
        their number, `components` the number of components; a point with a non-finite coordinate or more than 2^20 cells from
        the origin is a component of its own.  label and size are uint32 [N]: numpy arrays for host points; for device points
        torch tensors on their device holding the same bit patterns as int32, like `sources`.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.components: the points are closed")
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_uint32 * 1)()   # where an object without points gets its no labels: the library refuses NULL
        if self.on_device:
            import torch
            label, size = (torch.empty((self.count,), dtype=torch.int32, device=torch.device("cuda", self.device)) for _ in range(2))
            torch.cuda.synchronize(label.device)
            addresses = [a.data_ptr() if self.count else C.addressof(nothing) for a in (label, size)]
        else:
            label, size = np.zeros(self.count, np.uint32), np.zeros(self.count, np.uint32)
            addresses = [a.ctypes.data if self.count else C.addressof(nothing) for a in (label, size)]
        components = C.c_longlong(0)
        rc = L.apd_points_components(self._p, float(radius), org, C.c_void_p(addresses[0]), C.c_void_p(addresses[1]), C.byref(components))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return label, size, int(components.value)

    def remove_small_components(self, radius, min_size, origin=None):
        """apd_points_remove_small_components: (Points, removed, components) -- the points whose connected component (the relation of
        components()) has at least `min_size` points, in their order, with all seven arrays; `removed` is the number left out,
        `components` the number of components of these points.  min_size 0 and 1 keep every point.  The result carries what the
        result of remove_sparse carries.  Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.remove_small_components: the points are closed")
        if not 0 <= int(min_size) <= 0xFFFFFFFF:
            raise ValueError("Points.remove_small_components: a minimum of %r points, not in 0 .. 2^32 - 1" % (min_size,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, removed, components = C.c_void_p(), C.c_longlong(0), C.c_longlong(0)
        rc = L.apd_points_remove_small_components(self._p, float(radius), org, int(min_size), C.byref(out), C.byref(removed), C.byref(components))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(removed.value), int(components.value)

    def estimate_normals(self, radius, min_neighbours, origin=None):
        """apd_points_estimate_normals: (normals float32 [N, 3], variation float32 [N]) -- for a point with at least
        `min_neighbours` (2 .. 2^31 - 1) other points within `radius` (the relation of neighbour_counts) the direction of least
        variance of the point and those neighbours (contract C14: binary64 moment sums in cell order, a cyclic Jacobi eigen-solve),
        signed like the stored normal, and the smallest eigenvalue's share of the variance, 0 on a plane and at most 1/3; for any
        other point, one outside the grid among them, the stored normal and +inf.  numpy arrays for host points, torch tensors on
        their device for device points.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.estimate_normals: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.estimate_normals: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_float * 3)()   # where an object without points gets its no results: the library refuses NULL for both
        if self.on_device:
            import torch
            normals = torch.empty((self.count, 3), dtype=torch.float32, device=torch.device("cuda", self.device))
            variation = torch.empty((self.count,), dtype=torch.float32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(normals.device)
            addresses = [a.data_ptr() if self.count else C.addressof(nothing) for a in (normals, variation)]
        else:
            normals, variation = np.zeros((self.count, 3), np.float32), np.zeros(self.count, np.float32)
            addresses = [a.ctypes.data if self.count else C.addressof(nothing) for a in (normals, variation)]
        rc = L.apd_points_estimate_normals(self._p, float(radius), org, int(min_neighbours), C.c_void_p(addresses[0]), C.c_void_p(addresses[1]))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return normals, variation

    def with_estimated_normals(self, radius, min_neighbours, origin=None):
        """apd_points_with_estimated_normals: (Points, estimated) -- these points in their order with `normal` replaced by the
        normals of estimate_normals(radius, min_neighbours) and every other array and the lists as they are; `estimated` is the
        number of points that got an estimate, the others keep their stored normal.  A merged object gives a merged object.
        Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.with_estimated_normals: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.with_estimated_normals: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, estimated = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_points_with_estimated_normals(self._p, float(radius), org, int(min_neighbours), C.byref(out), C.byref(estimated))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(estimated.value)

    def smoothed_positions(self, radius, min_neighbours, origin=None):
        """apd_points_smoothed_positions: (xyz float32 [N, 3], offset float32 [N]) -- for a point with at least `min_neighbours`
        (2 .. 2^31 - 1) other points within `radius` (the relation of neighbour_counts) its position projected on the weighted
        least-squares plane of the point and those neighbours (contract C16: the weight (1 - d^2 / radius^2)^2, binary64 sums in cell
        order, the eigen-solve of estimate_normals) and the signed distance it moved along that plane's normal, which is signed
        like the stored one; for any other point, one outside the grid among them, its position and +inf.  One iteration.  numpy
        arrays for host points, torch tensors on their device for device points.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.smoothed_positions: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.smoothed_positions: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_float * 3)()   # where an object without points gets its no results: the library refuses NULL for both
        if self.on_device:
            import torch
            xyz = torch.empty((self.count, 3), dtype=torch.float32, device=torch.device("cuda", self.device))
            offset = torch.empty((self.count,), dtype=torch.float32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(xyz.device)
            addresses = [a.data_ptr() if self.count else C.addressof(nothing) for a in (xyz, offset)]
        else:
            xyz, offset = np.zeros((self.count, 3), np.float32), np.zeros(self.count, np.float32)
            addresses = [a.ctypes.data if self.count else C.addressof(nothing) for a in (xyz, offset)]
        rc = L.apd_points_smoothed_positions(self._p, float(radius), org, int(min_neighbours), C.c_void_p(addresses[0]), C.c_void_p(addresses[1]))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return xyz, offset

    def with_smoothed_positions(self, radius, min_neighbours, iterations=1, origin=None):
        """apd_points_with_smoothed_positions: (Points, moved) -- these points in their order with `xyz` replaced by the positions
        of smoothed_positions(radius, min_neighbours) applied `iterations` (1 .. 16) times, each iteration to every point at once
        on the grid of the positions before it, and every other array and the lists as they are; `moved` is the number of points
        that had an estimate in at least one iteration, the others keep their position.  A merged object gives a merged object.
        A curved surface shrinks towards its centre of curvature by up to radius^2 / (2 R) per iteration.  Computed on these
        points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.with_smoothed_positions: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.with_smoothed_positions: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        if not 0 <= int(iterations) <= 0xFFFFFFFF:
            raise ValueError("Points.with_smoothed_positions: %r iterations, not in 0 .. 2^32 - 1" % (iterations,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out, moved = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_points_with_smoothed_positions(self._p, float(radius), org, int(min_neighbours), int(iterations), C.byref(out), C.byref(moved))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(moved.value)

    def nearest(self, other, radius, origin=None):
        """apd_points_nearest: (distance float32 [N], index int32 [N]) -- per point the distance to the nearest point of `other` (a
        Points, which may be this one) within `radius` and that point's index in `other` (contract C17: both clouds on the grid of
        cell size `radius` with a corner at `origin`, 0, 0, 0 by default; the candidates are the points of `other` in the 27 cells
        around the point's; among equally near ones the smallest index), +inf and -1 where there is none.  numpy arrays for host
        points, torch tensors on their device for device points.  Computed on these points' device: host-resident `other` goes up
        for the call, device-resident `other` must live on that device."""
        if not self._p:
            raise ApdError("Points.nearest: the points are closed")
        if not isinstance(other, Points) or not other._p:
            raise ApdError("Points.nearest: the other points are closed or not a Points")
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_float * 1)()   # where an object without points gets its no results: the library refuses NULL for both
        if self.on_device:
            import torch
            distance = torch.empty((self.count,), dtype=torch.float32, device=torch.device("cuda", self.device))
            index = torch.empty((self.count,), dtype=torch.int32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(distance.device)
            addresses = [a.data_ptr() if self.count else C.addressof(nothing) for a in (distance, index)]
        else:
            distance, index = np.zeros(self.count, np.float32), np.zeros(self.count, np.int32)
            addresses = [a.ctypes.data if self.count else C.addressof(nothing) for a in (distance, index)]
        rc = L.apd_points_nearest(self._p, other._p, float(radius), org, C.c_void_p(addresses[0]), C.c_void_p(addresses[1]))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return distance, index

    def score(self, truth, threshold, origin=None):
        """apd_points_score: Score(n_p, n_q, p_within, q_within, precision, recall, fscore, mean_p, mean_q) of these points against
        `truth` (a Points) at `threshold`: precision is the share of these points that have a point of `truth` within the threshold
        (p_within of n_p), recall the share of `truth` that has one of these within it (q_within of n_q), fscore their harmonic
        mean, mean_p and mean_q the mean distances of those that have one (contract C17; nearest() with radius = threshold in
        both directions).  Nearest-neighbour precision and recall at one threshold: register() gives a registration from any start
        and align(), align_planes() and transformed() refine it first, but there is no cropping volume and no
        occlusion-aware evaluation as ETH3D's: scores compare with each other.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.score: the points are closed")
        if not isinstance(truth, Points) or not truth._p:
            raise ApdError("Points.score: the other points are closed or not a Points")
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out = PointsScore()
        rc = L.apd_points_score(self._p, truth._p, float(threshold), org, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Score(*[getattr(out, n) for n in Score._fields])

    def align(self, other, radius, origin=None, iterations=16, tolerance=1e-6, with_scale=False):
        """apd_points_align: Alignment(scale, rotation, translation, matched_before, matched_after, rms_before, rms_after, steps,
        stopped) -- the transform x' = scale * rotation @ x + translation that brings these points onto `other` (a Points) by
        point-to-point ICP (contract C18): per step every point is matched to its nearest point of `other` within `radius`
        (nearest(), on the grid at `origin`), the matched pairs give the rigid transform -- with_scale: the similarity -- that
        brings them closest in the least-squares sense (Horn's closed form), and the total moves these points' own positions for
        the next step.  It ends after `iterations` (1 .. 64) steps (stopped == ALIGN_ITERATIONS), when the rms distance of the
        matched pairs changes by no more than `tolerance` times itself (ALIGN_CONVERGED), or when fewer than 3 points are matched
        or all matched points coincide (ALIGN_TOO_FEW).  matched_ and rms_before describe the points as they are, _after under
        the returned transform.  Nothing is moved: transformed() does that.  The start must be within about a radius of the answer:
        register() gives such a start from anywhere.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.align: the points are closed")
        if not isinstance(other, Points) or not other._p:
            raise ApdError("Points.align: the other points are closed or not a Points")
        if not 0 <= int(iterations) <= 0xFFFFFFFF:
            raise ValueError("Points.align: %r iterations, not in 0 .. 2^32 - 1" % (iterations,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        options, out = PointsAlignOptions(int(iterations), float(tolerance), int(bool(with_scale))), PointsAlignment()
        rc = L.apd_points_align(self._p, other._p, float(radius), org, C.byref(options), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Alignment(out.scale, np.array(out.rotation, np.float64).reshape(3, 3), np.array(out.translation, np.float64), out.matched_before,
                         out.matched_after, out.rms_before, out.rms_after, out.steps, out.stopped)

    def align_planes(self, other, radius, origin=None, iterations=16, tolerance=1e-6):
        """apd_points_align_planes: PlaneAlignment(the fields of Alignment, planes_before, planes_after, plane_rms_before,
        plane_rms_after) -- the rigid transform x' = rotation @ x + translation that brings these points onto the tangent planes of
        `other` (a Points with normals; with_estimated_normals() makes them) by point-to-plane ICP (contract C20): per step every
        point is matched as in align(), the matches whose normal has a finite length > 0 are usable, and the small motion that
        brings the points closest to the planes through their matches is solved from the 6 x 6 normal equations.  Prefer it to
        align() once a start within about `radius` exists and `other` has normals: it slides along the surface where align()
        settles on the sampling offset.  It ends as align() does, with ALIGN_TOO_FEW also for fewer than 6 usable matches, or with
        stopped == ALIGN_DEGENERATE when the matched geometry does not constrain every motion (a plane, a cylinder along its
        axis, a sphere about its centre): the steps taken until then are returned.  scale is 1.0; rms_* are the point rms,
        plane_rms_* the rms distance to the planes over the planes_* usable matches.  Nothing is moved: transformed() does that.
        Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.align_planes: the points are closed")
        if not isinstance(other, Points) or not other._p:
            raise ApdError("Points.align_planes: the other points are closed or not a Points")
        if not 0 <= int(iterations) <= 0xFFFFFFFF:
            raise ValueError("Points.align_planes: %r iterations, not in 0 .. 2^32 - 1" % (iterations,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        options, out = PointsAlignPlanesOptions(int(iterations), float(tolerance)), PointsPlaneAlignment()
        rc = L.apd_points_align_planes(self._p, other._p, float(radius), org, C.byref(options), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return PlaneAlignment(out.scale, np.array(out.rotation, np.float64).reshape(3, 3), np.array(out.translation, np.float64), out.matched_before,
                              out.matched_after, out.rms_before, out.rms_after, out.steps, out.stopped, out.planes_before, out.planes_after,
                              out.plane_rms_before, out.plane_rms_after)

    def transformed(self, scale, rotation=None, translation=None):
        """apd_points_transformed: these points in their order with xyz replaced by scale * rotation @ x + translation and normal by
        rotation @ n (not scaled, not renormalised), each component as (float)(((m0 x + m1 y) + m2 z) + t) in binary64, and every
        other array and the lists as they are: transformed(alignment) with what align(), align_planes() or register() returned, or transformed(scale, rotation,
        translation) with a positive scale, a rotation (3 x 3, row-major, orthonormal to 1e-6) and a translation.  A merged object
        gives a merged object.  Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.transformed: the points are closed")
        if isinstance(scale, (Alignment, PlaneAlignment, Registration)):
            if rotation is not None or translation is not None:
                raise TypeError("Points.transformed: an Alignment or a Registration, or scale, rotation and translation")
            scale, rotation, translation = scale.scale, scale.rotation, scale.translation
        if rotation is None or translation is None:
            raise TypeError("Points.transformed: an Alignment or a Registration, or scale, rotation and translation")
        R, t = np.ascontiguousarray(rotation, np.float64), np.ascontiguousarray(translation, np.float64)
        if R.size != 9 or t.size != 3:
            raise ValueError("Points.transformed: a rotation of %d and a translation of %d numbers, not 9 and 3" % (R.size, t.size))
        L = lib()
        out = C.c_void_p()
        rc = L.apd_points_transformed(self._p, float(scale), R.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device)

    def _outputs(self, specs):
        """Arrays for a query's results, [(shape after the point count, numpy dtype)]: (arrays, addresses) -- numpy for host points,
        torch tensors on their device for device points; an object without points gets the address of a dummy, which the library wants and
        which lives as long as `addresses` does."""
        nothing = (C.c_float * 1)()
        if self.on_device:
            import torch
            device = torch.device("cuda", self.device)
            arrays = [torch.empty((self.count,) + shape, dtype=getattr(torch, np.dtype(dt).name), device=device) for shape, dt in specs]
            torch.cuda.synchronize(device)
            addresses = [C.c_void_p(a.data_ptr()) if self.count else C.cast(nothing, C.c_void_p) for a in arrays]
        else:
            arrays = [np.zeros((self.count,) + shape, dt) for shape, dt in specs]
            addresses = [C.c_void_p(a.ctypes.data) if self.count else C.cast(nothing, C.c_void_p) for a in arrays]
        return arrays, (addresses, nothing)

    def features(self, radius, min_neighbours=5, origin=None):
        """apd_points_features: (features float32 [N, 33], has uint8 [N]) -- every point's FPFH descriptor from the STORED normals
        and its neighbours within `radius` (contract C19: three histograms of 11 bins over the pair features of PCL's
        computePairFeatures, each block summing to 1), zeros and has = 0 for a point with fewer than `min_neighbours` (>= 3)
        admitted neighbours, a normal of length 0 or not finite, or a position outside the grid.  with_estimated_normals() first
        for points that carry no normals.  numpy arrays for host points, torch tensors on their device for device points."""
        if not self._p:
            raise ApdError("Points.features: the points are closed")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.features: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        (features, has), (addresses, _keep) = self._outputs([((FEATURE_WIDTH,), np.float32), ((), np.uint8)])
        rc = L.apd_points_features(self._p, float(radius), org, int(min_neighbours), addresses[0], addresses[1])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return features, has

    def match_features(self, other, radius, min_neighbours=5, mutual=True, origin=None, _pair_bound=None):
        """apd_points_match_features: (index int32 [N], distance float32 [N]) -- per point with a descriptor (features()) the index
        in `other` (a Points, which may be this one) of the point whose descriptor is nearest in the 33 dimensions and that
        distance, the smallest index among equals; `mutual`: only where the match's own match is the point; -1 and +inf where
        there is none.  The cost is the product of the two numbers of descriptors: at most 262144 points on either side
        (merge_voxels() thins a cloud).  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.match_features: the points are closed")
        if not isinstance(other, Points) or not other._p:
            raise ApdError("Points.match_features: the other points are closed or not a Points")
        if not 0 <= int(min_neighbours) <= 0xFFFFFFFF:
            raise ValueError("Points.match_features: a minimum of %r neighbours, not in 0 .. 2^32 - 1" % (min_neighbours,))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        (index, distance), (addresses, _keep) = self._outputs([((), np.int32), ((), np.float32)])
        if _pair_bound is None:
            rc = L.apd_points_match_features(self._p, other._p, float(radius), org, int(min_neighbours), int(bool(mutual)), addresses[0], addresses[1])
        else:
            rc = L.apd_points_match_features_bounded(self._p, other._p, float(radius), org, int(min_neighbours), int(bool(mutual)), int(_pair_bound),
                                                     addresses[0], addresses[1])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return index, distance

    def register(self, other, radius, inlier_distance=None, origin=None, trials=4096, seed=0, edge_ratio=0.9, min_neighbours=5, mutual=True,
                 with_scale=False):
        """apd_points_register: Registration(scale, rotation, translation, features_p, features_q, matches, trials_admitted,
        best_trial, inliers, inliers_after, rms_after, stopped) -- the transform x' = scale * rotation @ x + translation that
        brings these points onto `other` (a Points) from ANY start, for clouds whose scale is already about right (contract C19):
        the matches of match_features() at `radius`; `trials` (1 .. 65536) RANSAC trials, each on three matches drawn by a
        counter-based generator keyed by (seed, trial), admitted when the two triangles' edges agree within `edge_ratio`; the
        trial with the most matches within `inlier_distance` (radius / 2 by default) after its rigid transform; and that transform
        refitted on its inliers by align()'s solve -- with_scale: with a scale, which is only refined.  stopped is REGISTER_OK,
        REGISTER_TOO_FEW_MATCHES (fewer than 3 matches) or REGISTER_NO_TRIAL (no admitted trial, or fewer than 3 inliers); the
        failures give the identity.  The descriptors use the stored normals.  Nothing is moved: transformed(registration) does
        that, and align() then refines it.  The same call gives the same bits.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.register: the points are closed")
        if not isinstance(other, Points) or not other._p:
            raise ApdError("Points.register: the other points are closed or not a Points")
        if not (0 <= int(trials) <= 0xFFFFFFFF and 0 <= int(min_neighbours) <= 0xFFFFFFFF and 0 <= int(seed) < 2 ** 64):
            raise ValueError("Points.register: trials %r, min_neighbours %r or seed %r outside their unsigned types" % (trials, min_neighbours, seed))
        L = lib()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        distance = float(np.float32(radius) * np.float32(0.5)) if inlier_distance is None else float(inlier_distance)
        options = PointsRegisterOptions(int(trials), int(seed), distance, float(edge_ratio), int(min_neighbours), int(bool(mutual)), int(bool(with_scale)))
        out = PointsRegistration()
        rc = L.apd_points_register(self._p, other._p, float(radius), org, C.byref(options), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Registration(out.scale, np.array(out.rotation, np.float64).reshape(3, 3), np.array(out.translation, np.float64),
                            *[getattr(out, n) for n in Registration._fields[3:]])

    @classmethod
    def read_ply(cls, path, device=0, on_device=False):
        """apd_points_read_ply: a Points of the vertices of a binary little-endian PLY file -- what write_ply() writes and what ETH3D
        and Tanks and Temples ship as ground truth: float x y z, float nx ny nz and uchar red green blue (or diffuse_*) when the
        file has them (zeros otherwise), any other scalar property skipped, the faces of a mesh ignored.  The points name one view of
        1 x 1 without sources.  on_device: they live on GPU `device`; otherwise in host memory and no device is touched."""
        L = lib()
        out = C.c_void_p()
        rc = L.apd_points_read_ply(os.fspath(path).encode(), int(device), int(bool(on_device)), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return cls(out, device)

    def render(self, camera, splat=0):
        """apd_points_render: (depth float32 [height, width], index uint32 [height, width]) -- these points drawn into `camera` (a
        Camera: K, R, t, width, height) with a z-buffer (contract C15): per pixel the depth of the nearest point whose footprint of
        (2 * splat + 1)^2 pixels covers it and that point's index, the lowest among equal depths; 0 and 0xFFFFFFFF where no
        footprint reaches.  numpy arrays for host points; for device points torch tensors on their device, the index holding the
        same bit patterns as int32, like `sources`.  Computed on these points' device."""
        if not self._p:
            raise ApdError("Points.render: the points are closed")
        L = lib()
        cam = Camera.from_buffer_copy(camera)
        shape = (max(int(cam.height), 0), max(int(cam.width), 0))
        if self.on_device:
            import torch
            depth = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", self.device))
            index = torch.empty(shape, dtype=torch.int32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(depth.device)
            addresses = [depth.data_ptr(), index.data_ptr()]
        else:
            depth, index = np.zeros(shape, np.float32), np.zeros(shape, np.uint32)
            addresses = [depth.ctypes.data, index.ctypes.data]
        nothing = (C.c_uint32 * 1)()   # where a camera without pixels gets its no maps: the library refuses NULL for both, then the camera
        rc = L.apd_points_render(self._p, C.byref(cam), int(splat), *[C.c_void_p(a if shape[0] * shape[1] else C.addressof(nothing)) for a in addresses])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return depth, index

    def with_rendered_visibility(self, cameras, splat=1, rel_tolerance=0.01):
        """apd_points_rendered_visibility: (Points, unseen) -- these points in their order, every array copied, as a merged object
        whose visibility() list of a point holds the cameras (indices into `cameras`, a ctypes array or a sequence of Camera, not
        necessarily the fusion's) that see it: the point is drawn into the camera and lies within rel_tolerance * z behind the
        depth z that render(camera, splat) has at its own pixel.  support is min(255, length - 1), 0 for an empty list; `unseen`
        is the number of points no camera sees.  Computed on these points' device; the result lives where they live."""
        if not self._p:
            raise ApdError("Points.with_rendered_visibility: the points are closed")
        L = lib()
        V = len(cameras)
        cams = cameras if isinstance(cameras, C.Array) else (Camera * max(V, 1))(*[Camera.from_buffer_copy(c) for c in cameras])
        out, unseen = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_points_rendered_visibility(self._p, V, C.byref(cams), int(splat), float(rel_tolerance), C.byref(out), C.byref(unseen))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device), int(unseen.value)

    def __len__(self):
        return self.count

    def visibility(self):
        """(offsets int64 [N + 1], views int32 [offsets[N]]): point k is seen by views[offsets[k]:offsets[k + 1]], its own view first,
        then its agreeing sources as indices of views of the fusion call in ascending bit order of sources[k].  Built by the library
        on the first call, on the device for a device result."""
        if self._lists is None:
            if not self._p:
                raise ApdError("Points.visibility: the points are closed")
            L = lib()
            offsets, views = C.c_void_p(), C.c_void_p()
            rc = L.apd_points_visibility(self._p, C.byref(offsets), C.byref(views))
            if rc != 0:
                raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
            off = self._array(offsets.value, (self.count + 1,), "<i8", 8)
            self._lists = (off, self._array(views.value, (int(off[-1]),), "<i4", 4))
        return self._lists

    def write_vis(self, path):
        """COLMAP's fused.ply.vis of these points (apd_points_write_vis): the lists of visibility()."""
        if not self._p:
            raise ApdError("Points.write_vis: the points are closed")
        L = lib()
        rc = L.apd_points_write_vis(self._p, str(path).encode())
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    def average(self, cameras, depths, normals, maps_on_device=False):
        """apd_points_average: a new Points with every point's xyz and normal replaced by the mean over its own view and its agreeing
        sources, sources / support reduced to the sources that contributed; these points stay as they are.  cameras: the fusion
        call's (a ctypes array or a sequence of Camera); depths, normals: per view float32 [H, W] and [H, W, 3] at the fusion
        call's sizes, numpy arrays or, with maps_on_device, torch tensors on the points' device.  The result lives where these points live."""
        if not self._p:
            raise ApdError("Points.average: the points are closed")
        L = lib()
        V = len(cameras)
        if len(depths) != V or len(normals) != V:
            raise ValueError("Points.average: %d cameras, %d depth maps, %d normal maps" % (V, len(depths), len(normals)))
        cams = cameras if isinstance(cameras, C.Array) else (Camera * V)(*cameras)

        def prepared(a):
            if maps_on_device:
                import torch
                return a.to(torch.float32).contiguous()
            return np.ascontiguousarray(a, np.float32)

        deps, nors = [prepared(d) for d in depths], [prepared(n) for n in normals]
        for d, n in zip(deps, nors):
            if d.ndim != 2 or tuple(n.shape) != tuple(d.shape) + (3,):
                raise ValueError("Points.average: depth maps are [H, W], normal maps [H, W, 3]")
        rows, cols = (C.c_int * V)(*[d.shape[0] for d in deps]), (C.c_int * V)(*[d.shape[1] for d in deps])
        if maps_on_device:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))  # the tensors' producers, before the library's stream reads them
        out = C.c_void_p()
        rc = L.apd_points_average(self._p, V, C.byref(cams), (C.c_void_p * V)(*[_ptr(a) for a in deps]), (C.c_void_p * V)(*[_ptr(a) for a in nors]),
                                  rows, cols, int(bool(maps_on_device)), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Points(out, self.device)

    def write_ply(self, path, normals=False):
        """The PLY file of these points (apd_points_write_ply): ExportPointCloud's header and records, with nx ny nz when `normals`."""
        if not self._p:
            raise ApdError("Points.write_ply: the points are closed")
        L = lib()
        rc = L.apd_points_write_ply(self._p, str(path).encode(), int(bool(normals)))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    def close(self):
        if self._p:
            lib().apd_points_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mesh:
    """An indexed triangle mesh (apd_mesh_t) as Volume.extract_mesh() or Mesh.from_arrays() makes it: vertices float32 [n, 3], colours
    uint8 [n, 3] (blue, green, red; None for a mesh without colour), normals float32 [n, 3] (None until with_vertex_normals() has
    made them) and faces int32 [m, 3], numpy arrays that are copies and outlive the object; write_ply() writes the library's file
    (apd_mesh_write_ply).  weld(), remove_small_components(), smooth(), simplify() and with_vertex_normals() each give a new Mesh and
    leave this one as it is (arithmetic contracts C22, C23 and C24); components() labels the faces, adjacency() tells every vertex's
    valence and whether the mesh is closed and manifold.  render() rasterises the mesh into a camera, face_visibility() counts the
    cameras that see each face and remove_unseen() drops the faces too few see (contract C25); colour_from_views() gives the Mesh whose
    vertices have the colour of the images of the cameras that see them (contract C26).  nearest() gives the closest point of the
    surface for every point of a Points, sample_points() a Points drawn on the surface by area and score() the precision, recall and
    F-score of the surface against a ground-truth Points (contract C27).  `moved`: after smooth(), on this mesh and on the result, the vertices the first step moved.  A mesh may
    be empty."""

    PLACEMENTS = {"mean": 0, "quadric": 1}   # APD_SIMPLIFY_MEAN, APD_SIMPLIFY_QUADRIC
    BOUNDARIES = {"fixed": 0, "along": 1, "free": 2}   # APD_SMOOTH_BOUNDARY_FIXED, _ALONG, _FREE
    CULLS = {"none": 0, "back": 1}   # APD_RENDER_CULL_NONE, _BACK
    moved = None
    unseen = None          # after face_visibility(): the faces no camera sees
    removed_faces = None   # after remove_unseen(), on this mesh and on the result: the faces that went
    uncoloured = None      # after colour_from_views(), on this mesh and on the result: the vertices no camera gave a colour
    coloured_views = None  # on the result of colour_from_views(): uint32 [n], the views each vertex took a sample from

    def __init__(self, handle):
        self._m = handle
        self.refresh()

    def refresh(self):
        """Reads vertices, colours, normals and faces from the device again.  No call changes a mesh, so this changes nothing; it is
        how a test shows that."""
        if not self._m:
            raise ApdError("Mesh.refresh: the mesh is closed")
        L = lib()
        handle = self._m
        nv, nf = C.c_longlong(0), C.c_longlong(0)
        rc = L.apd_mesh_counts(handle, C.byref(nv), C.byref(nf))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        self.vertices, self.faces = np.zeros((nv.value, 3), np.float32), np.zeros((nf.value, 3), np.int32)
        self.colours = np.zeros((nv.value, 3), np.uint8) if L.apd_mesh_has_colour(handle) else None
        if nv.value or nf.value:
            rc = L.apd_mesh_download(handle, C.c_void_p(self.vertices.ctypes.data), None if self.colours is None else C.c_void_p(self.colours.ctypes.data),
                                     C.c_void_p(self.faces.ctypes.data))
            if rc != 0:
                raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        self.normals = None
        if L.apd_mesh_has_normals(handle):
            self.normals = np.zeros((nv.value, 3), np.float32)
            rc = L.apd_mesh_download_normals(handle, C.c_void_p(self.normals.ctypes.data))
            if rc != 0:
                raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    @classmethod
    def from_arrays(cls, vertices, faces, colours=None, device=0):
        """apd_mesh_create: a Mesh on GPU `device` of copies of the arrays: vertices [n, 3] float32, faces [m, 3] int32 with every index
        in [0, n), colours [n, 3] uint8 (blue, green, red) or None.  A face may repeat an index."""
        L = lib()
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        c = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
        if c is not None and len(c) != len(v):
            raise ValueError("Mesh.from_arrays: %d colours for %d vertices" % (len(c), len(v)))
        out = C.c_void_p()
        rc = L.apd_mesh_create(int(device), len(v), C.c_void_p(v.ctypes.data) if len(v) else None, None if c is None else C.c_void_p(c.ctypes.data),
                               len(f), C.c_void_p(f.ctypes.data) if len(f) else None, 0, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return cls(out)

    def _open(self, what):
        if not self._m:
            raise ApdError("Mesh.%s: the mesh is closed" % what)
        return lib()

    def weld(self, tolerance, origin=None):
        """apd_mesh_weld: the Mesh whose vertices within `tolerance` of each other, through chains, are the one of them with the
        smallest index; faces that name a vertex twice after that and vertices no face names are gone.  origin: of the grid of cell
        size `tolerance`, (0, 0, 0) unless given.  A tolerance far below the voxel size welds only coincident vertices."""
        L = self._open("weld")
        out = C.c_void_p()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        rc = L.apd_mesh_weld(self._m, float(tolerance), org, C.byref(out), None, None)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Mesh(out)

    def components(self):
        """apd_mesh_components: (label uint32 [m], size uint32 [m], count) of the faces' connected components, two faces being
        adjacent when they name a common vertex: the smallest face index of each face's component and its number of faces."""
        L = self._open("components")
        label, size = np.zeros(len(self.faces), np.uint32), np.zeros(len(self.faces), np.uint32)
        count = C.c_longlong(0)
        rc = L.apd_mesh_components(self._m, C.c_void_p(label.ctypes.data), C.c_void_p(size.ctypes.data), C.byref(count))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return label, size, count.value

    def remove_small_components(self, min_faces):
        """apd_mesh_remove_small_components: the Mesh of the faces whose component has at least min_faces faces, and of the vertices they
        name."""
        L = self._open("remove_small_components")
        if not 0 <= int(min_faces) < 2 ** 32:
            raise ValueError("Mesh.remove_small_components: min_faces %r" % (min_faces,))
        out = C.c_void_p()
        rc = L.apd_mesh_remove_small_components(self._m, int(min_faces), C.byref(out), None, None)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Mesh(out)

    def adjacency(self):
        """apd_mesh_adjacency: (valence uint32 [n], boundary bool [n], edges, boundary_edges, nonmanifold_edges) of the vertex-to-vertex
        adjacency (contract C24): every vertex's number of distinct neighbours and whether one of its edges has a single face side, and
        the numbers of undirected edges, of edges with one face side and of edges with three or more.  A closed mesh has no boundary
        edge, a manifold one no non-manifold edge."""
        L = self._open("adjacency")
        valence, boundary = np.zeros(len(self.vertices), np.uint32), np.zeros(len(self.vertices), np.uint8)
        counts = [C.c_longlong(0) for _ in range(3)]
        rc = L.apd_mesh_adjacency(self._m, C.c_void_p(valence.ctypes.data), C.c_void_p(boundary.ctypes.data), *[C.byref(c) for c in counts])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return (valence, boundary.astype(bool)) + tuple(c.value for c in counts)

    def smooth(self, iterations, lam=0.5, mu=-0.53, boundary="along"):
        """apd_mesh_smooth: the Mesh after `iterations` iterations of smoothing (arithmetic contract C24): every vertex moves by `lam`
        towards the mean of its neighbours and then, unless mu is 0, by `mu` (negative: away from it).  lam = 0.5 with mu = -0.53 is
        Taubin's pair, which does not shrink the surface; mu = 0 is plain Laplacian smoothing.  boundary: what becomes of the vertices
        on an edge with a single face: "fixed" holds them, "along" moves them among their neighbours along the border, "free" treats
        them as the rest.  Same faces, colours and vertex count; no normals: with_vertex_normals() is the step to run after.
        `moved` of this Mesh and of the result is then the number of vertices the first step moved."""
        L = self._open("smooth")
        if boundary not in self.BOUNDARIES:
            raise ValueError("Mesh.smooth: boundary %r, none of 'fixed', 'along' and 'free'" % (boundary,))
        out, moved = C.c_void_p(), C.c_longlong(0)
        rc = L.apd_mesh_smooth(self._m, int(iterations), float(lam), float(mu), self.BOUNDARIES[boundary], C.byref(out), C.byref(moved))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        result = Mesh(out)
        self.moved = result.moved = moved.value
        return result

    def _cull(self, what, cull):
        if cull not in self.CULLS:
            raise ValueError("Mesh.%s: cull %r, neither 'none' nor 'back'" % (what, cull))
        return self.CULLS[cull]

    def render(self, camera, cull="none"):
        """apd_mesh_render: (depth float32 [height, width], face uint32 [height, width]) -- this mesh rasterised into `camera` (a
        Camera: K, R, t, width, height) with a z-buffer (arithmetic contract C25): per pixel the perspective-correct depth of the
        nearest face that covers the pixel centre and that face's index, the lowest among equal depths; 0 and 0xFFFFFFFF where no
        face covers.  cull: "none" draws both sides, "back" only the faces whose right-hand normal points at the camera.  A face
        with a corner behind the camera or beyond the guard band of 2^19 pixels is not drawn at all: there is no clipping."""
        L = self._open("render")
        cam = Camera.from_buffer_copy(camera)
        shape = (max(int(cam.height), 0), max(int(cam.width), 0))
        depth, face = np.zeros(shape, np.float32), np.zeros(shape, np.uint32)
        nothing = (C.c_uint32 * 1)()   # where a camera without pixels gets its no maps: the library refuses the camera, not a NULL
        rc = L.apd_mesh_render(self._m, C.byref(cam), self._cull("render", cull),
                               *[C.c_void_p(a.ctypes.data if a.size else C.addressof(nothing)) for a in (depth, face)])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return depth, face

    @staticmethod
    def _cameras(cameras):
        return cameras if isinstance(cameras, C.Array) else (Camera * max(len(cameras), 1))(*[Camera.from_buffer_copy(c) for c in cameras])

    def face_visibility(self, cameras, cull="back", min_pixels=1, rel_tolerance=0.01):
        """apd_mesh_face_visibility: (views uint32 [m], pixels uint64 [m]) -- per face the number of `cameras` (a ctypes array or a
        sequence of Camera) that see it and the pixels it owns in their face maps together; `unseen` of this Mesh is then the number
        of faces no camera sees.  A camera sees a face that is drawn into it and either owns at least min_pixels pixels of
        render(camera, cull)'s face map or has all three corners within rel_tolerance * z behind the depth z at their own pixels."""
        L = self._open("face_visibility")
        views, pixels = np.zeros(len(self.faces), np.uint32), np.zeros(len(self.faces), np.uint64)
        unseen = C.c_longlong(0)
        cams = self._cameras(cameras)
        rc = L.apd_mesh_face_visibility(self._m, len(cameras), C.byref(cams), self._cull("face_visibility", cull), int(min_pixels), float(rel_tolerance),
                                        C.c_void_p(views.ctypes.data), C.c_void_p(pixels.ctypes.data), C.byref(unseen))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        self.unseen = unseen.value
        return views, pixels

    def remove_unseen(self, cameras, min_views=1, cull="back", min_pixels=1, rel_tolerance=0.01):
        """apd_mesh_remove_unseen: the Mesh of the faces that at least min_views of `cameras` see (face_visibility) and of the
        vertices they name, colours and normals carried; `removed_faces` of this Mesh and of the result is then the number of faces
        that went.  min_views = 0 keeps every face."""
        L = self._open("remove_unseen")
        out, faces = C.c_void_p(), C.c_longlong(0)
        cams = self._cameras(cameras)
        rc = L.apd_mesh_remove_unseen(self._m, len(cameras), C.byref(cams), self._cull("remove_unseen", cull), int(min_pixels), float(rel_tolerance),
                                      int(min_views), C.byref(out), C.byref(faces), None)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        result = Mesh(out)
        self.removed_faces = result.removed_faces = faces.value
        return result

    def colour_from_views(self, cameras, images, rel_tolerance=0.01, min_cos=0.1):
        """apd_mesh_colour_from_views: the Mesh with these vertices, faces and normals whose every vertex has the colour of the
        `images` of the `cameras` (a ctypes array or a sequence of Camera) that see it (arithmetic contract C26): a view gives a vertex
        a bilinear sample when the four pixels around its projection are inside the image and not more than rel_tolerance * z behind
        the depth z of this mesh rendered into the view (both sides drawn), and the vertex normal (with_vertex_normals()'s, where
        this mesh has none) makes a cosine above min_cos with the direction to the camera; that cosine weighs the sample.  images:
        per view float32 [height, width] or [height, width, 3] (blue, green, red), all alike: numpy arrays, or torch tensors on the
        mesh's device.  A vertex no view colours keeps its colour, (0, 0, 0) on a mesh without.  `coloured_views` of the result is
        the number of views each vertex took a sample from, `uncoloured` of this Mesh and of the result the vertices with none."""
        L = self._open("colour_from_views")
        V = len(cameras)
        if len(images) != V:
            raise ValueError("Mesh.colour_from_views: %d cameras, %d images" % (V, len(images)))
        cams = self._cameras(cameras)
        on_device = V > 0 and all(hasattr(a, "data_ptr") for a in images)
        if on_device:
            import torch
            imgs = [a.to(torch.float32).contiguous() for a in images]
            for a in imgs:
                if not a.is_cuda:
                    raise ValueError("Mesh.colour_from_views: torch tensors are images on the mesh's device, not on %s" % a.device)
            torch.cuda.synchronize(imgs[0].device)  # the tensors' producers, before the library's stream reads them
        else:
            if any(hasattr(a, "data_ptr") for a in images):
                raise ValueError("Mesh.colour_from_views: the images are numpy arrays or torch tensors on the mesh's device, all alike")
            imgs = [np.ascontiguousarray(a, np.float32) for a in images]
        channels = 3 if V > 0 and imgs[0].ndim == 3 else 1
        for s in range(V):
            shape = (int(cams[s].height), int(cams[s].width))
            if shape[0] > 0 and shape[1] > 0 and tuple(imgs[s].shape) != shape + ((3,) if channels == 3 else ()):   # a camera without pixels is the library's to refuse
                raise ValueError("Mesh.colour_from_views: view %d has an image of %r and a camera of %r; images are [H, W] or [H, W, 3], all alike" % (
                    s, tuple(imgs[s].shape), shape))
        table = (C.c_void_p * max(V, 1))(*[_ptr(a) for a in imgs])
        out, none = C.c_void_p(), C.c_longlong(0)
        views = np.zeros(len(self.vertices), np.uint32)
        rc = L.apd_mesh_colour_from_views(self._m, V, C.byref(cams), table, channels, int(on_device), float(rel_tolerance), float(min_cos), C.byref(out),
                                          C.c_void_p(views.ctypes.data) if len(views) else None, C.byref(none))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        result = Mesh(out)
        result.coloured_views = views
        self.uncoloured = result.uncoloured = none.value
        return result

    def nearest(self, points, radius, origin=None):
        """apd_mesh_nearest: (distance float32 [N], face int32 [N], closest float32 [N, 3]) -- per point of `points` (a Points) the
        distance to the closest point of this mesh's surface within `radius`, the face it lies on and the point itself (arithmetic
        contract C27: binary64 on the widened coordinates, among equally near faces the smallest index; the grid of cell size
        `radius` with a corner at `origin`, 0, 0, 0 by default, bounds what is searched), +inf, -1 and NaN where there is none.
        numpy arrays for host points, torch tensors on their device for device points.  Computed on the mesh's device: host points go
        up for the call, device points must live there."""
        L = self._open("nearest")
        if not isinstance(points, Points) or not points._p:
            raise ApdError("Mesh.nearest: the points are closed or not a Points")
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        nothing = (C.c_float * 3)()   # where an object without points gets its no results: the library refuses NULL for all three
        n = points.count
        if points.on_device:
            import torch
            dev = torch.device("cuda", points.device)
            distance, face = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            closest = torch.empty((n, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            addresses = [a.data_ptr() if n else C.addressof(nothing) for a in (distance, face, closest)]
        else:
            distance, face, closest = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
            addresses = [a.ctypes.data if n else C.addressof(nothing) for a in (distance, face, closest)]
        rc = L.apd_mesh_nearest(self._m, points._p, float(radius), org, *[C.c_void_p(a) for a in addresses])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return distance, face, closest

    def sample_points(self, density, seed=0, on_device=True):
        """apd_mesh_sample_points: a Points of points drawn on the surface uniformly by area, `density` per unit of area in
        expectation (face f gets floor(area * density + u) of them, u in [0, 1) from a counter-based generator keyed by seed and f),
        each with the unit normal of its face and the barycentric mix of its face's vertex colours; faces ascending.  `face` of the
        result is int32 [N]: the face each sample lies on.  A function of (mesh, density, seed) alone.  on_device: the points live on
        the mesh's GPU; otherwise in host memory.  A Points like that of Points.read_ply: one view of 1 x 1 without sources."""
        L = self._open("sample_points")
        density, seed = float(density), int(seed)
        if not (density > 0.0 and np.isfinite(density)):
            raise ValueError("Mesh.sample_points: a density of %r, not a positive finite number" % (density,))
        if not 0 <= seed < 2 ** 64:
            raise ValueError("Mesh.sample_points: seed %r, not in 0 .. 2^64 - 1" % (seed,))
        # room for every sample's face: per face at most floor(area * density) + 1, and 1 more for this estimate's own rounding
        with np.errstate(all="ignore"):
            v = self.vertices.astype(np.float64)
            cross = np.cross(v[self.faces[:, 1]] - v[self.faces[:, 0]], v[self.faces[:, 2]] - v[self.faces[:, 0]]) if len(self.faces) else np.zeros((0, 3))
            room = np.floor(0.5 * np.sqrt((cross * cross).sum(1)) * density) + 2.0
        room = float(np.where(np.isfinite(room), room, 2.0).sum())
        if room >= 2.0 ** 31 + 2.0 * len(self.faces):
            raise ApdError("Mesh.sample_points: about %.3g samples at a density of %g, 2^31 or more" % (room, density))
        face = np.zeros(int(room), np.int32)
        out = C.c_void_p()
        rc = L.apd_mesh_sample_points(self._m, density, seed, int(bool(on_device)), C.byref(out), C.c_void_p(face.ctypes.data) if face.size else None)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        result = Points(out, int(L.apd_mesh_device(self._m)))
        result.face = face[:result.count].copy()
        return result

    def score(self, truth, threshold, density=None, seed=0, origin=None):
        """apd_mesh_score: Score(n_p, n_q, p_within, q_within, precision, recall, fscore, mean_p, mean_q) of this surface against
        `truth` (a Points) at `threshold` (contract C27).  Precision: the share of sample_points(density, seed) that have a point of
        `truth` within the threshold (p_within of n_p samples); recall: the share of `truth` whose closest point of the surface is
        within it (q_within of n_q) -- exact, independent of the sampling; fscore their harmonic mean; mean_p and mean_q the mean
        distances of those that have one.  density: None gives 4 / threshold^2.  As Points.score: no cropping volume and no
        occlusion-aware evaluation; scores compare with each other.  Computed on the mesh's device."""
        L = self._open("score")
        if not isinstance(truth, Points) or not truth._p:
            raise ApdError("Mesh.score: the truth is closed or not a Points")
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("Mesh.score: seed %r, not in 0 .. 2^64 - 1" % (seed,))
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        out = PointsScore()
        rc = L.apd_mesh_score(self._m, truth._p, float(threshold), org, 0.0 if density is None else float(density), seed, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Score(*[getattr(out, n) for n in Score._fields])

    def simplify(self, cell, origin=None, placement="quadric"):
        """apd_mesh_simplify: the Mesh thinned by vertex clustering (arithmetic contract C23): the vertices of one cell of the grid of
        cell size `cell` at `origin` ((0, 0, 0) unless given) become one vertex, at their mean ("mean") or where the quadric of the
        faces around them puts it ("quadric": on the surface, on creases and corners); faces that collapse and all but the first
        of equal faces go.  The result has colours as this mesh and no normals: with_vertex_normals() is the step to run after."""
        L = self._open("simplify")
        if placement not in self.PLACEMENTS:
            raise ValueError("Mesh.simplify: placement %r, neither 'mean' nor 'quadric'" % (placement,))
        out = C.c_void_p()
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        rc = L.apd_mesh_simplify(self._m, float(cell), org, self.PLACEMENTS[placement], C.byref(out), None, None)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Mesh(out)

    def with_vertex_normals(self):
        """apd_mesh_with_vertex_normals: the Mesh with area-weighted vertex normals (`normals`), summed in binary64 in a fixed order."""
        L = self._open("with_vertex_normals")
        out = C.c_void_p()
        rc = L.apd_mesh_with_vertex_normals(self._m, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Mesh(out)

    def write_ply(self, path):
        """apd_mesh_write_ply: binary little-endian, x y z float (with normals nx ny nz float; with colour red green blue uchar), then
        the faces as lists of three ints.  Points.read_ply reads the file back as its vertices."""
        if not self._m:
            raise ApdError("Mesh.write_ply: the mesh is closed")
        L = lib()
        rc = L.apd_mesh_write_ply(self._m, os.fspath(path).encode())
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    def close(self):
        if self._m:
            lib().apd_mesh_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Volume:
    """A truncated signed distance volume on GPU `device` (apd_volume_t; arithmetic contract C21): dims = (nx, ny, nz) samples, sample
    (i, j, k) at origin + (i, j, k) * voxel with the linear index i + nx * (j + ny * k); per sample a distance in units of `trunc`,
    clamped above at 1, and a weight that saturates at max_weight; with colour=True also blue, green, red and a colour weight.
    integrate() adds views, extract_mesh() gives the marching-tetrahedra Mesh of the zero level, state() / set_state() copy the
    samples to and from numpy.  Making one touches no device; its memory (8 bytes a sample, 24 with colour) is allocated by the
    first call that needs it."""

    def __init__(self, dims, origin, voxel, trunc, max_weight=64.0, colour=False, device=0):
        L = lib()
        nx, ny, nz = [int(d) for d in dims]
        out = C.c_void_p()
        rc = L.apd_volume_create(int(device), nx, ny, nz, (C.c_float * 3)(*[float(x) for x in origin]), float(voxel), float(trunc), float(max_weight),
                                 int(bool(colour)), C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        self._v = out
        self.dims, self.origin = (nx, ny, nz), np.array([float(x) for x in origin], np.float32)
        self.voxel, self.trunc, self.max_weight = np.float32(voxel), np.float32(trunc), np.float32(max_weight)
        self.colour, self.device = bool(colour), int(device)

    @classmethod
    def around(cls, lo, hi, voxel, trunc, margin=None, **kw):
        """A Volume whose samples cover the box lo .. hi grown by `margin` (trunc unless given) on every side: origin = lo - margin
        in binary32, and per axis the fewest samples, at least 2, whose last one is at or past hi + margin."""
        margin = np.float32(trunc if margin is None else margin)
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
            raise ValueError("Volume.around: a box from %r to %r" % (lo.tolist(), hi.tolist()))
        origin = (lo - margin).astype(np.float32)
        extent = ((hi + margin) - origin).astype(np.float64)
        dims = np.maximum(2, np.ceil(extent / float(np.float32(voxel))).astype(np.int64) + 1)
        return cls(tuple(int(d) for d in dims), origin, voxel, trunc, **kw)

    @property
    def samples(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def integrate(self, cameras, depths, images=None, weights=None, maps_on_device=False):
        """apd_volume_integrate: the views, in order, into the volume.  cameras: a ctypes array or a sequence of Camera whose K and
        width / height are those of the maps; depths: per view float32 [height, width]; images: per view float32 [height, width] or
        [height, width, 3] (blue, green, red), for a volume with colour; weights: per view, 1 unless given.  numpy arrays, or with
        maps_on_device torch tensors on the volume's device."""
        if not self._v:
            raise ApdError("Volume.integrate: the volume is closed")
        L = lib()
        V = len(cameras)
        if len(depths) != V or (images is not None and len(images) != V) or (weights is not None and len(weights) != V):
            raise ValueError("Volume.integrate: %d cameras, %d depth maps%s%s" % (V, len(depths), "" if images is None else ", %d images" % len(images),
                                                                                "" if weights is None else ", %d weights" % len(weights)))
        cams = cameras if isinstance(cameras, C.Array) else (Camera * max(V, 1))(*[Camera.from_buffer_copy(c) for c in cameras])

        def prepared(a):
            if maps_on_device:
                import torch
                if not hasattr(a, "data_ptr") or a.device != torch.device("cuda", self.device):
                    raise ValueError("Volume.integrate: with maps_on_device every map is a torch tensor on cuda:%d, not %s" % (
                        self.device, "on %s" % a.device if hasattr(a, "device") else type(a).__name__))
                return a.to(torch.float32).contiguous()
            return np.ascontiguousarray(a, np.float32)

        deps = [prepared(d) for d in depths]
        imgs = None if images is None else [prepared(m) for m in images]
        channels = 1
        for s in range(V):
            shape = (int(cams[s].height), int(cams[s].width))
            if shape[0] > 0 and shape[1] > 0 and tuple(deps[s].shape) != shape:   # a camera without pixels is the library's to refuse
                raise ValueError("Volume.integrate: view %d has a depth map of %r and a camera of %r" % (s, tuple(deps[s].shape), shape))
            if imgs is not None:
                channels = 3 if imgs[s].ndim == 3 else 1
                if tuple(imgs[s].shape) != tuple(deps[s].shape) + ((3,) if channels == 3 else ()) or (imgs[s].ndim == 3) != (imgs[0].ndim == 3):
                    raise ValueError("Volume.integrate: images are [H, W] or [H, W, 3] at the size of the depth maps, all alike")
        if maps_on_device:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))  # the tensors' producers, before the library's stream reads them
        table = lambda arrs: None if arrs is None else (C.c_void_p * max(V, 1))(*[_ptr(a) for a in arrs])
        w = None if weights is None else (C.c_float * max(V, 1))(*[float(x) for x in weights])
        rc = L.apd_volume_integrate(self._v, V, C.byref(cams), table(deps), table(imgs), channels, w, int(bool(maps_on_device)))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    def state(self):
        """apd_volume_download: (tsdf float32 [samples], weight float32 [samples], colour float32 [samples, 4] or None), in linear
        order."""
        if not self._v:
            raise ApdError("Volume.state: the volume is closed")
        L = lib()
        tsdf, weight = np.zeros(self.samples, np.float32), np.zeros(self.samples, np.float32)
        colour = np.zeros((self.samples, 4), np.float32) if self.colour else None
        rc = L.apd_volume_download(self._v, C.c_void_p(tsdf.ctypes.data), C.c_void_p(weight.ctypes.data),
                                   None if colour is None else C.c_void_p(colour.ctypes.data))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return tsdf, weight, colour

    def set_state(self, tsdf, weight, colour=None):
        """apd_volume_upload: the samples from arrays in the shapes of state(); None leaves an array as it is."""
        if not self._v:
            raise ApdError("Volume.set_state: the volume is closed")
        L = lib()
        arrays = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (tsdf, weight, colour)]
        for a, width in zip(arrays, (1, 1, 4)):
            if a is not None and a.size != self.samples * width:
                raise ValueError("Volume.set_state: an array of %d elements for %d samples" % (a.size, self.samples))
        rc = L.apd_volume_upload(self._v, *[None if a is None else C.c_void_p(a.ctypes.data) for a in arrays])
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))

    def extract_mesh(self):
        """apd_volume_extract_mesh: the Mesh of the volume as it is now."""
        if not self._v:
            raise ApdError("Volume.extract_mesh: the volume is closed")
        L = lib()
        out = C.c_void_p()
        rc = L.apd_volume_extract_mesh(self._v, C.byref(out))
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
        return Mesh(out)   # the mesh is the object's from its first line on

    def close(self):
        if self._v:
            lib().apd_volume_destroy(self._v)
            self._v = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_camera(K, R, t, width, height, depth_min, depth_max):
    """Fills a camera the way ReadCamera does (APD.cpp:51-92): c = -R^T t evaluated in double."""
    cam = Camera()
    K = np.asarray(K, np.float32).reshape(9)
    R = np.asarray(R, np.float32).reshape(9)
    t = np.asarray(t, np.float32).reshape(3)
    for i in range(9):
        cam.K[i] = float(K[i])
        cam.R[i] = float(R[i])
    for i in range(3):
        cam.t[i] = float(t[i])
    Rd, td = R.astype(np.float64), t.astype(np.float64)
    for j in range(3):
        cam.c[j] = float(np.float32(-(Rd[0 + j] * td[0] + Rd[3 + j] * td[1] + Rd[6 + j] * td[2])))
    cam.width, cam.height = int(width), int(height)
    cam.depth_min, cam.depth_max = float(depth_min), float(depth_max)
    return cam


def _ptr(a):
    """Raw address of a numpy array or torch tensor (host or device), or None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


_STATE_DTYPES = {
    STATE_PLANES: (np.float32, 4), STATE_FIT_PLANES: (np.float32, 4), STATE_COSTS: (np.float32, 1),
    STATE_RNG: (np.uint32, 6), STATE_SELECTED_VIEWS: (np.uint32, 1), STATE_VIEW_WEIGHT: (np.uint8, 32),
    STATE_WEAK_INFO: (np.uint8, 1), STATE_WEAK_RELIABLE: (np.uint8, 1), STATE_NEAREST_STRONG: (np.int16, 2),
    STATE_NEIGHBOURS_MAP: (np.int32, 1),
}


class SharedImage:
    """apd_image_create: one W x H float image (numpy or torch, host or device) on the device, tested and packed once."""

    def __init__(self, width, height, pixels, device=0):
        if hasattr(pixels, "data_ptr"):
            import torch
            pixels = pixels.to(torch.float32).contiguous()
            assert pixels.numel() == width * height
        else:
            pixels = np.ascontiguousarray(pixels, np.float32)
            assert pixels.size == width * height
        self._keep = pixels
        p = C.c_void_p()
        _check(lib().apd_image_create(C.byref(p), device, width, height, _ptr(pixels)))
        self.ptr = p.value

    def close(self):
        if self.ptr:
            lib().apd_image_destroy(self.ptr)
            self.ptr = None


class Handle:
    """One (reference view, pass): the C-ABI equivalent of the reference's `APD` object (APD.h:67-145)."""

    def __init__(self, width, height, params, device=-1):
        self._h = C.c_void_p()
        self.W, self.H = int(width), int(height)
        self.params = params
        self.device = int(device)
        self._keep = []
        _check(lib().apd_create(C.byref(self._h), device, self.W, self.H, C.byref(params)))

    def close(self):
        if self._h:
            lib().apd_destroy(self._h)
            self._h = C.c_void_p()

    def reset(self, params):
        """Re-arms the handle for another (view, pass) of the same size (apd_reset): same initial state as a new one."""
        _check(lib().apd_reset(self._h, C.byref(params)))   # a refused reset leaves the handle, and this object, as they were
        self.params = params
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        """apd_set_option; `option` is an OPT_* constant or one of OPTION_NAMES.  Upload-time options (source_quads,
        tiled_copy) must be set before upload_views."""
        opt = OPTION_NAMES[option] if isinstance(option, str) else int(option)
        _check(lib().apd_set_option(self._h, opt, int(value)))

    def get_option(self, option):
        opt = OPTION_NAMES[option] if isinstance(option, str) else int(option)
        v = C.c_int()
        _check(lib().apd_get_option(self._h, opt, C.byref(v)))
        return v.value

    def upload_views(self, cameras, images, depths=None):
        """images/depths: lists of float32 [H, W] numpy arrays or torch tensors (host or device)."""
        n = len(cameras)
        imgs = [self._as_f32(im) for im in images]
        deps = None if depths is None else [self._as_f32(d) for d in depths]
        self._keep = [imgs, deps]
        cam_arr = (Camera * n)(*cameras)
        ip = (C.c_void_p * n)(*[_ptr(a) for a in imgs])
        dp = None if deps is None else (C.c_void_p * n)(*[_ptr(a) for a in deps])
        _check(lib().apd_upload_views(self._h, n, cam_arr, ip, dp))
        self.params.num_images = n

    def upload_views_split(self, cameras, images):
        """apd_upload_views_split: a geometric pass whose depth maps follow with upload_depths."""
        n = len(cameras)
        imgs = [self._as_f32(im) for im in images]
        self._keep = [imgs, None]
        cam_arr = (Camera * n)(*cameras)
        ip = (C.c_void_p * n)(*[_ptr(a) for a in imgs])
        _check(lib().apd_upload_views_split(self._h, n, cam_arr, ip))
        self.params.num_images = n

    def upload_views_shared(self, cameras, images):
        """apd_upload_views_shared: `images` are SharedImage objects (created once, used by any number of handles); in a geometric
        pass the depth maps follow with upload_depths."""
        n = len(cameras)
        self._keep = [list(images), None]
        cam_arr = (Camera * n)(*cameras)
        ip = (C.c_void_p * n)(*[im.ptr for im in images])
        _check(lib().apd_upload_views_shared(self._h, n, cam_arr, ip))
        self.params.num_images = n

    def upload_depths(self, depths):
        deps = [self._as_f32(d) for d in depths]
        dp = (C.c_void_p * len(deps))(*[_ptr(a) for a in deps])
        _check(lib().apd_upload_depths(self._h, len(deps), dp))

    def run_before_depths(self):
        _check(lib().apd_run_before_depths(self._h))

    def run_after_depths(self):
        _check(lib().apd_run_after_depths(self._h))
        self.synchronize()

    def _as_f32(self, a):
        if hasattr(a, "data_ptr"):
            import torch
            a = a.to(torch.float32).contiguous()
            assert a.numel() == self.W * self.H
            return a
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == self.W * self.H
        return a

    def upload_prior(self, planes=None, selected_views=None, weak_info=None):
        """numpy arrays or torch tensors (host or device): planes float32 [H, W, 4], selected views 32-bit, weak uint8."""
        def prep(a, np_dtype, itemsize):
            if a is None:
                return None
            if hasattr(a, "data_ptr"):
                a = a.contiguous()
                assert a.element_size() == itemsize
                return a
            return np.ascontiguousarray(a, np_dtype)
        p, v, w = prep(planes, np.float32, 4), prep(selected_views, np.uint32, 4), prep(weak_info, np.uint8, 1)
        self._keep_prior = (p, v, w)
        _check(lib().apd_upload_prior(self._h, _ptr(p), _ptr(v), _ptr(w)))

    def upload_mask(self, mask):
        """apd_upload_mask: uint8 (or bool) [H, W] numpy array or torch tensor (host or device), non-zero = process,
        zero = masked out; None clears the mask.  Before the first kernel of the pass."""
        if mask is None:
            m = None
        elif hasattr(mask, "data_ptr"):
            import torch
            m = mask.to(torch.uint8).contiguous()
            assert m.numel() == self.W * self.H
        else:
            m = np.ascontiguousarray(mask).astype(np.uint8, copy=False)
            assert m.size == self.W * self.H
        _check(lib().apd_upload_mask(self._h, _ptr(m)))

    def masked_count(self):
        return lib().apd_masked_count(self._h)

    def run(self):
        _check(lib().apd_run(self._h))
        self.synchronize()

    def run_kernel(self, kid, it=0, sync=True):
        _check(lib().apd_run_kernel(self._h, kid, it))
        if sync:
            self.synchronize()

    def run_sweeps(self, first_iter, iters, sync=True):
        _check(lib().apd_run_sweeps(self._h, first_iter, iters))
        if sync:
            self.synchronize()

    def synchronize(self):
        _check(lib().apd_synchronize(self._h))

    def download(self):
        n = self.W * self.H
        planes = np.empty((self.H, self.W, 4), np.float32)
        weak = np.empty((self.H, self.W), np.uint8)
        views = np.empty((self.H, self.W), np.uint32)
        _check(lib().apd_download(self._h, planes.ctypes.data, weak.ctypes.data, views.ctypes.data))
        return planes, weak, views

    def download_device(self):
        """The same three maps as torch tensors on the handle's device (device-to-device copies): planes float32
        [H, W, 4], weak uint8 [H, W], selected views as int32 bit patterns [H, W]."""
        import torch
        dev = torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())
        planes = torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev)
        weak = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        views = torch.empty((self.H, self.W), dtype=torch.int32, device=dev)
        _check(lib().apd_download(self._h, planes.data_ptr(), weak.data_ptr(), views.data_ptr()))
        return planes, weak, views

    def state(self, which):
        nbytes = lib().apd_state_bytes(self._h, which)
        if which == STATE_NEIGHBOURS:
            out = np.empty((nbytes // 36, 9, 2), np.int16)
        else:
            dt, k = _STATE_DTYPES[which]
            shape = (self.H, self.W, k) if k > 1 else (self.H, self.W)
            out = np.empty(shape, dt)
        assert out.nbytes == nbytes, (which, out.nbytes, nbytes)
        _check(lib().apd_download_state(self._h, which, out.ctypes.data, nbytes))
        return out

    def set_state(self, which, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib().apd_upload_state(self._h, which, arr.ctypes.data, arr.nbytes))

    def export_depth_normal(self, depth_dev, normal_dev=None):
        """depth_dev / normal_dev: torch CUDA tensors ([H,W] and [H,W,3] float32)."""
        _check(lib().apd_export_depth_normal_device(self._h, _ptr(depth_dev), _ptr(normal_dev)))

    def export_state(self, planes_dev=None, weak_dev=None, views_dev=None, depth_dev=None):
        """apd_export_state_device: torch CUDA tensors ([H,W,4] float32, [H,W] uint8, [H,W] int32, [H,W] float32) or None."""
        _check(lib().apd_export_state_device(self._h, _ptr(planes_dev), _ptr(weak_dev), _ptr(views_dev), _ptr(depth_dev)))

    @property
    def weak_count(self):
        return lib().apd_weak_count(self._h)

    def profile_enable(self, on=True):
        _check(lib().apd_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        _check(lib().apd_profile_reset(self._h))

    def profile(self):
        """{kernel_id: (total_ms, launches)} accumulated since the last reset."""
        out = {}
        for k in range(1, 16):
            ms, n = C.c_double(), C.c_int()
            _check(lib().apd_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            if n.value:
                out[k] = (ms.value, n.value)
        return out


def device_count():
    return lib().apd_device_count()
