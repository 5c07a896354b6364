"""In-memory multi-view, multi-scale pass scheduler for the PatchMatch path, sharded over ranks.

Mirrors the reference's driver (main.cpp:140-217): `round_num` pyramid levels x (1 photometric + 3 geometric)
passes over every reference view, with the per-pass parameters of main.cpp:171-212 and the level handling of
APD::InuputInitialization (APD.cpp:464-581).  Two things differ from the reference, both by design:

* state between passes (depth, normal, weak map, selected views per view) stays in memory instead of travelling
  through depths.dmb / normals.dmb / weak.bin / selected_views.bin; decoded and rescaled images are cached per level
  instead of being re-read for every (view, pass);
* views are sharded round-robin over the ranks of a torch.distributed group (one process per GPU).  After every
  pass the ranks all-gather the depth maps (the geometric term of the next pass reads the sources' depth maps,
  APD.cpp:492-509, APD.cu:760-772) and, after the last pass, depth + normal + weak maps (what fusion consumes).

With one rank the order of evaluation is the reference's (Gauss-Seidel over views inside a pass: later views read the
depth maps earlier views have just written) and the results are bit-identical to the drop-in binary
(tests/test_gpu_dropin_binary.py).  With G ranks a view sees this pass's maps of the views its own rank has already
processed and the previous pass's maps of everybody else's.

The compute backend is injected: `HipBackend` (the product) drives the C ABI; the CPU tests plug the oracle in.
"""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import sharding


@dataclass
class MvsScene:
    """cameras[i] (full resolution, `apd_camera`), images[i] (float32 [H, W]), pairs[i] = source view ids of view i.
    Views 0 .. num_views-1 are reference views (one pair.txt entry each).  Further cameras / images, if any, are SOURCE-ONLY
    views: images that pair.txt lists as sources but that have no entry of their own (a subset run).  The reference simply
    loads them (APD.cpp:419-452); they are never processed, contribute no depth map to the geometric term (the reference
    reads a file that does not exist there, APD.cpp:497-500) and take no part in the fusion.
    masks[i], optional: uint8 [H, W] at full resolution, non-zero = process, zero = masked out (apd_upload_mask); None for a
    view without a mask, and `masks` itself may be None."""
    cameras: list
    images: list
    pairs: list
    masks: list = None

    @property
    def num_views(self):
        return len(self.pairs)


@dataclass
class PassSpec:
    """One pass over all views (main.cpp:169-215)."""
    round_index: int
    iteration_index: int
    scale_size: int
    params: dict = field(default_factory=dict)


@dataclass
class ViewState:
    depth: np.ndarray      # float32 [H, W], 0 = invalid (main.cpp:109-112)
    normal: np.ndarray     # float32 [H, W, 3], world frame
    weak: np.ndarray       # uint8 [H, W]
    views: np.ndarray      # uint32 [H, W] selected-view bitmask


def compute_round_num(width, height):
    """main.cpp:72-88: halve until max(W, H) <= 1000 (host/schedule.h: RoundNum)."""
    return int(host_lib().apdhost_round_num(int(width), int(height)))


def pass_schedule(round_num, iters=3, single_level=False):
    """Per-pass parameters of main.cpp:168-215.  ONE implementation: the table host/schedule.h builds for the C++ schedulers
    (BuildSchedule), read through libapd_host.so; level 0 leaves ransac_threshold / rotate_time at the struct defaults, as the
    reference's long-lived PatchMatchParams does (schedule.h: Configure)."""
    L = host_lib()
    n = L.apdhost_schedule(int(round_num), 1 if single_level else 0, None, 0)
    rows = (C.c_int * (9 * n))()
    L.apdhost_schedule(int(round_num), 1 if single_level else 0, rows, n)
    out = []
    for k in range(n):
        level, iteration, scale, state, geom, use_apd, peak, rotate, thr_bits = rows[9 * k:9 * k + 9]
        p = dict(state=state, geom_consistency=geom, max_iterations=iters, weak_peak_radius=peak, use_APD=use_apd)
        if use_apd:
            p.update(ransac_threshold=float(np.array([thr_bits], np.int32).view(np.float32)[0]), rotate_time=rotate)
        out.append(PassSpec(level, iteration, scale, p))
    return out


def resize_linear(src, new_cols, new_rows):
    """cv::resize(..., INTER_LINEAR) on a float image as the C++ host does it (host/APD.cpp ResizeLinear):
    fx = (dx + 0.5) * (src/dst) - 0.5 in double, taps floor(fx), floor(fx)+1 clamped, float weights, rows after columns."""
    src = np.ascontiguousarray(src, np.float32)
    rows, cols = src.shape

    def taps(n_new, n_old):
        f = ((np.arange(n_new, dtype=np.float64) + 0.5) * (float(n_old) / n_new) - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        a = (f - i.astype(np.float32)).astype(np.float32)
        lo = i < 0
        i[lo], a[lo] = 0, 0
        hi = i >= n_old - 1
        i[hi], a[hi] = n_old - 1, 0
        return i, np.minimum(i + 1, n_old - 1), a

    x0, x1, ax = taps(new_cols, cols)
    y0, y1, ay = taps(new_rows, rows)
    one = np.float32(1.0)
    r0, r1 = src[y0], src[y1]
    top = r0[:, x0] * (one - ax) + r0[:, x1] * ax
    bot = r1[:, x0] * (one - ax) + r1[:, x1] * ax
    ay = ay[:, None]
    return (top * (one - ay) + bot * ay).astype(np.float32)


def rescale_nearest(src, target_width, target_height):
    """RescaleMatToTargetSize (APD.cpp:752-774) including its swapped factors: row / scale_x, column / scale_y."""
    rows, cols = src.shape[:2]
    if cols == target_width and rows == target_height:
        return src
    if hasattr(src, "data_ptr"):  # torch tensor (host or device): the same index arithmetic in float32
        import torch
        sx = np.float32(target_width) / np.float32(cols)
        sy = np.float32(target_height) / np.float32(rows)
        o_r = (torch.arange(target_height, dtype=torch.float32) / float(sx)).to(torch.int64)
        o_c = (torch.arange(target_width, dtype=torch.float32) / float(sy)).to(torch.int64)
        ok_r, ok_c = o_r < rows, o_c < cols
        out = torch.zeros((target_height, target_width) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
        rr = o_r.clamp(max=rows - 1).to(src.device)
        cc = o_c.clamp(max=cols - 1).to(src.device)
        picked = src[rr][:, cc]
        mask = (ok_r[:, None] & ok_c[None, :]).to(src.device)
        out[mask] = picked[mask]
        return out
    scale_x = np.float32(target_width) / np.float32(cols)
    scale_y = np.float32(target_height) / np.float32(rows)
    o_r = (np.arange(target_height, dtype=np.float32) / scale_x).astype(np.int64)
    o_c = (np.arange(target_width, dtype=np.float32) / scale_y).astype(np.int64)
    out = np.zeros((target_height, target_width) + src.shape[2:], src.dtype)
    ok_r, ok_c = o_r < rows, o_c < cols
    out[np.ix_(ok_r, ok_c)] = src[np.ix_(o_r[ok_r], o_c[ok_c])]
    return out


MASK_THRESHOLD = 128   # grey value below which a pixel of a mask file is masked out (the reference's block masks, APD.cpp:849-853)


def mask_from_grey(grey):
    """Mask file -> uint8 mask: 255 where the grey value is >= 128 (process), 0 below (masked out)."""
    return np.where(np.asarray(grey) < MASK_THRESHOLD, 0, 255).astype(np.uint8)


def level_mask(mask, width, height):
    """The full-resolution mask of a view at a pyramid level of width x height: RescaleMatToTargetSize, one byte per pixel."""
    return np.ascontiguousarray(rescale_nearest(np.ascontiguousarray(mask, np.uint8), width, height))


def level_inputs(scene, scale_size, camera_type):
    """Scaled images and intrinsics of one pyramid level (APD.cpp:464-488): every image by its own rounded size."""
    cams, imgs = [], []
    for cam, img in zip(scene.cameras, scene.images):
        c = camera_type.from_buffer_copy(cam)
        rows, cols = img.shape
        c.width, c.height = cols, rows
        if scale_size != 1:
            factor = np.float32(1.0) / np.float32(scale_size)
            new_cols = int(math.floor(float(np.float32(cols) * factor) + 0.5))   # std::round of a positive float
            new_rows = int(math.floor(float(np.float32(rows) * factor) + 0.5))
            sx = np.float32(new_cols) / np.float32(cols)
            sy = np.float32(new_rows) / np.float32(rows)
            img = resize_linear(img, new_cols, new_rows)
            c.K[0] = float(np.float32(c.K[0]) * sx)
            c.K[2] = float(np.float32(c.K[2]) * sx)
            c.K[4] = float(np.float32(c.K[4]) * sy)
            c.K[5] = float(np.float32(c.K[5]) * sy)
            c.width, c.height = new_cols, new_rows
        cams.append(c)
        imgs.append(np.ascontiguousarray(img, np.float32))
    return cams, imgs


class HipBackend:
    """One (view, pass) on the MI355X through the C ABI (== ProcessProblem, main.cpp:91-115)."""

    accepts_tensors = True  # run_pass takes and returns torch tensors on `device`: no host copies between the passes

    def __init__(self, pkg, device=0):
        self.pkg = pkg
        self.device = device
        self._pool = {}  # (width, height) -> recycled handle: no hipMalloc / hipFree per (view, pass)

    def close(self):
        for h in self._pool.values():
            h.close()
        self._pool.clear()

    @property
    def camera_type(self):
        return self.pkg.Camera

    def run_pass(self, width, height, params, cameras, images, depths, prior, mask=None):
        import torch
        # the inputs were produced on torch's stream, the handle copies and computes on its own: hand over on the host
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
        pkg = self.pkg
        h = self._pool.get((width, height))
        if h is None:
            if len(self._pool) >= 2:  # one level at a time (+ views of another size): drop what is no longer used
                self.close()
            h = pkg.Handle(width, height, pkg.default_params(**params), device=self.device)
            self._pool[(width, height)] = h
        else:
            h.reset(pkg.default_params(**params))
        h.upload_views(cameras, images, depths)
        if prior is not None:
            h.upload_prior(*prior)
        if mask is not None:   # apd_reset has forgotten the mask of the handle's previous (view, pass)
            h.upload_mask(mask)
        h.run()
        return h.download_device()


def run_pipeline(scene, backend, iters=3, seed=12345, single_level=False, group=None, max_rounds=None, max_passes=None, log=None):
    """Runs every pass of the schedule on this rank's views; returns {view: ViewState} for ALL views on every rank."""
    import torch
    import torch.distributed as dist

    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    V = scene.num_views
    mine = sharding.shard_views(V, world, rank)
    h0, w0 = scene.images[0].shape
    round_num = 1 if single_level else compute_round_num(w0, h0)
    if max_rounds is not None:
        round_num = min(round_num, max_rounds)
    schedule = pass_schedule(round_num, iters, single_level)
    if max_passes is not None:
        schedule = schedule[:max_passes]
    # Everything between the passes lives in torch tensors on the backend's device (the GPU of this rank for the HIP
    # backend): level images, depth maps of all views, prior state, post-processing, nearest-neighbour upsampling
    # (APD.cpp:752-774) and the all-gathers.  Only the final result is copied to the host.
    on_gpu = getattr(backend, "device", None) is not None and torch.cuda.is_available()
    device = torch.device("cuda", backend.device) if on_gpu else torch.device("cpu")
    tensors_in = bool(getattr(backend, "accepts_tensors", False))

    def to_dev(a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if dtype is not None:
            t = t.to(dtype)
        return t.to(device)

    def call_backend(W, H, p, cams_, imgs_, depths_, prior_, mask_=None):
        # the mask travels as a keyword, and only for a view that has one: a backend without masks keeps working for unmasked scenes
        kw = {} if mask_ is None else {"mask": mask_ if tensors_in else mask_.contiguous().numpy()}
        if tensors_in:
            return backend.run_pass(W, H, p, cams_, imgs_, depths_, prior_, **kw)
        # numpy backend (the CPU oracle in the tests): zero-copy views of the CPU tensors
        npy = lambda t: None if t is None else t.contiguous().numpy()
        pr = None if prior_ is None else (npy(prior_[0]), None if prior_[1] is None else npy(prior_[1]).view(np.uint32), npy(prior_[2]))
        planes, weak, views = backend.run_pass(W, H, p, cams_, [npy(t) for t in imgs_],
                                               None if depths_ is None else [npy(t) for t in depths_], pr, **kw)
        return to_dev(planes), to_dev(weak), to_dev(views.view(np.int32))

    state = {}        # own views: (planes4 = world normal xyz + depth w, weak, views as int32 bits) at the level last written
    depth_store = {}  # every view's depth map as this rank knows it
    level_cache = {}
    masks = getattr(scene, "masks", None) or [None] * V
    for spec in schedule:
        if spec.scale_size not in level_cache:
            level_cache.clear()
            cams, imgs = level_inputs(scene, spec.scale_size, backend.camera_type)
            # the masks of the level: nearest-neighbour like the state maps (RescaleMatToTargetSize, APD.cpp:752-774)
            lmasks = [None if masks[v] is None else to_dev(level_mask(masks[v], cams[v].width, cams[v].height)) for v in range(V)]
            level_cache[spec.scale_size] = (cams, [to_dev(im) for im in imgs], lmasks)
        cams, imgs, lmasks = level_cache[spec.scale_size]
        for idx in mine:
            order = [idx] + list(scene.pairs[idx])
            W, H = cams[idx].width, cams[idx].height
            p = dict(spec.params)
            p["num_images"] = len(order)
            p["depth_min"] = float(np.float32(cams[idx].depth_min) * np.float32(0.6))   # APD.cpp:454-455
            p["depth_max"] = float(np.float32(cams[idx].depth_max) * np.float32(1.2))
            p["seed"] = seed + spec.iteration_index * 7919 + idx
            depths = None
            if p["geom_consistency"]:
                for j in order:
                    if j >= V and j not in depth_store:  # source-only view: no estimate anywhere
                        depth_store[j] = torch.zeros((H, W), dtype=torch.float32, device=device)
                depths = [rescale_nearest(depth_store[j], W, H).contiguous() for j in order]
            prior = None
            if p["state"] != 0:
                planes0, weak0, views0 = state[idx]
                prior = (rescale_nearest(planes0, W, H).contiguous(), rescale_nearest(views0, W, H).contiguous(),
                         rescale_nearest(weak0, W, H).contiguous() if p["use_APD"] else None)
            planes, weak, views = call_backend(W, H, p, [cams[j] for j in order], [imgs[j] for j in order], depths, prior, lmasks[idx])
            d = planes[..., 3]
            bad = (d < p["depth_min"]) | (d > p["depth_max"])   # main.cpp:109-112 (float32 comparisons)
            d.masked_fill_(bad, 0)      # in place on the strided view; no host synchronisation (unlike d[bad] = 0)
            weak.masked_fill_(bad, 2)
            state[idx] = (planes, weak, views)
            depth_store[idx] = d.contiguous()
            if log:
                log("pass %d (round %d, scale %d) view %d done on rank %d" % (spec.iteration_index, spec.round_index, spec.scale_size, idx, rank))
        if distributed:  # also with one rank under an initialised process group: the collective path is the only path then
            gathered = sharding.allgather_maps({v: depth_store[v][..., None] for v in mine}, V, group=group)
            for v in range(V):
                if v not in state:
                    depth_store[v] = gathered[v, ..., 0].contiguous()

    def to_view_state(planes, weak, views):
        # split depth / normal on the device: the host then receives two contiguous arrays instead of re-packing 16 bytes per pixel
        return ViewState(planes[..., 3].contiguous().cpu().numpy(), planes[..., :3].contiguous().cpu().numpy(),
                         weak.cpu().numpy().astype(np.uint8, copy=False), views.contiguous().cpu().numpy().view(np.uint32))

    # before fusion: everybody gets every view's depth + normal + weak (+ selected views)
    if distributed:
        packed = {}
        for v in mine:
            planes, weak, views = state[v]
            packed[v] = torch.cat([planes[..., 3:4], planes[..., :3], weak[..., None].to(torch.float32),
                                   views.contiguous()[..., None].view(torch.float32)], -1)
        g = sharding.allgather_maps(packed, V, group=group)
        out = {}
        for v in range(V):
            gv = g[v]
            out[v] = to_view_state(torch.cat([gv[..., 1:4], gv[..., 0:1]], -1), gv[..., 4].to(torch.uint8),
                                   gv[..., 5].contiguous().view(torch.int32))
        return out
    return {v: to_view_state(*state[v]) for v in state}


def synthetic_ring(synth, width, height, num_views, num_src, camera_factory, seed=0, textureless=0.0):
    """`num_views` reference views on the generator's camera ring, each paired with its `num_src` nearest neighbours.
    camera_factory(K, R, t, W, H, depth_min, depth_max) builds the backend's camera struct."""
    sc = synth.make_scene(width, height, num_views - 1, seed=seed, textureless=textureless)
    imgs = sc.images_numpy()
    cams = [camera_factory(sc.K[i], sc.R[i], sc.t[i], width, height, sc.depth_min, sc.depth_max) for i in range(num_views)]
    pairs = []
    for i in range(num_views):
        others = sorted((j for j in range(num_views) if j != i), key=lambda j: (abs(j - i), j))
        pairs.append(others[:num_src])
    return MvsScene(cams, [np.ascontiguousarray(im, np.float32) for im in imgs], pairs)


# ------------------------------------------------------------------------------------------------------------------
# dense-folder I/O (the reference's on-disk contract) through the C++ host library
# ------------------------------------------------------------------------------------------------------------------

_host = None


def host_lib():
    """libapd_host.so: ReadCamera / ReadGrayImage / ReadBinMat / WriteBinMat of the drop-in host (host/APD.cpp)."""
    global _host
    if _host is None:
        import ctypes as C
        import os
        from . import lib as product_lib, LIB_PATH
        product_lib()  # libapd_host.so links against libapd_mi355x.so
        L = C.CDLL(os.path.join(os.path.dirname(LIB_PATH), "libapd_host.so"))
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        L.apdhost_read_camera.argtypes = [C.c_char_p, C.c_void_p]
        L.apdhost_read_gray_image.argtypes = [C.c_char_p, ip, ip, fp, C.c_size_t]
        L.apdhost_write_bin_mat.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.apdhost_fuse.restype = C.c_longlong
        L.apdhost_round_num.argtypes = [C.c_int, C.c_int]
        L.apdhost_schedule.argtypes = [C.c_int, C.c_int, ip, C.c_int]
        _host = L
    return _host


def read_mask_file(stem, rows, cols):
    """<stem>.jpg / .pgm as a mask of rows x cols, None if there is no such file; a file of another size is refused."""
    import ctypes as C
    import os
    if not any(os.path.exists(stem + ext) for ext in (".jpg", ".pgm")):
        return None
    L = host_lib()
    name = stem + (".jpg" if os.path.exists(stem + ".jpg") else ".pgm")
    r, c = C.c_int(), C.c_int()
    if L.apdhost_read_gray_image(stem.encode(), C.byref(r), C.byref(c), None, 0) != 0:
        raise IOError("cannot read mask %s" % name)
    if (r.value, c.value) != (rows, cols):
        raise ValueError("mask %s is %dx%d, its image is %dx%d" % (name, c.value, r.value, cols, rows))
    grey = np.empty((rows, cols), np.float32)
    L.apdhost_read_gray_image(stem.encode(), C.byref(r), C.byref(c), grey.ctypes.data_as(C.POINTER(C.c_float)), grey.size)
    return mask_from_grey(grey)


def load_dense_folder(folder, camera_type, masks_dir=None):
    """pair.txt (main.cpp:6-49: sources with score <= 0 dropped), cams/%08d_cam.txt, images/%08d.{jpg,pgm}.
    View i of the returned scene is the i-th entry of pair.txt; `ids` maps it back to the image id.
    masks_dir (e.g. "masks"): <folder>/<masks_dir>/%08d.{jpg,pgm} become scene.masks for the reference views (grey < 128 =
    masked out; a view without a file is unmasked; a file of another size than its image raises ValueError).  None: nothing
    is read, even if the directory exists."""
    import ctypes as C
    import os
    L = host_lib()
    tok = open(os.path.join(folder, "pair.txt")).read().split()
    n = int(tok[0])
    pos = 1
    ids, src_ids = [], []
    for _ in range(n):
        ids.append(int(tok[pos]))
        m = int(tok[pos + 1])
        pos += 2
        srcs = []
        for _ in range(m):
            sid, score = int(tok[pos]), float(tok[pos + 1])
            pos += 2
            if score > 0.0:
                srcs.append(sid)
        src_ids.append(srcs)
    index_of = {v: i for i, v in enumerate(ids)}
    # Sources without an entry of their own (a subset of the views is reconstructed): loaded as source-only views after the
    # reference views, like the reference loads any id it is given (APD.cpp:419-452).
    extra = []
    for v, srcs in zip(ids, src_ids):
        for s_id in srcs:
            if s_id == v:
                raise ValueError("pair.txt: view %d lists itself as a source" % v)
            if s_id not in index_of:
                index_of[s_id] = len(ids) + len(extra)
                extra.append(s_id)
    def load_view(v):
        cam = camera_type()
        if L.apdhost_read_camera(os.path.join(folder, "cams", "%08d_cam.txt" % v).encode(), C.byref(cam)) != 0:
            raise IOError("cannot read camera %d" % v)
        rows, cols = C.c_int(), C.c_int()
        stem = os.path.join(folder, "images", "%08d" % v).encode()
        if L.apdhost_read_gray_image(stem, C.byref(rows), C.byref(cols), None, 0) != 0:
            raise IOError("cannot read image %d" % v)
        img = np.empty((rows.value, cols.value), np.float32)
        L.apdhost_read_gray_image(stem, C.byref(rows), C.byref(cols), img.ctypes.data_as(C.POINTER(C.c_float)), img.size)
        cam.width, cam.height = cols.value, rows.value
        return cam, img

    # the decoder runs outside the GIL (ctypes) and the host library's image cache is locked: one thread per image
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, max(1, len(ids)))) as pool:
        loaded = list(pool.map(load_view, ids + extra))
    cams = [c for c, _ in loaded]
    imgs = [im for _, im in loaded]
    scene = MvsScene(cams, imgs, [[index_of[s] for s in srcs] for srcs in src_ids])
    scene.ids = ids + extra   # image id of every loaded view; the first scene.num_views are the reference views
    if masks_dir is not None:
        scene.masks = [read_mask_file(os.path.join(folder, masks_dir, "%08d" % v), *imgs[i].shape) for i, v in enumerate(ids)]
    return scene


def save_results(folder, scene, results):
    """<dense>/APD/<%08d>/{depths.dmb, normals.dmb, weak.bin, selected_views.bin} as ProcessProblem writes them
    (main.cpp:117-124), for the fusion step."""
    import os
    L = host_lib()
    ids = getattr(scene, "ids", list(range(scene.num_views)))
    for v, st in results.items():
        d = os.path.join(folder, "APD", "%08d" % ids[v])
        os.makedirs(d, exist_ok=True)
        rows, cols = st.depth.shape
        for name, code, arr in (("depths.dmb", 5, st.depth), ("normals.dmb", 21, st.normal), ("weak.bin", 0, st.weak),
                                ("selected_views.bin", 4, st.views)):
            a = np.ascontiguousarray(arr)
            if L.apdhost_write_bin_mat(os.path.join(d, name).encode(), rows, cols, code, a.ctypes.data) != 0:
                raise IOError("cannot write " + os.path.join(d, name))


def load_colour_images(folder, ids):
    """images/%08d.{jpg,ppm,pgm} as cv::imread(IMREAD_COLOR) returns them: float32 [H, W, 3], blue first (APD.cpp:859)."""
    import ctypes as C
    import os
    L = host_lib()
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.apdhost_read_color_image.argtypes = [C.c_char_p, ip, ip, fp, C.c_size_t]
    def load(v):
        stem = os.path.join(folder, "images", "%08d" % v).encode()
        r, c = C.c_int(), C.c_int()
        # size from the grey read (served from the process cache after load_dense_folder) instead of a second colour decode
        if not os.path.exists(stem.decode() + ".ppm") and L.apdhost_read_gray_image(stem, C.byref(r), C.byref(c), None, 0) == 0:
            pass
        elif L.apdhost_read_color_image(stem, C.byref(r), C.byref(c), None, 0) != 0:
            raise IOError("cannot read image %d of %s" % (v, folder))
        a = np.zeros((r.value, c.value, 3), np.float32)
        if L.apdhost_read_color_image(stem, C.byref(r), C.byref(c), a.ctypes.data_as(fp), a.size) != 0 or a.shape[:2] != (r.value, c.value):
            raise IOError("cannot read image %d of %s" % (v, folder))
        return a

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, max(1, len(ids)))) as pool:
        return list(pool.map(load, ids))


FUSION_VARIANTS = {"eth": 0, "tat_intermediate": 1, "tat_advanced": 2}  # APD_FUSION_* of include/apd_mi355x.h


def read_vis(path):
    """COLMAP's fused.ply.vis (little endian: uint64 number of points, then per point uint32 n and n x uint32 view index) as
    (offsets int64 [N + 1], views int32): point k is seen by views[offsets[k]:offsets[k + 1]].  ValueError for a file that is
    short or has bytes left over."""
    raw = open(path, "rb").read()
    if len(raw) < 8 or (len(raw) - 8) % 4:
        raise ValueError("%s: not a .vis file (%d bytes)" % (path, len(raw)))
    n = int(np.frombuffer(raw, "<u8", 1)[0])
    words = np.frombuffer(raw, "<u4", offset=8)
    offsets = np.zeros(n + 1, np.int64)
    at = 0
    for k in range(n):   # the position of each count depends on the counts before it
        if at >= len(words):
            raise ValueError("%s: ends in point %d of %d" % (path, k, n))
        at += 1 + int(words[at])
        offsets[k + 1] = at - (k + 1)
    if at != len(words):
        raise ValueError("%s: %d words for %d points, %d expected" % (path, len(words), n, at))
    keep = np.ones(len(words), bool)
    keep[offsets[:-1] + np.arange(n)] = False
    return offsets, words[keep].astype(np.int32)


def _fusion_views(scene, results):
    """What fuse() hands over of every view besides its image: the camera with K scaled to the maps when the image has another
    size (RescaleImageAndCamera, APD.cpp:729-750), the depth map and the normal map."""
    cam_t = type(scene.cameras[0])
    cams = (cam_t * scene.num_views)()
    deps, nors = [], []
    for v in range(scene.num_views):
        st = results[v]
        h, w = st.depth.shape
        cam = cam_t.from_buffer_copy(scene.cameras[v])
        img = scene.images[v]
        if img.shape[:2] != (h, w):
            sx = np.float32(w) / np.float32(img.shape[1])
            sy = np.float32(h) / np.float32(img.shape[0])
            cam.K[0] = float(np.float32(cam.K[0]) * sx)
            cam.K[2] = float(np.float32(cam.K[2]) * sx)
            cam.K[4] = float(np.float32(cam.K[4]) * sy)
            cam.K[5] = float(np.float32(cam.K[5]) * sy)
        cams[v] = cam
        deps.append(np.ascontiguousarray(st.depth, np.float32))
        nors.append(np.ascontiguousarray(st.normal, np.float32))
    return cams, deps, nors


def average_points(scene, results, points, device=0):
    """Points.average with the cameras and the depth and normal maps fuse() passes for (scene, results): the mean position and
    normal of every point of `points` (a Points of fuse(..., return_points=True) on the same scene and results) over the views
    that agree on it.  Returns a new Points where `points` lives; on GPU `points.device` (`device` must name it)."""
    if int(device) != points.device:
        raise ValueError("average_points: the points live on device %d, not %d" % (points.device, int(device)))
    cams, deps, nors = _fusion_views(scene, results)
    return points.average(cams, deps, nors)


def fuse(scene, results, ply_path, device=0, colour_images=None, block_masks=None, variant="eth", options=None, return_points=False,
         vis_path=None, average=False, voxel=None, voxel_origin=None, radius_filter=None, stat_filter=None, component_filter=None,
         estimate_normals=None, render_visibility=None, smooth=None, score=None, align=None, register=None, align_planes=None):
    """RunFusion (APD.cpp:826-977) on the gathered maps: consistency check and merge into a binary PLY on GPU `device`
    (apd_fuse_views, csrc/apd_fusion.hip).  variant: "eth" (RunFusion), "tat_intermediate" or "tat_advanced" (the Tanks and
    Temples loops RunFusion_TAT_Intermediate / RunFusion_TAT_advanced, APD.cpp:979-1296, csrc/apd_fusion_tat.hip; they ignore
    the weak maps).  Every view must be at one resolution per view; images are
    resampled to the depth-map size if it differs (RescaleImageAndCamera, APD.cpp:729-750).  colour_images: optional
    float32 [H, W, 3] arrays (blue, green, red, as load_colour_images returns them) for the point colours; the grey
    images of the scene otherwise (blue = green = red).  block_masks: optional uint8 [H, W] arrays (or None per view), the
    `blocks/mask_<id>.jpg` of APD.cpp:849-853: reference pixels below 128 are not fused.  Returns the number of points.
    options: a FusionOptions (default_fusion_options(min_consistent=2, ...): the ETH loop's acceptance rule, ply_normals,
    result_on_device; its `variant` is set from `variant`), None for the reference's behaviour.  return_points: also return the
    points as a Points object (numpy views, or torch tensors on `device` with result_on_device): (count, Points); ply_path may
    then be None and no file is written.  vis_path: also write COLMAP's fused.ply.vis of the same fusion there (per point the
    views that see it, as indices of the scene's views; Points.write_vis), with or without a PLY file or the points.
    The options below rework the fused points.  They are applied in this order, each to what the ones before it have produced:
    average, voxel, stat_filter, radius_filter, component_filter, smooth, estimate_normals, render_visibility, register, align, align_planes;
    score comes after all of them.  With any of them but score alone, the file (written by Points.write_ply, with normals when the options
    say ply_normals), the returned points, the .vis file and the count returned are those of the last step's points.
    average: the mean geometry (average_points): positions and normals are means over the agreeing views, and a source that did
    not contribute is no longer listed.
    voxel: a cell size -- Points.merge_voxels(voxel, voxel_origin): one point per occupied cell of the cubic grid, the mean of the
    cell's points with the union of their lists; the count returned is that of the cells.
    stat_filter: (radius, k, std_ratio) -- Points.remove_statistical(radius, k, std_ratio): the points whose mean distance to their k
    nearest neighbours within the radius is at most the cloud's mean + std_ratio * deviation of that value.
    radius_filter: (radius, min_neighbours) -- Points.remove_sparse(radius, min_neighbours): the points with at least that many other
    points within the radius.
    component_filter: (radius, min_size) -- Points.remove_small_components(radius, min_size): the points whose connected component
    within the radius has at least that many points.
    smooth: (radius, min_neighbours, iterations) -- Points.with_smoothed_positions(radius, min_neighbours, iterations): the same
    points with each position projected on the weighted plane of its neighbourhood, `iterations` times; normals estimated and
    visibility rendered afterwards belong to the smoothed cloud.
    estimate_normals: (radius, min_neighbours) -- Points.with_estimated_normals(radius, min_neighbours): the same points with their
    normals re-estimated from the geometry of the cloud that is kept.  Without ply_normals in the options the step changes no byte
    of the file; it still acts on the returned points.
    render_visibility: (splat, rel_tolerance) -- Points.with_rendered_visibility(scene.cameras, splat, rel_tolerance): the same
    points as a merged object whose lists name the views that see each point of the cloud as it is then, occlusion included: the
    cloud is drawn into the scene's full-resolution cameras, in view order.  The step changes no byte of the PLY file.
    register: (truth, radius, inlier_distance[, trials[, seed]]) -- Points.register(truth, radius, inlier_distance, trials=trials,
    seed=seed) (4096 trials, seed 0, unless given) -- global registration from any start by FPFH descriptors of the STORED normals,
    their matches and RANSAC -- and Points.transformed by its answer, as `align` moves them; the Registration is returned as one
    more value before the Alignment: (count, Registration[, Alignment][, Score]), or (count, Points, Registration, ..) with
    return_points.
    align: (truth, radius[, iterations[, with_scale]]) -- Points.align(truth, radius, iterations=iterations, with_scale=with_scale)
    (16 iterations, rigid, unless given) and Points.transformed by its answer: the file and the returned points are the moved ones
    -- positions and normals; the .vis file is what it is without the option, since moving changes no list -- and the Alignment
    is returned as one more value after the count and the points and before the score: (count, Alignment), (count, Points,
    Alignment), (count, Points, Alignment, Score).
    align_planes: (truth, radius[, iterations]) -- Points.align_planes(truth, radius, iterations=iterations) (16 iterations unless
    given) -- point-to-plane ICP onto the STORED normals of `truth`, the refinement to prefer once `register` or `align` has
    brought the points within about a radius -- and Points.transformed by its answer, as `align` moves them; the PlaneAlignment is
    returned as one more value after the Alignment and before the Score.
    score: (truth, threshold) -- changes no point nor a byte of a file: Points.score(truth, threshold) of the final points against
    `truth` (a Points: Points.read_ply of a ground truth, or another fusion's), the precision, recall and F-score at the threshold,
    returned as one more value after the others: (count, Score), or (count, Points, Score) with return_points.  With `align` the
    points scored are the moved ones."""
    if variant not in FUSION_VARIANTS:
        raise ValueError("unknown fusion variant %r: one of %s" % (variant, ", ".join(sorted(FUSION_VARIANTS))))
    if ply_path is None and not return_points and vis_path is None:
        raise ValueError("fuse: neither a PLY file nor the points nor the visibility file are asked for")
    # The reworking steps, each `points -> (new points, value to return or None)`.  They are unpacked from the last applied to the
    # first, the order in which a malformed option has always been refused, before any device work.
    steps = []

    def kept_by(name, method, *args):   # a step whose method returns (new points, figures..)
        steps.append((name, lambda p: (getattr(p, method)(*args)[0], None)))

    def moved_by(method, *args, **kw):  # register, align, align_planes: the transform the method finds, and the points moved by it
        def step(p):
            found = getattr(p, method)(*args, **kw)
            return p.transformed(found), found
        steps.append((method, step))

    if score is not None:
        truth, threshold = score
    if align_planes is not None:
        onto, radius, *rest = align_planes
        if len(rest) > 1:
            raise ValueError("fuse: align_planes=(truth, radius[, iterations]), not %d values" % len(align_planes))
        iterations, = (rest + [16][len(rest):])
        moved_by("align_planes", onto, radius, iterations=iterations)
    if align is not None:
        onto, radius, *rest = align
        if len(rest) > 2:
            raise ValueError("fuse: align=(truth, radius[, iterations[, with_scale]]), not %d values" % len(align))
        iterations, with_scale = (rest + [16, False][len(rest):])
        moved_by("align", onto, radius, iterations=iterations, with_scale=with_scale)
    if register is not None:
        onto, radius, inlier_distance, *rest = register
        if len(rest) > 2:
            raise ValueError("fuse: register=(truth, radius, inlier_distance[, trials[, seed]]), not %d values" % len(register))
        trials, seed = (rest + [4096, 0][len(rest):])
        moved_by("register", onto, radius, inlier_distance, trials=trials, seed=seed)
    if render_visibility is not None:
        splat, rel_tolerance = render_visibility
        kept_by("render_visibility", "with_rendered_visibility", [scene.cameras[v] for v in range(scene.num_views)], splat, rel_tolerance)
    if estimate_normals is not None:
        radius, min_neighbours = estimate_normals
        kept_by("estimate_normals", "with_estimated_normals", radius, min_neighbours)
    if smooth is not None:
        radius, min_neighbours, iterations = smooth
        kept_by("smooth", "with_smoothed_positions", radius, min_neighbours, iterations)
    if component_filter is not None:
        radius, min_size = component_filter
        kept_by("component_filter", "remove_small_components", radius, min_size)
    if radius_filter is not None:
        radius, min_neighbours = radius_filter
        kept_by("radius_filter", "remove_sparse", radius, min_neighbours)
    if stat_filter is not None:
        radius, k, std_ratio = stat_filter
        kept_by("stat_filter", "remove_statistical", radius, k, std_ratio)
    if voxel is not None:
        kept_by("voxel", "merge_voxels", voxel, voxel_origin)
    if average:
        steps.append(("average", lambda p: (average_points(scene, results, p, device), None)))
    steps.reverse()

    # With a reworking step the file is written from the final points; otherwise it is the fusion's own, and the points are wrapped
    # only where they are returned or scored (the .vis file alone is written from the raw handle).
    wrap = bool(return_points or steps or score is not None)
    n, points = _fuse_views(scene, results, None if steps else ply_path, device, colour_images, block_masks, variant, options, wrap,
                            None if wrap else vis_path)
    if points is None:
        return n
    values = []
    try:
        for _, step in steps:
            new, value = step(points)
            points.close()
            points = new
            if value is not None:
                values.append(value)
        if steps:
            if [name for name, _ in steps] != ["average"]:   # averaging alone keeps every point: the fusion's own count
                n = points.count
            if ply_path is not None:
                points.write_ply(ply_path, normals=bool(options is not None and options.ply_normals))
        if vis_path is not None:
            points.write_vis(vis_path)
        if score is not None:
            values.append(points.score(truth, threshold))
    except BaseException:
        points.close()
        raise
    if return_points:
        return (n, points, *values)
    points.close()
    return (n, *values) if values else n


def _fuse_views(scene, results, ply_path, device, colour_images, block_masks, variant, options, wrap, vis_path):
    """The one fusion of fuse(): (count, Points or None).  ply_path: the fusion writes the file itself, unless None.  wrap: the points
    come back as a Points on `device`; otherwise vis_path, unless None, is written from the raw handle, which is then released."""
    import ctypes as C
    from . import Points, default_fusion_options
    L = host_lib()
    L.apdhost_set_fusion_device(int(device))
    L.apdhost_set_fusion_variant(FUSION_VARIANTS[variant])
    L.apdhost_fuse_opt.restype = C.c_longlong
    opt = default_fusion_options()
    if options is not None:
        C.memmove(C.byref(opt), C.byref(options), C.sizeof(opt))
    opt.variant = FUSION_VARIANTS[variant]
    V = scene.num_views
    cam_t = type(scene.cameras[0])
    cams = (cam_t * V)()
    imgs, deps, nors, weaks = [], [], [], []
    rows, cols = (C.c_int * V)(), (C.c_int * V)()
    for v in range(V):
        st = results[v]
        h, w = st.depth.shape
        cam = cam_t.from_buffer_copy(scene.cameras[v])
        img = scene.images[v] if colour_images is None else colour_images[v]
        if img.shape[:2] != (h, w):
            sx = np.float32(w) / np.float32(img.shape[1])
            sy = np.float32(h) / np.float32(img.shape[0])
            if img.ndim == 3:
                img = np.stack([np.rint(resize_linear(img[..., k], w, h)) for k in range(3)], -1).astype(np.float32)
            else:
                img = np.rint(resize_linear(img, w, h)).astype(np.float32)
            cam.K[0] = float(np.float32(cam.K[0]) * sx)
            cam.K[2] = float(np.float32(cam.K[2]) * sx)
            cam.K[4] = float(np.float32(cam.K[4]) * sy)
            cam.K[5] = float(np.float32(cam.K[5]) * sy)
        cams[v] = cam
        rows[v], cols[v] = h, w
        imgs.append(np.ascontiguousarray(img, np.float32))
        deps.append(np.ascontiguousarray(st.depth, np.float32))
        nors.append(np.ascontiguousarray(st.normal, np.float32))
        weaks.append(np.ascontiguousarray(rescale_nearest(st.weak, w, h), np.uint8))
    offs = (C.c_int * (V + 1))()
    flat = []
    for v in range(V):
        offs[v] = len(flat)
        flat += [s for s in scene.pairs[v] if s < V]  # source-only views have no maps to check against
    offs[V] = len(flat)
    idx = (C.c_int * max(len(flat), 1))(*flat)

    def ptrs(arrs):
        return (C.c_void_p * V)(*[a.ctypes.data for a in arrs])

    channels = 3 if imgs[0].ndim == 3 else 1
    blocks = None
    if block_masks is not None:
        keep = [None if b is None else np.ascontiguousarray(b, np.uint8) for b in block_masks]
        blocks = (C.c_void_p * V)(*[None if b is None else b.ctypes.data for b in keep])
    handle = C.c_void_p()
    n = L.apdhost_fuse_opt(C.byref(opt), V, C.byref(cams), ptrs(imgs), channels, ptrs(deps), ptrs(nors), ptrs(weaks), blocks, rows, cols, offs,
                           idx, None if ply_path is None else str(ply_path).encode(),
                           C.byref(handle) if wrap or vis_path is not None else None)
    if n < 0:
        raise RuntimeError("device fusion failed (apd_fuse_views_opt, %s): see stderr" % variant)
    if wrap:
        return int(n), Points(handle, device)
    if vis_path is not None:  # the file alone: no array is copied or wrapped
        from . import ApdError, lib
        rc = lib().apd_points_write_vis(handle, str(vis_path).encode())
        why = lib().apd_fusion_last_error().decode() if rc != 0 else ""
        lib().apd_points_destroy(handle)
        if rc != 0:
            raise ApdError("apd error %d: %s" % (rc, why))
    return int(n), None


class FilteredMaps:
    """One view of filter_maps: depth float32 [H, W] (0 where the pixel is rejected), votes uint8 [H, W] (agreeing sources),
    consistency float32 [H, W] (sum of exp(-score) over the agreeing sources)."""

    def __init__(self, depth, votes, consistency):
        self.depth, self.votes, self.consistency = depth, votes, consistency

    def __iter__(self):
        return iter((self.depth, self.votes, self.consistency))


def filter_maps(scene, results, device=0, block_masks=None, options=None, on_device=False):
    """The geometric filter (apd_filter_views, csrc/apd_filter.hip) on the gathered maps: per view what the vote test of RunFusion
    (APD.cpp:896-951) says about its own pixels, every view judged against the unfiltered maps of its sources (nothing is
    consumed, so the result of a view depends on no other view's).  Takes the maps of `results` like fuse() (weak maps resampled
    to the depth-map size, K scaled when the maps are not at the camera's size) and no images.  block_masks as in fuse().
    options: a FusionOptions (the ETH loop's acceptance rule; default_fusion_options(min_consistent=2, ...)), None for the
    reference's literals.  Returns a list of FilteredMaps, one per view: numpy arrays, or with on_device=True torch tensors on
    `device` (the maps go up as tensors, the filter writes into the returned ones, nothing comes down)."""
    import ctypes as C
    from . import ApdError, default_fusion_options, lib
    L = lib()
    opt = default_fusion_options()
    if options is not None:
        C.memmove(C.byref(opt), C.byref(options), C.sizeof(opt))
    V = scene.num_views
    cam_t = type(scene.cameras[0])
    cams = (cam_t * V)()
    rows, cols = (C.c_int * V)(), (C.c_int * V)()
    if on_device:
        import torch
        dev = torch.device("cuda", int(device))
        place = lambda a: torch.from_numpy(a).to(dev)
        empty = lambda shape, dt: torch.empty(shape, dtype={np.float32: torch.float32, np.uint8: torch.uint8}[dt], device=dev)
        addr = lambda a: a.data_ptr()
    else:
        place = lambda a: a
        empty = lambda shape, dt: np.empty(shape, dt)
        addr = lambda a: a.ctypes.data
    deps, nors, weaks, outs = [], [], [], []
    for v in range(V):
        st = results[v]
        h, w = st.depth.shape
        cam = cam_t.from_buffer_copy(scene.cameras[v])
        if cam.width > 0 and cam.height > 0 and (cam.height, cam.width) != (h, w):  # RescaleImageAndCamera, APD.cpp:729-750
            sx = np.float32(w) / np.float32(cam.width)
            sy = np.float32(h) / np.float32(cam.height)
            cam.K[0] = float(np.float32(cam.K[0]) * sx)
            cam.K[2] = float(np.float32(cam.K[2]) * sx)
            cam.K[4] = float(np.float32(cam.K[4]) * sy)
            cam.K[5] = float(np.float32(cam.K[5]) * sy)
        cams[v] = cam
        rows[v], cols[v] = h, w
        deps.append(place(np.ascontiguousarray(st.depth, np.float32)))
        nors.append(place(np.ascontiguousarray(st.normal, np.float32)))
        weaks.append(place(np.ascontiguousarray(rescale_nearest(st.weak, w, h), np.uint8)))
        outs.append(FilteredMaps(empty((h, w), np.float32), empty((h, w), np.uint8), empty((h, w), np.float32)))
    offs = (C.c_int * (V + 1))()
    flat = []
    for v in range(V):
        offs[v] = len(flat)
        flat += [s for s in scene.pairs[v] if s < V]  # source-only views have no maps to check against
    offs[V] = len(flat)
    idx = (C.c_int * max(len(flat), 1))(*flat)

    def ptrs(arrs):
        return (C.c_void_p * V)(*[None if a is None else addr(a) for a in arrs])

    blocks = None
    if block_masks is not None:
        keep = [None if b is None else place(np.ascontiguousarray(b, np.uint8)) for b in block_masks]
        blocks = ptrs(keep)
    if on_device:
        torch.cuda.synchronize(dev)  # the uploads, before the library's own stream reads them
    rc = L.apd_filter_views(C.byref(opt), int(device), V, C.byref(cams), ptrs(deps), ptrs(nors), ptrs(weaks), blocks, rows, cols, offs, idx,
                            int(on_device), ptrs([o.depth for o in outs]), ptrs([o.votes for o in outs]),
                            ptrs([o.consistency for o in outs]), int(on_device))
    if rc != 0:
        raise ApdError("apd error %d: %s" % (rc, L.apd_fusion_last_error().decode()))
    return outs


def mesh_views(scene, results, colour_images):
    """What mesh() hands to Volume.integrate of every view besides its filtered depth map: the camera at the size of the maps, with
    K scaled when the image has another size (RescaleImageAndCamera, APD.cpp:729-750), and the image resampled as fuse() does."""
    cam_t = type(scene.cameras[0])
    cams, imgs = [], []
    for v in range(scene.num_views):
        h, w = results[v].depth.shape
        cam = cam_t.from_buffer_copy(scene.cameras[v])
        img = scene.images[v] if colour_images is None else colour_images[v]
        if img.shape[:2] != (h, w):
            sx = np.float32(w) / np.float32(img.shape[1])
            sy = np.float32(h) / np.float32(img.shape[0])
            if img.ndim == 3:
                img = np.stack([np.rint(resize_linear(img[..., k], w, h)) for k in range(3)], -1).astype(np.float32)
            else:
                img = np.rint(resize_linear(img, w, h)).astype(np.float32)
            cam.K[0] = float(np.float32(cam.K[0]) * sx)
            cam.K[2] = float(np.float32(cam.K[2]) * sx)
            cam.K[4] = float(np.float32(cam.K[4]) * sy)
            cam.K[5] = float(np.float32(cam.K[5]) * sy)
        cam.width, cam.height = w, h
        cams.append(cam)
        imgs.append(np.ascontiguousarray(img, np.float32))
    return cams, imgs


def mesh_bounds(bounds):
    """(lo, hi) float32 [3] of mesh()'s `bounds`: a pair of corners, or a Points whose finite positions give the box."""
    if hasattr(bounds, "xyz"):
        xyz = bounds.xyz
        xyz = np.asarray(xyz.cpu().numpy() if hasattr(xyz, "cpu") else xyz, np.float32).reshape(-1, 3)
        xyz = xyz[np.isfinite(xyz).all(1)]
        if len(xyz) == 0:
            raise ValueError("mesh: the points that should give the box have no finite position")
        return xyz.min(0), xyz.max(0)
    lo, hi = bounds
    return np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)


def mesh(scene, results, ply_path, voxel, trunc=None, bounds=None, device=0, colour_images=None, block_masks=None, options=None,
         return_mesh=False, weld=None, min_component=None, normals=False, simplify=None, smooth=None, trim=None, depth_maps=False,
         score=None, recolour=None):
    """A surface from the gathered maps: filter_maps(..., on_device=True) leaves every view's consistent depth map on GPU `device`,
    Volume.integrate fuses them, at each view's depth-map resolution, into a truncated signed distance volume with samples `voxel`
    apart (apd_volume_integrate, contract C21), and Volume.extract_mesh takes the marching-tetrahedra mesh of its zero level, which
    is written to ply_path (unless None).  trunc: the truncation distance, 4 * voxel unless given.  bounds: (lo, hi), the corners of
    the box to cover, or a Points whose box is taken; None: the box of the points fuse(..., return_points=True) makes of the same
    inputs.  The volume covers the box grown by trunc (Volume.around).  colour_images, block_masks, options: as in fuse() and
    filter_maps(); the images are resampled as fuse() resamples them and colour the vertices.  Every view weighs 1.
    weld (a tolerance), trim (min_views, or (min_views, min_pixels, rel_tolerance); Mesh.remove_unseen's defaults: 1 pixel, 0.01, back
    faces culled), min_component (a number of faces), smooth (a number of iterations, or (iterations, lam, mu), or (iterations,
    lam, mu, boundary); Mesh.smooth's defaults: Taubin's 0.5 and -0.53, "along"), simplify (a cell size, or (cell, placement) with
    placement "mean" or "quadric", the default) and normals, each off by default, clean the mesh after extraction in this fixed
    order: Mesh.weld, Mesh.remove_unseen, Mesh.remove_small_components, Mesh.smooth, Mesh.simplify, Mesh.with_vertex_normals,
    Mesh.colour_from_views (contracts C22, C25, C24, C23 and C26): trimming drops the faces that fewer than min_views of the views the volume was built from see
    -- the sheets with which the extraction closes the surface at depth discontinuities and at the frame border -- and goes before
    the component filter so that the fragments it detaches are removed; smoothing goes before simplification so that the quadric
    reads denoised planes; the file and the counts are the final mesh's.  depth_maps: the final mesh is also rendered into every
    view (Mesh.render, both sides), at the size of that view's maps.  recolour (True, or (rel_tolerance, min_cos); Mesh.colour_from_views'
    defaults: 0.01 and 0.1): the last step, after the normals: the vertices take their colour from the views' images through the final
    mesh's own z-buffer (contract C26) instead of from the volume, which is then made without colour -- a third of the memory -- and
    integrated without the images; the geometry is the same.  The images go to the device once.
    score: (truth, threshold[, density[, seed]]) -- after every other step, changes no vertex nor a byte of the file:
    Mesh.score(truth, threshold, density, seed) of the final mesh against `truth` (a Points: Points.read_ply of a ground truth, or a
    fusion's), the precision, recall and F-score of the surface at the threshold (contract C27), as fuse(score=...) gives them for points.
    Returns (vertices, faces), the counts, or with return_mesh (vertices, faces, Mesh); with depth_maps the list of the views'
    rendered depth maps (float32 [h, w]) follows, and with score the Score comes last."""
    from . import Volume
    import torch
    smoothing = tuple(smooth) if isinstance(smooth, (tuple, list)) else (smooth,)
    if smooth is not None and len(smoothing) not in (1, 3, 4):
        raise ValueError("mesh: smooth %r, neither iterations nor (iterations, lam, mu) nor (iterations, lam, mu, boundary)" % (smooth,))
    trimming = tuple(trim) if isinstance(trim, (tuple, list)) else (trim,)
    if trim is not None and len(trimming) not in (1, 3):
        raise ValueError("mesh: trim %r, neither min_views nor (min_views, min_pixels, rel_tolerance)" % (trim,))
    recolouring = () if recolour is True else tuple(recolour) if isinstance(recolour, (tuple, list)) else (recolour,)
    if recolour is not None and (recolour is False or len(recolouring) not in (0, 2)):
        raise ValueError("mesh: recolour %r, neither True nor (rel_tolerance, min_cos)" % (recolour,))
    scoring = tuple(score) if isinstance(score, (tuple, list)) else (score,)
    if score is not None and len(scoring) not in (2, 3, 4):
        raise ValueError("mesh: score %r, not (truth, threshold[, density[, seed]])" % (score,))
    trunc = 4.0 * float(voxel) if trunc is None else trunc
    if bounds is None:
        _, points = fuse(scene, results, None, device=device, colour_images=colour_images, block_masks=block_masks, options=options, return_points=True)
        try:
            lo, hi = mesh_bounds(points)
        finally:
            points.close()
    else:
        lo, hi = mesh_bounds(bounds)
    maps = filter_maps(scene, results, device=device, block_masks=block_masks, options=options, on_device=True)
    cams, imgs = mesh_views(scene, results, colour_images)
    dev = torch.device("cuda", int(device))
    volume = Volume.around(lo, hi, voxel, trunc, colour=recolour is None, device=device)
    on_device = [torch.from_numpy(a).to(dev) for a in imgs]
    try:
        volume.integrate(cams, [m.depth for m in maps], on_device if recolour is None else None, maps_on_device=True)
        found = volume.extract_mesh()
    finally:
        volume.close()
    steps = [] if weld is None else [lambda m: m.weld(weld)]
    if trim is not None:
        min_views, min_pixels, rel_tolerance = trimming if len(trimming) == 3 else (trimming[0], 1, 0.01)
        steps += [lambda m: m.remove_unseen(cams, min_views, "back", min_pixels, rel_tolerance)]
    steps += [] if min_component is None else [lambda m: m.remove_small_components(min_component)]
    steps += [] if smooth is None else [lambda m: m.smooth(*smoothing)]
    if simplify is not None:
        cell, placement = simplify if isinstance(simplify, (tuple, list)) else (simplify, "quadric")
        steps += [lambda m: m.simplify(cell, placement=placement)]
    steps += [lambda m: m.with_vertex_normals()] if normals else []
    steps += [] if recolour is None else [lambda m: m.colour_from_views(cams, on_device, *recolouring)]
    for step in steps:
        before = found
        try:
            found = step(before)
        finally:
            before.close()
    if ply_path is not None:
        found.write_ply(ply_path)
    counts = (len(found.vertices), len(found.faces))
    rendered = ([found.render(cam)[0] for cam in cams],) if depth_maps else ()
    try:
        scored = () if score is None else (found.score(*scoring),)
    except Exception:
        found.close()
        raise
    if return_mesh:
        return counts + (found,) + rendered + scored
    found.close()
    return counts + rendered + scored
