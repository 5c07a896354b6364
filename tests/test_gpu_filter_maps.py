"""The geometric filter on the device (apd_filter_views, csrc/apd_filter.hip): all three maps of every view bit for bit the
sequential checker's (tests/helpers/filter_ref.cpp), host and device inputs and outputs, single outputs, untouched inputs, the
relation to the ETH fusion (consumption can only take votes away), pipeline.filter_maps, and the binary's --filtered-maps."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import eth_fusion_checker as E
import filter_checker as F
import fusion_cases
from test_gpu_dropin_binary import APD_BIN, _read_dmb, _write_dense_folder
from test_gpu_fusion_options import _fuse, _scene

pytestmark = pytest.mark.gpu

RULES = dict(E.OPTION_SETS, default={})
NAMES = ["tiny_9x7", "blocks_641x409", "mixed_sizes", "all_blocked", "sources_32", "empty_between", "rolled_aniso", "source_behind"]


def _case(name):
    """tiny: fewer pixels than a wave; 641 x 409 = 1024 * 256 + 25 pixels, block masks; views of two sizes; every pixel blocked;
    33 views, view 0 with 32 sources; five views of which the second is blocked entirely."""
    if name != "empty_between":
        return fusion_cases.case(name)
    case = copy.deepcopy(fusion_cases.case("mixed_sizes"))
    case.blocks = [None, np.zeros(case.depths[1].shape, np.uint8), None, None, None]
    return case


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("filter_checker"))


@pytest.fixture(scope="module")
def expected(ob, checker):
    """The checker's maps of (case, rule), computed once and read only."""
    cache = {}

    def get(name, key="default"):
        if (name, key) not in cache:
            cache[name, key] = F.filter_case(checker, ob, _case(name), **RULES[key])
            for maps in cache[name, key]:
                for a in maps:
                    a.setflags(write=False)
        return cache[name, key]
    return get


def _filter(pkg, ob, case, options, on_device=False, outputs=(True, True, True), expect=0):
    """apd_filter_views through ctypes.  on_device: every map and every output in a torch tensor on cuda:0.  outputs: which of
    depth, votes, consistency are asked for (the others' tables are NULL).  Returns per view [depth, votes, consistency] as
    numpy arrays (None where not asked for) and the input arrays as they are after the call."""
    import torch
    L = pkg.lib()
    V = case.num_views
    arrays = [[np.array(a, dt, order="C", copy=True) for a in arrs] for arrs, dt in ((case.depths, np.float32), (case.normals, np.float32),
                                                                                    (case.weaks, np.uint8))]
    blocks = None if case.blocks is None else [None if b is None else np.array(b, np.uint8, order="C", copy=True) for b in case.blocks]
    shapes = [d.shape for d in case.depths]
    outs = [[np.full(s, fill, dt) if want else None for s in shapes] for want, (dt, fill) in zip(outputs, ((np.float32, -7.0), (np.uint8, 77),
                                                                                                         (np.float32, -7.0)))]
    if on_device:
        up = lambda a: None if a is None else torch.from_numpy(a).cuda()
        arrays = [[up(a) for a in arrs] for arrs in arrays]
        blocks = None if blocks is None else [up(b) for b in blocks]
        outs = [[up(a) for a in arrs] for arrs in outs]
        torch.cuda.synchronize()
        addr = lambda a: None if a is None else a.data_ptr()
    else:
        addr = lambda a: None if a is None else a.ctypes.data
    table = lambda arrs: (C.c_void_p * V)(*[addr(a) for a in arrs])
    rows = (C.c_int * V)(*[s[0] for s in shapes])
    cols = (C.c_int * V)(*[s[1] for s in shapes])
    flat = [s for p in case.pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in case.pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    st = L.apd_filter_views(C.byref(options), 0, V, case.cameras(ob.make_camera), table(arrays[0]), table(arrays[1]), table(arrays[2]),
                            None if blocks is None else table(blocks), rows, cols, offs, idx, int(on_device),
                            *[table(arrs) if want else None for arrs, want in zip(outs, outputs)], int(on_device))
    assert st == expect, L.apd_fusion_last_error()
    down = lambda a: None if a is None else (a.cpu().numpy() if on_device else a)
    result = [[down(outs[k][v]) for k in range(3)] for v in range(V)]
    inputs = [[down(a) for a in arrs] for arrs in arrays] + [None if blocks is None else [down(b) for b in blocks]]
    return result, inputs


def _same(got, want):
    """Two maps equal as bits"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _assert_equal(result, want, what):
    assert len(result) == len(want)
    for v, (got, ref) in enumerate(zip(result, want)):
        for k, field in enumerate(("depth", "votes", "consistency")):
            assert _same(got[k], ref[k]), (what, v, field, int((got[k] != ref[k]).sum()))


# --------------------------------------------------------------------------------------------------------------------
# the device == the sequential checker
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_cases_are_not_vacuous(expected, name):
    """What the checker says about the case with the reference's literals: something accepted, something rejected that had votes
    (or at least a pixel with a depth and no vote); three different vote counts where there are many sources."""
    case, want = _case(name), expected(name)
    accepted = sum(int((d > 0).sum()) for d, _, _ in want)
    rejected_with_votes = sum(int(((v >= 1) & (d == 0)).sum()) for d, v, _ in want)
    valid_without_votes = sum(int(((v == 0) & (given > 0)).sum()) for (_, v, _), given in zip(want, case.depths))
    counts = sorted(set(np.concatenate([v.ravel() for _, v, _ in want]).tolist()))
    print(name, "accepted", accepted, "rejected with votes", rejected_with_votes, "valid without votes", valid_without_votes, "votes", counts)
    if name == "all_blocked":
        assert accepted == 0 and counts == [0] and all((s == 0).all() for _, _, s in want)
        return
    assert accepted > 0
    assert rejected_with_votes > 0 or valid_without_votes > 0
    if name == "sources_32":
        assert len(counts) >= 3


@pytest.mark.parametrize("key", sorted(RULES))
@pytest.mark.parametrize("name", NAMES)
def test_all_three_maps_equal_the_checker(gpu_pkg, ob, expected, name, key):
    case, want = _case(name), expected(name, key)
    result, _ = _filter(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(**RULES[key]))
    _assert_equal(result, want, (name, key))


@pytest.mark.parametrize("name", NAMES)
def test_device_maps_and_outputs_equal_host_ones_and_inputs_stay(gpu_pkg, ob, expected, name):
    case, want = _case(name), expected(name, "a")
    options = gpu_pkg.default_fusion_options(**RULES["a"])
    for on_device in (False, True):
        result, inputs = _filter(gpu_pkg, ob, case, options, on_device=on_device)
        _assert_equal(result, want, (name, on_device))
        given = [case.depths, case.normals, case.weaks, case.blocks]
        for after, before in zip(inputs, given):
            assert (after is None) == (before is None)
            for a, b in zip(after or [], before or []):
                assert (a is None and b is None) or _same(a, np.ascontiguousarray(b, a.dtype))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_single_output_equals_its_map_of_the_full_call(gpu_pkg, ob, expected, which, on_device):
    case, want = _case("mixed_sizes"), expected("mixed_sizes")
    outputs = tuple(k == which for k in range(3))
    result, _ = _filter(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(), on_device=on_device, outputs=outputs)
    for got, ref in zip(result, want):
        assert _same(got[which], ref[which]) and all(got[k] is None for k in range(3) if k != which)


def test_single_entries_may_be_null(gpu_pkg, ob, expected):
    """Only view 2's votes and view 0's depth are asked for: nothing else is written."""
    case, want = _case("mixed_sizes"), expected("mixed_sizes")
    L = gpu_pkg.lib()
    V = case.num_views
    keep = [[np.ascontiguousarray(a, dt) for a in arrs] for arrs, dt in ((case.depths, np.float32), (case.normals, np.float32), (case.weaks, np.uint8))]
    table = lambda arrs: (C.c_void_p * V)(*[None if a is None else a.ctypes.data for a in arrs])
    depth0, votes2 = np.full(case.depths[0].shape, -7.0, np.float32), np.full(case.depths[2].shape, 77, np.uint8)
    shapes = [d.shape for d in case.depths]
    flat = [s for p in case.pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in case.pairs]).tolist())
    opt = gpu_pkg.default_fusion_options()
    st = L.apd_filter_views(C.byref(opt), 0, V, case.cameras(ob.make_camera), table(keep[0]), table(keep[1]), table(keep[2]), None,
                            (C.c_int * V)(*[s[0] for s in shapes]), (C.c_int * V)(*[s[1] for s in shapes]), offs, (C.c_int * len(flat))(*flat), 0,
                            table([depth0, None, None, None, None]), table([None, None, votes2, None, None]), None, 0)
    assert st == 0, L.apd_fusion_last_error()
    assert _same(depth0, want[0][0]) and _same(votes2, want[2][1])


def test_timing_reports_setup_and_views_and_no_file(gpu_pkg, ob):
    _filter(gpu_pkg, ob, _case("tiny_9x7"), gpu_pkg.default_fusion_options())
    ms = [C.c_double(-1.0) for _ in range(3)]
    assert gpu_pkg.lib().apd_fusion_last_timing(*[C.byref(m) for m in ms]) == 0
    assert ms[0].value > 0.0 and ms[1].value > 0.0 and ms[2].value == 0.0


# --------------------------------------------------------------------------------------------------------------------
# the fusion: consumption can only take votes away
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,key", [("mixed_sizes", "default"), ("blocks_641x409", "a"), ("sources_32", "a")])
def test_every_fused_point_has_at_most_the_filters_votes(gpu_pkg, ob, expected, name, key):
    case, want = _case(name), expected(name, key)
    n, pts = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(**RULES[key]), points=True)
    assert n > 0
    votes = np.array([want[v][1].reshape(-1)[p] for v, p in zip(pts.view, pts.pixel)])
    assert (votes >= pts.support).all()
    kept = np.array([want[v][0].reshape(-1)[p] for v, p in zip(pts.view, pts.pixel)])
    print(name, key, "points", n, "with all their votes", int((votes == pts.support).sum()), "kept by the filter", int((kept > 0).sum()))


# --------------------------------------------------------------------------------------------------------------------
# pipeline.filter_maps
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,key", [("mixed_sizes", "c"), ("blocks_641x409", "default")])
def test_pipeline_filter_maps_gives_the_arrays_of_the_direct_call(gpu_pkg, ob, expected, name, key):
    from apd_mvs_amd import pipeline
    case, want = _case(name), expected(name, key)
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(**RULES[key])
    host = pipeline.filter_maps(scene, results, block_masks=case.blocks, options=options)
    assert all(isinstance(a, np.ndarray) for m in host for a in m)
    _assert_equal([list(m) for m in host], want, "host")
    dev = pipeline.filter_maps(scene, results, block_masks=case.blocks, options=options, on_device=True)
    for m in dev:
        assert all(t.is_cuda and t.device.index == 0 for t in m)
    _assert_equal([[t.cpu().numpy() for t in m] for m in dev], want, "device")
    assert isinstance(host[0], pipeline.FilteredMaps) and host[0].votes is list(host[0])[1]


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

NEW_FILES = ("depths_filtered.dmb", "consistency.dmb", "votes.bin")
RUNS = {
    "memory": ["--filtered-maps", "--keep-maps"],
    "files": ["--files", "--filtered-maps", "--keep-maps"],
    "plain": ["--keep-maps"],
    "strict": ["--fusion-min-consistent", "2", "--filtered-maps", "--keep-maps"],
    "no_fusion": ["--no-fusion", "--filtered-maps"],
}
VIEWS = 4


def _tree(folder):
    out = {}
    for root, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(gpu_pkg, synth, tmp_path_factory):
    """The smallest synthetic dense folder of the drop-in tests, one level, one iteration: every file each command line leaves."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, VIEWS)
    out = {}
    for name, extra in RUNS.items():
        shutil.copytree(a, root / name)
        r = subprocess.run([APD_BIN, str(root / name), "0", "--seed", "21", "--iters", "1", "--single-level"] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
        out[name] = (root / name, _tree(root / name))
    return out


def _new_files(tree):
    return {k: v for k, v in tree.items() if os.path.basename(k) in NEW_FILES}


def _pipeline_on_saved_maps(pkg, folder, **rule):
    from apd_mvs_amd import pipeline
    scene = pipeline.load_dense_folder(str(folder), pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % v)
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"),
                                        _read_dmb(d / "selected_views.bin"))
    return pipeline.filter_maps(scene, results, options=pkg.default_fusion_options(**rule))


def _assert_files_equal_maps(folder, maps):
    for v, m in enumerate(maps):
        d = folder / "APD" / ("%08d" % v)
        for name, want in zip(NEW_FILES, (m.depth, m.consistency, m.votes)):
            assert _same(_read_dmb(d / name), want), (v, name)


def test_binary_writes_the_same_three_files_in_memory_and_through_files(runs):
    memory, files = _new_files(runs["memory"][1]), _new_files(runs["files"][1])
    assert len(memory) == 3 * VIEWS and memory == files


def test_binary_files_equal_the_pipeline_on_the_saved_maps(gpu_pkg, runs):
    folder, _ = runs["memory"]
    maps = _pipeline_on_saved_maps(gpu_pkg, folder)
    _assert_files_equal_maps(folder, maps)
    assert sum(int((m.depth > 0).sum()) for m in maps) > 0 and any((m.depth == 0).any() for m in maps)


def test_binary_takes_the_fusion_rule(gpu_pkg, runs):
    folder, tree = runs["strict"]
    maps = _pipeline_on_saved_maps(gpu_pkg, folder, min_consistent=2)
    _assert_files_equal_maps(folder, maps)
    plain = _new_files(runs["memory"][1])
    strict = _new_files(tree)
    changed = sorted(os.path.basename(k) for k in strict if strict[k] != plain[k])
    assert changed and set(changed) == {"depths_filtered.dmb"}   # votes and consistency do not depend on the acceptance


def test_binary_without_the_flag_writes_what_it_wrote(runs):
    with_flag, without = runs["memory"][1], runs["plain"][1]
    assert not _new_files(without)
    assert {k: v for k, v in with_flag.items() if k not in _new_files(with_flag)} == without


def test_binary_filters_without_a_fusion(runs):
    _, tree = runs["no_fusion"]
    assert not any(k.endswith(".ply") for k in tree)
    assert _new_files(tree) == _new_files(runs["memory"][1])
