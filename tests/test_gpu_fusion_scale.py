"""The three device fusions (apd_fuse_views_variant: ETH, csrc/apd_fusion.hip; Tanks and Temples, csrc/apd_fusion_tat.hip;
the shared scan and compaction of csrc/apd_fusion_call.hip) against their sequential loops (oracle/fusion_oracle.cpp,
tests/helpers/tat_fusion_ref.cpp) on the committed cases of tests/fusion_cases.py: full frames whose scans split the blocks
over partitions, the block counts at the partitions' boundaries, the generated edge cases and non-finite inputs.  Every case
runs through the C ABI with maps on the host and on the device; the PLY files must be byte-identical, but for the sign and
payload of a NaN coordinate (contract C9)."""
import ctypes as C

import numpy as np
import pytest

import fusion_cases
import tat_checker
from test_fusion_cases import VARIANTS, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def _device(gpu_pkg, ob, case, variant, path, on_device):
    """apd_fuse_views_variant through ctypes; on_device: every map (blocks included) in a torch tensor on cuda:0."""
    import torch
    L = gpu_pkg.lib()
    L.apd_fusion_last_error.restype = C.c_char_p
    V = case.num_views
    arrays = [[np.ascontiguousarray(a, dt) for a in arrs] for arrs, dt in ((case.images, np.float32), (case.depths, np.float32),
                                                                            (case.normals, np.float32), (case.weaks, np.uint8))]
    blocks = None if case.blocks is None else [None if b is None else np.ascontiguousarray(b, np.uint8) for b in case.blocks]
    if on_device:
        arrays = [[torch.from_numpy(a).cuda() for a in arrs] for arrs in arrays]
        blocks = None if blocks is None else [None if b is None else torch.from_numpy(b).cuda() for b in blocks]
        torch.cuda.synchronize()
        addr = lambda a: None if a is None else a.data_ptr()
    else:
        addr = lambda a: None if a is None else a.ctypes.data
    ptr = [(C.c_void_p * V)(*[addr(a) for a in arrs]) for arrs in arrays]
    bptr = None if blocks is None else (C.c_void_p * V)(*[addr(b) for b in blocks])
    rows = (C.c_int * V)(*[d.shape[0] for d in case.depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in case.depths])
    flat = [s for p in case.pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in case.pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    channels = 3 if case.images[0].ndim == 3 else 1
    n = C.c_longlong(-1)
    st = L.apd_fuse_views_variant(VARIANTS.index(variant), 0, V, case.cameras(ob.make_camera), ptr[0], channels, ptr[1], ptr[2], ptr[3],
                                  bptr, rows, cols, offs, idx, int(on_device), str(path).encode(), C.byref(n))
    assert st == 0, L.apd_fusion_last_error()
    return n.value


def _assert_same_ply(got, want, nan_bits_may_differ=False):
    """Byte-identical files; with nan_bits_may_differ, a coordinate that is NaN in both files may differ in sign and payload."""
    a, b = got.read_bytes(), want.read_bytes()
    if a == b:
        return
    ha, _, body_a = a.partition(b"end_header\n")
    hb, _, body_b = b.partition(b"end_header\n")
    assert ha == hb, (ha, hb)
    rec = np.dtype([("xyz", "<u4", 3), ("bgr", "u1", 3)])
    ra, rb = np.frombuffer(body_a, rec), np.frombuffer(body_b, rec)
    assert len(ra) == len(rb)
    assert np.array_equal(ra["bgr"], rb["bgr"]), "colours differ at %s" % np.nonzero((ra["bgr"] != rb["bgr"]).any(1))[0][:10]
    nan_a = (ra["xyz"] & 0x7FFFFFFF) > 0x7F800000
    nan_b = (rb["xyz"] & 0x7FFFFFFF) > 0x7F800000
    same = (ra["xyz"] == rb["xyz"]) | (nan_a & nan_b if nan_bits_may_differ else False)
    bad = np.nonzero(~same.all(1))[0]
    assert len(bad) == 0, "%d of %d points differ, first %s: %s != %s" % (len(bad), len(ra), bad[:5], ra["xyz"][bad[:5]].tolist(),
                                                                         rb["xyz"][bad[:5]].tolist())


def _compare(gpu_pkg, ob, checker, tmp_path, name, variant, nan_bits_may_differ=False):
    case = fusion_cases.case(name)
    n_ref = reference(ob, checker, case, variant, tmp_path / "ref.ply")
    for on_device in (False, True):
        path = tmp_path / ("dev.ply" if on_device else "host.ply")
        assert _device(gpu_pkg, ob, case, variant, path, on_device) == n_ref, (name, variant, on_device)
        _assert_same_ply(path, tmp_path / "ref.ply", nan_bits_may_differ)
    return case, n_ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", fusion_cases.names("full_frame"))
def test_full_frame(gpu_pkg, ob, checker, tmp_path, name, variant):
    """1920 x 1080, 4 views, 3 sources: 8100 blocks, 8 per partition of the scans; plain and with a carry over ~7900 blocks.
    ETH also through pipeline.fuse."""
    case, n_ref = _compare(gpu_pkg, ob, checker, tmp_path, name, variant)
    if variant == "eth":
        from apd_mvs_amd import pipeline
        scene = pipeline.MvsScene(list(case.cameras(gpu_pkg.make_camera)), case.images, case.pairs)
        results = {v: pipeline.ViewState(case.depths[v], case.normals[v], case.weaks[v], np.zeros(case.depths[v].shape, np.uint32))
                   for v in range(case.num_views)}
        assert pipeline.fuse(scene, results, tmp_path / "pipe.ply") == n_ref
        assert (tmp_path / "pipe.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", fusion_cases.names("boundary"))
def test_block_count_boundaries(gpu_pkg, ob, checker, tmp_path, name, variant):
    """1024 blocks (one per scan thread), 1025 (two per partition, the last partition holds one), 2052 (three per partition,
    threads 684-1023 empty)."""
    _compare(gpu_pkg, ob, checker, tmp_path, name, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", fusion_cases.names("generated"))
def test_generated_case(gpu_pkg, ob, checker, tmp_path, name, variant):
    _compare(gpu_pkg, ob, checker, tmp_path, name, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", fusion_cases.names("non_finite"))
def test_non_finite_and_denormal_inputs(gpu_pkg, ob, checker, tmp_path, name, variant):
    """NaN, +-inf, -0.0, denormal and 1e30 depths, NaN normals: every byte equal but the sign and payload of a NaN coordinate
    (x86 and the device make different default NaNs); which coordinates are NaN, infinities, denormals, colours and counts
    exactly."""
    _compare(gpu_pkg, ob, checker, tmp_path, name, variant, nan_bits_may_differ=True)
