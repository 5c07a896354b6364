"""bench.py's options without a GPU: a plain run is the headline alone (--full adds the rest), --only-workloads only means something
with --full, and --dump-outputs writes the caller's maps as float32 / float64 .npy within 64 MB, sampled at the same pixels every run."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_is_the_default_and_full_is_an_option():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def _run(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def test_refused_combinations_exit_before_any_work():
    r = _run("--only-workloads", "configs1_office_6iter")   # the block it restricts exists with --full only
    assert r.returncode == 2 and "--full" in r.stderr and r.stdout == "", r.stderr
    r = _run("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == "", r.stderr


class _Handle:
    def __init__(self, h, w, seed):
        rng = np.random.default_rng(seed)
        self.planes = rng.standard_normal((h, w, 4)).astype(np.float32)
        self.weak = rng.integers(0, 3, (h, w)).astype(np.uint8)
        self.views = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)

    def download(self):
        return self.planes.copy(), self.weak.copy(), self.views.copy()


def test_dump_of_a_small_frame_is_the_whole_frame(tmp_path):
    bench = _bench()
    h = _Handle(48, 64, 1)
    bench.dump_outputs(str(tmp_path), h, np)
    planes, weak, views = (np.load(tmp_path / (n + ".npy")) for n in ("planes", "weak_info", "selected_views"))
    assert planes.dtype == np.float32 and weak.dtype == np.float32 and views.dtype == np.float64
    assert np.array_equal(planes, h.planes.reshape(-1, 4)) and np.array_equal(weak, h.weak.reshape(-1).astype(np.float32))
    assert np.array_equal(views.astype(np.uint32), h.views.reshape(-1))   # 32-bit view masks survive float64 exactly


def test_dump_of_a_large_frame_is_a_fixed_sample_within_64_mb(tmp_path):
    bench = _bench()
    hh, ww = 1100, 1000   # 1.1 Mpix: above DUMP_MAX_PIXELS
    assert hh * ww > bench.DUMP_MAX_PIXELS
    for run, seed in (("a", 1), ("b", 2)):
        bench.dump_outputs(str(tmp_path / run), _Handle(hh, ww, seed), np)
        files = sorted(os.listdir(tmp_path / run))
        assert files == ["planes.npy", "selected_views.npy", "weak_info.npy"]
        assert sum(os.path.getsize(tmp_path / run / f) for f in files) <= 64 * 1024 * 1024
    # the sampled pixels are the same in both runs: find them through the planes of run a
    h = _Handle(hh, ww, 1)
    flat = h.planes.reshape(-1, 4)
    got = np.load(tmp_path / "a" / "planes.npy")
    assert got.shape == (bench.DUMP_MAX_PIXELS, 4)
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(hh * ww, size=bench.DUMP_MAX_PIXELS, replace=False))
    assert np.array_equal(got, flat[idx])
    h2 = _Handle(hh, ww, 2)
    assert np.array_equal(np.load(tmp_path / "b" / "planes.npy"), h2.planes.reshape(-1, 4)[idx])
    assert np.array_equal(np.load(tmp_path / "b" / "selected_views.npy").astype(np.uint32), h2.views.reshape(-1)[idx])
