"""The device sort and the device scan of csrc/apd_sort.h called directly (tools/sort_check.hip, linked against the library the build
made) and held to a uint64_t running sum and to std::stable_sort: sizes past those any merge reaches (two block sums in a lane of
the top scan: more than 2^21 scan entries, more than 2^24 keys), bit 63 of a key, totals past 2^32, the contract of `passes` and
`in_alt`, keys chosen against the ballot ranking, payloads that are no indices; canary words behind every buffer, every sort run
twice.  One child process per group; measured on the MI355X: scan_sizes 0.8 s, scan_values 0.4 s, sort_sizes 0.4 s, sort_keys 0.4 s,
sort_large 3.8 s -- the time limits are 30 to 150 times that.  That the comparisons can fail: test_sort_check.py."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "sort_check")


def run_group(group, cases, timeout):
    assert os.path.exists(EXE), "tools/_build/sort_check not built: run __graft_entry__.build()"
    r = subprocess.run([EXE, "--group", group], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    checks = dict(line.split("=", 1) for line in r.stdout.splitlines() if line.startswith("CHECK_"))
    count = checks.pop("CHECK_%s_cases" % group, None)
    assert count == str(cases) and len(checks) == cases, (count, len(checks), cases)   # a group that ran fewer cases fails
    assert all(k.startswith("CHECK_%s_" % group) for k in checks), sorted(checks)
    wrong = {k: v for k, v in checks.items() if v != "0"}
    assert not wrong, wrong


def test_scan_sizes(gpu_pkg):
    """16 sizes from 0 to 3 S P + 5 S + 3, around a lane's run, a block, and the S P entries at which a lane of the top scan takes a
    second block sum; inputs random in 0..3 and all ones."""
    run_group("scan_sizes", 32, 60)


def test_scan_values(gpu_pkg):
    """All zero; all 0xFFFFFFFF at 2, S + 1 and S P + 1 entries (totals past 2^32, block prefixes near 2^53); random 32-bit values;
    one non-zero entry at 0, S - 1, S and n - 1."""
    run_group("scan_values", 10, 60)


def test_sort_sizes(gpu_pkg):
    """17 sizes from 0 to 100 T + 5 of random 64-bit keys: all eight passes, bit 63 set in half of the keys."""
    run_group("sort_sizes", 17, 60)


def test_sort_keys(gpu_pkg):
    """27 key patterns at 3 T + 17 (equal keys, one varying digit or bit, sorted, reversed, few distinct keys, waves of one digit,
    waves of 64 digits, a tile of one digit, digit 0 in the last wave, random payloads), each with and without a payload."""
    run_group("sort_keys", 54, 60)


def test_sort_large(gpu_pkg):
    """8192 T keys and one more: the [digit][block] table of a pass has S P entries and S P + 256.  Most of the time is the host's
    std::stable_sort of 16.8 million pairs."""
    run_group("sort_large", 2, 120)
