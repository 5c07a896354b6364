"""tools/sort_check.hip without a device: the program is built, and its self-test -- reference results of the scan and the sort,
damaged the way a subtly wrong kernel would damage them -- reports every damage.  That is what shows that the comparisons
test_gpu_sort_scan.py relies on can fail."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "sort_check")

# the damages a run has to name (each at several sizes, with a suffix) and catch
DAMAGES = ("sort_equal_neighbours_swapped", "scan_off_by_one_from_an_index_on", "scan_total_truncated_to_32_bits", "scan_last_element_dropped",
           "scan_last_input_dropped", "sort_last_element_dropped", "sort_last_key_dropped_novals", "sort_last_payload_dropped",
           "scan_canary_overwritten", "scan_input_canary_overwritten", "sort_key_canary_overwritten_result_side",
           "sort_key_canary_overwritten_other_side", "sort_payload_canary_overwritten_result_side", "sort_payload_canary_overwritten_other_side",
           "sort_in_alt_flipped", "sort_passes_one_too_many", "scan_input_changed", "sort_second_run_differs", "sort_no_pass_but_result_moved")


def test_the_program_is_built():
    assert os.path.exists(EXE), "tools/_build/sort_check not built: run __graft_entry__.build()"


def test_self_test_catches_every_damage():
    r = subprocess.run([EXE, "--self-test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    lines = dict(line.split("=", 1) for line in r.stdout.splitlines() if line.startswith("SELFTEST_"))
    clean = [k for k in lines if k.startswith("SELFTEST_clean_")]
    damaged = [k for k in lines if k not in clean and k != "SELFTEST_checks"]
    assert clean and all(lines[k] == "0" for k in clean), r.stdout          # an undamaged reference result passes
    assert all(lines[k].split()[0] == "caught" for k in damaged), r.stdout
    for d in DAMAGES:
        assert sum(k.startswith("SELFTEST_" + d) for k in damaged) >= 1, d
    assert lines["SELFTEST_checks"] == "%d passed=%d" % (len(clean) + len(damaged), len(clean) + len(damaged)), r.stdout


def test_an_unknown_group_is_refused():
    for args in (["--group", "no_such_group"], ["--group"], []):
        r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stdout and "CHECK_" not in r.stdout, (args, r.stdout)
