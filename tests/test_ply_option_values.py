"""The values of the --ply-* flags as the drop-in's command line reads them (apd-mvs_amd/host/ply_options.h, through
host_capi.cpp: apdhost_parse_ply_option): verdict, parsed fields and the exact message of a refusal.

The expected column, tests/golden/ply_option_values.json, was recorded from the hand-written parsing that ply_options.h replaced
(the ParseOptions of host/main.cpp before it, compiled into a scratch program and run on every row), not from the code under test.
It holds every bad and good value of the test_binary_refuses_a_bad_value_* tests, file names with commas, `,scale`, the optional
tails, the bounds of every count and radii whose square leaves the floats.  The rows of PADDED are the only ones on which the two
differ: the old parsing capped K of --ply-stat-filter at 9 characters and ITERATIONS of --ply-smooth at 2 instead of checking the
number, so a count in range with that many leading zeros was refused; it now reads as the same count without them.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "apd-mvs_amd", "_build", "libapd_host.so")
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "ply_option_values.json")))
PADDED = {("--ply-stat-filter", "1,0000000008,1"): "1,8,1", ("--ply-stat-filter", "1,00000000000000000000064,1"): "1,64,1",
          ("--ply-smooth", "1,2,003"): "1,2,3", ("--ply-smooth", "1,2,016"): "1,2,16", ("--ply-smooth", "1,2,0000000000000000000016"): "1,2,16"}


@pytest.fixture(scope="module")
def parse(pkg):
    assert os.path.exists(HOST_LIB), "run __graft_entry__.build() first"
    pkg.lib()  # libapd_host.so depends on libapd_mi355x.so
    L = C.CDLL(HOST_LIB)
    L.apdhost_parse_ply_option.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]

    def call(flag, value):
        fields, message = C.create_string_buffer(4096), C.create_string_buffer(1024)
        rc = L.apdhost_parse_ply_option(flag.encode(), value.encode(), fields, len(fields), message, len(message))
        return rc, dict(line.split(" ", 1) for line in fields.value.decode().splitlines()), message.value.decode()
    return call


def test_the_table_holds_what_it_should():
    rows = {(r["flag"], r["value"]): r for r in TABLE["rows"]}
    assert len(rows) == len(TABLE["rows"]) > 300
    assert {flag for flag, _ in rows} == {"--ply-voxel", "--ply-stat-filter", "--ply-radius-filter", "--ply-component-filter", "--ply-smooth",
                                          "--ply-estimate-normals", "--ply-render-vis", "--ply-register", "--ply-align", "--ply-score"}
    for key, plain in PADDED.items():   # refused before, and the value without the zeros is a row to take the fields from
        assert not rows[key]["good"] and rows[(key[0], plain)]["good"], key
    # the bounds: K, iterations of --ply-smooth and of --ply-align, splat, trials
    for flag, value, good in (("--ply-stat-filter", "1,1,1", True), ("--ply-stat-filter", "1,64,1", True), ("--ply-stat-filter", "1,0,1", False),
                              ("--ply-stat-filter", "1,65,1", False), ("--ply-smooth", "1,2,16", True), ("--ply-smooth", "1,2,17", False),
                              ("--ply-render-vis", "8,0", True), ("--ply-render-vis", "9,0", False), ("--ply-register", "truth.ply,1,1,65536", True),
                              ("--ply-align", "truth.ply,0.5,64", True)):
        assert rows[(flag, value)]["good"] is good, (flag, value)
    # one past the trials and the iterations is no count, so it reads as the number before it and the file's name grows
    assert rows[("--ply-register", "truth.ply,1,1,65537")]["fields"]["register_truth"] == "truth.ply,1"
    assert rows[("--ply-align", "truth.ply,0.5,65")]["fields"]["align_truth"] == "truth.ply,0.5"


def test_every_row(parse):
    rows = {(r["flag"], r["value"]): r for r in TABLE["rows"]}
    for key, row in rows.items():
        rc, fields, message = parse(*key)
        want = rows[(key[0], PADDED[key])] if key in PADDED else row
        if want["good"]:
            assert (rc, message) == (0, "") and fields == {**TABLE["defaults"], **want["fields"]}, (key, rc, message, fields)
        else:
            assert (rc, message) == (1, want["message"]) and fields == TABLE["defaults"], (key, rc, message, fields)


def test_the_special_cases(parse):
    assert parse("--ply-render-vis", "1,0.01")[1]["vis"] == "1"   # implies --ply-vis
    assert parse("--ply-vis", "")[0] == parse("--ply-mean", "")[0] == parse("--ply-normals", "1")[0] == parse("--seed", "1")[0] == -1
    _, fields, _ = parse("--ply-align", "a,b.ply,0.5,7,scale")
    assert (fields["align_truth"], fields["align_radius"], fields["align_iterations"], fields["align_scale"]) == ("a,b.ply", "0.5", "7", "1")
    _, fields, _ = parse("--ply-register", "a,1,2,3,4,5")        # the longest tail that parses
    assert [fields["register_" + k] for k in ("truth", "radius", "distance", "trials", "seed")] == ["a,1", "2", "3", "4", "5"]
    _, fields, _ = parse("--ply-score", "a,b,c.ply,0.25")         # split at the last comma
    assert (fields["score_truth"], fields["score_threshold"]) == ("a,b,c.ply", "0.25")
