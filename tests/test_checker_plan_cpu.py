"""The collision checker's host-side decisions, checked without a device.

mink_amd/csrc/checker_plan.h decides from integers whether a checker handle can serve a call (code and message of the refusal) and
how many items of a chunked launch its buffers hold.  tests/host/checker_cases.cpp walks it over a matrix of shapes and uses —
built with the host's address and undefined-behaviour sanitizers, run as a child process — and prints beside every cell what the
functions it replaced answered: clearance_refuse / sweep_refuse as the host side had them before the split, copied into the program
and called as the entry points called them.  Equality is asserted cell by cell; for every served cell the chunk sizes are held to
their guarantee (at least one item, never more items than the buffer has rows).
"""

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")
MKH_E_INVALID, MKH_E_LIMIT = -1, -4            # include/minkhip.h


@pytest.fixture(scope="module")
def cells(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("checker_cases")
    flags = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC]
    src, obj, exe = os.path.join(REPO, "tests", "host", "checker_cases.cpp"), str(d / "checker_cases.o"), str(d / "checker_cases")
    r = subprocess.run([hipcc] + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    subprocess.run([hipcc, "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined", obj, "-o", exe], check=True)   # (host code only: the sanitizers never see the device)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]             # the sanitized run: nothing reported
    return [json.loads(line) for line in r.stdout.splitlines()]


def served(cells):
    return [c for c in cells if c["rc"] == 0]


def test_matrix_is_complete(cells):
    """n_cv in {0, 3}; sweep_rows in {0, M - 1, M, 10 M + 1}; check_rows in {0, item - 1, item, 3 item + 1} for both item sizes; every
    use at M in {1, 2} and at the sample counts below 1 that reach the refusal clamped; the structural refusals."""
    groups = {c["group"] for c in cells}
    assert groups == {"analytic", "convex", "no_pairs", "no_wide", "convex_not_pre", "bodies_1170", "bodies_1171", "sweep_lds_fits",
                      "sweep_lds_over", "quarter_lds", "whole_lds"}
    for g in groups:
        of = [c for c in cells if c["group"] == g]
        assert {c["use"] for c in of} == {"clearance", "sweep", "tracking", "refinement", "ladder", "ladder_refined"}
        assert {c["n_samples"] for c in of if c["use"] == "sweep"} == {1, 2}
        for use in ("tracking", "refinement", "ladder", "ladder_refined"):
            assert {c["n_samples"] for c in of if c["use"] == use} == {-1, 0, 1, 2}
        for c in of:
            M = max(c["n_samples"], 1)
            mine = [x for x in of if (x["use"], x["n_samples"]) == (c["use"], c["n_samples"])]
            assert {x["sweep_rows"] for x in mine} == {0, M - 1, M, 10 * M + 1}
            want = {0} | {r for item in (1 + M, 1 + 2 * M) for r in (item - 1, item, 3 * item + 1)}
            assert {x["check_rows"] for x in mine} == want
            assert len(mine) == len({(x["sweep_rows"], x["check_rows"]) for x in mine}) == len({0, M - 1, M, 10 * M + 1}) * len(want)
    assert {c["n_cv"] for c in cells if c["group"] in ("analytic", "convex")} == {0, 3}
    assert len(cells) > 4000


def test_uses_are_what_the_entry_points_passed(cells):
    for c in cells:
        M = max(c["n_samples"], 1)
        want = {"clearance": (0, 0), "sweep": (M, 0), "tracking": (0, 1 + M), "refinement": (M, 1 + 2 * M), "ladder": (M, 0),
                "ladder_refined": (M, 1 + 2 * M)}[c["use"]]
        assert (c["sweeps_edges"], c["item_rows"]) == want, c


def test_refusals_equal_the_reference_cell_by_cell(cells):
    for c in cells:
        assert (c["rc"], c["err"]) == (c["ref_rc"], c["ref_err"]), c
        assert (c["rc"] == 0) == (c["err"] == ""), c


def test_every_refusal_is_reached(cells):
    """Each test of the refusal wins somewhere in the matrix, with its code — and the two orders that matter: check_rows is judged
    before sweep_rows, 'no room' before 'too little room'."""
    def count(code, text, **where):
        return sum(1 for c in cells if c["rc"] == code and text in c["err"] and all(c[k] == v for k, v in where.items()))
    assert count(MKH_E_INVALID, "has no collision pairs", group="no_pairs") == sum(1 for c in cells if c["group"] == "no_pairs")
    assert count(MKH_E_INVALID, "MKH_DIAG_NO_WIDE_REDO", group="no_wide") == sum(1 for c in cells if c["group"] == "no_wide")
    assert count(MKH_E_INVALID, "not pre-evaluated on this handle", group="convex_not_pre") == sum(1 for c in cells if c["group"] == "convex_not_pre")
    assert count(MKH_E_LIMIT, "1171 bodies: the poses of one row", group="bodies_1171") == sum(1 for c in cells if c["group"] == "bodies_1171")
    assert count(MKH_E_LIMIT, "the poses of one row") == sum(1 for c in cells if c["group"] == "bodies_1171")
    assert count(MKH_E_INVALID, "this call judges rows it produces inside a launch") > 0
    assert count(MKH_E_INVALID, "and check_rows, but this call also sweeps edges") > 0
    assert count(MKH_E_INVALID, "the samples of a sweep are never written there (mkh_problem_set_sweep_rows") > 0
    assert count(MKH_E_LIMIT, "check_rows = 4 holds less than one item of 5 rows", use="refinement", n_samples=2) > 0
    assert count(MKH_E_LIMIT, "check_rows = 1 holds less than one item of 2 rows", use="tracking", n_samples=0) > 0
    assert count(MKH_E_LIMIT, "sweep_rows = 1 holds less than one edge of n_samples = 2 samples") > 0
    assert count(MKH_E_LIMIT, "1000 bodies, nq = 398", group="sweep_lds_over") > 0
    assert count(MKH_E_LIMIT, "32 bodies, nq = 700", group="quarter_lds") > 0
    assert count(MKH_E_LIMIT, "do not fit 64 KB of LDS (7 nbody + 3 nq", group="whole_lds") == 0
    assert count(MKH_E_LIMIT, "do not fit 64 KB of LDS", group="sweep_lds_fits") == 0
    # the clearance alone is served whatever the buffers hold, and on the shapes only a sweep's LDS slice refuses
    for c in cells:
        if c["use"] == "clearance" and c["group"] not in ("no_pairs", "no_wide", "convex_not_pre", "bodies_1171"):
            assert c["rc"] == 0, c
    # a checker without general convex pairs needs no room at all
    assert all(c["rc"] == 0 for c in cells if c["group"] == "analytic")
    # no room (INVALID) wins over too little room (LIMIT) of the other buffer
    for c in cells:
        if c["n_cv"] > 0 and c["rc"] == MKH_E_LIMIT and "rows =" in c["err"]:
            assert (c["item_rows"] == 0 or c["check_rows"] > 0) and (c["sweeps_edges"] == 0 or c["sweep_rows"] > 0), c
    both_short = [c for c in cells if c["group"] == "convex" and 0 < c["check_rows"] < c["item_rows"] and 0 < c["sweep_rows"] < c["sweeps_edges"]]
    assert both_short and all("check_rows =" in c["err"] for c in both_short)


def test_chunks_of_served_cells(cells):
    """A served use never meets a chunk of zero items (a loop of launches that does not advance), and a chunk never holds more rows
    than its buffer."""
    ok = served(cells)
    assert len(ok) > 1000 and any(c["n_cv"] > 0 and c["item_rows"] and c["sweeps_edges"] for c in ok)
    for c in ok:
        assert c["clearance_chunk"] == c["max_batch"] >= 1, c
        if c["n_cv"] == 0:
            continue                                           # (one launch: nothing goes through a buffer)
        if c["sweeps_edges"]:
            assert c["sweep_chunk"] >= 1 and c["sweep_chunk"] * c["sweeps_edges"] <= c["sweep_rows"], c
            assert (c["sweep_chunk"] + 1) * c["sweeps_edges"] > c["sweep_rows"], c           # (and no smaller than it has to be)
        else:
            assert c["sweep_chunk"] == 0, c
        if c["item_rows"]:
            assert c["check_chunk"] >= 1 and c["check_chunk"] * c["item_rows"] <= c["check_rows"], c
            assert (c["check_chunk"] + 1) * c["item_rows"] > c["check_rows"], c
        else:
            assert c["check_chunk"] == 0, c
    # per == 1 and a remainder are both in the matrix
    assert any(c["sweep_chunk"] == 1 for c in ok if c["n_cv"] and c["sweeps_edges"] == 2)
    assert any(c["check_chunk"] == 1 for c in ok if c["n_cv"] and c["item_rows"] == 5)
    assert any(c["check_chunk"] == 3 and c["check_rows"] % c["item_rows"] for c in ok if c["n_cv"] and c["item_rows"])
