"""The plain solve's host-side decisions, checked without a device.

mink_amd/csrc/solve_plan.h decides from integers whether a plain solve is served (code and message of the refusal), how its arrays
travel (device pointers, the pinned scratch, staged copies, staged copies in chunks) and where each lies in the pinned scratch.
tests/host/solve_plan_cases.cpp walks it over a matrix of shapes and calls — built with the host's address and undefined-behaviour
sanitizers, run as a child process — and prints beside every cell what the code it replaced answered: run() as the host side had
it before the split, its refusals, byte sum, cursor and chunk rule copied into the program.  Equality is asserted cell by cell.
"""

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")
MKH_E_INVALID = -1                              # include/minkhip.h
SHAPES = {"g1_like", "g1", "ur5e_like", "no_frame", "com", "big_tree", "dense_rows", "dense_limits", "dense_box"}
MAX_BATCH = {"g1_like": 131072, "g1": 131072, "ur5e_like": 262144}
A_ITERS, A_CONV = 6, 7                          # solve_plan.h SolveArray: the two rows inside the int32 block


@pytest.fixture(scope="module")
def cells(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("solve_plan_cases")
    flags = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC]
    src, obj, exe = os.path.join(REPO, "tests", "host", "solve_plan_cases.cpp"), str(d / "solve_plan_cases.o"), str(d / "solve_plan_cases")
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
    """Every shape at every batch size of the list and at its own two boundaries; every call kind, pointer kind and tap set; targets
    batched or not; each input NULL in turn; dt and n_steps out of range; the no-chunks switch where chunks are possible."""
    assert {c["shape"] for c in cells} == SHAPES
    for sh in SHAPES:
        of = [c for c in cells if c["shape"] == sh]
        mb = MAX_BATCH.get(sh, 65536)
        assert {0, 1, 7, 48, 96, 16383, 16384, 26000, 36315, 36316, 40001, 65536, mb, mb + 1} <= {c["B"] for c in of}
        assert {c["kind"] for c in of} == {"eval", "solve", "steps", "until", "until_no_counts"}
        for key, want in (("batched", {0, 1}), ("taps", {0, 1, 2}), ("devp", {0, 1}), ("null_input", {-1, 0, 1, 2, 3}), ("dt_ok", {0, 1}),
                          ("n_steps", {0, 1, 3}), ("no_chunks", {0, 1}), ("unwind", {0, 1})):
            assert {c[key] for c in of} == want, (sh, key)
        assert {c["dense"] for c in of} == ({0, 1, 2, 3, 4} if sh.startswith("dense") else {0, 1})
    assert len(cells) > 40000


def test_refusals_equal_the_reference_cell_by_cell(cells):
    for c in cells:
        assert (c["rc"], c["err"]) == (c["ref_rc"], c["ref_err"]), c
        assert (c["rc"] == 0) == (c["err"] == "") == (c["refusal"] == 0), c
        assert c["rc"] in (0, MKH_E_INVALID), c


def test_every_refusal_is_reached(cells):
    """Each test of solve_refusal wins somewhere in the matrix, under its message as the source has it."""
    texts = {
        1: "B must be >= 1",
        2: "a solve: MKH_FLAG_UNWIND_TURNS is honoured by mkh_solve_multistart_set and mkh_solve_trajectory_ladder_nodes only",
        3: "q is null",
        4: "frame_targets is null (TargetNotSet)",
        5: "posture_target is null (TargetNotSet)",
        6: "com_target is null (TargetNotSet)",
        7: "dt must be > 0",
        8: "n_steps must be >= 1",
        9: "limit_lo / limit_hi need a problem created with dense_limit_box = 1",
        10: "this problem has dense (plugin) rows: call mkh_solve_dense",
        11: "dense task_e / task_J is null",
        12: "dense limit_G / limit_h is null",
        13: "dense (plugin) rows are evaluated by the caller at q: no fused steps",
        15: "mkh_solve_until needs at least one frame task to test the thresholds on",
    }
    seen = {}
    for c in cells:
        seen.setdefault(c["refusal"], set()).add(c["err"])
    for code, text in texts.items():
        assert seen.get(code) == {text}, (code, seen.get(code))
    assert seen[14] >= {"B=65537 exceeds max_batch=65536 of this problem", "B=131073 exceeds max_batch=131072 of this problem"}
    assert set(seen) == set(range(16))
    # the orders that matter: B before everything, the unwind flag before a NULL q, dt before n_steps, max_batch before the
    # threshold loop without a frame task
    assert all(c["refusal"] == 1 for c in cells if c["B"] == 0)
    assert all(c["refusal"] == 2 for c in cells if c["unwind"] and c["B"] >= 1)
    assert all(c["refusal"] == 7 for c in cells if not c["dt_ok"] and c["n_steps"] == 0 and c["B"] >= 1 and not c["unwind"])
    over = [c for c in cells if c["shape"] == "no_frame" and c["kind"].startswith("until") and c["B"] == 65537 and c["null_input"] < 0
            and c["dt_ok"] and c["n_steps"] >= 1 and c["dense"] == 0 and not c["unwind"]]
    assert over and all(c["refusal"] == 14 for c in over)


def test_routes_chunks_and_layouts_equal_the_reference_cell_by_cell(cells):
    ok = served(cells)
    assert len(ok) > 8000
    for c in ok:
        assert (c["route"], c["n_chunks"], c["chunk"]) == (c["ref_route"], c["ref_n_chunks"], c["ref_chunk"]), c
        assert (c["route"] == "device") == bool(c["devp"]), c
        if not c["devp"]:
            assert c["pinned_total"] == c["ref_pinned_total"], c
            assert (c["route"] == "pinned") == (c["pinned_total"] <= 65536 and not c["shape"].startswith("dense")), c
        if c["route"] == "pinned":
            assert c["off"] == c["ref_off"], c
            assert c["ref_q_out_in_place"] == 1, c
            assert all(o % 8 == 0 for i, o in enumerate(c["off"]) if i not in (A_ITERS, A_CONV) and o >= 0), c
            assert max(c["off"]) < c["pinned_total"], c
        else:
            assert "off" not in c, c


def test_chunks_tile_the_batch(cells):
    chunked = [c for c in served(cells) if c["route"] == "chunked"]
    assert len(chunked) > 100
    for c in chunked:
        n, chunk, B = c["n_chunks"], c["chunk"], c["B"]
        assert 2 <= n <= 4 and chunk >= 8192 and chunk % 64 == 0, c
        spans = [(k * chunk, chunk if k + 1 < n else B - k * chunk) for k in range(n)]
        assert spans[0][0] == 0 and all(s[1] >= chunk for s in spans), c        # (the last one takes the remainder: never shorter)
        assert all(spans[k][0] + spans[k][1] == spans[k + 1][0] for k in range(n - 1)) and spans[-1][0] + spans[-1][1] == B, c
        assert not c["no_chunks"] and c["taps"] == 0 and c["kind"] != "eval", c
    assert {c["n_chunks"] for c in chunked} == {2, 3, 4}
    assert any(c["B"] % c["chunk"] for c in chunked)                            # a ragged last chunk
    # the switch: the same cell without chunks is staged
    key = lambda c: tuple(c[k] for k in ("shape", "B", "kind", "batched", "taps", "devp", "null_input", "dt_ok", "n_steps", "dense", "unwind"))
    plain = {key(c): c for c in served(cells) if c["no_chunks"]}
    twins = [plain[key(c)] for c in chunked if key(c) in plain]
    assert len(twins) > 50 and all(t["route"] == "staged" for t in twins)


def test_every_route_and_both_sides_of_each_boundary(cells):
    ok = served(cells)
    assert {c["route"] for c in ok} == {"device", "pinned", "staged", "chunked"}
    key = lambda c: tuple(c[k] for k in ("shape", "kind", "batched", "taps", "devp", "null_input", "dt_ok", "n_steps", "dense", "no_chunks", "unwind"))
    by = {}
    for c in ok:
        by.setdefault(key(c), {})[c["B"]] = c["route"]
    # 64 KB: some cell is pinned and the cell with one more instance staged; 32 MB: staged, and chunked with one more
    assert any(r == "pinned" and of.get(B + 1) == "staged" for of in by.values() for B, r in of.items())
    assert any(r == "staged" and of.get(B + 1) == "chunked" for of in by.values() for B, r in of.items())
    # B >= 2 * 8192 on its own: 16 383 instances are never chunked, whatever they stage
    assert all(c["route"] != "chunked" for c in ok if c["B"] < 16384)
