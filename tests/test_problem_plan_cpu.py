"""The host tables of problem creation, checked without a device.

mink_amd/csrc/problem_plan.hip plans a problem as plain data (problem_plan.h); tests/host/plan_cases.cpp drives it over synthetic
models and descriptors that put every fixed-size array of the device descriptor at its edge, built with the host's address and
undefined-behaviour sanitizers and run as a child process.  The tables it prints are recomputed here from the models' parent
arrays and the descriptors' costs, not from the plan.

Lists of limits (the `lim_*` cases): 2 to 4 ConfigurationLimits and VelocityLimits with their own gain, bounds and index subset
(two of them disjoint, one velocity term naming a dof four times), two PostureTasks and two CollisionAvoidanceLimits that share
a geom pair.  Every entry of every copy the plan makes — lane tables at stride 64, LaneProblem2 and its narrowed LaneProblem,
the wide arrays at stride nv, the parameters per pair — is recomputed from the descriptor and compared exactly; five limits of a
kind are refused with MKH_E_LIMIT and the cap in the text.

The large models of tests/wide_cases.py (the `wide` cases; the program reads them from a file this test writes from the same MJCF
text the device tests load): the layout of the workgroup-per-problem kernel is recomputed here from the model's counts
(`wide_layout`, which shares no code with plan_wide), the chain bit table from the parent arrays, and each model is held to the
branch it was chosen for — the device tests of tests/test_gpu_wide_sizes.py run exactly these models.
"""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import wide_cases as wc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")
KMU, KMU_BIG, KWOOD_LIST = 18, 24, 16          # lds_layout.h kMu / kMuBig, mkh_types.h kWoodList


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    from mink_amd.csrc import build as hipbuild

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("plan_cases")
    # the table of variants.h from the same list as the library's, with null launch pointers
    table = d / "variant_table.hip"
    table.write_text(hipbuild.variant_table_source(launchers=False).replace('"../variants.h"', '"variants.h"'))
    flags = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC]
    srcs = [os.path.join(REPO, "tests", "host", "plan_cases.cpp"), os.path.join(CSRC, "problem_plan.hip"), str(table)]
    objs = [str(d / (os.path.basename(s) + ".o")) for s in srcs]
    procs = [subprocess.Popen([hipcc] + flags + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for s, o in zip(srcs, objs)]
    for p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, out
    exe = str(d / "plan_cases")
    subprocess.run([hipcc, "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined"] + objs + ["-o", exe], check=True)   # (host code only: the sanitizers never see the device)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]             # the sanitized run: nothing reported
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    # the large models of tests/wide_cases.py, from a description file
    spec = d / "wide_models.txt"
    spec.write_text("".join(wc.spec_line(name) + "\n" for name in wc.HOST_MODELS))
    r = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    rows += [json.loads(line) for line in r.stdout.splitlines()]
    return {(c["model"], c["case"]): c for c in rows}


def chain_of(c, body):
    """Dofs on the chain world -> body, from the parent array alone."""
    dofs = []
    while body > 0:
        if c["body_dofnum"][body] > 0:
            dofs += range(c["body_dofadr"][body], c["body_dofadr"][body] + c["body_dofnum"][body])
        body = c["body_parentid"][body]
    return sorted(dofs)


def task_rows(c):
    """Per frame task: its active rows (cost != 0) — then the ComTask's."""
    return [[r for r in range(6) if t["cost"][r] != 0] for t in c["tasks"]]


def ok_cases(plans, wavefront=True):
    return [c for c in plans.values() if c["rc"] == 0 and (not wavefront or not c["big"])]


def tables_in_effect(c):
    return c["sel"]["wood_nt"] != 0 or c["sel"]["woodr_tables"] != 0


def test_every_case_planned(plans):
    assert len(plans) > 200
    wide = {m for m, case in plans if case == "wide"}
    assert wide == set(wc.HOST_MODELS) and len(wide) == 11
    models = {m for m, _ in plans} - wide
    assert models == {"chain6", "chain16", "chain17", "chain44", "chain63", "chain64", "tree44", "tree62", "ball11", "chain68"}
    assert {m: plans[(m, "wide")]["nv"] for m in wide} == {
        "chain123": 123, "chain124": 124, "chain130": 130, "chain300": 300, "chain_last": wc.CHAIN_LAST, "chain_last+1": wc.CHAIN_LAST + 1,
        "ball80": 80, "ball86": 86, "ball92": 92, "fixed30": 30, "hinge80": 80}
    assert {plans[(m, "t1_r6")]["nv"] for m in models} == {6, 16, 17, 44, 63, 64, 62, 11, 68}
    # enough of them take the low-rank start for the table checks below to mean something
    assert sum(1 for c in ok_cases(plans) if tables_in_effect(c)) >= 40
    assert sum(1 for c in ok_cases(plans) if c["sel"]["woodr_tables"]) >= 8
    assert sum(1 for c in ok_cases(plans) if c["dev"]["wood_trip"] > 0) >= 15


def test_task_rows_and_tap_layout(plans):
    for c in ok_cases(plans, wavefront=False):
        rows = task_rows(c)
        n_jrows = sum(len(r) for r in rows) + c["com_rows"]
        d = c["dev"] if not c["big"] else c["wide"]
        assert d["n_jrows"] == n_jrows, (c["model"], c["case"])
        assert d["n_rows_tap"] == 6 * len(rows) + c["n_posture"] * c["nv"] + 3 * c["n_com"] + (3 if c["dense"] else 0)
        assert c["dev"]["n_rows_tap"] == d["n_rows_tap"]


def test_direct_pair_lanes(plans):
    """dpair_*: the (task, dof) bits in task-major, dof-ascending order — the frame's chain and, for a RelativeFrameTask, its root's
    — and none at all beyond 64."""
    for c in ok_cases(plans):
        want = []
        for t, task in enumerate(c["tasks"]):
            dofs = set(chain_of(c, task["body"])) | (set(chain_of(c, task["root"])) if task["root"] >= 0 else set())
            want += [(t, k) for k in sorted(dofs)]
        d = c["dev"]
        if len(want) <= 64:
            assert d["n_dpairs"] == len(want)
            assert list(zip(d["dpair_task"], d["dpair_dof"]))[:len(want)] == want, (c["model"], c["case"])
        else:
            assert d["n_dpairs"] == 0
    assert plans[("chain16", "dpairs64")]["dev"]["n_dpairs"] == 64
    assert plans[("chain17", "dpairs65")]["dev"]["n_dpairs"] == 0


def test_low_rank_tables(plans):
    for c in ok_cases(plans):
        if not tables_in_effect(c):
            continue
        key = (c["model"], c["case"])
        d, nv = c["dev"], c["nv"]
        rows = task_rows(c)
        n = d["n_jrows"]
        # which task owns compact row r; the ComTask's rows are dense over the robot's dofs
        owner = [t for t, r in enumerate(rows) for _ in r] + [-1] * c["com_rows"]
        assert len(owner) == n
        groups = 64 // n
        rpc = -(-(n + 1) // groups)
        assert d["wood_rpc"] == rpc and d["wood_jrhs"] == n % rpc, key
        # rows [wood_row0, +wood_rpc) over the chunks of one column cover 0 … n_jrows once
        for col in range(n):
            covered = np.zeros(groups * rpc, dtype=int)
            for lane in range(64):
                if d["wood_col"][lane] == col:
                    covered[d["wood_row0"][lane]:d["wood_row0"][lane] + rpc] += 1
            assert (covered[:n + 1] == 1).all(), key
        lens = []
        for lane in range(64):
            if lane >= groups * n:
                assert d["wood_col"][lane] == -1
                continue
            col = lane % n
            assert d["wood_col"][lane] == col and d["wood_row0"][lane] == (lane // n) * rpc, key
            dofs = chain_of(c, c["tasks"][owner[col]]["body"]) if owner[col] >= 0 else list(range(nv))
            assert int(d["wood_mask"][lane]) == sum(1 << k for k in dofs), key
            lens.append(len(dofs))
        # the packed lists: the mask's bits ascending, one byte each, padded to the longest with a dof off the chain
        off_chain = lambda dofs: [k for k in range(nv) if k not in dofs]
        lanes = [lane for lane in range(groups * n)]
        chains = {lane: (chain_of(c, c["tasks"][owner[lane % n]]["body"]) if owner[lane % n] >= 0 else list(range(nv))) for lane in lanes}
        trip = max(lens)
        applies = trip <= KWOOD_LIST and all(len(chains[l]) == trip or off_chain(chains[l]) for l in lanes)
        assert d["wood_trip"] == (trip if applies else 0), key
        if applies:
            lists = np.array(d["wood_list"], dtype=np.uint32).reshape(64, 4)
            for lane in lanes:
                got = [int(lists[lane][i >> 2] >> (8 * (i & 3))) & 255 for i in range(trip)]
                m = len(chains[lane])
                assert got[:m] == chains[lane], key
                assert all(g not in chains[lane] and 0 <= g < nv for g in got[m:]), key
                assert len(set(got[m:])) <= 1
        # (task, dof) pair lanes of the Jacobian rows and the source of each row's weighted error
        want = [(t, k) for t, task in enumerate(c["tasks"]) for k in chain_of(c, task["body"])]
        assert d["n_jpairs"] == len(want) <= 256, key
        assert list(zip(d["jpair_task"], d["jpair_dof"]))[:len(want)] == want, key
        mu = [t * 64 + 30 + r for t, rr in enumerate(rows) for r in rr]
        assert d["mu_src"][:len(mu)] == mu, key
        assert all(x < 0 for x in d["mu_src"][len(mu):n])           # ComTask rows: computed on the device
    # 256 pair lanes are the capacity: one more and the plan drops the low-rank start
    assert plans[("chain44", "jpairs256")]["sel"]["wood_nt"] == 44 and plans[("chain44", "jpairs256")]["dev"]["n_jpairs"] == 256
    assert plans[("chain44", "jpairs257")]["sel"]["wood_nt"] == 0
    # kMu / kMuBig and one past each
    assert plans[("tree44", "t4_rows18")]["sel"]["wood_big"] == 0 and plans[("tree44", "t4_rows19")]["sel"]["wood_big"] == 1
    assert plans[("tree44", "t4_rows24")]["sel"]["wood_nt"] == 44 and plans[("tree44", "t5_rows25")]["sel"]["wood_nt"] == 0
    # chains of 6 + 12 / 13 dofs are beyond the packed lists; 6 + 9 / 10 fill them exactly
    assert plans[("tree44", "t4_rows18")]["dev"]["wood_trip"] == KWOOD_LIST
    assert plans[("chain17", "t1_r6")]["sel"]["wood_nt"] and plans[("chain17", "t1_r6")]["dev"]["wood_trip"] == 0


def test_reserved_lds_is_the_layout_statement(plans):
    """Every *_lds_bytes* figure a launch reserves is 8 x total of build_lds_layout for that build on that descriptor (the program
    prints both: this checks the plumbing between plan and layout), and the four-waves figure only where 16 wavefronts fit."""
    for c in ok_cases(plans):
        s, lay = c["sel"], c["layout"]
        names = ["lds_bytes", "lds_bytes_full", "lds_bytes_w3", "wood_lds_bytes_w3", "wood_lds_bytes_w4", "woodr_lds", "lds_tight",
                 "woodr_lds_tight"] + (["wood_lds_bytes"] if s["wood_nt"] else [])
        for name in names:
            if s[name]:
                assert s[name] == lay[name], (c["model"], c["case"], name)
        assert s["lds_bytes"] > 0 and s["lds_bytes_full"] > 0
        assert s["wood_lds_bytes_w4"] <= 10240
        if s["wood_lds_bytes_w4"]:
            assert s["wood_nt"] == 44 and s["wood_lds_bytes_w3"] > 0
        assert (s["nt_tight"] == 48) == bool(c["tight"]) == (s["lds_tight"] > 0)
    assert sum(1 for c in ok_cases(plans) if c["sel"]["wood_lds_bytes_w4"]) >= 5
    assert sum(1 for c in ok_cases(plans) if c["sel"]["lds_tight"]) >= 4
    assert plans[("tree44", "t2_rows9_boxpairs4")]["sel"]["woodr_lds"] > 0
    assert plans[("tree44", "t2_rows9_boxpairs21")]["sel"]["woodr_lds_tight"] > 0


def test_humanoid_shape_selects_the_headline_builds(plans):
    """The project's own record (docs/HISTORY.md): a 44-dof floating-base tree with feet (6 rows) and palms (3 rows) — 18 task
    rows — plus a posture task runs the low-rank start on the 44-row builds with one more wave."""
    s = plans[("tree44", "t4_rows18")]["sel"]
    assert s["wood_nt"] == 44 and s["wood_nr"] == 44 and s["wood_lds_bytes_w3"] > 0
    print("wood_lds_bytes_w4 =", s["wood_lds_bytes_w4"])
    assert plans[("tree44", "t3_rows18")]["dev"]["wood_refine"] == 1
    assert plans[("tree44", "t3_rows18_norefine")]["dev"]["wood_refine"] == 0


def test_kernel_families(plans):
    for c in ok_cases(plans, wavefront=False):
        s, key = c["sel"], (c["model"], c["case"])
        rows = c["n_pairs_in"]
        if c["big"]:
            assert s["wide_only"] == 1 and c["wide"]["built"] == 1 and c["wide"]["chain_words"] == (c["nv"] + 63) // 64 and c["lane"]["cls"] == 0, key
            assert c["wide"]["chain_words"] == 2 or c["case"] == "wide", key
            continue
        assert s["wide_only"] == 0 and c["wide"]["built"] == (1 if rows else 0), key
        assert c["dev"]["n_pairs"] == rows and c["dev"]["max_rows"] == min(rows, 64 - c["nv"]), key
        assert c["dev"]["nt"] == s["nt"] >= c["nv"] + c["dev"]["max_rows"], key
        assert c["n_cv"] == (1 if c["cylbox"] else 0) and s["convex_pairs"] == c["cylbox"], key
        if c["cylbox"]:
            # the chains root -> body of the pair's two geoms: the last body, then body 1
            last = c["nbody"] - 1
            up = []
            b = last
            while b > 0:
                up.append(b)
                b = c["body_parentid"][b]
            assert c["cv_pair"] == [rows - 1] and c["cv_chain"] == up[::-1] + [1] and c["cv_adr"] == [0, len(up), len(up) + 1], key
        if c["lane"]["cls"]:
            assert c["lane"]["nv"] == c["nv"] and c["lane"]["nq"] == c["nq"] and c["nv"] <= 32 and not rows and not c["dense"], key
    assert plans[("chain6", "t1_r6")]["sel"]["lane_nv"] == 6 and plans[("chain16", "t1_r6")]["sel"]["quad_nt"] == 16
    assert plans[("chain17", "t1_r6")]["sel"]["quad_nt"] == 32 and plans[("chain44", "t1_r6")]["sel"]["quad_nt"] == 0
    assert plans[("ball11", "t1_r6")]["lane"]["cls"] == 0                      # (a ball joint: wavefront kernel)
    assert plans[("chain16", "t1_r6_relative")]["sel"]["has_relative"] == 1


KMAX_BOX, KMAX_POSTURE = 4, 4                  # mkh_types.h kMaxBoxTerms, kMaxPostureTasks
INF = float("inf")
LIST_MODELS = {"chain6": (6, 16), "chain16": (16, 16), "chain17": (32, None), "ball11": (0, None), "chain68": (0, None)}


def box_tables(c, stride, filled=True):
    """[term][stride] arrays of a list of limits from the descriptor alone: a configuration term bounds the dofs it names by
    lower / upper at the joint's qpos address (a dof named twice: the same value), a velocity term by the smallest limit given
    for the dof; every other entry is -inf / +inf / +inf — and a list without terms still has one such row."""
    nv, desc = c["nv"], c["desc"]
    nc, nl, npost = len(desc["cfg"]), len(desc["vel"]), len(desc["post"])
    clo = np.full((max(nc, 1), stride), -INF); chi = np.full((max(nc, 1), stride), INF)
    vlim = np.full((max(nl, 1), stride), INF); pcost = np.zeros((max(npost, 1), stride))
    if filled:
        for t, term in enumerate(desc["cfg"]):
            for dof in term["indices"]:
                clo[t, dof] = term["lower"][c["dof_qposadr"][dof]]
                chi[t, dof] = term["upper"][c["dof_qposadr"][dof]]
        for t, term in enumerate(desc["vel"]):
            for dof, lim in zip(term["indices"], term["limit"]):
                vlim[t, dof] = min(vlim[t, dof], lim)
        for t, term in enumerate(desc["post"]):
            pcost[t, :nv] = term["cost"]
    return pcost, clo, chi, vlim


def list_cases(plans):
    return [c for c in plans.values() if c.get("lists") and c["rc"] == 0]


def same(got, want, key, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (key, what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)            # (exact: the plan copies, it does not compute; no NaN anywhere)
    assert len(bad) == 0, (key, what, bad[:8], got[bad[:8]], want[bad[:8]])


def test_limit_lists_cover_every_table(plans):
    """The list cases reach every copy of the box tables: lane tables, both lane descriptors with and without the narrowed one,
    the wide arrays of small and large models, and two collision limits."""
    cases = list_cases(plans)
    assert len(cases) == 60
    for m, (cls, narrowed) in LIST_MODELS.items():
        c = plans[(m, "lim_c4_v4")]
        assert c["lane"]["cls"] == cls and ("lane2" in c["tables"]) == bool(cls) and ("lane1" in c["tables"]) == bool(narrowed), m
        assert "wide" in plans[(m, "lim_c4_v4_col2")]["tables"], m
    assert "wide" in plans[("chain68", "lim_c4_v4")]["tables"] and plans[("chain68", "lim_c4_v4")]["big"]
    for c in cases:
        desc = c["desc"]
        want = {"lim_c2_v2": (2, 2, 0), "lim_c4_v4": (4, 4, 0), "lim_c3_v0": (3, 0, 0), "lim_c0_v3": (0, 3, 0),
                "lim_c2_v2_col2": (2, 2, 2), "lim_c4_v4_col2": (4, 4, 2)}[c["case"]]
        assert (len(desc["cfg"]), len(desc["vel"]), len(desc["col"])) == want and len(desc["post"]) == 2
        # what the terms were made to be: own gains, disjoint subsets (a dof of term 1 is in no term before it), one dof named
        # four times in velocity term 1 (once in its half, three more behind it) with the smallest limit between two larger ones
        if len(desc["cfg"]) >= 2:
            i0, i1 = set(desc["cfg"][0]["indices"]), set(desc["cfg"][1]["indices"])
            assert i0 and i1 and not (i0 & i1)
            assert len({t["gain"][0] for t in desc["cfg"]}) == len(desc["cfg"])
            assert desc["cfg"][0]["lower"] != desc["cfg"][1]["lower"] and desc["cfg"][0]["upper"] != desc["cfg"][1]["upper"]
        if len(desc["vel"]) >= 2:
            idx, lim = desc["vel"][1]["indices"], desc["vel"][1]["limit"]
            twice = [k for k in range(len(idx)) if idx[k] == idx[-1]]
            assert len(twice) == 4 and min(lim[k] for k in twice) == lim[twice[2]] < lim[twice[3]]
            assert not (set(desc["vel"][0]["indices"]) & set(idx))
        if len(desc["col"]) == 2:
            p0 = {tuple(desc["col"][0]["pairs"][i:i + 2]) for i in range(0, len(desc["col"][0]["pairs"]), 2)}
            p1 = {tuple(desc["col"][1]["pairs"][i:i + 2]) for i in range(0, len(desc["col"][1]["pairs"]), 2)}
            assert len(p0 & p1) == 1 and p0 - p1 and p1 - p0
            assert all(a != b for a, b in zip(desc["col"][0]["par"], desc["col"][1]["par"])) and desc["col"][1]["par"][3] == 1e-3


def test_limit_list_tables(plans):
    """Every entry of every planned copy, recomputed from the descriptor: the lane tables of the wavefront kernels (stride 64; a
    model beyond one wavefront keeps the defaults), LaneProblem2 and its narrowed LaneProblem ([term][MD], every term and dof
    beyond the problem's at -inf / +inf / +inf, posture costs 0), the wide arrays (stride nv) and the four parameters of
    every pair in list order."""
    for c in list_cases(plans):
        key, nv, T, desc = (c["model"], c["case"]), c["nv"], c["tables"], c["desc"]
        nc, nl, npost = len(desc["cfg"]), len(desc["vel"]), len(desc["post"])
        gains = [t["gain"][0] for t in desc["cfg"]]
        assert (T["n_cfg"], T["n_vel"]) == (nc, nl), key
        same(T["cfg_gain"][:nc], gains, key, "cfg_gain")
        pcost, clo, chi, vlim = box_tables(c, 64, filled=not c["big"])
        for name, want in (("pcost", pcost), ("clo", clo), ("chi", chi), ("vlim", vlim)):
            same(T[name], want, key, name)
        for lane in ("lane2", "lane1"):
            if lane not in T:
                continue
            L = T[lane]
            md = L["md"]
            assert md == (32 if lane == "lane2" else 16) and nv <= md
            assert (L["n_posture"], L["n_cfg"], L["n_vel"]) == (npost, nc, nl), key
            pc, lo, hi, vl = box_tables(c, md)
            wlo, whi, wvl = np.full((KMAX_BOX, md), -INF), np.full((KMAX_BOX, md), INF), np.full((KMAX_BOX, md), INF)
            wpc = np.zeros((KMAX_POSTURE, md))
            wlo[:nc], whi[:nc], wvl[:nl], wpc[:npost] = lo[:nc], hi[:nc], vl[:nl], pc[:npost]
            wpc[:, :nv] *= 1 - np.asarray(c["dof_free"])             # (free-joint dofs: no posture error)
            same(L["cfg_lower"], wlo, key, lane + ".cfg_lower")
            same(L["cfg_upper"], whi, key, lane + ".cfg_upper")
            same(L["vel_limit"], wvl, key, lane + ".vel_limit")
            same(L["posture_cost"], wpc, key, lane + ".posture_cost")
            same(L["cfg_gain"], gains + [0.0] * (KMAX_BOX - nc), key, lane + ".cfg_gain")
            same(L["posture_gain"][:npost], [t["gain_lm"][0] for t in desc["post"]], key, lane + ".posture_gain")
            same(L["posture_lm"][:npost], [t["gain_lm"][1] for t in desc["post"]], key, lane + ".posture_lm")
        if "wide" in T:
            W = T["wide"]
            assert (W["n_posture"], W["n_cfg"], W["n_vel"]) == (npost, nc, nl), key
            same(W["cfg_gain"][:nc], gains, key, "wide.cfg_gain")
            pc, lo, hi, vl = box_tables(c, nv)
            for name, want in (("pcost", pc), ("clo", lo), ("chi", hi), ("vlim", vl)):
                same(W[name], want, key, "wide." + name)
        want = [x for t in desc["col"] for _ in range(len(t["pairs"]) // 2) for x in t["par"]]
        same(T["pair_par"], want, key, "pair_par")
        assert len(T["pair_par"]) == 4 * c["n_pairs_in"]


def test_dof_outside_a_term_is_unbounded(plans):
    """Read off the printed tables themselves, on the case whose terms 0 and 1 are disjoint: a dof of term 1 reads
    -inf / +inf in term 0 and finite bounds in term 1, on every copy."""
    for m in LIST_MODELS:
        c = plans[(m, "lim_c4_v4_col2" if m != "chain68" else "lim_c4_v4")]
        nv, T, desc = c["nv"], c["tables"], c["desc"]
        only1 = sorted(set(desc["cfg"][1]["indices"]) - set(desc["cfg"][0]["indices"]))
        v_only1 = sorted(set(desc["vel"][1]["indices"]) - set(desc["vel"][0]["indices"]))
        assert len(only1) >= 2 and len(v_only1) >= 2
        copies = [(T["wide"], nv)] + ([(T, 64)] if not c["big"] else [])
        c2 = plans[(m, "lim_c4_v4")]["tables"]
        copies += [(c2[k], c2[k]["md"]) for k in ("lane2", "lane1") if k in c2]
        for tab, stride in copies:
            lo, hi = tab.get("clo", tab.get("cfg_lower")), tab.get("chi", tab.get("cfg_upper"))
            vl = tab.get("vlim", tab.get("vel_limit"))
            for dof in only1:
                assert lo[dof] == -INF and hi[dof] == INF and np.isfinite([lo[stride + dof], hi[stride + dof]]).all(), (m, dof)
            for dof in v_only1:
                assert vl[dof] == INF and np.isfinite(vl[stride + dof]), (m, dof)


def test_refused_descriptors(plans):
    """Code and text of mkh_last_error, as before the split."""
    for (m, case), c in plans.items():
        nv, nb = c["nv"], c["nbody"]
        if case == "bad_dof_range":
            assert (c["rc"], c["err"]) == (-1, "configuration limit: dof %d out of range" % nv)
        elif case == "bad_cost":
            assert (c["rc"], c["err"]) == (-1, "frame task 0: cost must be >= 0")
        elif case == "bad_frame_id":
            assert (c["rc"], c["err"]) == (-1, "frame task 0: body id %d out of range" % nb)
        elif case in ("bad_cfg5", "bad_vel5"):
            # MKH_E_LIMIT, and the text names the cap (kMaxBoxTerms)
            assert (c["rc"], c["err"]) == (-4, "at most 4 configuration and 4 velocity limits")
        elif case == "bad_ball_slots":
            # (the kernels rebuild a ball joint's bound from one value per dof: a quaternion of its own in the four slots is refused)
            assert (c["rc"], c["err"]) == (-1, "configuration limit 0: lower / upper differ over the four qpos slots of the ball joint of dof 5 "
                                               "(one value per ball joint, as the reference's constructor writes its range)")
        elif case == "bad_free_limit":
            assert (c["rc"], c["err"]) == (-1, "configuration limit on free-joint dof 0 (the reference skips free joints)")
        elif m == "chain_last+1":
            # MKH_E_LIMIT, and the text carries the LDS figure (test_wide_models_plan_their_branch)
            assert c["rc"] == -4 and c["err"].startswith("model too large for the workgroup-per-problem kernel: "), c["err"]
        else:
            assert c["rc"] == 0, (m, case, c["err"])
    assert ("tree44", "bad_free_limit") in plans and ("tree62", "bad_free_limit") in plans and ("ball11", "bad_ball_slots") in plans


# ---- the large models of tests/wide_cases.py on the workgroup-per-problem kernel

KWIDE_THREADS, KWIDE_MAX_ROWS = 256, 448           # wide_types.h kWideThreads, kWideMaxRows
LDS_CAP, TWO_WG = (160 * 1024 - 2048) // 8, 80 * 1024 // 8     # doubles one workgroup may take / that leave room for a second one


def wide_layout(nq, nbody, njnt, nv, n_frame, n_com, n_jrows, n_pairs):
    """LDS of one problem in doubles, as DESIGN.md §8 describes it (no general convex pairs, no caller-defined rows): the
    per-problem state, the staging vectors of the block pivots, the dense fallback's factors, the tableau.
    → dict(blk, tableau_in_lds, t_lds_doubles, lds_doubles); lds_doubles > LDS_CAP: refused."""
    ev = lambda x: x + (x & 1)
    ncap = nv + min(n_pairs, KWIDE_MAX_ROWS)
    poses = ev(7 * nbody) + ev(6 * max(njnt, 1))               # body poses + joint axes / anchors: free again once the dofs have theirs
    state = ev(nq) + poses + 10 * nv + 64 * max(n_frame, 1) + (4 * nbody if n_com else 0) + ev(max(n_jrows, 1))
    state += 4 * ev(nv) + 5 * ev(ncap)                         # c, posture diagonal, lo, hi | z, w, row norms, reference, column
    state += KWIDE_THREADS + KWIDE_THREADS // 2 + ev((ncap + 1) // 2)
    t = ncap * ncap
    stage = 8 * ev(ncap)
    total = lambda o: o + (t if o + t <= LDS_CAP else 0)
    if stage <= poses:
        blk = "overlay"
    elif (state + stage <= LDS_CAP and (state + stage + t <= LDS_CAP) == (state + t <= LDS_CAP)
          and (total(state + stage) <= TWO_WG) == (total(state) <= TWO_WG)):
        blk = "appended"
        state += stage
    else:
        blk = "absent"
    in_lds = state + t <= LDS_CAP
    if n_pairs:
        gi = 2 * nv * (nv | 1) + 4 * (nv + 2)
        if state + gi + (nv + 8) ** 2 <= TWO_WG:
            state += gi
    if in_lds:
        t_lds = t
    else:
        room = TWO_WG - state
        if room < (nv + 8) ** 2:
            room = LDS_CAP - state
        t_lds = max(room, 0)
    return {"blk": blk, "tableau_in_lds": int(in_lds), "t_lds_doubles": t_lds, "lds_doubles": state + t_lds}


def _wide_counts(c):
    return dict(nq=c["nq"], nbody=c["nbody"], njnt=c["njnt"], nv=c["nv"], n_frame=len(c["tasks"]), n_com=c["n_com"],
                n_jrows=sum(len(r) for r in task_rows(c)) + c["com_rows"], n_pairs=c["n_pairs_in"])


def test_wide_layout_recomputed(plans):
    """chain_words, the LDS total and the three layout decisions of EVERY planned model beyond one wavefront (the fixed set's
    chain68 among them), recomputed from the model's counts."""
    seen = 0
    for c in ok_cases(plans, wavefront=False):
        if not c["big"] or c["dense"] or c["cylbox"]:
            continue
        w, want = c["wide"], wide_layout(**_wide_counts(c))
        key = (c["model"], c["case"])
        assert w["chain_words"] == -(-c["nv"] // 64), key
        assert {k: w[k] for k in want} == want, (key, want, {k: w[k] for k in want})
        assert want["lds_doubles"] <= LDS_CAP and c["sel"]["wide_lds"] == 8 * want["lds_doubles"], key
        seen += 1
    assert seen >= 20 + len(wc.HOST_MODELS) - 1             # (chain68: every case without plugin rows or convex pairs)


def test_wide_chain_bit_table(plans):
    """The chain bit table of the large models — word k >> 6, bit k & 63 of body b: dof k moves b — from the parent arrays."""
    for name in wc.HOST_MODELS:
        c = plans[(name, "wide")]
        nw = c["model_chain_words"]
        assert nw == -(-c["nv"] // 64) and len(c["chain"]) == c["nbody"] * nw, name
        for b in range(c["nbody"]):
            mask = sum(1 << k for k in chain_of(c, b))
            assert [int(x) for x in c["chain"][b * nw:(b + 1) * nw]] == [(mask >> (64 * i)) & (2 ** 64 - 1) for i in range(nw)], (name, b)
    # the models are the device tests': parent arrays and dof counts of the MJCF text itself
    for name in wc.HOST_MODELS:
        m, c = wc.model(name), plans[(name, "wide")]
        assert (m.nq, m.nv, m.nbody, m.njnt) == (c["nq"], c["nv"], c["nbody"], c["njnt"]), name
        assert [int(x) for x in m.body_parentid] == c["body_parentid"] and [int(x) for x in m.body_dofnum] == c["body_dofnum"], name
        assert len(c["tasks"]) == len(wc.mjcf_text(name)[1]) <= 16, name


def test_wide_models_plan_their_branch(plans):
    """Each model of tests/wide_cases.py plans the branch it was chosen for (the sizes were found by sweeping this program)."""
    W = {name: plans[(name, "wide")] for name in wc.HOST_MODELS}
    for name, c in W.items():
        if name != "chain_last+1":
            w = c["wide"]
            print("%-10s nv %3d nbody %3d: tableau_in_lds %d, chain_words %d, staging %-8s, %6d doubles of LDS (tableau %5d), "
                  "ws_stride %d, use_cull %d" % (name, c["nv"], c["nbody"], w["tableau_in_lds"], w["chain_words"], w["blk"], w["lds_doubles"],
                                                 w["t_lds_doubles"], w["ws_stride"], w["use_cull"]))
            assert c["rc"] == 0 and c["big"] and c["sel"]["wide_only"] == 1, name
    wide = lambda name: W[name]["wide"]
    # the tableau's place: 123 dofs is the last chain with it in LDS
    assert wide("chain123")["tableau_in_lds"] == 1 and wide("chain123")["t_lds_doubles"] == 123 * 123
    for name in ("chain124", "chain130", "chain300", "chain_last"):
        assert wide(name)["tableau_in_lds"] == 0 and wide(name)["t_lds_doubles"] < W[name]["nv"] ** 2, name
        assert wide(name)["ws_stride"] >= W[name]["nv"] ** 2, name           # (the slice of device memory holds it)
    assert (wide("chain124")["chain_words"], wide("chain130")["chain_words"], wide("chain300")["chain_words"]) == (2, 3, 5)
    assert wide("chain_last")["chain_words"] == 9 and W["chain300"]["nv"] > KWIDE_THREADS and W["chain_last"]["nv"] > 2 * KWIDE_THREADS
    # the largest chain and the first that is refused: code, and the LDS figure in the text
    assert W["chain_last"]["nv"] + 1 == W["chain_last+1"]["nv"] and wide("chain_last")["lds_doubles"] == LDS_CAP
    bad = W["chain_last+1"]
    need = wide_layout(**_wide_counts(bad))["lds_doubles"]
    assert need > LDS_CAP and bad["rc"] == -4
    assert bad["err"].startswith("model too large for the workgroup-per-problem kernel: %d KB of LDS per problem, 158 KB available" % (need // 128))
    # staging of the block pivots: over the poses on serial hinge chains, appended / absent / appended on the ball chains
    assert {wide(n)["blk"] for n in ("chain123", "chain124", "chain130", "chain300", "chain_last", "fixed30")} == {"overlay"}
    assert (wide("ball80")["blk"], wide("ball86")["blk"], wide("ball92")["blk"]) == ("appended", "absent", "appended")
    assert wide("ball86")["o_blk"] < 0 and wide("ball80")["o_blk"] > wide("ball80")["o_X"]
    assert all(wide(n)["tableau_in_lds"] == 1 for n in ("ball80", "ball86", "ball92", "fixed30"))
    # the wide route by body count alone
    assert (W["fixed30"]["nv"], W["fixed30"]["nbody"]) == (30, 91)
    # collision pairs on a wide-only model: more than a wavefront of them, culled by bounding spheres
    assert 70 <= W["hinge80"]["n_pairs_in"] <= 100 and wide("hinge80")["n_pairs"] == len(wc.HINGE80_PAIRS) > 64
    assert wide("hinge80")["use_cull"] == 1 and wide("hinge80")["max_rows"] == len(wc.HINGE80_PAIRS)
    assert all(wide(n)["use_cull"] == 0 for n in W if n not in ("hinge80", "chain_last+1"))
