"""Build libminkhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).

    python -m mink_amd.csrc.build            # or: python mink_amd/csrc/build.py [--force]

Each kernel variant of VARIANTS below is compiled in its own generated translation unit
(_build/variant_<name>.hip) so that the variants build in parallel, and _build/dispatch.hip holds the
table of them that the host side of the C ABI (minkhip.hip) queries and launches through (variants.h).  The shared library is written next to the Python package
(mink_amd/libminkhip.so) so that it travels with the repo snapshot; it is git-ignored (*.so).
"""

import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
# Same-box A/B of compiler flags: MKH_BUILD_TAG=x builds _build_x/ → libminkhip_x.so next to the default library
# (mink_amd/_native.py loads it when MKH_LIB_TAG=x); unset = the product build.
_TAG = os.environ.get("MKH_BUILD_TAG", "")
LIB = os.path.join(PKG, f"libminkhip_{_TAG}.so" if _TAG else "libminkhip.so")
RESOURCES = os.path.join(PKG, f"kernel_resources_{_TAG}.json" if _TAG else "kernel_resources.json")   # written next to the library at build time (_write_resources)
BUILD = os.path.join(HERE, f"_build_{_TAG}" if _TAG else "_build")
def _sources() -> list:
    """Every file the library is built from: whatever sits in csrc/ (kernel headers, generators, host code) plus the
    public header — derived from the directory, not listed by hand (a hand-kept list once missed convex_dev.h)."""
    fs = [os.path.join(HERE, f) for f in sorted(os.listdir(HERE))
          if f.endswith((".h", ".hip", ".py", ".inc")) and f not in ("tab_asm.inc", "__init__.py")]
    return fs + [os.path.join(HERE, "..", "..", "include", "minkhip.h")]


NTS = (8, 16, 24, 32, 44, 48, 64)          # tableau rows per lane
FEATS = (0, 16, 6, 8, 72, 88, 136, 30, 31, 256)      # lean, + fused step loop, RelativeFrameTask/ComTask, collision rows only, collision rows with plane / sphere / capsule pairs only, the same + fused step loop, collision rows with general convex pairs (GJK), every feature but taps, everything, dense (plugin) rows only (ik_kernel.h F_*)
# low-rank ("Woodbury") start: (NT, NR) = (tableau rows ≥ nv + task rows, dof rows ≥ nv); F_WOOD = 32
WOOD = ((16, 16), (24, 24), (32, 32), (44, 44), (48, 48))   # (NT, NR): the task residuals are eliminated outside the tableau (ik_kernel.h wood_start), NT = NR ≥ nv
# 3-waves-per-SIMD register map (TabW3 in tab_asm.inc, 168 VGPRs, compact LDS layout): (NT, FEAT) without collision rows
W3 = ((44, 0),)                        # (44_6 and 44_16 still spill 34–76 VGPRs at 74 registers: scratch traffic makes them slower than their 2-waves builds)
W3_WOOD = ((44, 44, 32), (44, 44, 48), (32, 32, 32), (32, 32, 48),    # (NT, NR, FEAT) of the low-rank start with the 3-waves map
           (24, 24, 32), (24, 24, 48), (16, 16, 32), (16, 16, 48),    # ... and, for NT ≤ 24, the 4-waves map (TabW4; same suffix _w3: "one more wave")
           (44, 44, 36), (44, 44, 52))                                # F_COM (ComTask rows / up to 24 task rows) and its fused loops: round 5, ik_kernel.h MKH_WOOD_SPLIT
# one problem per workgroup (round 6; ik_kernel.h MKH_ONE_SHOT): a twin of the humanoid-size one-more-wave build WITHOUT the persistent
# loop's machinery (ticket draws, double-buffered inputs, loop-carried scalars) — launched when the grid is the batch (solve_host.hip plan_launch()).
# Measured: `44_32_r44_w3o` 0.713 -> 0.703 ms on the headline; the F_COM twin `44_36_r44_w3o` (12 spilled VGPRs) 0.350 -> 0.352 ms at
# 16 384 instances of the G1 full example — not built.
# ... and its twin on FOUR waves per SIMD, `44_32_r44_w4o` (a fourth entry "w4"; ik_kernel.h MKH_W4P, tab_asm.inc TabW4<44>: the product form
# alone below 128 VGPRs, history slots of one double, everything in LDS that is dead after the pair lanes in one union) — the headline's
# build from the batch size at which it measures faster (solve_host.hip plan_launch()).
W3_WOOD_ONE_SHOT = ((44, 44, 32), (44, 44, 32, "w4"))
WOOD_FEATS = (32, 48, 33, 36, 52)      # F_WOOD, | F_STEPS, | F_TAPS (cycle-counter profiling only), | F_COM, | F_COM | F_STEPS
# low-rank start WITH half-space rows (round 6; ik_kernel.h wood_start "half-space rows"): (NT, NR, FEAT) on the 2-waves map,
# NR = NT (the rows' columns of the elimination sit behind the dofs in the tableau-wide rows of Jh).
# 40 = F_WOOD | F_COLL (analytic pairs, phases as calls)
WOOD_ROWS = ((48, 48, 40),)


class Variant(NamedTuple):
    """One compiled ik_solve_kernel build.  Its name — "44_32_r44_w3o" — names the translation unit (variant_<name>.hip), the
    launcher (launch_<name>) and the kernel (ik_solve_kernel_<name>)."""
    nt: int
    feat: int
    nr: int = 0
    w3: bool = False
    one_shot: bool = False
    w4 = False                 # (class attribute, not a field: VariantW4 below)

    @property
    def name(self) -> str:
        return f"{self.nt}_{self.feat}" + (f"_r{self.nr}" if self.nr else "") + (("_w4" if self.w4 else "_w3") if self.w3 else "") + ("o" if self.one_shot else "")

    def translation_unit(self) -> str:
        defs = [f"MKH_NT {self.nt}"] + ([f"MKH_NR {self.nr}"] if self.nr else []) + [f"MKH_FEAT {self.feat}"]
        if self.w3:
            defs.append("MKH_W3 1")
            if self.w4:
                defs.append("MKH_W4P 1")           # (the four-waves product-form map of the humanoid-size twin)
            elif self.nr and self.nt <= 24 and not self.one_shot:
                defs.append("MKH_W4 1")            # (the 4-waves map of the small low-rank builds, W3_WOOD)
        if self.one_shot:
            defs.append("MKH_ONE_SHOT 1")
        if self.name != f"{self.nt}_{self.feat}":  # (ik_kernel.h composes the plain builds' kernel name itself)
            defs.append(f"MKH_KERNEL_NAME ik_solve_kernel_{self.name}")
        return "// generated by build.py\n" + "".join(f"#define {d}\n" for d in defs) + f"""#include "../ik_kernel.h"
namespace mkh {{
void launch_{self.name}(int grid, int lds_bytes, hipStream_t stream, const DeviceProblem* P, const SolveArgs& a,
                      const TapArgs* taps) {{
  hipLaunchKernelGGL(ik_solve_kernel_{self.name}, dim3(grid), dim3(kWave), lds_bytes, stream, P, a, taps);
}}
}}  // namespace mkh
"""


class VariantW4(Variant):
    """The twin of a one-more-wave build on the four-waves product-form map: the same five fields — the host's table tells the two
    apart by the kernel's name, `_w4` for `_w3`."""
    __slots__ = ()
    w4 = True


# every compiled build, once: the translation units, the host's table (_build/dispatch.hip → variants.h) and
# kernel_resources.json all follow from this list
VARIANTS = tuple([Variant(nt, ft) for nt in NTS for ft in FEATS]
                 + [Variant(nt, ft, nr) for nt, nr in WOOD for ft in WOOD_FEATS]
                 + [Variant(nt, ft, nr) for nt, nr, ft in WOOD_ROWS]
                 + [Variant(nt, ft, w3=True) for nt, ft in W3]
                 + [Variant(nt, ft, nr, w3=True) for nt, nr, ft in W3_WOOD]
                 + [(VariantW4 if e[3:] == ("w4",) else Variant)(e[0], e[2], e[1], w3=True, one_shot=True) for e in W3_WOOD_ONE_SHOT])
# the hand-written translation units behind the generated ones, in link order: (name, what it holds)
HAND_WRITTEN = (
    ("minkhip", "host side of the C ABI: handles, problem upload, the outer-loop entry points"),
    ("solve_host", "host side of the plain solve: launch planning, launching, the routes of a call's arrays, its five entry points (host code only)"),
    ("checker_host", "host side of the collision checker: its entry points and the stages of the checked calls (host code only)"),
    ("problem_plan", "host-only planning of models and problems (no HIP runtime call)"),
    ("lane_variants", "the lane-per-problem and row-per-problem kernels of small arms"),
    ("wide_variants", "the workgroup-per-problem kernel"),
    ("convex_pre", "convex_contacts_kernel: general convex pairs in front of a plain solve or a clearance"),
    ("multistart", "seeding / fan-out / selection of mkh_solve_multistart"),
    ("solution_set", "distinct-set selection of mkh_solve_multistart_set / mkh_select_distinct (same flags as multistart.hip: d_ref is bitwise multi-start's)"),
    ("goalset", "two-level selection of mkh_solve_goalset / mkh_select_goalset (same flags as multistart.hip: d_ref is bitwise multi-start's)"),
    ("seed_table", "key layout / K-nearest query of mkh_seed_table_*"),
    ("trajectory", "layout transposes / waypoint velocity of mkh_solve_trajectory"),
    ("keyframes", "target blends between keyframes of mkh_solve_keyframes"),
    ("trajectory_multistart", "path scoring / selection / gather of mkh_solve_trajectory_multistart"),
    ("ladder", "dynamic program / back-trace / gather of mkh_ladder_select and mkh_solve_trajectory_ladder"),
    ("ladder_refine", "step / guard kernels of mkh_ladder_refine"),
    ("unwind", "turn unwinding of mkh_unwind_turns / MKH_FLAG_UNWIND_TURNS"),
    ("ladder_nodes", "node flags of mkh_solve_trajectory_ladder_nodes"),
    ("clearance", "clearance of a batch of rows: mkh_clearance, the collision check behind the multi-start loops"),
    ("ladder_refine_free", "lr_check_kernel: the collision check between the loops of mkh_ladder_refine_free"),
    ("sweep", "swept clearance of edges: mkh_swept_clearance, the edge mask of the checked ladder calls"),
    ("certified_sweep", "certified sweep of edges: mkh_certified_sweep — motion-bounded sample counts and the bound between samples (sweep.hip's flags)"),
    ("convex_sweep", "convex_sweep_kernel: the general convex pairs of a sweep's samples, in front of sweep_kernel (convex_pre.hip's flags)"),
    ("convex_check", "convex_check_kernel: the general convex pairs of the rows tmf_check_cv_kernel / lr_check_cv_kernel judge inside their launch (convex_sweep.hip's flags)"),
    ("trajectory_free", "tmf_check_kernel: nodes and edges of mkh_solve_trajectory_multistart_free / mkh_select_trajectory_candidates (sweep.hip's flags)"),
)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-null-conversion"]
# experiments: extra compiler flags for every translation unit (e.g. MKH_EXTRA_FLAGS="-DMKH_FORCE_COLL_CALL"); part of the
# per-object command tag, so changing it recompiles
FLAGS += os.environ.get("MKH_EXTRA_FLAGS", "").split()
# Kernel TUs only: MachineLICM hoists every constant materialisation (v_mov of fp64 polynomial
# coefficients) and lane-address computation out of the per-problem loop, where it then lives across
# the whole QP and gets SPILLED (G1 lean variant: 31 VGPR + 31 SGPR spills, 128 B scratch per lane whose
# write-back was 30 % of the kernel's HBM writes).  Without the pass the same kernel has no spills.
KERNEL_FLAGS = ["-mllvm", "-disable-machine-licm",
                # the pinned tableau / staging registers sit above the amdgpu_num_vgpr cap on purpose: clang reports
                # every asm clobber of them as "reserved" (≈2 000 warnings per build; tools/check_vgpr_cap.py is the check)
                "-Wno-inline-asm"]


def _hipcc() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _stale() -> bool:
    if not os.path.exists(LIB) or not os.path.exists(RESOURCES) or not os.path.exists(BUILD_INFO):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > t for p in _sources()) \
        or not os.path.exists(os.path.join(HERE, "tab_asm.inc"))      # (generated by gen_tab_asm.py, untracked)


def _deps(depfile: str) -> list:
    """Prerequisites from a compiler-written Makefile fragment (-MD -MF)."""
    txt = open(depfile).read().replace("\\\n", " ")
    return [d for d in txt.split(":", 1)[1].split() if d]


def _obj_stale(src: str, obj: str, cmd_tag: str) -> bool:
    """A translation unit is recompiled when its object is missing, was built with other flags, or is older than the
    source or any header the compiler reported for it (so an incremental rebuild compiles only what an edit touches)."""
    dep, tag = obj + ".d", obj + ".cmd"
    if not (os.path.exists(obj) and os.path.exists(dep) and os.path.exists(tag)) or open(tag).read() != cmd_tag:
        return True
    t = os.path.getmtime(obj)
    try:
        return any(os.path.getmtime(d) > t for d in [src] + _deps(dep))
    except OSError:
        return True


def _parse_resource_remarks(stderr: str) -> dict:
    """{function: {vgprs, sgpr_spills, vgpr_spills, scratch_bytes_per_lane, occupancy_waves_per_simd}} from the compiler's
    -Rpass-analysis=kernel-resource-usage remarks of one translation unit (kernels and their real callees)."""
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
            "LDS Size [bytes/block]": "lds_bytes_per_block"}       # (static LDS: a launch's dynamic bytes are the launcher's)
    for m in re.finditer(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass-analysis", stderr):
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None and k in keys:
            cur[keys[k]] = int(v)
    return out


def _short_name(mangled: str) -> str:
    m = re.match(r"_ZN(?:3mkh|12_GLOBAL__N_1)(\d+)", mangled)
    if not m:
        return mangled
    n, a = int(m.group(1)), m.end()
    name, rest = mangled[a:a + n], mangled[a + n:]
    if rest.startswith("I"):                      # template arguments: integer / bool literals (lane kernels)
        args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        if args:
            name += "<" + ",".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">"
    return name


def _sha256(path: str) -> str:
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def _device_code_sha256(obj: str) -> str:
    """SHA-256 of the DEVICE code of a translation unit: the .text and .rodata (kernel descriptors) sections of the gfx950 code
    object inside the host object's fat binary.  The host object itself carries the build directory (the module id of the fat
    binary wrapper is derived from the source path), so its hash changed with the directory the library was built in and every
    committed profile looked stale after a rebuild elsewhere (round-4 review); the device code does not."""
    import hashlib
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    try:
        with tempfile.TemporaryDirectory() as d:
            fat, co = os.path.join(d, "x.fatbin"), os.path.join(d, "x.co")
            subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "x.o")], check=True, capture_output=True)
            subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={fat}", f"--output={co}"], check=True, capture_output=True)
            h = hashlib.sha256()
            for sec in (".text", ".rodata"):
                out = os.path.join(d, "sec.bin")
                subprocess.run([f"{llvm}/llvm-objcopy", "-O", "binary", f"--only-section={sec}", co, out], check=True, capture_output=True)
                with open(out, "rb") as fh:
                    h.update(fh.read())
            return h.hexdigest()
    except (OSError, subprocess.CalledProcessError):
        return _sha256(obj)                # (no LLVM tools: fall back to the object file)


def _git_state() -> dict:
    """HEAD and whether the sources under it were modified when the library was linked (the GPU box has no .git)."""
    root = os.path.dirname(PKG)
    try:
        head = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", root, "status", "--porcelain", "--", "mink_amd", "include"], capture_output=True,
                               text=True, check=True).stdout.strip() != ""
        return {"git_head": head, "git_dirty_sources": dirty}
    except (OSError, subprocess.CalledProcessError):
        return {"git_head": None, "git_dirty_sources": None}


BUILD_INFO = os.path.join(PKG, f"build_info_{_TAG}.json" if _TAG else "build_info.json")


def _write_resources(objs: list) -> None:
    """mink_amd/kernel_resources.json: registers, spills and scratch of every kernel in the library, from the compiler's
    own remarks at build time (bench.py reports `vgpr_spills` of the kernel it ran from here; tests/test_abi.py reads it)."""
    table = {}
    for o in objs:
        path = o + ".res.json"
        if not os.path.exists(path):
            continue
        fns = json.load(open(path))
        kernels = {f: r for f, r in fns.items() if "ik_solve_kernel" in f or "ik_lane_kernel" in f or "_kernel" in _short_name(f)}
        callees = {f: r for f, r in fns.items() if f not in kernels}
        code = _device_code_sha256(o)      # the translation unit's DEVICE code: what the kernel's counters are a property of
        for f, r in kernels.items():
            e = dict(r)
            e["code_sha256"] = code
            # real callees of the 3-waves builds (pre_phases, wood_start, ...) run inside the kernel: their spills count
            e["callees"] = {_short_name(c): cr for c, cr in callees.items()}
            e["vgpr_spills_with_callees"] = r.get("vgpr_spills", 0) + sum(cr.get("vgpr_spills", 0) for cr in callees.values())
            e["sgpr_spills_with_callees"] = r.get("sgpr_spills", 0) + sum(cr.get("sgpr_spills", 0) for cr in callees.values())
            table[_short_name(f)] = e
    with open(RESOURCES, "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
    # provenance of the library itself (tools/rocprof_summary.py stamps profiles with it, bench.py compares)
    info = {"library": os.path.basename(LIB), "library_sha256": _sha256(LIB)}
    info.update(_git_state())
    with open(BUILD_INFO, "w") as fh:
        json.dump(info, fh, indent=1, sort_keys=True)


def _write_if_changed(path: str, text: str) -> None:
    if os.path.exists(path) and open(path).read() == text:
        return
    with open(path, "w") as fh:
        fh.write(text)


def variant_table_source(launchers: bool = True) -> str:
    """The translation unit that defines the table of variants.h, one row per entry of VARIANTS.  `launchers` = False: null launch
    pointers — the table of a host-only program that plans problems and never launches (tests/test_problem_plan_cpu.py)."""
    decls = "\n".join(f"void launch_{v.name}(int, int, hipStream_t, const DeviceProblem*, const SolveArgs&, const TapArgs*);"
                      for v in VARIANTS) if launchers else ""
    rows = "\n".join(f'    {{{v.nt}, {v.nr}, {v.feat}, {str(v.w3).lower()}, {str(v.one_shot).lower()}, "ik_solve_kernel_{v.name}", '
                     + (f"&launch_{v.name}" if launchers else "nullptr") + "}," for v in VARIANTS)
    return f"""// generated by build.py: the table of compiled kernel variants (variants.h)
#include <hip/hip_runtime.h>
#include "../variants.h"
namespace mkh {{
{decls}
const VariantRow* variant_table() {{
  static const VariantRow table[] = {{
{rows}
  }};
  return table;
}}
const int kNumVariants = {len(VARIANTS)};
}}  // namespace mkh
"""


def _generate() -> list:
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run([sys.executable, os.path.join(HERE, "gen_tab_asm.py")], check=True)
    srcs = []
    for v in VARIANTS:
        _write_if_changed(os.path.join(BUILD, f"variant_{v.name}.hip"), v.translation_unit())
        srcs.append(f"variant_{v.name}")
    _write_if_changed(os.path.join(BUILD, "dispatch.hip"), variant_table_source())
    srcs.append("dispatch")
    # translation units of variants that are no longer built (tools/check_vgpr_cap.py walks the directory)
    for f in os.listdir(BUILD):
        if f.startswith("variant_") and f.endswith((".hip", ".o")) and f.rsplit(".", 1)[0] not in srcs:
            os.remove(os.path.join(BUILD, f))
    return srcs


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not _stale():
        return LIB
    hipcc = _hipcc()
    srcs = _generate()
    jobs = [(os.path.join(BUILD, s + ".hip"), os.path.join(BUILD, s + ".o")) for s in srcs]
    jobs += [(os.path.join(HERE, name + ".hip"), os.path.join(BUILD, name + ".o")) for name, _ in HAND_WRITTEN]

    def compile_one(job):
        src, obj = job
        extra = KERNEL_FLAGS if os.path.basename(src).startswith("variant_") else []
        cmd = [hipcc] + FLAGS + extra
        tag = " ".join(cmd)
        if not force and not _obj_stale(src, obj, tag):
            return obj, False
        r = subprocess.run(cmd + ["-MD", "-MF", obj + ".d", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj],
                           stdout=subprocess.DEVNULL if not verbose else None, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise subprocess.CalledProcessError(r.returncode, cmd)
        with open(obj + ".res.json", "w") as fh:
            json.dump(_parse_resource_remarks(r.stderr), fh)
        with open(obj + ".cmd", "w") as fh:
            fh.write(tag)
        return obj, True

    if verbose:
        print(f"[mink_amd] {len(jobs)} translation units for gfx950 (recompiling what changed) ...", flush=True)
    # (MAX_JOBS, when set: what a shared machine allows this build — os.cpu_count() is the whole machine)
    workers = os.cpu_count() or 4
    if os.environ.get("MAX_JOBS", "").isdigit() and int(os.environ["MAX_JOBS"]) > 0:
        workers = min(workers, int(os.environ["MAX_JOBS"]))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as ex:
        res = list(ex.map(compile_one, jobs))
    objs = [o for o, _ in res]
    if verbose:
        print(f"[mink_amd] compiled {sum(1 for _, c in res if c)} of {len(jobs)}", flush=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs, check=True)
    _write_resources(objs)
    if verbose:
        print(f"[mink_amd] linked {LIB}", flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
