"""Static ratchet on the headline kernel's code (`ik_solve_kernel_44_32_r44_w3o`, its callees `pre_phases` and `wood_start`):
the translation unit is compiled to gfx950 assembly with build.py's flags and must keep

  (a) zero spilled VGPRs and no more scratch than the parent of the instruction-diet change had (8 B per lane), for every
      function the compiler reports (its own kernel-resource-usage remarks, parsed as build.py parses them),
  (b) fewer static VALU instructions in the three functions together than that parent: 4 514 then (pre_phases 1 736 +
      wood_start 1 109 + kernel body 1 669, counted by `count_valu` below on the parent's assembly), 4 248 with the change
      (1 736 + 985 + 1 527),
  (c) every compiler-allocated VGPR of the kernel body below the pinned tableau range (tools/check_vgpr_cap.py's check).

A ratchet against drifting back, not a proof of speed: that is the same-box A/B recorded in docs/HISTORY.md."""

import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")
sys.path.insert(0, CSRC)
sys.path.insert(0, os.path.join(REPO, "tools"))

PARENT_STATIC_VALU = 4514
PARENT_SCRATCH_BYTES = 8
FUNCTIONS = ("pre_phases", "wood_start", "ik_solve_kernel_44_32_r44_w3o")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def count_valu(asm: str) -> dict:
    """{function symbol: static VALU instructions} of an assembly listing (inline-asm bodies included)."""
    func, table = None, {}
    for line in asm.split("\n"):
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not line.startswith(".L"):
            func = m.group(1)
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":") or func is None:
            continue
        if code.split()[0].startswith("v_"):
            table[func] = table.get(func, 0) + 1
    return table


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    import build as hipbuild
    import gen_tab_asm
    gen_tab_asm.main()                    # (tab_asm.inc is generated, as in build())
    nt, nr, ft = hipbuild.W3_WOOD_ONE_SHOT[0]
    src = tmp_path_factory.mktemp("isa") / "twin.hip"
    src.write_text(f"""#define MKH_NT {nt}
#define MKH_NR {nr}
#define MKH_FEAT {ft}
#define MKH_W3 1
#define MKH_ONE_SHOT 1
#define MKH_KERNEL_NAME ik_solve_kernel_{nt}_{ft}_r{nr}_w3o
#include "{os.path.join(CSRC, 'ik_kernel.h')}"
""")
    r = subprocess.run([hipbuild._hipcc()] + hipbuild.FLAGS + hipbuild.KERNEL_FLAGS +
                       ["-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", "-", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, hipbuild._parse_resource_remarks(r.stderr)


def test_no_spilled_vgpr_and_no_more_scratch(twin):
    _, res = twin
    assert any("ik_solve_kernel_44_32_r44_w3o" in f for f in res), list(res)
    for f, r in res.items():
        print(f, r)
        assert r["vgpr_spills"] == 0, (f, r)
        assert r["scratch_bytes_per_lane"] <= PARENT_SCRATCH_BYTES, (f, r)


def test_static_valu_below_the_parent(twin):
    asm, _ = twin
    table = count_valu(asm)
    per = {name: sum(n for f, n in table.items() if name in f) for name in FUNCTIONS}
    print("static VALU:", per, "total", sum(per.values()), "parent", PARENT_STATIC_VALU)
    assert all(per.values()), per                      # the three functions exist as functions (the phases are real calls)
    assert sum(per.values()) < PARENT_STATIC_VALU, per


def test_pinned_tableau_above_the_compilers_registers(twin):
    import check_vgpr_cap
    asm, _ = twin
    nt = 44
    cap = 168 - 2 * nt - 2 * ((nt + 15) // 16)         # TabW3<44>: tableau v[80, 168), planes v[74, 80)
    m = re.search(r"\.vgpr_count:\s+(\d+)", asm)
    assert m and int(m.group(1)) == 168, m
    assert check_vgpr_cap.max_compiler_vgpr(asm) < cap, (check_vgpr_cap.max_compiler_vgpr(asm), cap)
