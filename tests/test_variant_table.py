"""CPU-side checks that the list of compiled ik_solve_kernel builds exists ONCE: mink_amd/csrc/build.py VARIANTS.  The translation
units, the host's table (variants.h, generated into _build/dispatch.hip) and kernel_resources.json follow from it; minkhip.hip
asks the table which builds exist instead of restating the tuples."""

import json
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")


@pytest.fixture(scope="module")
def hipbuild():
    from mink_amd.csrc import build
    build.build(verbose=False)
    return build


def test_variant_names_are_unique_and_cover_the_tuples(hipbuild):
    names = [v.name for v in hipbuild.VARIANTS]
    assert len(set(names)) == len(names)
    # one build per entry of the tuples that record why each exists (what the six loops of the old generator produced)
    expected = (len(hipbuild.NTS) * len(hipbuild.FEATS) + len(hipbuild.WOOD) * len(hipbuild.WOOD_FEATS) + len(hipbuild.WOOD_ROWS)
                + len(hipbuild.W3) + len(hipbuild.W3_WOOD) + len(hipbuild.W3_WOOD_ONE_SHOT))
    assert len(names) == expected
    by_name = {v.name: v for v in hipbuild.VARIANTS}
    assert by_name["44_32_r44_w3o"] == hipbuild.Variant(44, 32, 44, w3=True, one_shot=True)
    assert by_name["8_0"] == hipbuild.Variant(8, 0)
    assert by_name["44_0_w3"] == hipbuild.Variant(44, 0, w3=True)
    assert by_name["48_40_r48"] == hipbuild.Variant(48, 40, 48)


def test_translation_unit_macros(hipbuild):
    """Plain builds let ik_kernel.h compose the kernel's name; MKH_W4 belongs to the low-rank one-more-wave builds up to 24 rows."""
    def macros(v):
        return dict(re.findall(r"^#define (\w+) (\S+)$", v.translation_unit(), re.M))
    assert macros(hipbuild.Variant(8, 0)) == {"MKH_NT": "8", "MKH_FEAT": "0"}
    assert macros(hipbuild.Variant(44, 0, w3=True)) == {"MKH_NT": "44", "MKH_FEAT": "0", "MKH_W3": "1",
                                                         "MKH_KERNEL_NAME": "ik_solve_kernel_44_0_w3"}
    assert macros(hipbuild.Variant(24, 48, 24, w3=True)) == {"MKH_NT": "24", "MKH_NR": "24", "MKH_FEAT": "48", "MKH_W3": "1", "MKH_W4": "1",
                                                              "MKH_KERNEL_NAME": "ik_solve_kernel_24_48_r24_w3"}
    assert "MKH_W4" not in macros(hipbuild.Variant(32, 32, 32, w3=True))
    assert macros(hipbuild.Variant(44, 32, 44, w3=True, one_shot=True)) == {
        "MKH_NT": "44", "MKH_NR": "44", "MKH_FEAT": "32", "MKH_W3": "1", "MKH_ONE_SHOT": "1",
        "MKH_KERNEL_NAME": "ik_solve_kernel_44_32_r44_w3o"}
    for v in hipbuild.VARIANTS:
        assert ("MKH_W4" in macros(v)) == (v.w3 and v.nr != 0 and v.nt <= 24), v.name


def test_resources_hold_exactly_the_listed_kernels(hipbuild):
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    built = {k for k in table if k.startswith("ik_solve_kernel_")}
    assert built == {"ik_solve_kernel_" + v.name for v in hipbuild.VARIANTS}


def test_generate_leaves_one_translation_unit_per_variant(hipbuild):
    srcs = hipbuild._generate()
    want = {f"variant_{v.name}" for v in hipbuild.VARIANTS}
    assert set(srcs) == want | {"dispatch"}
    left = {f[:-len(".hip")] for f in os.listdir(hipbuild.BUILD) if f.startswith("variant_") and f.endswith(".hip")}
    assert left == want
    stems = {f.split(".", 1)[0] for f in os.listdir(hipbuild.BUILD) if f.startswith("variant_")}
    assert stems == want                      # (objects, dependency files: nothing of a variant that is not listed)
    # the host's table: one row per variant, with the kernel's name and its launcher
    dispatch = open(os.path.join(hipbuild.BUILD, "dispatch.hip")).read()
    rows = re.findall(r'^\s*\{(\d+), (\d+), (\d+), (true|false), (true|false), "ik_solve_kernel_(\w+)", &launch_(\w+)\},$', dispatch, re.M)
    assert len(rows) == len(hipbuild.VARIANTS)
    for (nt, nr, ft, w3, one, kernel, launcher), v in zip(rows, hipbuild.VARIANTS):
        assert (int(nt), int(ft), int(nr), w3 == "true", one == "true") == tuple(v), v.name
        assert kernel == launcher == v.name


def test_sources_do_not_restate_the_list(hipbuild):
    host = open(os.path.join(CSRC, "minkhip.hip")).read()
    # no array literal of tableau sizes, no kernel name composed by a format string
    nt = "(?:" + "|".join(str(n) for n in hipbuild.NTS) + ")"
    assert not re.search(r"\{\s*%s\s*(?:,\s*%s\s*)+\}" % (nt, nt), host)
    for m in re.finditer(r"snprintf\s*\(([^;]*);", host):
        assert "ik_solve_kernel_" not in m.group(1), m.group(0)
    assert "ik_solve_kernel_" not in re.sub(r"//[^\n]*", "", host)
    build_py = open(os.path.join(CSRC, "build.py")).read()
    assert "must match" not in build_py
    assert build_py.count('#include "../ik_kernel.h"') == 1       # one translation-unit template
