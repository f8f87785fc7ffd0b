"""Static ratchet behind the low-rank start's host tables (dof lists of the product lanes, the right-hand side's chunk entry,
the joint-anchor flag; docs/HISTORY.md "Low-rank start: model constants out of the solve"): the headline kernel's translation
unit, compiled and counted exactly as tests/test_headline_isa_cpu.py does, must stay below what its parent had —

  pre_phases 1 736 + wood_start 985 + kernel body 1 527 = 4 248 static VALU instructions,

with `wood_start`, where the tables are read, below its own 985.  A ratchet against drifting back; the speed is the same-box A/B
of docs/HISTORY.md."""

import pytest

from test_headline_isa_cpu import FUNCTIONS, count_valu, pytestmark, twin  # noqa: F401  (the fixture compiles the twin once per module)

PARENT_STATIC_VALU = 4248
PARENT_WOOD_START_VALU = 985


def test_static_valu_below_the_parent_of_the_lane_lists(twin):
    asm, _ = twin
    table = count_valu(asm)
    per = {name: sum(n for f, n in table.items() if name in f) for name in FUNCTIONS}
    print("static VALU:", per, "total", sum(per.values()), "parent", PARENT_STATIC_VALU, "wood_start then", PARENT_WOOD_START_VALU)
    assert all(per.values()), per
    assert sum(per.values()) < PARENT_STATIC_VALU, per
    assert per["wood_start"] < PARENT_WOOD_START_VALU, per
