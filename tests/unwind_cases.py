"""Designed inputs of the turn unwinding (tests/test_ladder_nodes_cpu.py, tests/test_gpu_ladder_nodes.py): a small model that has
every kind of joint the rule tells apart — a free joint, an unlimited hinge, a hinge whose range spans three turns, a hinge of
less than a turn, a slide, a ball — and rows that sit on the rule's edges."""

import numpy as np

import unwind_ref as uw

TURNS_XML = """
<mujoco model="turns">
  <compiler angle="radian"/>
  <default><geom type="sphere" size=".05" mass=".1"/></default>
  <worldbody>
    <body name="float" pos="0 0 1">
      <freejoint name="root"/>
      <geom/>
      <body name="a" pos="0.1 0 0">
        <joint type="hinge" name="unlimited" axis="0 0 1"/>
        <geom/>
        <body name="b" pos="0.1 0 0">
          <joint type="hinge" name="wide" axis="0 1 0" range="-9.5 9.5"/>
          <geom/>
          <body name="c" pos="0.1 0 0">
            <joint type="hinge" name="short" axis="1 0 0" range="-3.1415 3.1415"/>
            <geom/>
            <body name="d" pos="0.1 0 0">
              <joint type="slide" name="slide" axis="1 0 0" range="-20 20"/>
              <geom/>
              <body name="e" pos="0.1 0 0">
                <joint type="ball" name="ball"/>
                <geom/>
                <site name="tip" pos="0.05 0 0"/>
              </body>
            </body>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
</mujoco>
"""
# qpos addresses of TURNS_XML: free 0 … 6, unlimited 7, wide 8, short 9, slide 10, ball 11 … 14
FREE, UNLIMITED, WIDE, SHORT, SLIDE, BALL = 0, 7, 8, 9, 10, 11
PI = np.float64(np.pi)


def turns_model():
    import mink_amd
    return mink_amd.loads_mjcf(TURNS_XML)


def designed_rows(m, n_ref=3, rows_per_ref=64, seed=3):
    """(q_rows (n_ref·rows_per_ref, nq), q_ref (n_ref, nq)) for `m`: random rows spread over several turns around random
    references, and — where `m` is the turns model or the UR5e — the designed ones in the first rows of every reference."""
    rng = np.random.default_rng(seed)
    n = n_ref * rows_per_ref
    base = np.asarray(m.qpos0, dtype=np.float64)
    q_ref = np.tile(base, (n_ref, 1))
    rows = np.tile(base, (n, 1))
    hinges = [(int(m.jnt_qposadr[j]), bool(m.jnt_limited[j]), float(m.jnt_range[j][0]), float(m.jnt_range[j][1]))
              for j in range(m.njnt) if int(m.jnt_type[j]) == uw.JNT_HINGE]
    for qa, limited, lo, hi in hinges:
        a, b = (lo, hi) if limited else (-12.0, 12.0)
        q_ref[:, qa] = rng.uniform(a, b, size=n_ref)
        rows[:, qa] = rng.uniform(a, b, size=n) if limited else rng.uniform(-40.0, 40.0, size=n)
    for j in range(m.njnt):                                     # the other joints: anything at all — they are bit copies
        jt, qa = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt == 2:
            rows[:, qa] = rng.uniform(-15.0, 15.0, size=n)
        elif jt in (0, 1):
            w = 7 if jt == 0 else 4
            rows[:, qa:qa + w] = rng.normal(size=(n, w))        # (not normalised on purpose: the rule does not touch them)
    if not hinges:
        return rows, q_ref
    qa, limited, lo, hi = next((h for h in hinges if h[1] and h[3] - h[2] >= float(uw.TWO_PI)), hinges[0])
    free = next((h[0] for h in hinges if not h[1]), None)
    for g in range(n_ref):
        r0 = g * rows_per_ref
        ref = np.float64(0.25)
        q_ref[g, qa] = ref
        col = rows[r0:r0 + rows_per_ref, qa]
        col[0] = ref - PI                       # r - x exactly +pi … (quotient 0.5 up to rounding: the even k = 0)
        col[1] = ref + PI                       # … and -pi
        col[2] = ref - 3.0 * PI                 # 1.5 -> 2 when exact
        col[3] = hi                             # at the limits, and one ulp inside
        col[4] = lo
        col[5] = np.nextafter(hi, -np.inf)
        col[6] = np.nextafter(lo, np.inf)
        col[7] = np.nan
        col[8] = np.inf
        col[9] = -np.inf
        col[10] = -0.0
        col[11] = ref + 1e7                     # |quotient| > 1e6
        if g == 1:                              # a reference near the upper limit, rows a turn and two turns below a value
            q_ref[g, qa] = hi - 0.1             # whose nearest turn lies beyond the limit: cut back by one
            col[12] = hi - 0.1 - float(uw.TWO_PI) + 3.0
            col[13] = lo + 0.05
        if g == 2:                              # a reference OUTSIDE the range, turns away: the shift is cut back by two turns
            q_ref[g, qa] = hi + 2.0 * float(uw.TWO_PI) + 0.3 if hi - lo > 3.0 * float(uw.TWO_PI) else hi + 9.0
            col[12] = hi - 0.5                  # (none of the quotient's turns fits: stays)
            col[13] = hi - 0.5 - float(uw.TWO_PI)
            col[14] = lo + 0.2
        if free is not None:
            f = rows[r0:r0 + rows_per_ref, free]
            q_ref[g, free] = 1.0
            f[0], f[1], f[2], f[3], f[4] = 1.0 - PI, 1.0 + PI, 1.0 + 5.0 * PI, np.nan, 1.0 - 1e7
    return rows, q_ref
