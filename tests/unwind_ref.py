"""numpy restatement of the turn unwinding (include/minkhip.h "THE RULE OF THE UNWINDING": mkh_unwind_turns,
MKH_FLAG_UNWIND_TURNS).  Written from the header's text, not from the kernel.  Every product and sum is a numpy scalar operation
of its own — rounded once, never fused — and np.rint rounds half to even, so the device's rows are reproduced bit for bit."""

import numpy as np

JNT_HINGE = 3
TWO_PI = np.float64(6.283185307179586)


def eligible(model):
    """[(qposadr, limited, range_lo, range_hi)] of the hinges the rule moves: unlimited, or with a range of at least TWO_PI."""
    out = []
    for j in range(model.njnt):
        if int(model.jnt_type[j]) != JNT_HINGE:
            continue
        lo, hi = np.float64(model.jnt_range[j][0]), np.float64(model.jnt_range[j][1])
        limited = bool(model.jnt_limited[j])
        if not limited or hi - lo >= TWO_PI:
            out.append((int(model.jnt_qposadr[j]), limited, lo, hi))
    return out


def unwind_value(x, r, limited, lo, hi):
    """One entry: x moved toward r by whole turns."""
    x, r = np.float64(x), np.float64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        quot = (r - x) / TWO_PI
        k = np.rint(quot)
        if not (np.isfinite(x) and np.isfinite(r) and np.isfinite(quot)) or abs(quot) > 1e6:
            k = np.float64(0.0)
        if limited:
            while k > 0.0 and x + k * TWO_PI > hi:
                k = k - 1.0
            while k < 0.0 and x + k * TWO_PI < lo:
                k = k + 1.0
        return x if k == 0.0 else x + k * TWO_PI


def unwind(model, q_rows, q_ref, rows_per_ref=1):
    """mkh_unwind_turns on host arrays: q_rows (n, nq), row i toward q_ref[i // rows_per_ref].  A new array."""
    q_rows = np.ascontiguousarray(q_rows, dtype=np.float64)
    q_ref = np.ascontiguousarray(q_ref, dtype=np.float64)
    out = q_rows.copy()
    for qa, limited, lo, hi in eligible(model):
        for i in range(len(q_rows)):
            out[i, qa] = unwind_value(q_rows[i, qa], q_ref[i // rows_per_ref, qa], limited, lo, hi)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
