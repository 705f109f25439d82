"""The feature front end's matching cost (DESIGN.md 5.3 "Matching cost"; include/flame_hip.h, flame_hip_frontend_set_cost) restated
in NumPy: the rules tests/frontend_ref.py's FrontEndRef applies after `set_cost`.  A helper, not a test: tests/test_fe_zm_ref.py
checks it on hand-written windows, for exact offset invariance and against ground truth, tests/test_gpu_fe_zm.py compares the
library with it bit for bit.

In mode ZSSD the cost of a sample is the integer rule  n = win^2, S1 = sum D, S2 = sum D^2, C = n S2 - S1^2  on the window of
differences (Python integers: no width to overflow; the kernel forms S1 in an int32, S2 and C in 64 bits), and BAD_MATCH is
C > n bad, the product saturated at 2^64 - 1."""
import numpy as np

F = np.float32
COST_SSD, COST_ZSSD = 0, 1
U64_MAX = 2 ** 64 - 1


def sat_mul(n, bad):
    """n * bad, saturated at UINT64_MAX the way the host forms it (the quotient test, no wide product)."""
    return U64_MAX if bad > U64_MAX // n else n * bad


def bad_threshold(max_match_error, win, mode):
    """BAD_MATCH is C > this: bad = (uint64)(max_match_error win^2 65536) for SSD, n bad (saturated) for ZSSD."""
    n = win * win
    bad = int(float(F(max_match_error)) * float(n) * 65536.0)
    return bad if mode == COST_SSD else sat_mul(n, bad)


def zssd(Dm):
    """The rule on a window of differences D_i (any integer array)."""
    d = [int(x) for x in np.asarray(Dm).reshape(-1)]
    n, S1, S2 = len(d), sum(d), sum(x * x for x in d)
    return n * S2 - S1 * S1
