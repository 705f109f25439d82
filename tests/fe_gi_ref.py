"""The feature front end's gain-invariant matching cost (DESIGN.md 5.3 "Matching cost"; include/flame_hip.h,
flame_hip_frontend_set_gain_invariant) restated in NumPy: the rules tests/frontend_ref.py's FrontEndRef applies after
`set_gain_invariant`.  A helper, not a test: tests/test_fe_gi_ref.py checks it on hand-written windows, for exact invariance under
a power-of-two gain with offsets and against ground truth, tests/test_gpu_fe_gi.py compares the library with it bit for bit.

With the switch on (it does not touch `cost_mode`) the cost of a sample is `gi_cost` of its window: the sums in Python integers
(no width to overflow; the kernel holds SI in 32 bits and the others in 64) and three np.float64 operations, each rounded once.
BAD_MATCH is C > n bad (ZSSD's threshold) and, before the threshold, a reference window with ZR == 0."""
import numpy as np

F = np.float32
F64 = np.float64


def window_sums(Iw, Rw):
    """(n, ZI, ZR, ZIR) of a window: Iw = the bilinear sums of the current image (0 ... 65 280), Rw = 256 x the reference pixels."""
    a = [int(x) for x in np.asarray(Iw).reshape(-1)]
    b = [int(x) for x in np.asarray(Rw).reshape(-1)]
    assert len(a) == len(b)
    n = len(a)
    SI, SII = sum(a), sum(x * x for x in a)
    SR, SRR = sum(b), sum(x * x for x in b)
    SIR = sum(x * y for x, y in zip(a, b))
    return n, n * SII - SI * SI, n * SRR - SR * SR, n * SIR - SI * SR


def gi_from_sums(ZI, ZR, ZIR):
    """C of the three integers: ZR when ZI == 0 or ZIR <= 0, else floor(ZR - ZIR^2 / ZI) clamped at 0, in float64."""
    assert 0 <= ZI < 2 ** 45 and 0 <= ZR < 2 ** 45 and abs(ZIR) < 2 ** 45
    if ZI == 0 or ZIR <= 0:
        return ZR
    z = F64(ZIR)  # (< 2^53: exact)
    q = (z * z) / F64(ZI)
    Cd = F64(ZR) - q
    return int(np.floor(Cd)) if Cd > 0 else 0


def gi_cost(Iw, Rw):
    """The rule on a window; returns (C, ZR)."""
    _, ZI, ZR, ZIR = window_sums(Iw, Rw)
    return gi_from_sums(ZI, ZR, ZIR), ZR
