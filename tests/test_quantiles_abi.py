"""The boundary of the on-device quantiles (CPU only): include/gen_hip.h
declares gh_pf_quantiles and lists it among the replaced reference functions,
libgen_hip.so exports it, the ctypes binding has its signature and the package
its Python forms; and `reference_quantiles`, the host restatement of the
header's definition that tests/test_quantiles.py compares the device against
bit for bit, is pinned here against cases worked by hand.

The restatement uses Python integers for q, S, u and r (nothing rounds), the
oracle's orc_exp for the exp (tests/test_gpu_parity.py pins it bit for bit to
the device's) and the total-order key for the sort.
"""
import ctypes
import itertools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gen_hip.h")


# ----------------------------------------------------------- the reference
def quant_shift(n):
    """The resampler's shift: 62 - ceil(log2 n), at most 52."""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(62 - lg, 52)


def reference_weights(lw, pending=False):
    """The integer weights q_i = floor(exp(lw_i - M) 2^shift) as Python ints
    (2^shift each while a resample is pending)."""
    from oracle import oracle as O

    n = len(lw)
    shift = quant_shift(n)
    if pending:
        return [1 << shift] * n
    L = O.lib()
    M = float(np.max(lw))
    scale = 2.0 ** shift
    # (e <= 1 and a scaling by a power of two: the product is exact, the floor an integer <= 2^52)
    return [0 if v == -math.inf else int(math.floor(L.orc_exp(float(v) - M) * scale)) for v in lw]


def total_order_key(col):
    """uint64 keys whose unsigned order is the total order of the doubles:
    all bits flipped for negatives, the sign bit flipped otherwise."""
    b = np.ascontiguousarray(col, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))


def reference_quantiles(x, lw, probs, pending=False):
    """Q_k(p_j) of states x [n, d] under log-weights lw [n]: [len(probs), d],
    each entry with the bits of the particle that holds it."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    q = reference_weights(np.asarray(lw, dtype=np.float64), pending)
    S = sum(q)
    assert S > 0
    ranks = []
    for p in probs:
        u = int(math.floor(float(p) * 2.0 ** 53))  # exact
        ranks.append(max(1, -((-u * S) >> 53)))   # ceil(u S / 2^53)
    out = np.empty((len(probs), d), dtype=np.float64)
    for k in range(d):
        order = np.argsort(total_order_key(x[:, k]), kind="stable")
        order = [int(i) for i in order if q[int(i)] > 0]  # the support
        cum = list(itertools.accumulate(q[i] for i in order))
        for j, r in enumerate(ranks):
            lo, hi = 0, len(cum) - 1  # the first position whose cumulative weight reaches r
            while lo < hi:
                mid = (lo + hi) // 2
                if cum[mid] >= r:
                    hi = mid
                else:
                    lo = mid + 1
            out[j, k] = x[order[lo], k]
    return out


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------ the boundary
def test_boundary_of_the_quantiles():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    s = "gh_pf_quantiles"
    assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*" % s, code)  # declared
    assert s in table
    assert hasattr(lib, s)
    c_int, c_void_p, pd = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES[s] == (c_int, [c_void_p, c_int, c_int, pd, pd])
    for f in ("quantiles", "weighted_median", "credible_interval"):
        assert callable(getattr(gen, f)) and f in gen.__all__


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    p, out = (ctypes.c_double * 1)(0.5), (ctypes.c_double * 1)()
    assert lib.gh_pf_quantiles(None, 0, 1, p, out) == 1
    assert b"null" in lib.gh_last_error()


# ------------------------------------- the reference, on cases worked by hand
def test_reference_equal_weights():
    """n = 4: shift = 52, q = 2^52 each, S = 2^54.  r = max(1, ceil(u 2^54 /
    2^53)) = max(1, 2 u): p = 0 -> 1, 0.25 -> 2^52 (the 1st order statistic's
    cumulative weight), 0.5 -> 2^53 (the 2nd's, reached exactly), 0.5 + 2^-53 ->
    2^53 + 2 (the 3rd), 1 -> 2^54 (the 4th)."""
    assert quant_shift(4) == 52 and quant_shift(1) == 52 and quant_shift(1025) == 51 and quant_shift(1 << 20) == 42
    x = np.array([[3.0], [1.0], [4.0], [2.0]])
    lw = np.full(4, -7.25)
    assert reference_weights(lw) == [1 << 52] * 4
    got = reference_quantiles(x, lw, [0.0, 0.25, 0.5, 0.5 + 2.0 ** -53, 1.0])
    assert got[:, 0].tolist() == [1.0, 1.0, 2.0, 3.0, 4.0]
    assert np.array_equal(reference_quantiles(x, np.zeros(4), [0.5], pending=True), [[2.0]])


def test_reference_zero_weight_below_the_support():
    x = np.array([[-5.0, 9.0], [1.0, 8.0], [2.0, 7.0]])
    lw = np.array([-math.inf, 0.0, 0.0])
    assert reference_weights(lw) == [0, 1 << 52, 1 << 52]
    got = reference_quantiles(x, lw, [0.0, 0.5, 1.0])
    assert got.tolist() == [[1.0, 7.0], [1.0, 7.0], [2.0, 8.0]]  # never -5 (nor its 9), not even at p = 0


def test_reference_ties_in_value():
    """x = 1, 1, 1, 2 with equal weights: the tie holds 3/4 of the weight."""
    x = np.array([[1.0], [2.0], [1.0], [1.0]])
    got = reference_quantiles(x, np.zeros(4), [0.0, 0.5, 0.75, 0.75 + 2.0 ** -53, 1.0])
    assert got[:, 0].tolist() == [1.0, 1.0, 1.0, 2.0, 2.0]


def test_reference_negative_zero_is_below_positive_zero():
    x = np.array([[0.0], [-0.0]])
    got = reference_quantiles(x, np.zeros(2), [0.0, 0.5, 0.5 + 2.0 ** -53, 1.0])
    assert _bits(got[:, 0]).tolist() == [1 << 63, 1 << 63, 0, 0]
    k = total_order_key(np.array([-math.inf, -1.0, -0.0, 0.0, 1.0, math.inf]))
    assert (np.diff(k.astype(object)) > 0).all()


def test_reference_one_particle_carries_the_weight():
    """exp(-2000) is 0: q = 0, 2^52, 0, and every p returns the middle particle."""
    x = np.array([[-1.0], [5.0], [7.0]])
    lw = np.array([-2000.0, 0.0, -2000.0])
    assert reference_weights(lw) == [0, 1 << 52, 0]
    got = reference_quantiles(x, lw, [0.0, 0.3, 1.0])
    assert got[:, 0].tolist() == [5.0, 5.0, 5.0]


def test_reference_unequal_weights():
    """lw = log 1, log 1/2 (to an ulp): q = 2^52 and about 2^51; the median is
    the heavier particle wherever it sorts, p just above its share the other."""
    x = np.array([[2.0], [1.0]])
    lw = np.array([0.0, math.log(0.5)])
    q = reference_weights(lw)
    assert q[0] == 1 << 52 and abs(q[1] - (1 << 51)) <= 4
    got = reference_quantiles(x, lw, [0.0, 0.3, 0.34, 1.0])
    assert got[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0]
