"""The boundary of the path summaries (CPU only): include/gen_hip.h declares
gh_pf_estimate_path and gh_pf_quantiles_path and lists them among the replaced
reference functions, libgen_hip.so exports them, the ctypes binding has their
signatures and the package their Python forms; and
`reference_path_diagnostics`, the host restatement of the header's `distinct`
and `ess` that tests/test_path.py compares the device against, is pinned here
against cases worked by hand.

The restatement never sees an ancestor index: it groups the rows of
states(t) that are the same bits (current particles with one ancestor at step
t read the same row; for a continuous latent distinct ancestors hold distinct
rows), sums their integer weights as Python ints (nothing rounds) and forms
S^2 / sum m^2 as a fraction.
"""
import ctypes
import re
from fractions import Fraction

import numpy as np

from tests.test_quantiles_abi import HEADER


# ----------------------------------------------------------- the reference
def reference_path_diagnostics(x_t, q):
    """(distinct, ess) of one step: x_t = states(t) [n, d], q the current
    particles' integer weights (Python ints, reference_weights)."""
    x_t = np.ascontiguousarray(x_t, dtype=np.float64)
    m = {}
    for row, qi in zip(x_t.view(np.uint64), q):
        key = row.tobytes()
        m[key] = m.get(key, 0) + int(qi)
    S = sum(m.values())
    distinct = sum(1 for v in m.values() if v > 0)
    return distinct, float(Fraction(S * S, sum(v * v for v in m.values())))


# ------------------------------------------------------------ the boundary
def test_boundary_of_the_path_summaries():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    sigs = {"gh_pf_estimate_path": (c_int, [c_void_p, c_int, c_int, pd, pi, pd, pd]),
            "gh_pf_quantiles_path": (c_int, [c_void_p, c_int, c_int, c_int, pd, pd])}
    for s, sig in sigs.items():
        assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*" % s, code)  # declared
        assert s in table
        assert hasattr(lib, s)
        assert _lib.SIGNATURES[s] == sig
    for f in ("estimate_path", "quantiles_path", "median_path", "credible_band"):
        assert callable(getattr(gen, f)) and f in gen.__all__
    assert "ParticlePathEstimate" in gen.__all__
    assert gen.ParticlePathEstimate._fields == ("ess", "distinct", "mean", "cov")


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    p, out, n = (ctypes.c_double * 1)(0.5), (ctypes.c_double * 1)(), (ctypes.c_int64 * 1)()
    assert lib.gh_pf_estimate_path(None, 1, 0, out, n, None, None) == 1
    assert b"null" in lib.gh_last_error()
    assert lib.gh_pf_quantiles_path(None, 1, 0, 1, p, out) == 1
    assert b"null" in lib.gh_last_error()


# ------------------------------------- the reference, on cases worked by hand
def test_reference_two_particles_share_an_ancestor():
    """Four equal weights, the middle two on one row: m = 1, 2, 1, S = 4,
    ess = 16 / 6."""
    x = np.array([[1.0, 5.0], [2.0, 6.0], [2.0, 6.0], [3.0, 7.0]])
    assert reference_path_diagnostics(x, [1, 1, 1, 1]) == (3, 16 / 6)
    q = 1 << 52  # (the scale cancels exactly)
    assert reference_path_diagnostics(x, [q] * 4) == (3, 16 / 6)
    # rows that differ in one bit are two ancestors
    y = x.copy()
    y[2, 1] = np.nextafter(6.0, 7.0)
    assert reference_path_diagnostics(y, [1, 1, 1, 1]) == (4, 4.0)
    z = np.array([[0.0], [-0.0]])
    assert reference_path_diagnostics(z, [1, 1]) == (2, 2.0)


def test_reference_a_shared_row_of_weight_zero_is_not_counted():
    x = np.array([[1.0], [1.0], [2.0], [3.0]])
    assert reference_path_diagnostics(x, [0, 0, 3, 1]) == (2, 16 / 10)
    assert reference_path_diagnostics(x, [0, 2, 3, 0]) == (2, 25 / 13)


def test_reference_one_particle_carries_the_weight():
    x = np.array([[-1.0], [5.0], [7.0]])
    assert reference_path_diagnostics(x, [0, 1 << 52, 0]) == (1, 1.0)
