"""The boundary of the on-device estimates (CPU only): include/gen_hip.h
declares gh_pf_estimate and lists it among the replaced reference functions,
libgen_hip.so exports it, the ctypes binding has its signature and the package
its Python forms; and LinearGaussianSSM.kalman_filter, the analytic answer the
estimates are checked against, is the recursion of kalman_log_marginal.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gen_hip.h")


def test_boundary_of_the_estimates():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    s = "gh_pf_estimate"
    assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*" % s, code)  # declared
    assert s in table and "effective_sample_size" in table and "normalize_weights" in table
    assert hasattr(lib, s)
    c_int, c_void_p, pd = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES[s] == (c_int, [c_void_p, c_int, pd, pd, pd])
    for f in ("estimate", "effective_sample_size", "weighted_mean", "weighted_covariance", "ParticleEstimate"):
        assert callable(getattr(gen, f)) and f in gen.__all__
    assert gen.ParticleEstimate._fields == ("ess", "mean", "cov")
    assert isinstance(gen.ParticleFilterState.ess, property)


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    e = ctypes.c_double()
    assert lib.gh_pf_estimate(None, 0, ctypes.byref(e), None, None) == 1
    assert b"null" in lib.gh_last_error()


@pytest.mark.parametrize("name", ["lg2", "lg10"])
def test_kalman_filter_is_the_recursion_of_the_log_marginal(name):
    """Final-step mean and covariance against a recursion written out here (the
    predict / update of kalman_log_marginal), to 1e-12; and the same pass gives
    the golden log marginal."""
    import gen_amd as gen

    k = json.load(open(os.path.join(ROOT, "tests", "golden", "kalman.json")))[name]
    d = k["d"]
    A, ys = np.array(k["A"]), np.array(k["ys"]).reshape(-1, d)
    Q, H, R = 0.1 * np.eye(d), np.eye(d), 0.5 * np.eye(d)
    m = gen.LinearGaussianSSM(A, Q, H, R, np.zeros(d), np.eye(d))
    means, covs = m.kalman_filter(ys)
    assert means.shape == (len(ys), d) and covs.shape == (len(ys), d, d)
    mu, P, ll = np.zeros(d), np.eye(d), 0.0
    for t, y in enumerate(ys):
        if t > 0:
            mu, P = A @ mu, A @ P @ A.T + Q
        S = H @ P @ H.T + R
        r = y - H @ mu
        ll += -0.5 * (d * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + r @ np.linalg.solve(S, r))
        G = np.linalg.solve(S, H @ P).T  # the gain P H' S^-1 (S and P symmetric)
        mu, P = mu + G @ r, P - G @ H @ P
        assert np.allclose(means[t], mu, rtol=0, atol=1e-12) and np.allclose(covs[t], P, rtol=0, atol=1e-12)
    assert np.abs(means[-1] - mu).max() <= 1e-12 and np.abs(covs[-1] - P).max() <= 1e-12
    assert abs(ll - k["log_ml"]) <= 1e-9 * abs(k["log_ml"])
    assert abs(m.kalman_log_marginal(ys) - ll) <= 1e-9 * abs(ll)
