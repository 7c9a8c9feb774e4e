"""On-device ESS, weighted mean and covariance (gh_pf_estimate, gh_moments.h)
against the same sums taken on the host from the engine's own accessors.

Reference: x = state.states(t), lw = get_log_weights(state), w = exp(lw -
max lw); zero-weight rows dropped; every sum by math.fsum; the covariance
centred on the fsum mean.

Tolerances (derived, not tuned; eps = 2^-52, n the particle count):
    A_k  = sum w |x_k| / W,   B_kl = sum w |x_k - m_k| |x_l - m_l| / W
    ess:  relative (2 n + 16) eps
    mean: (n + 16) eps A_k
    cov:  (n + 32) eps B_kl + 4 eps (A_k sqrt(B_ll) + A_l sqrt(B_kk))
the any-order summation bound (n - 1) u sum |terms| (u = eps / 2) with room for
the one-ulp exp and the division, so they hold for whatever reduction tree
the kernel uses; the second cov term is the first-order effect of the mean's
own rounding on the centred sums.

An all -inf weight vector is reachable through the public API (an HMM
observation of probability 0 in every state: the step itself does not
refuse), and the estimate then returns GH_E_NUMERIC (test_refusals).
"""
import functools
import json
import math
import os

import numpy as np
import pytest

import gen_amd as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
SEED = 23
SIZES = [1, 63, 64, 65, 257, 4097, 20011]
LAYOUT_CASES = [(d, n) for d in (10, 9) for n in SIZES] + [(d, n) for d in (1, 2, 3, 11, 16) for n in (65, 4097)]


# ----------------------------------------------------------- the reference
def reference(x, lw):
    """(ess, mean, cov, A, B) by fsum from states [n, d] and log-weights [n]."""
    w = np.exp(lw - lw.max())
    keep = w > 0
    x, w = x[keep], w[keep]
    d = x.shape[1]
    W = math.fsum(w)
    ess = W * W / math.fsum(w * w)
    mean = np.array([math.fsum(w * x[:, k]) / W for k in range(d)])
    A = np.array([math.fsum(w * np.abs(x[:, k])) / W for k in range(d)])
    dx = x - mean
    cov, B = np.empty((d, d)), np.empty((d, d))
    for k in range(d):
        for l in range(k, d):
            cov[k, l] = cov[l, k] = math.fsum(w * dx[:, k] * dx[:, l]) / W
            B[k, l] = B[l, k] = math.fsum(w * np.abs(dx[:, k]) * np.abs(dx[:, l])) / W
    return ess, mean, cov, A, B


def bounds(n, A, B):
    sd = np.sqrt(np.diag(B))
    return ((2 * n + 16) * EPS, (n + 16) * EPS * A,
            (n + 32) * EPS * B + 4 * EPS * (np.outer(A, sd) + np.outer(sd, A)))


def check(st, t=None, what=""):
    """estimate(st, t) within the bounds of the host reference; returns the estimate."""
    n = st.n_local
    ess, mean, cov, A, B = reference(st.states(t), gen.get_log_weights(st))
    b_ess, b_mean, b_cov = bounds(n, A, B)
    est = gen.estimate(st, t)
    assert not (np.isnan(est.ess) or np.isnan(est.mean).any() or np.isnan(est.cov).any()), what
    e_ess, e_mean, e_cov = abs(est.ess - ess) / ess, np.abs(est.mean - mean), np.abs(est.cov - cov)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = (e_ess / b_ess, np.nanmax(np.where(e_mean > 0, e_mean / b_mean, 0.0)),
                 np.nanmax(np.where(e_cov > 0, e_cov / b_cov, 0.0)))
    print(f"{what} t={t} n={n}: error / bound  ess {worst[0]:.3g}  mean {worst[1]:.3g}  cov {worst[2]:.3g}")
    assert e_ess <= b_ess, (what, est.ess, ess)
    assert (e_mean <= b_mean).all(), (what, worst[1])
    assert (e_cov <= b_cov).all(), (what, worst[2])
    assert np.array_equal(est.cov, est.cov.T), what  # exactly symmetric
    only_mean = gen.estimate(st, t, cov=False)
    assert only_mean.cov is None and _bits(only_mean.mean, est.mean) and _bits(only_mean.ess, est.ess), what
    return est


def _bits(a, b):
    return np.array_equal(np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64),
                          np.atleast_1d(np.asarray(b, dtype=np.float64)).view(np.uint64))


# ------------------------------------------------------------- the filters
@functools.lru_cache(maxsize=None)
def _model(d=10):
    return gen.LinearGaussianSSM.benchmark(d)


@functools.lru_cache(maxsize=None)
def _observations(d=10, peaked=False):
    _, ys = _model(d).simulate(7, np.random.default_rng(5))
    ys = np.array(ys, dtype=np.float64)
    if peaked:
        ys[1] += 400.0  # far from every particle: the nearest one takes all the weight
    ys.setflags(write=False)
    return ys


def _obs_at(model, y, t):
    if isinstance(y, dict):
        return {("chain", t, k): v for k, v in y.items()}
    return {model.obs_address(t): y}


def _init(model, ys, n, **kw):
    return gen.initialize_particle_filter(model, (1,), _obs_at(model, ys[0], 1), n, seed=SEED, **kw)


def _steps(st, model, ys, steps, thr):
    """`steps` more steps, a maybe_resample(thr) before each; the decisions."""
    did = []
    for _ in range(steps):
        t = st.t + 1
        did.append(gen.maybe_resample(st, thr))
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(model, ys[t - 1], t))
    return did


# ------------------------------------------------------------------- cases
@pytest.mark.parametrize("d,n", LAYOUT_CASES)
def test_layouts_and_tails(gh_ctx, d, n):
    """Row tiles (d = 10) and pair tiles, full and partial last tiles, one block
    and several: after init and after 3 steps without a resample (accumulated
    weights, the identity path)."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        for stage in ("init", "3 steps"):
            est = check(st, what=f"d={d} {stage}")
            if n == 1:
                assert est.ess == 1.0 and not est.cov.any()  # exactly the zero matrix
            if stage == "init":
                assert not any(_steps(st, m, ys, 3, 0))
    finally:
        st.close()


@pytest.mark.parametrize("d", [10, 9])
@pytest.mark.parametrize("n", [65, 4097, 20011])
def test_pending_resample(gh_ctx, d, n):
    """Between a resample that fired and the next step the particles are the
    resampled ones, equally weighted, as states() and get_log_weights report."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 1, 0)
        assert gen.maybe_resample(st, n)
        assert not gen.get_log_weights(st).any()
        est = check(st, what=f"d={d} pending")
        assert est.ess == float(n) and gen.effective_sample_size(st) == float(n) and st.ess == float(n)
        _steps(st, m, ys, 1, 0)  # (the pending resample is consumed by this step)
        check(st, what=f"d={d} after the resampled step")
    finally:
        st.close()


@pytest.mark.parametrize("d", [10, 3])
def test_earlier_steps(gh_ctx, d):
    n = 4097
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        assert any(_steps(st, m, ys, 4, n / 2))  # (the walk crosses at least one resample)
        for t in range(1, st.t + 1):
            est = check(st, t, what=f"d={d} earlier step")
            assert _bits(gen.weighted_mean(st, t), est.mean) and _bits(gen.weighted_covariance(st, t), est.cov)
    finally:
        st.close()
    st = _init(m, ys, n, record_history=False)
    try:
        _steps(st, m, ys, 2, n / 2)
        with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
            gen.estimate(st, 1)
        check(st, what=f"d={d} without history")
    finally:
        st.close()


def test_cancellation(gh_ctx):
    """States offset by 1e6 with unit spread: one-pass raw moments would lose
    |mean|^2 / var = 1e12 of the covariance's digits."""
    d, n = 3, 20011
    I = np.eye(d)
    m = gen.LinearGaussianSSM(I, 0.1 * I, I, 0.5 * I, 1e6 * np.ones(d), I)
    _, ys = m.simulate(3, np.random.default_rng(5))
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 2, 0)
        est = check(st, what="offset 1e6")
        assert (np.abs(est.mean) > 9e5).all() and (np.diag(est.cov) < 10).all()
    finally:
        st.close()


def test_degenerate_weights(gh_ctx):
    n = 4133
    m, ys = _model(), _observations(peaked=True)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 1, 0)
        lw = gen.get_log_weights(st)
        w = np.exp(lw - lw.max())
        assert np.count_nonzero(w) < n // 2 and w.sum() < 1.5  # one particle carries the weight
        est = check(st, what="degenerate")
        assert est.ess < 1.5
    finally:
        st.close()


def _hmm():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "hmm.json")))["pf_test"]
    return gen.DiscreteHMM(g["prior"], np.array(g["transition"]), np.array(g["emission"])), g["obs"]


def _kitagawa():
    m = gen.KitagawaSSM(10.0, 1.0)
    return m, m.simulate(4, np.random.default_rng(5))[1]


def _slots():
    from tests.test_slots import count_obs

    m, obs = count_obs()
    return m, obs[:4]


@pytest.mark.parametrize("family", [_kitagawa, _hmm, _slots], ids=["kitagawa", "hmm", "slots"])
def test_other_families(gh_ctx, family):
    """The estimate is of the stored doubles (the HMM's: the class index)."""
    m, ys = family()
    st = _init(m, ys, 4097)
    try:
        _steps(st, m, ys, 3, 4097 / 2)
        check(st, what=family.__name__)
    finally:
        st.close()


def test_regression(gh_ctx):
    m, ys = gen.BayesianLinearRegression.quickstart()
    st = gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys), 4097, seed=SEED)
    try:
        est = check(st, what="regression")
        assert est.mean.shape == (2,) and est.cov.shape == (2, 2)
    finally:
        st.close()


def test_batched_run(gh_ctx):
    """After gh_pf_run the weight sums are recomputed on demand (ensure_stats)."""
    n = 20011
    m, ys = _model(), _observations()
    st = _init(m, ys, n)
    try:
        gen.run_particle_filter(st, list(ys[1:6]))
        est = check(st, what="after run_particle_filter")
        assert _bits(gen.effective_sample_size(st), est.ess) and _bits(st.ess, est.ess)
    finally:
        st.close()


def test_reproducible_and_read_only(gh_ctx):
    n = 20011
    m, ys = _model(), _observations()
    ests = []
    for _ in range(2):
        st = _init(m, ys, n)
        try:
            _steps(st, m, ys, 3, n / 2)
            before = (gen.get_log_weights(st), st.states(), gen.log_ml_estimate(st))
            ests += [gen.estimate(st), gen.estimate(st)]
            after = (gen.get_log_weights(st), st.states(), gen.log_ml_estimate(st))
            assert all(_bits(a, b) for a, b in zip(before, after))
        finally:
            st.close()
    for e in ests[1:]:
        assert _bits(e.ess, ests[0].ess) and _bits(e.mean, ests[0].mean) and _bits(e.cov, ests[0].cov)


def test_known_answer(gh_ctx):
    """The golden lg2 model against its Kalman filter, within six standard
    errors at the filter's own ESS: |mean_k - mu_k| <= 6 sqrt(P_kk / ess),
    |cov_kl - P_kl| <= 6 sqrt((P_kk P_ll + P_kl^2) / ess).  (On the CPU oracle,
    whose states and weights the GPU reproduces, this configuration stays at
    <= 1.30 sigma for the mean and <= 1.98 sigma for the covariance, ess
    between 581 and 3432.)"""
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "kalman.json")))["lg2"]
    d, n = k["d"], 4097
    I = np.eye(d)
    m = gen.LinearGaussianSSM(np.array(k["A"]), 0.1 * I, I, 0.5 * I, np.zeros(d), I)
    ys = np.array(k["ys"]).reshape(-1, d)[:6]
    mus, Ps = m.kalman_filter(ys)
    st = _init(m, ys, n)
    try:
        for t in range(1, 7):
            if t > 1:
                _steps(st, m, ys, 1, n / 2)
            est = gen.estimate(st)
            P = Ps[t - 1]
            dP = np.diag(P)
            s_mean, s_cov = np.sqrt(dP / est.ess), np.sqrt((np.outer(dP, dP) + P * P) / est.ess)
            print(f"t={t} ess={est.ess:.0f} mean {np.abs(est.mean - mus[t - 1]).max() / s_mean.min():.2f} sigma")
            assert (np.abs(est.mean - mus[t - 1]) <= 6 * s_mean).all(), t
            assert (np.abs(est.cov - P) <= 6 * s_cov).all(), t
    finally:
        st.close()


def test_refusals(gh_ctx):
    """The multi-rank path, steps out of range, nothing to write, and log-weights
    that are all -inf (an HMM observation no state can emit)."""
    from gen_amd import _lib

    m, ys = _model(3), _observations(3)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        st = _init(m, ys, 64, ctx=ctx)
        for f in (gen.estimate, gen.effective_sample_size, gen.weighted_mean, gen.weighted_covariance):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f(st)
        st.close()
    finally:
        ctx.close()
    st = _init(m, ys, 64)
    try:
        _steps(st, m, ys, 1, 32)
        for t in (0, -1, 3, 1.5, True):
            with pytest.raises(gen.GenHipError, match=r"outside 1\.\.2"):
                gen.estimate(st, t)
        lib = _lib.load()
        e = gen.estimate(st)
        assert lib.gh_pf_estimate(st.h, 3, None, _lib.dptr(e.mean), None) == 1  # at the ABI
        assert b"outside 1..2" in lib.gh_last_error()
        assert lib.gh_pf_estimate(st.h, 0, None, None, None) == 1
        assert _bits(gen.estimate(st).mean, e.mean)  # the filter still works
    finally:
        st.close()
    hmm = gen.DiscreteHMM([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[1.0, 1.0], [0.0, 0.0]])
    st = gen.initialize_particle_filter(hmm, (1,), {hmm.obs_address(1): 0}, 257, seed=SEED)
    try:
        assert gen.estimate(st).ess == 257.0  # (observation 0 has probability 1 in both states)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), {hmm.obs_address(2): 1})
        assert np.isneginf(gen.get_log_weights(st)).all()
        for f in (gen.estimate, gen.effective_sample_size):
            with pytest.raises(gen.GenHipError, match="GH_E_NUMERIC"):
                f(st)
    finally:
        st.close()
