"""forecast (gh_pf_forecast, gh_forecast.h): the posterior predictive of
x_{T+k} and y_{T+k}, k = 1..H, from a filter at step T that is only read.

The latent draws are pinned bit for bit against the filter's own unobserved
steps (a twin filter stepped with observations=None and no resample), the
moments against the same sums taken on the host from the returned draws
(test_estimates.reference / bounds: the any-order summation bounds, nothing
tuned), the observation noise against simulate's, and the whole against the
Kalman prediction of the golden lg2 model.

Horizons: 1, 2, 5 and, at d = 10 (dy = 10), 11 — the pass-1 accumulators of 9
horizons fit a block's LDS there, so 11 runs two chunks — and 64, which also
splits pass 0.  The refusals "before init" and "d outside 1..16" of the C ABI
cannot be reached through a filter handle (no handle exists before init, and
no model of another size can be created), so they are not exercised here.
"""
import json
import os

import numpy as np
import pytest

import gen_amd as gen
from tests.test_estimates import (EPS, LAYOUT_CASES, SEED, _bits, _hmm, _init, _kitagawa, _model, _obs_at,
                                  _observations, _slots, _steps, bounds, reference)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZONS = (1, 2, 5, 11)


def _filter(m, ys, n, T=4, inputs=None, **kw):
    """A filter at step T: init, then T - 1 steps with a maybe_resample(n / 2) before each."""
    st = _init(m, ys, n, **kw)
    for t in range(2, T + 1):
        gen.maybe_resample(st, n / 2)
        na = (t,) if inputs is None or inputs[t - 1] is None else (t, inputs[t - 1])
        gen.particle_filter_step(st, na, (gen.UnknownChange(),) * len(na), _obs_at(m, ys[t - 1], t))
    return st


def _unobserved_step(st, u=None):
    t = st.t + 1
    na = (t,) if u is None else (t, u)
    gen.particle_filter_step(st, na, (gen.UnknownChange(),) * len(na), None)


def _draws_equal_steps(make, H, pending=False, inputs=None):
    """forecast(H, samples=True) on one filter against H unobserved steps of its twin."""
    a, b = make(), make()
    try:
        n = a.n_local
        if pending:
            assert gen.maybe_resample(a, n) and gen.maybe_resample(b, n)
        lw = gen.get_log_weights(b)
        if pending:
            assert not lw.any()
        fc = gen.forecast(a, H, inputs=inputs, samples=True)
        assert fc.xs.shape == (H, n, a.model.d) and fc.ys.shape[:2] == (H, n)
        for k in range(1, H + 1):
            _unobserved_step(b, None if inputs is None else inputs[k - 1])
            assert _bits(b.states(), fc.xs[k - 1]), (H, k)
            assert _bits(gen.get_log_weights(b), lw), (H, k)
        return fc
    finally:
        a.close()
        b.close()


# ------------------------------------------------ 1. the draws, bit for bit
@pytest.mark.parametrize("i,d,n", [(i, d, n) for i, (d, n) in enumerate(LAYOUT_CASES)])
def test_draws_equal_the_filters_own_unobserved_steps(gh_ctx, i, d, n):
    m, ys = _model(d), _observations(d)
    hs = {HORIZONS[i % 4]} | ({11} if d == 10 and n in (65, 4097) else set())
    for H in sorted(hs):
        _draws_equal_steps(lambda: _filter(m, ys, n), H)


def test_draws_over_both_passes_chunks(gh_ctx):
    m, ys = _model(10), _observations(10)
    _draws_equal_steps(lambda: _filter(m, ys, 257), 64)


@pytest.mark.parametrize("d,n", [(10, 4097), (9, 65), (10, 20011)])
def test_draws_with_a_resample_pending(gh_ctx, d, n):
    """maybe_resample(st, n) fired before forecast; the twin's first step
    consumes it.  The weights are all 0 on both sides."""
    m, ys = _model(d), _observations(d)
    _draws_equal_steps(lambda: _filter(m, ys, n), 5 if n < 20011 else 2, pending=True)


def _library():
    from tests.test_slots import library_obs

    return library_obs("m1")


def _switching():
    from tests.test_slots import slds_obs

    return slds_obs()


@pytest.mark.parametrize("family", [_kitagawa, _hmm, _slots, _library, _switching],
                         ids=["kitagawa", "hmm", "slots", "library", "switching"])
@pytest.mark.parametrize("H", [1, 5])
def test_draws_of_other_families(gh_ctx, family, H):
    m, ys = family()
    fc = _draws_equal_steps(lambda: _filter(m, ys, 4097), H)
    assert not np.isnan(fc.x_mean).any() and not np.isnan(fc.y_mean).any()


def test_draws_of_a_slot_model_with_inputs(gh_ctx):
    from tests.test_slots import count_inputs, count_model_inputs, count_obs

    mi = count_model_inputs()
    _, obs = count_obs()
    u = count_inputs()
    U = np.stack([v if v is not None else np.zeros(2) for v in u])[4:9]  # u_{T+1} .. u_{T+5}, T = 4
    _draws_equal_steps(lambda: _filter(mi, obs, 4099, inputs=u), 5, inputs=U)


# ------------------------------------------- 2. the moments of the draws
def _moments_match(fc, lw, n, what):
    """Every horizon's x and y moments within the bounds of the host reference on the draws."""
    for name, draws, mean, cov in (("x", fc.xs, fc.x_mean, fc.x_cov), ("y", fc.ys, fc.y_mean, fc.y_cov)):
        for k in range(len(draws)):
            _, r_mean, r_cov, A, B = reference(draws[k], lw)
            _, b_mean, b_cov = bounds(n, A, B)
            e_mean, e_cov = np.abs(mean[k] - r_mean), np.abs(cov[k] - r_cov)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = (np.nanmax(np.where(e_mean > 0, e_mean / b_mean, 0.0)),
                         np.nanmax(np.where(e_cov > 0, e_cov / b_cov, 0.0)))
            print(f"{what} {name} k={k + 1} n={n}: error / bound  mean {worst[0]:.3g}  cov {worst[1]:.3g}")
            assert not (np.isnan(mean[k]).any() or np.isnan(cov[k]).any()), (what, name, k)
            assert (e_mean <= b_mean).all(), (what, name, k, worst[0])
            assert (e_cov <= b_cov).all(), (what, name, k, worst[1])
            assert np.array_equal(cov[k], cov[k].T), (what, name, k)  # exactly symmetric


def _check_moments(st, H, what, inputs=None):
    n = st.n_local
    lw = gen.get_log_weights(st)
    fc = gen.forecast(st, H, inputs=inputs, samples=True)
    _moments_match(fc, lw, n, what)
    again = gen.forecast(st, H, inputs=inputs, samples=True)
    lean = gen.forecast(st, H, inputs=inputs)
    mean_only = gen.forecast(st, H, inputs=inputs, cov=False)
    assert lean.xs is None and lean.ys is None and mean_only.x_cov is None and mean_only.y_cov is None
    for f in ("x_mean", "x_cov", "y_mean", "y_cov", "xs", "ys"):
        assert _bits(getattr(again, f), getattr(fc, f)), (what, f)  # two calls, the same bits
    for f in ("x_mean", "x_cov", "y_mean", "y_cov"):
        assert _bits(getattr(lean, f), getattr(fc, f)), (what, f)  # samples=False
    assert _bits(mean_only.x_mean, fc.x_mean) and _bits(mean_only.y_mean, fc.y_mean), what  # cov=False
    return fc


# (one particle has ess 1, which no threshold of maybe_resample lies above: no pending case for it)
@pytest.mark.parametrize("i,d,n,pending", [(i, d, n, p) for i, (d, n) in enumerate(LAYOUT_CASES)
                                           for p in (False, True) if not (p and n == 1)])
def test_moments_equal_the_moments_of_the_draws(gh_ctx, i, d, n, pending):
    m, ys = _model(d), _observations(d)
    H = 2 if n > 5000 else (11 if d == 10 and n in (65, 257) else HORIZONS[i % 3])
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 3, 0)  # accumulated weights
        if pending:
            assert gen.maybe_resample(st, n)
        fc = _check_moments(st, H, f"d={d} {'pending' if pending else 'weighted'}")
        if n == 1:
            assert not fc.x_cov.any() and not fc.y_cov.any()  # exactly the zero matrices
    finally:
        st.close()


@pytest.mark.parametrize("family", [_kitagawa, _hmm, _slots], ids=["kitagawa", "hmm", "slots"])
def test_moments_of_other_families(gh_ctx, family):
    m, ys = family()
    st = _filter(m, ys, 4097)
    try:
        _check_moments(st, 3, family.__name__)
    finally:
        st.close()


def test_moments_cancellation(gh_ctx):
    """States offset by 1e6 with unit spread (test_estimates.test_cancellation)."""
    d, n = 3, 20011
    I = np.eye(d)
    m = gen.LinearGaussianSSM(I, 0.1 * I, I, 0.5 * I, 1e6 * np.ones(d), I)
    _, ys = m.simulate(3, np.random.default_rng(5))
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 2, 0)
        fc = _check_moments(st, 2, "offset 1e6")
        assert (np.abs(fc.x_mean) > 9e5).all() and (np.diagonal(fc.x_cov, axis1=1, axis2=2) < 10).all()
    finally:
        st.close()


def test_moments_degenerate_weights(gh_ctx):
    """One particle carries the weight (test_estimates.test_degenerate_weights)."""
    n = 4133
    m, ys = _model(), _observations(peaked=True)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 1, 0)
        lw = gen.get_log_weights(st)
        w = np.exp(lw - lw.max())
        assert np.count_nonzero(w) < n // 2 and w.sum() < 1.5
        _check_moments(st, 2, "degenerate")
    finally:
        st.close()


# ------------------------------------- 3. the observation noise is simulate's
def test_lg_observation_noise_is_simulates(gh_ctx):
    """y = c + H x + L_R z with z keyed by (seed, trace, t) only, so the
    residuals y - (c + H x) of simulate(model, (T + H,), n, seed) and of the
    forecast agree at every (T + k, i) although their latents differ.  Each side
    evaluates c_r + sum_j H_rj x_j + sum_k L_rk z_k by d + dy fused
    multiply-adds on the device (each within u = eps / 2 of its exact result,
    first-order (d + dy) u S_r with S_r = |c_r| + sum |H_rj x_j| + sum |L_rk z_k|),
    and c + H x again on the host (d + 1 roundings on at most S_r) before one
    subtraction: (2 d + dy + 2) u S_r <= (d + dy + 4) eps S_r per side, summed
    over the two sides."""
    d, dy, n, T, H = 3, 2, 4097, 3, 4
    A = np.array([[0.9, 0.1, 0.0], [-0.1, 0.8, 0.05], [0.0, 0.1, 0.7]])
    Hm = np.array([[1.0, 0.5, -0.3], [0.2, -1.0, 0.7]])
    R = np.array([[0.5, 0.2], [0.2, 0.4]])
    c = np.array([0.7, -1.3])
    m = gen.LinearGaussianSSM(A, 0.1 * np.eye(d), Hm, R, np.zeros(d), np.eye(d), b=np.array([0.1, 0.0, -0.2]), c=c)
    _, ys = m.simulate(T, np.random.default_rng(5))
    L = np.linalg.cholesky(R)
    sim = gen.simulate(m, (T + H,), num_traces=n, seed=SEED)
    st = _filter(m, ys, n, T=T)
    try:
        fc = gen.forecast(st, H, samples=True, cov=False)
    finally:
        st.close()
    worst = 0.0
    for k in range(1, H + 1):
        xs_s, ys_s = sim.xs[T + k - 1].T, sim.ys[T + k - 1].T  # [n, d], [n, dy]
        r_s = ys_s - (xs_s @ Hm.T + c)
        r_f = fc.ys[k - 1] - (fc.xs[k - 1] @ Hm.T + c)
        z = np.abs(np.linalg.solve(L, r_s.T).T)
        side = lambda x: (d + dy + 4) * EPS * (np.abs(c) + np.abs(x) @ np.abs(Hm).T + z @ np.abs(L).T)
        bound = side(xs_s) + side(fc.xs[k - 1])
        err = np.abs(r_s - r_f)
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all(), (k, (err / bound).max())
        assert np.abs(r_s).max() > 0.1  # (the noise is there)
    print(f"LG residuals: error / bound {worst:.3g}")


def test_kitagawa_observation_noise_is_simulates(gh_ctx):
    """y = x^2 / 20 + sd_y z: the device rounds x x, the division, sd_y z and
    the sum, the host x^2, the division and the subtraction — at most 7 u on
    terms no larger than |y| + x^2 / 20, within 8 eps (|y| + x^2 / 20) per
    side, summed over the two sides."""
    n, T, H = 4097, 4, 5
    m, ys = _kitagawa()
    sim = gen.simulate(m, (T + H,), num_traces=n, seed=SEED)
    st = _filter(m, ys, n, T=T)
    try:
        fc = gen.forecast(st, H, samples=True, cov=False)
    finally:
        st.close()
    worst = 0.0
    for k in range(1, H + 1):
        x_s, y_s = sim.xs[T + k - 1][0], sim.ys[T + k - 1][0]
        x_f, y_f = fc.xs[k - 1][:, 0], fc.ys[k - 1][:, 0]
        err = np.abs((y_s - x_s ** 2 / 20) - (y_f - x_f ** 2 / 20))
        bound = 8 * EPS * ((np.abs(y_s) + x_s ** 2 / 20) + (np.abs(y_f) + x_f ** 2 / 20))
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all(), (k, (err / bound).max())
    print(f"Kitagawa residuals: error / bound {worst:.3g}")


# ------------------------------------------------------- 4. the known answer
@pytest.mark.parametrize("pending", [False, True], ids=["weighted", "pending"])
def test_known_answer(gh_ctx, pending):
    """The golden lg2 model, n = 4097, seed 23, six filtered steps with
    maybe_resample(n / 2), H = 8, against the Kalman prediction mu_k = A^k
    mu_T, P_k = A P_{k-1} A^T + Q, within six standard errors at the filter's
    ESS when it forecasts (with a resample pending: n):
    |mean - mu_k| <= 6 sqrt(P_kk / ess), |cov - P_k| <= 6 sqrt((P_kk P_ll +
    P_kl^2) / ess) (test_estimates.test_known_answer's formulas).  On the CPU
    oracle, whose states and weights the GPU reproduces, this configuration
    stays at <= 0.93 sigma for the mean and <= 1.31 sigma for the covariance
    at ess 1693; with a resample pending first (ess 4097) at <= 1.25 sigma and
    <= 1.67 sigma.  (The y moments: the tests of sections 2 and 3.)"""
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "kalman.json")))["lg2"]
    d, n, H = k["d"], 4097, 8
    I = np.eye(d)
    A, Q = np.array(k["A"]), 0.1 * I
    m = gen.LinearGaussianSSM(A, Q, I, 0.5 * I, np.zeros(d), I)
    ys = np.array(k["ys"]).reshape(-1, d)[:6]
    mus, Ps = m.kalman_filter(ys)
    mu, P = mus[-1], Ps[-1]
    st = _filter(m, ys, n, T=6)
    try:
        if pending:
            assert gen.maybe_resample(st, n)
        ess = gen.effective_sample_size(st)  # (pending: n, the equal weights' own)
        fc = gen.forecast(st, H)
    finally:
        st.close()
    for h in range(H):
        mu, P = A @ mu, A @ P @ A.T + Q
        dP = np.diag(P)
        s_mean, s_cov = np.sqrt(dP / ess), np.sqrt((np.outer(dP, dP) + P * P) / ess)
        print(f"k={h + 1} ess={ess:.0f} mean {(np.abs(fc.x_mean[h] - mu) / s_mean).max():.2f} sigma  "
              f"cov {(np.abs(fc.x_cov[h] - P) / s_cov).max():.2f} sigma")
        assert (np.abs(fc.x_mean[h] - mu) <= 6 * s_mean).all(), h
        assert (np.abs(fc.x_cov[h] - P) <= 6 * s_cov).all(), h


# ------------------------------------------------------------ 5. read-only
@pytest.mark.parametrize("pending", [False, True], ids=["weighted", "pending"])
def test_read_only(gh_ctx, pending):
    n = 20011
    m, ys = _model(), _observations()
    a, b = _filter(m, ys, n), _filter(m, ys, n)
    try:
        if pending:
            assert gen.maybe_resample(a, n) and gen.maybe_resample(b, n)
        snap = lambda st: (gen.get_log_weights(st), st.states(), gen.log_ml_estimate(st), st.t, *st.ess_history())
        before = snap(a)
        gen.forecast(a, 5, samples=True)
        gen.forecast(a, 11)
        assert all(_bits(x, y) for x, y in zip(before, snap(a)))
        for st in (a, b):  # one observed step on the filter that forecast and on its twin
            gen.particle_filter_step(st, (5,), (gen.UnknownChange(),), _obs_at(m, ys[4], 5))
        assert all(_bits(x, y) for x, y in zip(snap(a), snap(b)))
        assert gen.maybe_resample(a, n / 2) == gen.maybe_resample(b, n / 2)
        assert _bits(a.states(), b.states()) and np.array_equal(a.parents, b.parents)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------- 6. refusals
def test_refusals(gh_ctx):
    from gen_amd import _lib
    from tests.test_slots import count_model_inputs, count_obs

    lib = _lib.load()
    m, ys = _model(3), _observations(3)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        st = _init(m, ys, 64, ctx=ctx)
        with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
            gen.forecast(st, 2)
        out = np.empty((2, 3))
        assert lib.gh_pf_forecast(st.h, 2, None, _lib.dptr(out), None, None, None, None, None) == 7  # GH_E_STATE
        assert b"multi-rank" in lib.gh_last_error()
        st.close()
    finally:
        ctx.close()
    st = _init(m, ys, 64)
    try:
        _steps(st, m, ys, 1, 32)
        good = gen.forecast(st, 3)
        out = np.empty((65, 3))
        for H in (0, -1, 65, 1.5, True):
            with pytest.raises(gen.GenHipError, match=r"outside 1\.\.64"):
                gen.forecast(st, H)
        for H in (0, -1, 65):
            assert lib.gh_pf_forecast(st.h, H, None, _lib.dptr(out), None, None, None, None, None) == 1  # GH_E_INVAL
            assert b"outside 1..64" in lib.gh_last_error()
        assert lib.gh_pf_forecast(st.h, 3, None, None, None, None, None, None, None) == 1  # nothing to write
        assert b"null" in lib.gh_last_error()
        with pytest.raises(gen.GenHipError, match="GH_E_INVAL"):  # inputs to a model that takes none
            gen.forecast(st, 3, inputs=np.zeros((3, 3)))
        assert lib.gh_pf_forecast(st.h, 3, _lib.dptr(np.zeros((3, 3))), _lib.dptr(out), None, None, None, None,
                                  None) == 1
        again = gen.forecast(st, 3)  # the filter still works
        assert _bits(again.x_mean, good.x_mean) and _bits(again.y_cov, good.y_cov)
    finally:
        st.close()
    reg, rys = gen.BayesianLinearRegression.quickstart()
    st = gen.initialize_particle_filter(reg, (reg.xs,), reg.constraints(rys), 257, seed=SEED)
    try:
        with pytest.raises(gen.GenHipError, match="GH_E_INVAL"):
            gen.forecast(st, 1)
        out = np.empty((1, 2))
        assert lib.gh_pf_forecast(st.h, 1, None, _lib.dptr(out), None, None, None, None, None) == 1
        assert b"regression" in lib.gh_last_error()
    finally:
        st.close()
    mi = count_model_inputs()
    _, obs = count_obs()
    st = _init(mi, obs, 257)
    try:
        with pytest.raises(gen.GenHipError, match="GH_E_INVAL"):  # inputs missing
            gen.forecast(st, 2)
        bad = np.zeros((2, 2))
        bad[1, 0] = np.inf
        with pytest.raises(gen.GenHipError, match="non-finite"):
            gen.forecast(st, 2, inputs=bad)
        assert not np.isnan(gen.forecast(st, 2, inputs=np.zeros((2, 2))).x_mean).any()
    finally:
        st.close()
    hmm = gen.DiscreteHMM([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[1.0, 1.0], [0.0, 0.0]])
    st = gen.initialize_particle_filter(hmm, (1,), {hmm.obs_address(1): 0}, 257, seed=SEED)
    try:
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), {hmm.obs_address(2): 1})
        assert np.isneginf(gen.get_log_weights(st)).all()  # (an observation no state can emit)
        with pytest.raises(gen.GenHipError, match="GH_E_NUMERIC"):
            gen.forecast(st, 2)
    finally:
        st.close()


def test_custom_proposal_filter_forecasts_with_the_models_transition(gh_ctx):
    """A filter stepped with the LG-SSM's optimal proposal forecasts as its
    twin's unobserved default-proposal steps do."""
    n = 4097
    m, ys = _model(3), _observations(3)

    def make():
        st = gen.initialize_particle_filter(m, (1,), _obs_at(m, ys[0], 1), gen.OptimalProposal, (), n, seed=SEED)
        for t in (2, 3):
            gen.maybe_resample(st, n / 2)
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(m, ys[t - 1], t),
                                     gen.OptimalProposal, ())
        return st

    _draws_equal_steps(make, 3)
