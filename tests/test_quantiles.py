"""On-device weighted quantiles (gh_pf_quantiles, gh_quantiles.h) against the
host restatement of the header's definition, bit for bit.

The check everywhere: gen.quantiles(st, probs, t) has the bits of
reference_quantiles(st.states(t), gen.get_log_weights(st), probs)
(tests/test_quantiles_abi.py: Python integers for the weights and the ranks,
the oracle's exp, the total-order key).  No tolerance: the definition is on the
resampler's integer weights, whose sums do not depend on order.

The refusals "before init" and "d outside 1..16" of the C ABI cannot be
reached through a filter handle, so they are not exercised here.
"""
import json
import os

import numpy as np
import pytest

import gen_amd as gen
from tests.test_estimates import (LAYOUT_CASES, SEED, _bits, _hmm, _init, _kitagawa, _model, _observations, _slots,
                                  _steps)
from tests.test_quantiles_abi import reference_quantiles, reference_weights, total_order_key

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = [0, 0.05, 0.25, 0.5, 0.75, 0.95, 1]


def check(st, t=None, probs=PROBS, what=""):
    """quantiles(st, probs, t) with the bits of the host reference; returns them."""
    ref = reference_quantiles(st.states(t), gen.get_log_weights(st), probs)
    got = gen.quantiles(st, probs, t)
    assert got.shape == ref.shape == (len(probs), st.model.d), what
    assert _bits(got, ref), (what, t, got, ref)
    return got


# ------------------------------------------------------------------- cases
@pytest.mark.parametrize("d,n", LAYOUT_CASES)
def test_layouts_and_tails(gh_ctx, d, n):
    """Row tiles (d = 10) and pair tiles, full and partial last tiles, one block
    and several: after init and after 3 steps without a resample."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        for stage in ("init", "3 steps"):
            q = check(st, what=f"d={d} n={n} {stage}")
            if n == 1:
                assert all(_bits(row, st.states()[0]) for row in q)  # the particle, for every p
            if stage == "init":
                assert not any(_steps(st, m, ys, 3, 0))
    finally:
        st.close()


@pytest.mark.parametrize("d,n", [(10, 65), (9, 4097), (10, 20011), (10, 64)])
def test_pending_resample(gh_ctx, d, n):
    """Between a resample that fired and the next step: equal integer weights
    over duplicated particles, exact ties in value and in rank.  At n = 64 the
    cumulative weight of the k-th order statistic is p S exactly for p = k / 64:
    the inverse CDF picks the k-th, not the next."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 1, 0)
        assert gen.maybe_resample(st, n)
        lw = gen.get_log_weights(st)
        assert not lw.any()
        q = check(st, what=f"d={d} n={n} pending")
        assert _bits(q, reference_quantiles(st.states(), lw, PROBS, pending=True))
        if n == 64:
            ks = [1, 2, 17, 32, 33, 63, 64]
            qk = check(st, probs=[k / 64 for k in ks], what="k / 64")
            x = st.states()
            for k in range(d):
                col = x[np.argsort(total_order_key(x[:, k]), kind="stable"), k]
                assert _bits(qk[:, k], col[[i - 1 for i in ks]]), k  # the k-th order statistic
        _steps(st, m, ys, 1, 0)  # (the pending resample is consumed by this step)
        check(st, what=f"d={d} n={n} after the resampled step")
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
            check(st, t, what=f"d={d} earlier step")
    finally:
        st.close()
    st = _init(m, ys, n, record_history=False)
    try:
        _steps(st, m, ys, 2, n / 2)
        with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
            gen.quantiles(st, PROBS, 1)
        check(st, what=f"d={d} without history")
    finally:
        st.close()


def test_degenerate_weights(gh_ctx):
    """Most q_i are 0: every quantile is the value of a particle that carries
    weight, and Q(0) is the smallest of those, not the smallest state."""
    n = 4133
    m, ys = _model(), _observations(peaked=True)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 1, 0)
        x, lw = st.states(), gen.get_log_weights(st)
        w = np.array([v > 0 for v in reference_weights(lw)])
        assert 0 < np.count_nonzero(w) < n // 2
        q = check(st, what="degenerate")
        below = 0
        for k in range(x.shape[1]):
            keys, support = total_order_key(x[:, k]), total_order_key(x[w, k])
            assert np.isin(total_order_key(q[:, k]), support).all(), k
            assert total_order_key(q[:1, k])[0] == support.min() and total_order_key(q[-1:, k])[0] == support.max(), k
            below += int(keys.min() < support.min())
        assert below  # (some component's smallest state weighs nothing: the case is not vacuous)
    finally:
        st.close()


def _switching():
    from tests.test_slots import switching_model

    m = switching_model()
    _, ys = m.simulate(4, np.random.default_rng(4))
    return m, [dict(y) for y in ys]


@pytest.mark.parametrize("family", [_kitagawa, _hmm, _slots, _switching],
                         ids=["kitagawa", "hmm", "slots", "switching"])
def test_other_families(gh_ctx, family):
    """The quantile is of the stored doubles (the HMM's: the class index, with
    massive ties)."""
    m, ys = family()
    st = _init(m, ys, 4097)
    try:
        _steps(st, m, ys, 3, 4097 / 2)
        q = check(st, what=family.__name__)
        if family is _hmm:
            assert np.array_equal(q, np.round(q))
    finally:
        st.close()


@pytest.mark.parametrize("d,n_probs", [(16, 16), (16, 1), (10, 16), (1, 16), (3, 1)])
def test_probability_count(gh_ctx, d, n_probs):
    """1 and 16 probabilities; 16 distinct ones at d = 16 is the largest pair
    count: every chunk of the histogram grid."""
    n = 4097
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 2, 0)
        probs = [0.5] if n_probs == 1 else [(3 * j + 1) / 47 for j in range(15)] + [1.0]
        assert len(set(probs)) == n_probs
        check(st, probs=probs, what=f"d={d} n_probs={n_probs}")
    finally:
        st.close()


def test_convenience_forms(gh_ctx):
    n = 4097
    m, ys = _model(), _observations()
    st = _init(m, ys, n)
    try:
        _steps(st, m, ys, 3, n / 2)
        for t in (None, 2):
            q = check(st, t, what="convenience")
            assert _bits(gen.weighted_median(st, t), q[3])
            lo, hi = gen.credible_interval(st, t=t)  # (level 0.9: its own probabilities, (1 - 0.9) / 2 is not 0.05)
            tails = gen.quantiles(st, [(1 - 0.9) / 2, (1 + 0.9) / 2], t)
            assert _bits(lo, tails[0]) and _bits(hi, tails[1])
            lo, hi = gen.credible_interval(st, 0.5, t)
            assert _bits(lo, q[2]) and _bits(hi, q[4])
            lo, hi = gen.credible_interval(st, 1, t)
            assert _bits(lo, q[0]) and _bits(hi, q[6])
            assert (np.diff(q, axis=0) >= 0).all()  # non-decreasing in p
            mean = gen.estimate(st, t, cov=False).mean
            assert (q[0] <= mean).all() and (mean <= q[6]).all()
    finally:
        st.close()


def test_reproducible_and_read_only(gh_ctx):
    """Two calls return the same bits, and a twin filter that never called
    quantiles has the same states, weights, parents and log-ML after one more
    maybe_resample + step."""
    n = 20011
    m, ys = _model(), _observations()
    a, b = _init(m, ys, n), _init(m, ys, n)
    try:
        for st in (a, b):
            _steps(st, m, ys, 3, n / 2)
        before = (gen.get_log_weights(a), a.states(), gen.log_ml_estimate(a))
        q1, q2, q3 = gen.quantiles(a, PROBS), gen.quantiles(a, PROBS), gen.quantiles(a, PROBS, 2)
        assert _bits(q1, q2) and _bits(gen.quantiles(a, PROBS, 2), q3)
        after = (gen.get_log_weights(a), a.states(), gen.log_ml_estimate(a))
        assert all(_bits(u, v) for u, v in zip(before, after))
        assert _steps(a, m, ys, 1, n) == _steps(b, m, ys, 1, n) == [True]
        assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), gen.get_log_weights(b))
        assert np.array_equal(a.parents, b.parents)
        assert _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b))
        for t in range(1, a.t + 1):
            assert _bits(a.states(t), b.states(t)), t
        assert _bits(gen.quantiles(a, PROBS), gen.quantiles(b, PROBS))
    finally:
        a.close()
        b.close()


def test_refusals(gh_ctx):
    from gen_amd import _lib

    m, ys = _model(3), _observations(3)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        st = _init(m, ys, 64, ctx=ctx)
        for f in (lambda s: gen.quantiles(s, PROBS), gen.weighted_median, gen.credible_interval):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f(st)
        st.close()
    finally:
        ctx.close()
    st = _init(m, ys, 64)
    try:
        _steps(st, m, ys, 1, 32)
        good = gen.quantiles(st, PROBS)
        for probs in ([], [0.5] * 17):
            with pytest.raises(gen.GenHipError, match=r"outside 1\.\.16"):
                gen.quantiles(st, probs)
        for p in (-0.1, 1.5, float("nan")):
            with pytest.raises(gen.GenHipError, match=r"outside \[0, 1\]"):
                gen.quantiles(st, [0.5, p])
        for t in (0, -1, 3, 1.5, True):
            with pytest.raises(gen.GenHipError, match=r"outside 1\.\.2"):
                gen.quantiles(st, PROBS, t)
        for level in (0, 1.5, -0.5, float("nan")):
            with pytest.raises(gen.GenHipError, match=r"outside \(0, 1\]"):
                gen.credible_interval(st, level)
        # at the ABI
        lib = _lib.load()
        out = np.empty((17, 3))
        one = np.array([0.5])
        assert lib.gh_pf_quantiles(st.h, 3, 1, _lib.dptr(one), _lib.dptr(out)) == 1
        assert b"outside 1..2" in lib.gh_last_error()
        for k in (0, 17):
            assert lib.gh_pf_quantiles(st.h, 0, k, _lib.dptr(np.full(17, 0.5)), _lib.dptr(out)) == 1
            assert b"outside 1..16" in lib.gh_last_error()
        assert lib.gh_pf_quantiles(st.h, 0, 1, None, _lib.dptr(out)) == 1
        assert lib.gh_pf_quantiles(st.h, 0, 1, _lib.dptr(one), None) == 1
        for p in (-0.1, 1.5, float("nan")):
            assert lib.gh_pf_quantiles(st.h, 0, 1, _lib.dptr(np.array([p])), _lib.dptr(out)) == 1
            assert b"outside [0, 1]" in lib.gh_last_error()
        assert _bits(gen.quantiles(st, PROBS), good)  # the filter still works
    finally:
        st.close()
    hmm = gen.DiscreteHMM([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[1.0, 1.0], [0.0, 0.0]])
    st = gen.initialize_particle_filter(hmm, (1,), {hmm.obs_address(1): 0}, 257, seed=SEED)
    try:
        assert gen.quantiles(st, [0.5]).shape == (1, 1)  # (observation 0 has probability 1 in both states)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), {hmm.obs_address(2): 1})
        assert np.isneginf(gen.get_log_weights(st)).all()
        with pytest.raises(gen.GenHipError, match="GH_E_NUMERIC"):
            gen.quantiles(st, [0.5])
    finally:
        st.close()


def test_median_against_the_kalman_mean(gh_ctx):
    """The golden lg2 model: the posterior is Gaussian, so its median is its
    mean.  |median_k - mu_k| over the sample median's standard error,
    1.2533 sqrt(P_kk / ess), stays below 8 (wide: after a resample the ESS
    overstates the number of independent particles).  The ratio is printed."""
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "kalman.json")))["lg2"]
    d, n = k["d"], 20011
    I = np.eye(d)
    m = gen.LinearGaussianSSM(np.array(k["A"]), 0.1 * I, I, 0.5 * I, np.zeros(d), I)
    ys = np.array(k["ys"]).reshape(-1, d)
    mus, Ps = m.kalman_filter(ys)
    st = _init(m, ys, n)
    try:
        for t in range(1, len(ys) + 1):
            if t > 1:
                _steps(st, m, ys, 1, n / 2)
            med, ess = gen.weighted_median(st), gen.estimate(st, cov=False).ess
            se = 1.2533 * np.sqrt(np.diag(Ps[t - 1]) / ess)
            ratio = np.abs(med - mus[t - 1]) / se
            print(f"t={t} ess={ess:.0f} |median - Kalman mean| / se = {ratio.max():.2f}")
            assert (ratio < 8).all(), (t, ratio)
    finally:
        st.close()
