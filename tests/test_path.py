"""Every step's summary in one walk (gh_pf_estimate_path, gh_pf_quantiles_path,
gh_path.h) against the per-step calls, bit for bit, and the genealogy's
diagnostics against their host restatement.

Equalities, everywhere: for every step t of the range, estimate_path's mean
and cov have the bits of estimate(st, t)'s and quantiles_path's row the bits
of quantiles(st, PROBS, t).  No tolerance: the path kernels take the same
weights, the same grid and the same order of every sum.

Diagnostics (continuous families, where distinct particles hold distinct
rows): `distinct` equals reference_path_diagnostics' count exactly
(tests/test_path_abi.py: the rows of states(t) grouped by their bits, the
integer weights summed as Python ints) and `ess` is within relative
(n + 16) 2^-52 of its S^2 / sum m^2.  Derived, not tuned, with u = 2^-53: each
m and S rounds once on conversion to a double (u), each square once more (3 u
with the conversions), an any-order sum of at most n positive terms adds
(n - 1) u, the division u.

The filters are built with an explicit resample pattern, so that both kinds of
step boundary (a resample preceded the step, or none did) occur in every walk:
a maybe_resample(thr) before each further step with thr = 0, n, 0, n, 0.  The
threshold n fires (the ESS of unequal weights is below n) and 0 does not; a
single particle's ESS is 1 = n, which is not below n, so at n = 1 nothing fires.
"""
import numpy as np
import pytest

import gen_amd as gen
from tests.test_estimates import SEED, _bits, _hmm, _init, _kitagawa, _model, _obs_at, _observations, _slots
from tests.test_path_abi import reference_path_diagnostics
from tests.test_quantiles_abi import reference_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PROBS = [0, 0.05, 0.25, 0.5, 0.75, 0.95, 1]
SIZES = [1, 64, 65, 257, 4097, 20011]
LAYOUT_CASES = [(d, n) for d in (10, 9) for n in SIZES] + [(d, n) for d in (1, 3, 16) for n in (65, 4097)]


def _pattern(st, model, ys, steps=5):
    """`steps` further steps, maybe_resample(thr) before each with thr = 0, n,
    0, n, 0; the decisions are asserted."""
    n = st.n_local
    for i in range(steps):
        t = st.t + 1
        fire = i % 2 == 1
        assert gen.maybe_resample(st, n if fire else 0) == (fire and n > 1), (i, n)
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(model, ys[t - 1], t))


def check_equal(st, what=""):
    """The path calls against the per-step ones for every step; returns the path estimate."""
    T, d = st.t, st.model.d
    path = gen.estimate_path(st)
    qp = gen.quantiles_path(st, PROBS)
    assert path.ess.shape == path.distinct.shape == (T,) and path.distinct.dtype == np.int64, what
    assert path.mean.shape == (T, d) and path.cov.shape == (T, d, d) and qp.shape == (T, len(PROBS), d), what
    for t in range(1, T + 1):
        e = gen.estimate(st, t)
        assert _bits(path.mean[t - 1], e.mean), (what, t)
        assert _bits(path.cov[t - 1], e.cov), (what, t)
        assert _bits(qp[t - 1], gen.quantiles(st, PROBS, t)), (what, t)
    return path


def check_diagnostics(st, path, pending=False, what=""):
    n, T = st.n_local, st.t
    q = reference_weights(gen.get_log_weights(st), pending)
    worst = 0.0
    for t in range(1, T + 1):
        distinct, ess = reference_path_diagnostics(st.states(t), q)
        assert path.distinct[t - 1] == distinct, (what, t, path.distinct, distinct)
        err = abs(path.ess[t - 1] - ess) / ess
        worst = max(worst, err / ((n + 16) * EPS))
        assert err <= (n + 16) * EPS, (what, t, path.ess[t - 1], ess)
    print(f"{what} n={n}: distinct {path.distinct.tolist()}  ess error / bound {worst:.3g}")
    assert (np.diff(path.distinct) >= 0).all(), (what, path.distinct)
    assert (path.ess <= path.distinct).all(), (what, path.ess, path.distinct)
    if pending:
        rows = {r.tobytes() for r in np.ascontiguousarray(st.states())}
        assert path.distinct[T - 1] == len(rows), what
    else:
        assert path.distinct[T - 1] == sum(1 for v in q if v > 0), what


# ------------------------------------------------------------------- cases
@pytest.mark.parametrize("d,n", LAYOUT_CASES)
def test_layouts_and_tails(gh_ctx, d, n):
    """Row tiles (d = 10) and pair tiles, full and partial last tiles, one block
    and several, across step boundaries of both kinds."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        _pattern(st, m, ys)
        path = check_equal(st, what=f"d={d} n={n}")
        check_diagnostics(st, path, what=f"d={d} n={n}")
        if n == 1:
            assert path.distinct.tolist() == [1] * st.t and path.ess.tolist() == [1.0] * st.t
    finally:
        st.close()


def test_ranges_and_forms(gh_ctx):
    """cov=False, a sub-range, the current step alone, and the convenience forms."""
    n = 4097
    m, ys = _model(), _observations()
    st = _init(m, ys, n)
    try:
        _pattern(st, m, ys)
        T = st.t
        full, qfull = gen.estimate_path(st), gen.quantiles_path(st, PROBS)
        lean = gen.estimate_path(st, cov=False)
        assert lean.cov is None and _bits(lean.mean, full.mean) and _bits(lean.ess, full.ess)
        assert np.array_equal(lean.distinct, full.distinct)
        sub, qsub = gen.estimate_path(st, 3, 5), gen.quantiles_path(st, PROBS, 3, 5)
        assert sub.mean.shape == (3, 10) and qsub.shape == (3, len(PROBS), 10)
        assert _bits(sub.mean, full.mean[2:5]) and _bits(sub.cov, full.cov[2:5]) and _bits(sub.ess, full.ess[2:5])
        assert np.array_equal(sub.distinct, full.distinct[2:5]) and _bits(qsub, qfull[2:5])
        last, e = gen.estimate_path(st, T, T), gen.estimate(st)
        assert _bits(last.mean[0], e.mean) and _bits(last.cov[0], e.cov)
        assert _bits(gen.estimate_path(st, T).mean, last.mean)  # (t1 defaults to the current step)
        assert _bits(gen.quantiles_path(st, PROBS, T, T)[0], gen.quantiles(st, PROBS))
        assert _bits(gen.median_path(st), qfull[:, 3]) and _bits(gen.median_path(st, 3, 5), qfull[2:5, 3])
        lo, hi = gen.credible_band(st)  # (level 0.9: credible_interval's probabilities)
        for t in range(1, T + 1):
            a, b = gen.credible_interval(st, t=t)
            assert _bits(lo[t - 1], a) and _bits(hi[t - 1], b), t
        lo, hi = gen.credible_band(st, 0.5, 2, 4)
        assert _bits(lo, qfull[1:4, 2]) and _bits(hi, qfull[1:4, 4])
    finally:
        st.close()


@pytest.mark.parametrize("d,n", [(10, 65), (9, 4097), (10, 20011)])
def test_pending_resample(gh_ctx, d, n):
    """Between a resample that fired and the next step the walk starts through
    the pending resample's ancestors and every weight is 2^shift."""
    m, ys = _model(d), _observations(d)
    st = _init(m, ys, n)
    try:
        _pattern(st, m, ys, 3)
        assert gen.maybe_resample(st, n)
        assert not gen.get_log_weights(st).any()
        path = check_equal(st, what=f"d={d} pending")
        check_diagnostics(st, path, pending=True, what=f"d={d} pending")
        assert path.distinct[-1] < n  # (the resample dropped some particles)
        t = st.t + 1
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(m, ys[t - 1], t))
        path = check_equal(st, what=f"d={d} after the resampled step")
        check_diagnostics(st, path, what=f"d={d} after the resampled step")
    finally:
        st.close()


def test_degenerate_weights(gh_ctx):
    """Most q_i are 0: only the ancestors of particles that carry weight count."""
    n = 4133
    m, ys = _model(), _observations(peaked=True)
    st = _init(m, ys, n)
    try:
        gen.maybe_resample(st, 0)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), _obs_at(m, ys[1], 2))
        q = reference_weights(gen.get_log_weights(st))
        live = sum(1 for v in q if v > 0)
        assert 0 < live < n // 2  # (the case is not vacuous)
        path = check_equal(st, what="degenerate")
        check_diagnostics(st, path, what="degenerate")
        assert path.distinct.tolist() == [live, live]  # (no resample: every particle is its own ancestor)
    finally:
        st.close()


def test_batched_run(gh_ctx):
    """After run_particle_filter the last resample's ancestors exist only as marks."""
    n = 20011
    m, ys = _model(), _observations()
    st = _init(m, ys, n)
    try:
        gen.run_particle_filter(st, list(ys[1:6]), ess_threshold=n / 2)
        path = check_equal(st, what="after run_particle_filter")
        check_diagnostics(st, path, what="after run_particle_filter")
        assert path.distinct[0] < n  # (a resample fired somewhere along the run)
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
    m, ys = family()
    st = _init(m, ys, 4097)
    try:
        _pattern(st, m, ys, 3)
        path = check_equal(st, what=family.__name__)
        if family is _kitagawa:
            check_diagnostics(st, path, what="kitagawa")
    finally:
        st.close()


def test_regression(gh_ctx):
    """T = 1: a path of length 1."""
    m, ys = gen.BayesianLinearRegression.quickstart()
    st = gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys), 4097, seed=SEED)
    try:
        path = check_equal(st, what="regression")
        assert path.mean.shape == (1, 2) and path.cov.shape == (1, 2, 2)
    finally:
        st.close()


def test_reproducible_and_read_only(gh_ctx):
    """Two calls return the same bits, and a twin filter that was never queried
    agrees with the queried one afterwards, and after two more steps with a
    resample."""
    n = 20011
    m, ys = _model(), _observations()
    a, b = _init(m, ys, n), _init(m, ys, n)

    def same():
        assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), gen.get_log_weights(b))
        assert _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b))
        assert np.array_equal(a.parents, b.parents)
        for t in range(1, a.t + 1):
            assert _bits(a.states(t), b.states(t)), t

    try:
        for st in (a, b):
            _pattern(st, m, ys, 3)
        p1, q1 = gen.estimate_path(a), gen.quantiles_path(a, PROBS)
        p2, q2 = gen.estimate_path(a), gen.quantiles_path(a, PROBS)
        assert _bits(p1.ess, p2.ess) and np.array_equal(p1.distinct, p2.distinct)
        assert _bits(p1.mean, p2.mean) and _bits(p1.cov, p2.cov) and _bits(q1, q2)
        same()
        # a pending resample is left pending
        assert gen.maybe_resample(a, n) and gen.maybe_resample(b, n)
        gen.estimate_path(a), gen.quantiles_path(a, PROBS)
        for st in (a, b):
            t = st.t + 1
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(m, ys[t - 1], t))
            _pattern(st, m, ys, 1)
        same()
        pa, pb = gen.estimate_path(a), gen.estimate_path(b)
        assert _bits(pa.ess, pb.ess) and np.array_equal(pa.distinct, pb.distinct) and _bits(pa.cov, pb.cov)
    finally:
        a.close()
        b.close()


def test_refusals(gh_ctx):
    from gen_amd import _lib

    m, ys = _model(3), _observations(3)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        st = _init(m, ys, 64, ctx=ctx)
        for f in (gen.estimate_path, lambda s: gen.quantiles_path(s, PROBS), gen.median_path, gen.credible_band):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f(st)
        st.close()
    finally:
        ctx.close()
    st = _init(m, ys, 64)
    try:
        _pattern(st, m, ys, 2)
        T = st.t
        good = gen.estimate_path(st)
        for t0, t1 in ((0, None), (1, T + 1), (3, 2), (1.5, None), (True, None), (1, -1)):
            with pytest.raises(gen.GenHipError, match=r"GH_E_INVAL.*outside 1\.\.3"):
                gen.estimate_path(st, t0, t1)
            with pytest.raises(gen.GenHipError, match=r"GH_E_INVAL.*outside 1\.\.3"):
                gen.quantiles_path(st, PROBS, t0, t1)
        for probs in ([], [0.5] * 17):
            with pytest.raises(gen.GenHipError, match=r"outside 1\.\.16"):
                gen.quantiles_path(st, probs)
        for p in (-0.1, 1.5, float("nan")):
            with pytest.raises(gen.GenHipError, match=r"outside \[0, 1\]"):
                gen.quantiles_path(st, [0.5, p])
        for level in (0, 1.5, float("nan")):
            with pytest.raises(gen.GenHipError, match=r"outside \(0, 1\]"):
                gen.credible_band(st, level)
        # at the ABI
        lib = _lib.load()
        pi = np.empty(4, dtype=np.int64).ctypes.data_as(_lib.POINTER(_lib.c_int64))
        out, one = np.empty((4, 17, 3)), np.array([0.5])
        for t0, t1 in ((0, 0), (1, T + 1), (3, 2)):
            assert lib.gh_pf_estimate_path(st.h, t0, t1, _lib.dptr(out), pi, None, None) == 1
            assert b"outside 1..3" in lib.gh_last_error()
            assert lib.gh_pf_quantiles_path(st.h, t0, t1, 1, _lib.dptr(one), _lib.dptr(out)) == 1
            assert b"outside 1..3" in lib.gh_last_error()
        assert lib.gh_pf_estimate_path(st.h, 1, 0, None, None, None, None) == 1
        for k in (0, 17):
            assert lib.gh_pf_quantiles_path(st.h, 1, 0, k, _lib.dptr(np.full(17, 0.5)), _lib.dptr(out)) == 1
            assert b"outside 1..16" in lib.gh_last_error()
        assert lib.gh_pf_quantiles_path(st.h, 1, 0, 1, None, _lib.dptr(out)) == 1
        assert lib.gh_pf_quantiles_path(st.h, 1, 0, 1, _lib.dptr(one), None) == 1
        assert lib.gh_pf_quantiles_path(st.h, 1, 0, 1, _lib.dptr(np.array([1.5])), _lib.dptr(out)) == 1
        assert b"outside [0, 1]" in lib.gh_last_error()
        again = gen.estimate_path(st)  # the filter still works
        assert _bits(again.mean, good.mean) and np.array_equal(again.distinct, good.distinct)
    finally:
        st.close()
    st = _init(m, ys, 64, record_history=False)
    try:
        _pattern(st, m, ys, 2)
        T = st.t
        for f in (lambda: gen.estimate_path(st), lambda: gen.quantiles_path(st, PROBS),
                  lambda: gen.estimate_path(st, T - 1, T)):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f()
        e = gen.estimate(st)
        only = gen.estimate_path(st, T, T)
        assert _bits(only.mean[0], e.mean) and _bits(only.cov[0], e.cov)
        assert _bits(gen.quantiles_path(st, PROBS, T, T)[0], gen.quantiles(st, PROBS))
    finally:
        st.close()
    hmm = gen.DiscreteHMM([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[1.0, 1.0], [0.0, 0.0]])
    st = gen.initialize_particle_filter(hmm, (1,), {hmm.obs_address(1): 0}, 257, seed=SEED)
    try:
        assert gen.estimate_path(st).distinct.tolist() == [257]  # (observation 0 has probability 1 in both states)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), {hmm.obs_address(2): 1})
        assert np.isneginf(gen.get_log_weights(st)).all()
        for f in (lambda: gen.estimate_path(st), lambda: gen.quantiles_path(st, [0.5])):
            with pytest.raises(gen.GenHipError, match="GH_E_NUMERIC"):
                f()
    finally:
        st.close()
