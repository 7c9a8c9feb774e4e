"""The weight history (record_weights), the backward weights and backward
simulation (gh_pf_get_log_weights_at, gh_pf_backward_weights, gh_pf_smooth;
gh_smooth.h) on the device.

1. the recorded weights of every step have the bits a twin filter's weights had
   right after that step, and recording changes nothing else;
2. the backward weights are, bit for bit, the recorded weight plus the latent
   score column of gh_pf_get_scores (which tests/test_scores.py pins to the
   oracle bit for bit);
3. every pick of `smooth` is the host restatement's (tests/test_smooth_abi.py:
   Python integers, the oracle's exp and Philox) on the device's own backward
   weights, and every state it returns has the bits of the picked particle;
4. impossible transitions (-inf) are never picked;
5. the call is reproducible and leaves the filter as it was;
6. the smoothed means agree with the closed form (RTS) on a 1-D LG model, and
   the draws keep more distinct ancestors at t = 1 than the genealogy does;
7. the refusals.

"Step t's particles" are the rows of the filter's states as step t left them
(what states() returned right after it, before any resample): the tests keep
them as they filter, since states(t) of a later filter follows the surviving
genealogy instead.
"""
import numpy as np
import pytest

import gen_amd as gen
from gen_amd import _lib
from tests.test_csmc import _lg1, _rts_means
from tests.test_estimates import LAYOUT_CASES, SEED, _bits, _hmm, _init, _kitagawa, _model, _obs_at, _observations, _slots
from tests.test_quantiles_abi import reference_weights
from tests.test_smooth_abi import reference_pick, reference_pick_q, reference_u53

pytestmark = pytest.mark.gpu

CHUNK = 64  # gh_smooth.h kBsChunk: the trajectories of one block


def _library():
    from tests.test_slots import library_obs

    return library_obs("m1")


def _switching():
    from tests.test_slots import slds_obs

    return slds_obs()


def _with_inputs():
    from tests.test_slots import count_inputs, count_model_inputs, count_obs

    return count_model_inputs(), count_obs()[1], count_inputs()


def _recorded(m, ys, n, T=4, inputs=None, last_thr=None, **kw):
    """A filter at step T made with record_weights (a maybe_resample(n / 2)
    before each step; last_thr: the threshold before the last one), with every
    step's rows and weights as the step left them."""
    st = _init(m, ys, n, record_weights=True, **kw)
    rows, lws = {1: st.states()}, {1: gen.get_log_weights(st)}
    for t in range(2, T + 1):
        gen.maybe_resample(st, n / 2 if t < T or last_thr is None else last_thr)
        na = (t,) if inputs is None or inputs[t - 1] is None else (t, inputs[t - 1])
        gen.particle_filter_step(st, na, (gen.UnknownChange(),) * len(na), _obs_at(m, ys[t - 1], t))
        rows[t], lws[t] = st.states(), gen.get_log_weights(st)
    return st, rows, lws


# ------------------------------------------------------ 1. the weight history
@pytest.mark.parametrize("d,n", LAYOUT_CASES)
def test_weight_history(gh_ctx, d, n):
    """Filter a records, its twin b does not: the same bits in states, weights,
    parents and log-ML at every step, and a's recorded weights of step t are
    the weights b had right after its step t."""
    m, ys = _model(d), _observations(d)
    a, b = _init(m, ys, n, record_weights=True), _init(m, ys, n)
    try:
        seen = {1: gen.get_log_weights(b)}
        for t in range(2, 5):
            assert gen.maybe_resample(a, n / 2) == gen.maybe_resample(b, n / 2)
            for st in (a, b):
                gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(m, ys[t - 1], t))
            seen[t] = gen.get_log_weights(b)
            assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), seen[t]), t
            assert np.array_equal(a.parents, b.parents), t
            assert _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b)), t
            for s in range(1, t + 1):  # nothing recorded earlier moved
                assert _bits(gen.get_log_weights(a, s), seen[s]), (t, s)
        with pytest.raises(gen.GenHipError) as e:
            gen.get_log_weights(b, 2)
        assert e.value.code == 7
        assert _bits(gen.get_log_weights(b, 4), seen[4])  # the current step needs no history
    finally:
        a.close()
        b.close()


def test_weight_history_of_a_conditional_filter(gh_ctx):
    """The pin launches write particle 0's weight after the step kernel: the snapshot follows them."""
    m = gen.LinearGaussianSSM.benchmark(4)
    xs, ys = m.simulate(5, np.random.default_rng(6))
    ref = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1) * 0.9
    n = 3001
    mk = lambda **kw: gen.initialize_conditional_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, n, ref[0],
                                                                 seed=17, **kw)
    a, b = mk(record_weights=True), mk()
    try:
        seen = {1: gen.get_log_weights(b)}
        for t in range(2, len(ys) + 1):
            assert gen.maybe_resample(a, n / 2) == gen.maybe_resample(b, n / 2)
            for st in (a, b):
                gen.conditional_particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]},
                                                     ref[t - 1])
            seen[t] = gen.get_log_weights(b)
            assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), seen[t]), t
        for t, lw in seen.items():
            assert _bits(gen.get_log_weights(a, t), lw), t
    finally:
        a.close()
        b.close()


# ------------------------------------------------------ 2. the backward weights
def _lg(d):
    return lambda: (_model(d), _observations(d))


def _lg_shaped(d, dense_q, dy):
    """An LG model of a chosen structure (the benchmark's Q and H are diagonal,
    LGModel<d, 3>): a dense chol(Q) runs the score's forward substitution
    (structures 0 and 2), dy != d or a dense H the general observation
    (structures 0 and 1)."""
    def make():
        rng = np.random.default_rng(40 + d)
        A = 0.9 * np.eye(d) + 0.05 * rng.standard_normal((d, d))
        G = 0.3 * rng.standard_normal((d, d))
        Q = 0.1 * np.eye(d) + (G @ G.T if dense_q else 0.0)
        H = np.eye(d) if dy == d else rng.standard_normal((dy, d))
        m = gen.LinearGaussianSSM(A, Q, H, 0.5 * np.eye(dy), np.zeros(d), np.eye(d), b=0.1 * rng.standard_normal(d))
        _, ys = m.simulate(7, np.random.default_rng(5))
        return m, np.array(ys, dtype=np.float64)
    return make


FAMILIES = {"lg10-dense": _lg_shaped(10, True, 4), "lg3-denseQ-diagH": _lg_shaped(3, True, 3),
            "lg3-diagQ-denseH": _lg_shaped(3, False, 2), "lg1": _lg(1), "lg2": _lg(2), "lg9": _lg(9), "lg10": _lg(10), "lg16": _lg(16), "kitagawa": _kitagawa,
            "hmm": _hmm, "slots": _slots, "library": _library, "switching": _switching, "inputs": _with_inputs}


@pytest.mark.parametrize("n", [65, 257, 4097])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_weights_equal_the_score_columns(gh_ctx, family, n):
    """T = t + 1 = 4 with a resample before the last step, so that
    gh_pf_get_parents names the parents step T consumed: for a current particle
    j with parent a, b_a for x_next = x_T^j is lw_t[a] + the latent score of j's
    step T, one fp64 add."""
    m, ys, *u = FAMILIES[family]()
    st, rows, lws = _recorded(m, ys, n, T=4, inputs=u[0] if u else None, last_thr=n)
    try:
        t = 3
        did = st.ess_history()[1]
        assert did[t - 1], "the resample before the last step fired"
        parents, x = st.parents, st.states()
        assert _bits(x, rows[4])
        lw = gen.get_log_weights(st, t)
        assert _bits(lw, lws[t])
        lat = gen.get_traces(st).scores(per_step=True)[1][t][0]
        js = sorted({j for j in (0, 63, 64, 127, 255, 256, n - 1) if j < n})
        for j in js:
            a = int(parents[j])
            b = gen.backward_weights(st, t, x[j])
            assert b.shape == (n,)
            assert _bits(b[a], lw[a] + lat[j]), (family, n, j, a, b[a], lw[a] + lat[j])
    finally:
        st.close()


def test_backward_weights_without_a_resample(gh_ctx):
    """No resample before the last step: every particle is its own parent."""
    m, ys = _model(10), _observations(10)
    n = 257
    st, rows, lws = _recorded(m, ys, n, T=3, last_thr=0)
    try:
        assert not st.ess_history()[1][1]
        lat = gen.get_traces(st).scores(per_step=True)[1][2][0]
        for j in (0, 64, 256):
            assert _bits(gen.backward_weights(st, 2, rows[3][j])[j], lws[2][j] + lat[j]), j
    finally:
        st.close()


# ----------------------------------------------------------- 3. the selection
def _check_selection(st, rows, M, seed, t0=1, pending=False):
    n, T = st.n_local, st.t
    sm = gen.smooth(st, M, seed=seed, t0=t0)
    L = T - t0 + 1
    assert sm.xs.shape == (L, M, st.model.d) and sm.idx.shape == (L, M) and sm.idx.dtype == np.int32
    assert (sm.idx >= 0).all() and (sm.idx < n).all()
    for t in range(t0, T + 1):  # every state has the bits of the picked particle of its step
        assert _bits(sm.xs[t - t0], rows[t][sm.idx[t - t0]]), t
    # the start: the current weights (equal while a resample is pending, on the resampled particles)
    q = reference_weights(gen.get_log_weights(st), pending)
    anc = st.parents if pending else np.arange(n)
    checked = 0
    for m in range(M):
        assert sm.idx[T - t0, m] == anc[reference_pick_q(q, reference_u53(seed, m, T))], ("start", m)
        checked += 1
    for t in range(T - 1, t0 - 1, -1):
        for m in range(M):
            b = gen.backward_weights(st, t, sm.xs[t + 1 - t0, m])
            assert sm.idx[t - t0, m] == reference_pick(b, reference_u53(seed, m, t), n), (t, m)
            checked += 1
    assert checked == L * M
    return sm


@pytest.mark.parametrize("M", [1, 3, 70])
@pytest.mark.parametrize("n", [65, 256, 257, 4097])
def test_selection_shapes(gh_ctx, n, M):
    m, ys = _model(10), _observations(10)
    st, rows, _ = _recorded(m, ys, n)
    try:
        _check_selection(st, rows, M, seed=5 + M)
    finally:
        st.close()


@pytest.mark.parametrize("n,M", [(20011, 3), (257, CHUNK + 1), (257, 1025)],
                         ids=["many-blocks", "chunk+1", "more-than-a-launch"])
def test_selection_larger_shapes(gh_ctx, n, M):
    """The block scan across many blocks; one trajectory past a chunk; more
    trajectories than one launch takes (1024), so the host loops."""
    m, ys = _model(9), _observations(9)
    st, rows, _ = _recorded(m, ys, n)
    try:
        _check_selection(st, rows, M, seed=77)
    finally:
        st.close()


@pytest.mark.parametrize("family", ["lg9", "lg10-dense", "lg3-denseQ-diagH", "kitagawa", "hmm", "switching", "slots", "library", "inputs"])
def test_selection_of_other_families(gh_ctx, family):
    m, ys, *u = FAMILIES[family]()
    st, rows, _ = _recorded(m, ys, 4097 if family in ("kitagawa", "hmm") else 257, inputs=u[0] if u else None)
    try:
        _check_selection(st, rows, 3, seed=11)
    finally:
        st.close()


@pytest.mark.parametrize("d,n", [(10, 4097), (9, 257)])
def test_selection_with_a_resample_pending(gh_ctx, d, n):
    m, ys = _model(d), _observations(d)
    st, rows, _ = _recorded(m, ys, n)
    try:
        assert gen.maybe_resample(st, n)
        assert not gen.get_log_weights(st).any()
        sm = _check_selection(st, rows, 70, seed=3, pending=True)
        # the start's states are the resampled particles'
        cur = st.states()
        assert all(any(_bits(x, c) for c in cur) for x in sm.xs[-1][:5])
    finally:
        st.close()


def test_selection_from_a_later_step_and_at_one_step(gh_ctx):
    m, ys = _model(10), _observations(10)
    st, rows, _ = _recorded(m, ys, 257)
    one = _init(m, ys, 257)  # T = 1: the start draw alone, no weight history needed
    try:
        a = _check_selection(st, rows, 70, seed=9, t0=3)
        full = gen.smooth(st, 70, seed=9)
        assert _bits(a.xs, full.xs[2:]) and np.array_equal(a.idx, full.idx[2:])  # (the same uniforms, the same picks)
        last = _check_selection(st, rows, 3, seed=9, t0=4)
        assert np.array_equal(last.idx[0], full.idx[3, :3])
        _check_selection(one, {1: one.states()}, 70, seed=1)
    finally:
        st.close()
        one.close()


# --------------------------------------------------- 4. -inf everywhere but one
def test_permutation_hmm_picks_the_only_preimage(gh_ctx):
    """z_t = perm(z_{t-1}) with probability 1: of a drawn z_{t+1} only the
    particles at perm^-1(z_{t+1}) have a finite backward weight."""
    perm = [1, 2, 3, 0]
    T_ = np.zeros((4, 4))
    for prev, new in enumerate(perm):
        T_[new, prev] = 1.0
    E = np.array([[0.4, 0.3, 0.2, 0.1], [0.1, 0.2, 0.3, 0.4], [0.5, 0.5, 0.5, 0.5]])
    E /= E.sum(axis=0)
    m = gen.DiscreteHMM([0.25, 0.25, 0.25, 0.25], T_, E)
    ys = [0, 1, 2, 0, 1]
    st, rows, _ = _recorded(m, ys, 1000, T=5)
    try:
        sm = gen.smooth(st, 300, seed=4)
        z = sm.xs[:, :, 0].astype(int)
        for t in range(4):
            assert np.array_equal(z[t + 1], np.array(perm)[z[t]]), t
        assert len(set(z[0].tolist())) > 1  # (several classes are drawn at all)
        b = gen.backward_weights(st, 2, sm.xs[2, 0])
        assert np.isinf(b).any() and np.isfinite(b).any()
    finally:
        st.close()


# ------------------------------------------- 5. read-only and reproducible
def test_reproducible_and_read_only(gh_ctx):
    m, ys = _model(10), _observations(10)
    n = 4097
    a, rows, _ = _recorded(m, ys, n)
    b, _, _ = _recorded(m, ys, n)
    try:
        s1, s2, s3 = gen.smooth(a, 70, seed=8), gen.smooth(a, 70, seed=8), gen.smooth(a, 70, seed=9)
        assert _bits(s1.xs, s2.xs) and np.array_equal(s1.idx, s2.idx)
        assert not np.array_equal(s1.idx, s3.idx)
        gen.backward_weights(a, 2, rows[3][0])
        assert a.t == b.t == 4
        assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), gen.get_log_weights(b))
        assert _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b))
        for st in (a, b):
            assert gen.maybe_resample(st, n / 2) in (True, False)
            gen.particle_filter_step(st, (5,), (gen.UnknownChange(),), _obs_at(m, ys[4], 5))
        assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), gen.get_log_weights(b))
        assert np.array_equal(a.parents, b.parents) and _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b))
        assert _bits(gen.smooth(a, 70, seed=8, t0=5).idx, gen.smooth(b, 70, seed=8, t0=5).idx)
    finally:
        a.close()
        b.close()


# ------------------------------------------------ 6. against the closed form
def _rts_vars(m, ys):
    """Exact smoothing variances of a 1-D LG model (the recursion of tests/test_csmc.py's _rts_means)."""
    a, q, h, r = m.A[0, 0], m.Q[0, 0], m.H[0, 0], m.R[0, 0]
    pf, pp = [], []
    P = m.P0[0, 0]
    for t in range(len(ys)):
        if t > 0:
            P = a * a * P + q
        pp.append(P)
        P = (1 - P * h / (h * h * P + r) * h) * P
        pf.append(P)
    ps = list(pf)
    for t in range(len(ps) - 2, -1, -1):
        g = pf[t] * a / pp[t + 1]
        ps[t] = pf[t] + g * g * (ps[t + 1] - pp[t + 1])
    return np.array(ps)


def test_smoothed_means_against_rts(gh_ctx):
    """Every step's mean of M = 2048 draws within 6 sqrt(P_t|T (1 / M + 1 /
    ess_t)) of the RTS mean: the Monte-Carlo error of the draws plus the
    filter's own, at six standard errors."""
    m = _lg1()
    _, ys = m.simulate(8, np.random.default_rng(12))
    n, M, T = 4096, 2048, 8
    st, _, _ = _recorded(m, ys, n, T=T)
    try:
        gen.maybe_resample(st, 0)  # never fires: records the ESS of step T
        ess = st.ess_history()[0]
        mean = gen.smooth(st, M, seed=21).mean()[:, 0]
        exact, P = _rts_means(m, ys), _rts_vars(m, ys)
        ratio = np.abs(mean - exact) / np.sqrt(P * (1.0 / M + 1.0 / ess))
        print(f"smoothed mean error in standard errors, worst {ratio.max():.3f} (per step {np.round(ratio, 2)}); ess {ess}")
        assert (ratio <= 6.0).all(), ratio
        c = gen.smooth(st, M, seed=21).cov()[:, 0, 0]
        print(f"smoothed variance / RTS variance per step {np.round(c / P, 3)}")
    finally:
        st.close()


def test_diversity_where_the_genealogy_has_coalesced(gh_ctx):
    m = _lg1()
    _, ys = m.simulate(50, np.random.default_rng(13))
    n, T = 1024, 50
    st, _, _ = _recorded(m, ys, n, T=T)
    try:
        genealogy = int(gen.estimate_path(st, 1, 1, cov=False).distinct[0])
        smoothed = len(set(gen.smooth(st, 1024, seed=2).idx[0].tolist()))
        print(f"distinct particles of step 1: the genealogy {genealogy}, 1024 smoothed trajectories {smoothed}")
        assert smoothed > genealogy
    finally:
        st.close()


# -------------------------------------------------------------- 7. refusals
def _code(f):
    with pytest.raises(gen.GenHipError) as e:
        f()
    return e.value.code


def test_refusals(gh_ctx):
    INVAL, STATE = 1, 7
    m, ys = _model(2), _observations(2)
    st, rows, _ = _recorded(m, ys, 65, T=3)
    plain = _init(m, ys, 65)
    nohist = gen.initialize_particle_filter(m, (1,), _obs_at(m, ys[0], 1), 65, seed=SEED, record_history=False)
    lib = _lib.load()
    xs = np.empty((3, 70, 2))
    try:
        for M in (0, -1, 65537):
            assert _code(lambda: gen.smooth(st, M)) == INVAL
        for t0 in (0, 4, -2):
            assert _code(lambda: gen.smooth(st, 3, t0=t0)) == INVAL
        assert lib.gh_pf_smooth(st.h, 1, 3, 0, None, None) == INVAL
        for t in (0, 3, 4, -1):
            assert _code(lambda: gen.backward_weights(st, t, rows[1][0])) == INVAL
        assert lib.gh_pf_backward_weights(st.h, 1, None, _lib.dptr(xs)) == INVAL
        assert _code(lambda: gen.backward_weights(st, 1, np.zeros(3))) == INVAL  # the latent has 2 components
        assert _code(lambda: gen.get_log_weights(st, 4)) == INVAL and _code(lambda: gen.get_log_weights(st, 0)) == INVAL
        assert lib.gh_pf_get_log_weights_at(st.h, -1, _lib.dptr(xs)) == INVAL
        assert lib.gh_pf_get_log_weights_at(st.h, 0, _lib.dptr(xs)) == 0  # (the C form of "the current step")
        # without the weight history: the start alone (one step) is served, an earlier step is not
        assert gen.smooth(plain, 3).idx.shape == (1, 3)
        gen.particle_filter_step(plain, (2,), (gen.UnknownChange(),), _obs_at(m, ys[1], 2))
        assert _code(lambda: gen.smooth(plain, 3)) == STATE
        assert gen.smooth(plain, 3, t0=2).idx.shape == (1, 3)
        assert _code(lambda: gen.backward_weights(plain, 1, rows[2][0])) == STATE
        assert _code(lambda: gen.get_log_weights(plain, 1)) == STATE
        assert _bits(gen.get_log_weights(plain, 2), gen.get_log_weights(plain))
        # record_weights needs record_history
        assert _code(lambda: gen.initialize_particle_filter(m, (1,), _obs_at(m, ys[0], 1), 65, record_history=False,
                                                            record_weights=True)) == INVAL
        assert gen.smooth(nohist, 3).idx.shape == (1, 3)
        # after a step under changed parameters the recorded weights belong to other densities
        m2 = gen.LinearGaussianSSM(m.A * 0.9, m.Q, m.H, m.R, m.mu0, m.P0, b=m.b, c=m.c)
        gen.particle_filter_step(st, (4, m2), (gen.UnknownChange(), gen.UnknownChange()), _obs_at(m, ys[3], 4))
        assert _bits(gen.get_log_weights(st, 4), gen.get_log_weights(st))  # (recorded after the re-scoring)
        assert _code(lambda: gen.smooth(st, 3)) == STATE
        assert _code(lambda: gen.backward_weights(st, 2, rows[3][0])) == STATE
    finally:
        for s in (st, plain, nohist):
            s.close()


def test_refusal_of_the_regression(gh_ctx):
    m, ys = gen.BayesianLinearRegression.quickstart()
    st = gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys), 257, seed=SEED)
    try:
        assert _code(lambda: gen.smooth(st, 3)) == 1
    finally:
        st.close()


def test_refusal_on_the_multi_rank_path(gh_ctx):
    m, ys = _model(3), _observations(3)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        st = _init(m, ys, 64, ctx=ctx, record_weights=True)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), _obs_at(m, ys[1], 2))
        assert _code(lambda: gen.smooth(st, 3)) == 7
        assert _code(lambda: gen.backward_weights(st, 1, np.zeros(3))) == 7
        assert _code(lambda: gen.get_log_weights(st, 1)) == 7
        assert gen.get_log_weights(st).shape == (64,)  # (without a step: as before)
        st.close()
    finally:
        ctx.close()


def test_numeric_refusal(gh_ctx):
    """An HMM observation no state can emit leaves every weight -inf (the step
    itself does not refuse): the start has no maximum."""
    hmm = gen.DiscreteHMM([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[1.0, 1.0], [0.0, 0.0]])
    st = gen.initialize_particle_filter(hmm, (1,), {hmm.obs_address(1): 0}, 257, seed=SEED, record_weights=True)
    try:
        assert gen.smooth(st, 3).idx.shape == (1, 3)
        gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), {hmm.obs_address(2): 1})
        assert np.isneginf(gen.get_log_weights(st)).all()
        assert _code(lambda: gen.smooth(st, 3)) == 3
        assert _code(lambda: gen.smooth(st, 3, t0=2)) == 3
    finally:
        st.close()
