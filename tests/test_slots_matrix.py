"""The slot family (SlotModel<D, EXT>, gen_amd/csrc/gh_slots.h) over its whole
instantiation matrix: D = 1..16, plain and extended; of each, k_step (INIT,
plain and through the ancestors), k_rejuv, k_mh_drift, k_scores and
k_simulate.  Not run here: k_pin_pre, k_mr_slot_scores and the linear
proposal's SlotLinModel<D, EXT>.

tests/test_slots.py pins the family's features on a few state sizes (d = 1,
2, 3, 4, 10 plain; 2 and 4 extended).  Each (D, EXT) is device code of its
own (registers, spills, unrolling), so here one generated model per
instantiation runs those kernels against the CPU oracle bit for bit:

1. sweep_model(d, ext): an affine latent with four slots (plain: Poisson,
   log-linear-sd normal, mvnormal, categorical; extended: gamma, a fixed-sd
   normal after the library slot with the gamma as its parent, neg_binom,
   beta with a parent), filtered over four steps with rejuvenation and drift
   moves after every step.  CPU tests hold the conditions the GPU comparison
   rests on: finite weights, moves that accept and reject, a resample that
   fires, and the oracle's scores equal to scipy's densities at the new sizes.
2. The moves (selection and Gaussian drift MH) on the feature models of
   test_slots.py: library slots, stochastic volatility, dependent slots and
   per-step inputs, at t = 1 and through the ancestors at t = 3.
3. A parameter change (gh_pf_step_params) on a four-slot model with per-step
   inputs whose steps constrain all four slots: five entries per step, the
   chain rebuilt from the log with the input last (Python) and first (a C
   caller).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gen_amd as gen  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.test_slots import (  # noqa: E402
    _arg, _obs_at, _same, _with_input, changed_count_model, count_inputs, count_model, count_model_inputs, count_obs,
    dep_obs, library_obs, sv_obs)

N = 1300  # six blocks of 256; the last ends in a wave with 20 live lanes
T = 4
SEED = 41
REJUV, DRIFT, DRIFT_SD = 2, 3, 0.15
DS = list(range(1, 17))
SWEEP = [(d, ext) for d in DS for ext in (False, True)]
SWEEP_IDS = [f"d{d}-{'ext' if ext else 'plain'}" for d, ext in SWEEP]


def sweep_model(d, ext, inputs=False):
    """One model per instantiation SlotModel<d, ext>: an affine latent with
    dense A, Q, P0 and four slots; every h scaled by 1/sqrt(d), so that the
    linear predictors stay O(1) at every d."""
    rng = np.random.default_rng(100 + d)
    A = 0.8 * np.eye(d) + 0.1 * rng.standard_normal((d, d)) / np.sqrt(d)
    G = rng.standard_normal((d, d))
    Q = 0.05 * (G @ G.T / d + np.eye(d))
    P = rng.standard_normal((d, d))
    P0 = 0.3 * (P @ P.T / d + np.eye(d))
    lat = {"form": "affine", "A": A, "b": 0.1 * rng.standard_normal(d), "Q": Q,
           "mu0": 0.2 * rng.standard_normal(d), "P0": P0}
    if inputs:
        lat["inputs"] = True
    h = lambda: (rng.standard_normal(d) / np.sqrt(d)).tolist()  # noqa: E731
    if not ext:
        m = min(d, 3)
        F = rng.standard_normal((m, m))
        slots = [{"name": "count", "dist": "poisson", "h": h(), "c": 0.2},
                 {"name": "r", "dist": "normal", "h": h(), "c": 0.1,
                  "log_sd": {"g": (0.5 * np.array(h())).tolist(), "s": -0.3}},
                 {"name": "y", "dist": "mvnormal", "H": rng.standard_normal((m, d)) / np.sqrt(d),
                  "c": np.zeros(m), "R": F @ F.T / m + 0.3 * np.eye(m)},
                 {"name": "kind", "dist": "categorical", "W": rng.standard_normal((3, d)) / np.sqrt(d),
                  "c": [0.0, 0.2, -0.1]}]
    else:
        slots = [{"name": "g", "dist": "gamma", "args": [_arg("exp", h(), 0.3), 2.0]},
                 {"name": "z", "dist": "normal", "h": h(), "c": 0.1, "sd": 0.7, "parents": {"g": 0.05}},
                 {"name": "nb", "dist": "neg_binom", "args": [3.0, _arg("logistic", h(), 0.2)]},
                 {"name": "b", "dist": "beta", "args": [_arg("exp", h(), 0.5), _arg("exp", h(), 0.7)],
                  "parents": {"nb": 0.02}}]
    return gen.SlotSSM(lat, slots)


@functools.lru_cache(maxsize=None)
def sweep_case(d, ext):
    """(model, observations of steps 1..T): one slot left out at step 3."""
    m = sweep_model(d, ext)
    _, ys = m.simulate(T, np.random.default_rng(7))
    obs = [dict(y) for y in ys]
    del obs[2]["b" if ext else "r"]
    return m, obs


# ------------------------------------------------ one protocol, two engines
class _Orc:
    """The oracle behind the calls of the protocol."""

    def __init__(self, model, n, seed):
        self.pf = O.OraclePF(model, n, seed)
        self.d = model.d

    def init(self, y):
        self.pf.init(y)

    def step(self, t, y, u=None):
        self.pf.step(_with_input(y, u))

    def resample(self, thr):
        return self.pf.maybe_resample(thr)[0]

    def rejuvenate(self, k):
        return self.pf.rejuvenate(k)

    def drift(self, sd, k):
        return self.pf.mh_drift(1, np.full(self.d, sd), k)

    def bits(self):
        return (self.pf.state().view(np.uint64).copy(), self.pf.log_weights().view(np.uint64).copy(),
                self.pf.parents().copy())


class _Gpu:
    """The device library behind the same calls."""

    def __init__(self, model, n, seed):
        self.m, self.n, self.seed, self.st = model, n, seed, None

    def init(self, y):
        self.st = gen.initialize_particle_filter(self.m, (1,), _obs_at(self.m, y, 1), self.n, seed=self.seed)

    def step(self, t, y, u=None):
        na = (t,) if u is None else (t, u)
        gen.particle_filter_step(self.st, na, (gen.UnknownChange(),) * len(na), _obs_at(self.m, y, t))

    def resample(self, thr):
        return gen.maybe_resample(self.st, thr)

    def rejuvenate(self, k):
        return gen.rejuvenate(self.st, k)

    def drift(self, sd, k):
        sel = gen.select(*self.m.latent_addresses(self.st.t))
        return gen.mh(self.st, gen.gaussian_drift, (sel, sd), n_moves=k)

    def bits(self):
        return (np.ascontiguousarray(self.st.states().T).view(np.uint64), gen.get_log_weights(self.st).view(np.uint64),
                self.st.parents)


def _moves(e, log, sd):
    log.append(("rejuvenate", e.rejuvenate(REJUV), e.bits()))
    log.append(("drift", e.drift(sd, DRIFT), e.bits()))


def _sweep_protocol(e, obs):
    """init, then {maybe_resample; step} over the observations, with
    rejuvenate(2) and 3 drift moves after the init and after every step (so
    the later calls start at move counter 5, 10, ...).  Returns the log of the
    calls: (name, what the call returned, the bits of states, log-weights and
    parents after it; None after a resample, whose states are the next
    step's to read)."""
    log = []
    e.init(obs[0])
    log.append(("init", None, e.bits()))
    _moves(e, log, DRIFT_SD)
    for t in range(2, len(obs) + 1):
        log.append((f"maybe_resample before step {t}", e.resample(N / 2), None))
        e.step(t, obs[t - 1])
        log.append((f"step {t}", None, e.bits()))
        _moves(e, log, DRIFT_SD)
    return log


def _assert_same_log(got, want, what):
    """Call by call; the first differing call and quantity are named."""
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, ((name, r, b), (_, r0, b0)) in enumerate(zip(got, want)):
        where = f"{what}: call {i} ({name})"
        if b is not None:
            for q, x, y in zip(("states", "log-weights", "parents"), b, b0):
                assert np.array_equal(x, y), f"{where}: {q} differ from the oracle's in {int(np.sum(x != y))} places"
        assert r == r0, f"{where}: returned {r}, the oracle {r0}"


@functools.lru_cache(maxsize=None)
def _sweep_oracle(d, ext):
    """The oracle's run of the protocol: (the filter at the end, the log)."""
    m, obs = sweep_case(d, ext)
    e = _Orc(m, N, SEED)
    return e.pf, _sweep_protocol(e, obs)


@functools.lru_cache(maxsize=None)
def _sweep_oracle_plain(d, ext):
    """The oracle's run of the same observations without moves."""
    m, obs = sweep_case(d, ext)
    return O.run_pf(m, obs, N, SEED, thr=N / 2)


def _assert_moves_mix(log, what):
    """Every move call accepts strictly between 0.1 and 0.95 of its moves x n:
    a kernel that accepted everything or nothing would otherwise compare
    equal to an oracle that does the same."""
    for name, r, _ in log:
        if name in ("rejuvenate", "drift"):
            k = REJUV if name == "rejuvenate" else DRIFT
            assert 0.1 * k * N < r < 0.95 * k * N, (what, name, r / (k * N))


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("d,ext", SWEEP, ids=SWEEP_IDS)
def test_oracle_sweep_conditions(d, ext):
    """What the GPU comparison of a sweep case rests on, on the oracle alone:
    finite weights after every call, rejuvenation and drift calls that accept
    strictly between 0.1 and 0.95 of their moves, and at least one of the
    three resample decisions firing (so the steps read through ancestors)."""
    pf, log = _sweep_oracle(d, ext)
    for name, _, b in log:
        if b is not None:
            assert np.all(np.isfinite(b[1].view(np.float64))), name
    assert np.all(np.isfinite(pf.log_weights())) and np.isfinite(pf.log_ml_estimate())
    _assert_moves_mix(log, (d, ext))
    fired = [r for name, r, _ in log if name.startswith("maybe_resample")]
    assert len(fired) == T - 1 and any(fired), fired
    plain = _sweep_oracle_plain(d, ext)
    assert np.all(np.isfinite(plain.log_weights()))


def _softmax_logp(logits, k):
    return logits[k] - logits.max() - np.log(np.exp(logits - logits.max()).sum())


def _sweep_obs_logpdf(m, ext, x, y):
    """The present slots' densities of a sweep model at latent x, restated
    with scipy under the reference's argument conventions (gamma(shape,
    scale), neg_binom counts failures)."""
    from scipy import stats

    s, tot = m.slots, 0.0
    if not ext:
        if "count" in y:
            tot += stats.poisson.logpmf(y["count"], np.exp(s[0]["h"] @ x + s[0]["c"]))
        if "r" in y:
            tot += stats.norm.logpdf(y["r"], s[1]["h"] @ x + s[1]["c"], np.exp(s[1]["g"] @ x + s[1]["s"]))
        if "y" in y:
            tot += stats.multivariate_normal.logpdf(np.atleast_1d(y["y"]), s[2]["H"] @ x + s[2]["c"], s[2]["R"])
        if "kind" in y:
            tot += _softmax_logp(s[3]["W"] @ x + s[3]["c"], int(y["kind"]))
        return tot

    def eta(k, i):
        _, h, c = s[k]["args"][i]
        return h @ x + c

    if "g" in y:
        tot += stats.gamma.logpdf(y["g"], np.exp(eta(0, 0)), scale=2.0)
    if "z" in y:
        tot += stats.norm.logpdf(y["z"], s[1]["h"] @ x + s[1]["c"] + 0.05 * y["g"], 0.7)
    if "nb" in y:
        tot += stats.nbinom.logpmf(y["nb"], 3.0, 1.0 / (1.0 + np.exp(-eta(2, 1))))
    if "b" in y:
        tot += stats.beta.logpdf(y["b"], np.exp(eta(3, 0) + 0.02 * y["nb"]), np.exp(eta(3, 1)))
    return tot


@pytest.mark.parametrize("d,ext", [(7, False), (7, True), (16, False), (16, True)],
                         ids=["d7-plain", "d7-ext", "d16-plain", "d16-ext"])
def test_oracle_sweep_scores_equal_scipy_densities(d, ext):
    """The oracle at state sizes nothing else pins: its per-step score columns
    on 64 particles equal scipy's multivariate_normal for the latent and the
    slots' densities for the observations, along each particle's genealogy."""
    from scipy import stats

    m, obs = sweep_case(d, ext)
    n = 64
    pf = O.run_pf(m, obs, n, 3)
    _, ps = pf.scores(per_step=True)
    X = [pf.trajectory(t) for t in range(1, T + 1)]
    for t in range(T):
        lat, ob = np.empty(n), np.empty(n)
        for j in range(n):
            x = X[t][:, j]
            mean, cov = (m.mu0, m.P0) if t == 0 else (m.A @ X[t - 1][:, j] + m.b, m.Q)
            lat[j] = stats.multivariate_normal.logpdf(x, mean, cov)
            ob[j] = _sweep_obs_logpdf(m, ext, x, obs[t])
        np.testing.assert_allclose(ps[t, 0], lat, rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(ps[t, 1], ob, rtol=1e-12, atol=1e-10)


# ------------------------------------------------------------------ GPU: the sweep
@pytest.mark.gpu
@pytest.mark.parametrize("d,ext", SWEEP, ids=SWEEP_IDS)
def test_gpu_sweep_with_moves_equals_oracle_bitexact(gh_ctx, d, ext):
    """SlotModel<d, ext> call by call: k_step (INIT, plain, through the
    ancestors), k_rejuv and k_mh_drift after every step, the resample
    decisions, then k_scores and k_simulate — states, log-weights and parents
    as bits after every call, the accepted counts, log-ML at 1e-9."""
    m, obs = sweep_case(d, ext)
    pf, want = _sweep_oracle(d, ext)
    e = _Gpu(m, N, SEED)
    try:
        _assert_same_log(_sweep_protocol(e, obs), want, SWEEP_IDS[SWEEP.index((d, ext))])
        a, b = gen.log_ml_estimate(e.st), pf.log_ml_estimate()
        assert abs(a - b) <= 1e-9 * abs(b), (a, b)
        tot, ps = gen.get_traces(e.st).scores(per_step=True)
        otot, ops = pf.scores(per_step=True)
        assert np.array_equal(ps, ops), "score columns"
        assert np.array_equal(tot, otot), "scores"
    finally:
        if e.st is not None:
            e.st.close()
    tr = gen.simulate(m, (3,), num_traces=321, seed=29)
    X, Y, PS, TOT = O.simulate(m, 3, 321, 29)
    assert np.array_equal(tr.xs, X), "simulate: latents"
    assert np.array_equal(tr.ys, Y), "simulate: observations"
    assert np.array_equal(tr.per_step, PS) and np.array_equal(tr.total, TOT), "simulate: scores"


@pytest.mark.gpu
@pytest.mark.parametrize("d,ext", SWEEP, ids=SWEEP_IDS)
def test_gpu_sweep_batched_equals_oracle_bitexact(gh_ctx, d, ext):
    """The same observations through run_particle_filter (the batched loop
    with the device-side resample decision), no moves."""
    m, obs = sweep_case(d, ext)
    orc = _sweep_oracle_plain(d, ext)
    st = gen.initialize_particle_filter(m, (1,), _obs_at(m, obs[0], 1), N, seed=SEED)
    try:
        gen.run_particle_filter(st, list(obs[1:]), N / 2)
        assert np.array_equal(st.states().T.view(np.uint64), orc.state().view(np.uint64))
        assert np.array_equal(gen.get_log_weights(st).view(np.uint64), orc.log_weights().view(np.uint64))
        _same(st, orc=orc)
        tot, ps = gen.get_traces(st).scores(per_step=True)
        otot, ops = orc.scores(per_step=True)
        assert np.array_equal(tot, otot) and np.array_equal(ps, ops)
    finally:
        st.close()


# ------------------------------------- moves on the feature models
FEATURE_NAMES = ("m1", "m2", "m3", "m4", "sv", "dep", "inputs")
FEATURES = [(name, t) for name in FEATURE_NAMES for t in (1, 3)]
FEATURE_IDS = [f"{name}-t{t}" for name, t in FEATURES]
FEATURE_MOVES = 3
FEATURE_SD = 0.3  # one drift sd serves every model (test_oracle_feature_moves_mix holds each to its bounds)
# The one call whose rate no setting of the test moves: a rejuvenation proposes
# from the prior, so its rate is the data's.  library_obs leaves m4's Poisson
# slot out of step 3; the Bernoulli and beta_uniform slots that remain say
# little about the latent, and the first rejuvenation there rejects under 5%
# of its proposals.  It is held to 0.1 and to rejecting more than a
# wavefront's worth (64) of its moves, so lanes of several waves took each
# branch; every other call, this case's second rejuvenation included, is held
# to 0.95.  (case, index of the call among the four)
FEATURE_WEAK_DATA = {("m4", 3, 0)}


def _feature_case(name):
    """(model, observations, inputs per step or None)"""
    if name in ("m1", "m2", "m3", "m4"):
        return (*library_obs(name), None)
    if name == "sv":
        return (*sv_obs(), None)
    if name == "dep":
        return (*dep_obs(), None)
    _, obs = count_obs()
    return count_model_inputs(), obs, count_inputs()


def _feature_protocol(e, obs, u, t_end):
    """Filter to t_end with a forced resample before steps 2 and 3 (the parent
    rows are then read through the ancestors), then two calls each of
    rejuvenate(3) and 3 drift moves, alternating."""
    log = []
    e.init(obs[0])
    for t in range(2, t_end + 1):
        assert e.resample(1e9)
        e.step(t, obs[t - 1], None if u is None else u[t - 1])
    log.append((f"step {t_end}", None, e.bits()))
    for _ in range(2):
        log.append(("rejuvenate", e.rejuvenate(FEATURE_MOVES), e.bits()))
        log.append(("drift", e.drift(FEATURE_SD, FEATURE_MOVES), e.bits()))
    return log


@functools.lru_cache(maxsize=None)
def _feature_oracle(name, t):
    m, obs, u = _feature_case(name)
    return _feature_protocol(_Orc(m, N, SEED), obs, u, t)


@pytest.mark.parametrize("name,t", FEATURES, ids=FEATURE_IDS)
def test_oracle_feature_moves_mix(name, t):
    """The oracle alone accepts strictly between 0.1 and 0.95 of the moves of
    each of the four calls, rejuvenations and drifts alike (the one exception
    and its bound: FEATURE_WEAK_DATA), and an input is present at the step the
    moves of the input model run on."""
    log = _feature_oracle(name, t)
    total = FEATURE_MOVES * N
    assert [c[0] for c in log[1:]] == ["rejuvenate", "drift"] * 2
    for i, (call, r, _) in enumerate(log[1:]):
        upper = total - 64 if (name, t, i) in FEATURE_WEAK_DATA else 0.95 * total
        assert 0.1 * total < r < upper, (name, t, i, call, r / total)
    if name == "inputs" and t == 3:
        assert count_inputs()[t - 1] is not None


@pytest.mark.gpu
@pytest.mark.parametrize("name,t", FEATURES, ids=FEATURE_IDS)
def test_gpu_feature_moves_equal_oracle_bitexact(gh_ctx, name, t):
    """k_rejuv and k_mh_drift of the library-slot models (m1..m4: every scalar
    library distribution), the log-linear-sd normal, dependent slots and a
    model with per-step inputs: states, weights and accepted counts as the
    oracle's, bit for bit after each of four calls of three moves."""
    m, obs, u = _feature_case(name)
    e = _Gpu(m, N, SEED)
    try:
        _assert_same_log(_feature_protocol(e, obs, u, t), _feature_oracle(name, t), f"{name} at t = {t}")
    finally:
        if e.st is not None:
            e.st.close()


# --------------------- a parameter change with inputs, all four slots constrained
K = 5


def _change_case():
    """(mi, m2i, observations of steps 1..6 with no slot left out, {t: u_t} for
    t >= 2): every step from the second carries five entries."""
    mi = count_model_inputs()
    m2 = changed_count_model()
    lat = dict(m2.latent)
    lat["inputs"] = True
    m2i = gen.SlotSSM(lat, [dict(sl) for sl in changed_count_model().slots])
    _, ys = count_model().simulate(6, np.random.default_rng(5))
    rng = np.random.default_rng(11)
    u = {t: 0.4 * rng.standard_normal(2) for t in range(2, 7)}
    return mi, m2i, [dict(y) for y in ys], u


def _change_oracle(n, seed, thr, upto=6, new=None):
    """The oracle's run: steps under mi, step K changing to `new` (default
    m2i), later steps under it; stops after step `upto`.  Returns (filter, the
    bits after every step, the resample decisions)."""
    mi, m2i, obs, u = _change_case()
    pf = O.OraclePF(mi, n, seed)
    pf.init(obs[0])
    bits = {1: (pf.state().copy(), pf.log_weights().copy(), pf.parents().copy())}
    did = {}
    for t in range(2, upto + 1):
        did[t] = pf.maybe_resample(thr)[0]
        y = _with_input(obs[t - 1], u[t])
        if t == K:
            pf.step_params(m2i if new is None else new, y)
        else:
            pf.step(y)
        bits[t] = (pf.state().copy(), pf.log_weights().copy(), pf.parents().copy())
    return pf, bits, did


def test_oracle_change_with_inputs_rescores_history_with_its_inputs():
    """No resampling: after the change the log-weights are the history's
    observation scores under the new numbers plus the latent scores' change,
    and the re-scored latent score of step 3 is scipy's
    mvnormal(A' x_2 + b' + u_3, Q') — without u_3 it is off by up to 5.7, so an
    input dropped from the history cannot pass."""
    from scipy import stats

    mi, m2i, obs, u = _change_case()
    n = 300
    new, _, _ = _change_oracle(n, 21, 0.0, upto=K)
    old, _, _ = _change_oracle(n, 21, 0.0, upto=K - 1)
    _, ps_new = new.scores(per_step=True)
    _, ps_old = old.scores(per_step=True)
    assert ps_new.shape == (K, 2, n) and ps_old.shape == (K - 1, 2, n)
    want = ps_new[:, 1].sum(axis=0) + (ps_new[:K - 1, 0] - ps_old[:, 0]).sum(axis=0)
    np.testing.assert_allclose(new.log_weights(), want, rtol=1e-12)
    x2, x3 = new.trajectory(2), new.trajectory(3)
    ref = np.array([stats.multivariate_normal.logpdf(x3[:, i], m2i.A @ x2[:, i] + m2i.b + u[3], m2i.Q)
                    for i in range(n)])
    np.testing.assert_allclose(ps_new[2, 0], ref, rtol=1e-12, atol=1e-10)
    no_u = np.array([stats.multivariate_normal.logpdf(x3[:, i], m2i.A @ x2[:, i] + m2i.b, m2i.Q) for i in range(n)])
    assert np.abs(no_u - ref).max() > 1.0  # (what the comparison above would miss by, had u_3 been dropped)


def test_oracle_change_with_inputs_to_the_same_numbers_is_the_plain_step():
    a, _, _ = _change_oracle(500, 4, None, new=count_model_inputs())
    mi, _, obs, u = _change_case()
    b = O.run_pf(mi, [obs[0]] + [_with_input(obs[t - 1], u[t]) for t in range(2, 7)], 500, 4)
    assert np.array_equal(a.state().view(np.uint64), b.state().view(np.uint64))
    assert np.array_equal(a.log_weights().view(np.uint64), b.log_weights().view(np.uint64))
    assert np.array_equal(a.parents(), b.parents())


def _chain_input_first(model, y, u):
    """One step's gh_obs chain as a C caller may give it: the GH_SLOT_INPUT
    entry first, then the slots in model order.  Returns (chain, what keeps
    its values alive)."""
    from gen_amd import _lib

    vals = ([(_lib.SLOT_INPUT, np.ascontiguousarray(u, dtype=np.float64))] if u is not None else []) + \
        [(k, np.atleast_1d(np.asarray(y[name], dtype=np.float64))) for k, name in enumerate(model.names)]
    chain = (_lib.Obs * len(vals))()
    for i, (k, v) in enumerate(vals):
        chain[i] = _lib.Obs(_lib.dptr(v), v.size, 1, k, 0, None)
    for i in range(len(vals) - 1):
        chain[i].next = ctypes.pointer(chain[i + 1])
    return chain, vals


def _assert_bits(st, want, t):
    x, w, p = want
    assert np.array_equal(gen.get_log_weights(st).view(np.uint64), w.view(np.uint64)), f"log-weights after step {t}"
    assert np.array_equal(st.states().T.view(np.uint64), x.view(np.uint64)), f"states after step {t}"
    assert np.array_equal(st.parents, p), f"parents after step {t}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["calls", "batched_history", "ctypes_input_first"])
def test_gpu_change_with_inputs_equals_oracle_bitexact(gh_ctx, form):
    """gh_pf_step_params at step 5 of a four-slot model with per-step inputs
    whose every step constrains all four slots (five entries per step): the
    history is re-scored with its inputs and all its observations, whichever
    way it was built and whichever place the input has in the chain.  Every
    step's states, weights and parents as the oracle's bit for bit; log-ML at
    1e-9; score columns equal."""
    from gen_amd import _lib

    mi, m2i, obs, u = _change_case()
    n, seed = N, 21
    orc, want, did = _change_oracle(n, seed, n / 2)
    unk = gen.UnknownChange()
    keep = None
    if form == "ctypes_input_first":
        lib = _lib.load()
        opts = _lib.PFOpts()
        lib.gh_pf_opts_default(ctypes.byref(opts))
        h = ctypes.c_void_p()
        chain, keep = _chain_input_first(mi, obs[0], None)
        _lib.check(lib.gh_pf_init(gh_ctx.model_handle(mi), ctypes.byref(chain[0]), 0, n, seed, ctypes.byref(opts),
                                  ctypes.byref(h)))
        st = gen.ParticleFilterState(gh_ctx, mi, h, n)
    else:
        st = gen.initialize_particle_filter(mi, (1,), _obs_at(mi, obs[0], 1), n, seed=seed)
    try:
        _assert_bits(st, want[1], 1)
        first = 2
        if form == "batched_history":
            gen.run_particle_filter(st, obs[1:K - 1], n / 2, inputs_per_step=[u[t] for t in range(2, K)])
            _assert_bits(st, want[K - 1], K - 1)
            first = K
        for t in range(first, 7):
            if form == "ctypes_input_first":
                r, ess = ctypes.c_int(), ctypes.c_double()
                _lib.check(lib.gh_pf_maybe_resample(st.h, n / 2, ctypes.byref(r), ctypes.byref(ess)))
                assert bool(r.value) == did[t], t
                chain, keep = _chain_input_first(mi, obs[t - 1], u[t])
                if t == K:
                    _lib.check(lib.gh_pf_step_params(st.h, ctypes.byref(chain[0]), 0, gh_ctx.model_handle(m2i)))
                    st.model = m2i
                else:
                    _lib.check(lib.gh_pf_step(st.h, ctypes.byref(chain[0]), 0))
            else:
                assert gen.maybe_resample(st, n / 2) == did[t], t
                mt = mi if t < K else m2i
                na = (t, m2i, u[t]) if t == K else (t, u[t])
                gen.particle_filter_step(st, na, (unk,) * len(na), _obs_at(mt, obs[t - 1], t))
            _assert_bits(st, want[t], t)
        a, b = gen.log_ml_estimate(st), orc.log_ml_estimate()
        assert abs(a - b) <= 1e-9 * abs(b), (a, b)
        tot, ps = gen.get_traces(st).scores(per_step=True)
        otot, ops = orc.scores(per_step=True)
        assert np.array_equal(ps, ops) and np.array_equal(tot, otot)
    finally:
        st.close()
    del keep
