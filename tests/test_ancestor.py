"""Ancestor sampling in conditional SMC (gh_pf_opts.ancestor_sampling,
gh_ancestor.h) on the device.

1. with the option the filter has, bit for bit, the states, weights and
   parents[1:] of a plain conditional filter, and parents[0] is the host
   restatement's pick (tests/test_smooth_abi.py: Python integers, the oracle's
   exp and Philox; the uniform of tests/test_ancestor_abi.py) on the device's
   own backward weights gh_pf_backward_weights(pf, t - 1, ref_t);
2. where no resample fires nothing changes at all;
3. the genealogy readers follow the new parent;
4. the run is reproducible;
5. the refusals, and the device error where no particle can precede the
   reference;
6. particle Gibbs with ancestor sampling reproduces the RTS means at 16
   particles over 40 steps and moves x_1 in most sweeps, where the plain chain
   hardly ever does.

The reference trajectory is the simulated latent times 0.9, as in
tests/test_csmc.py.  maybe_resample(st, n) fires whenever the ESS is below n,
which it is unless every weight is equal: the one-particle case (ESS = 1 = n
exactly) takes the threshold 1.5 instead, so that its resample fires too, and
the runs over the families take n + 1 (a step without an observation leaves
equal weights).
"""
import ctypes

import numpy as np
import pytest

import gen_amd as gen
from gen_amd import _lib, pf as _pf
from tests.test_ancestor_abi import reference_u53
from tests.test_csmc import _lg1, _rts_means
from tests.test_estimates import _bits, _model, _obs_at, _observations
from tests.test_slots import count_model, count_obs
from tests.test_smooth import FAMILIES
from tests.test_smooth_abi import reference_pick

pytestmark = pytest.mark.gpu

SEED = 2
INVAL, NUMERIC, STATE = 1, 3, 7


# the simulations that made each family's observations (tests/test_smooth.py FAMILIES and the helpers it
# names): (steps, seed) of model.simulate, (7, 5) unless listed (the nonlinear SSM's four observations are the
# first four of that simulation); the HMM's observations are a golden file
SIMULATED = {"slots": (10, 5), "library": (10, 6), "switching": (12, 4)}


def _reference(m, T, family=None):
    """[T, d]: the simulated latent trajectory times 0.9, as in tests/test_csmc.py:
    the latent of the simulation that made the observations (for the HMM, whose
    observations are given, a chain drawn here)."""
    if isinstance(m, gen.DiscreteHMM):
        rng = np.random.default_rng(6)
        z = [rng.choice(m.k, p=m.prior)]
        for _ in range(T - 1):
            z.append(rng.choice(m.k, p=m.T[:, z[-1]]))
        xs = np.array(z, dtype=np.float64)
    else:
        steps, seed = SIMULATED.get(family, (7, 5))
        xs = m.simulate(steps, np.random.default_rng(seed))[0]
    ref = np.ascontiguousarray(np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)[:T] * 0.9)
    assert ref.shape == (T, m.d)
    return ref


def _cond(m, ys, n, ref, seed=SEED, **kw):
    return gen.initialize_conditional_particle_filter(m, (1,), _obs_at(m, ys[0], 1), n, ref[0], seed=seed, **kw)


def _step(st, m, ys, ref, t):
    gen.conditional_particle_filter_step(st, (t,), (gen.UnknownChange(),), _obs_at(m, ys[t - 1], t), ref[t - 1])


def _twins(m, ys, ref, n, T, thr):
    """Filter a samples ancestors (and records its weights, for
    backward_weights), its twin b does not.  After every step: equal bits in
    states and weights, equal parents[1:], and a's parents[0] = the host pick
    where the resample fired, 0 where it did not.  Returns the picks."""
    a, b = _cond(m, ys, n, ref, ancestor_sampling=True, record_weights=True), _cond(m, ys, n, ref)
    picks = []
    try:
        assert _bits(a.states(), b.states()) and _bits(gen.get_log_weights(a), gen.get_log_weights(b))
        for t in range(2, T + 1):
            fired = gen.maybe_resample(a, thr)
            assert gen.maybe_resample(b, thr) == fired
            assert fired == (thr > 0), (t, "the resample fires at every step" if thr > 0 else "no resample")
            for st in (a, b):
                _step(st, m, ys, ref, t)
            assert _bits(a.states(), b.states()), t
            assert _bits(gen.get_log_weights(a), gen.get_log_weights(b)), t
            pa, pb = a.parents, b.parents
            assert np.array_equal(pa[1:], pb[1:]), t
            assert pb[0] == 0, t
            if fired:
                bw = gen.backward_weights(a, t - 1, ref[t - 1])
                want = reference_pick(bw, reference_u53(SEED, 0, t), n)
                assert pa[0] == want, (t, int(pa[0]), want)
            else:
                assert pa[0] == 0, t
            picks.append(int(pa[0]))
        assert _bits(gen.log_ml_estimate(a), gen.log_ml_estimate(b))
    finally:
        a.close()
        b.close()
    return picks


# ------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 257, 4097])
def test_bit_for_bit(gh_ctx, n):
    m, ys = _model(10), _observations(10)
    T = 7
    picks = _twins(m, ys, _reference(m, T), n, T, n if n > 1 else 1.5)
    print(f"n={n}: picks {picks}")
    assert len(picks) == T - 1 and all(0 <= j < n for j in picks)
    if n >= 64:
        assert any(picks), "every pick is 0: the case shows nothing"


def test_bit_for_bit_across_more_than_256_blocks(gh_ctx):
    """n = 65 537 + 300: 258 block sums, so bs_cross takes a second round."""
    m, ys = _model(10), _observations(10)
    n, T = 65537 + 300, 7
    picks = _twins(m, ys, _reference(m, T), n, T, n)
    print(f"n={n}: picks {picks}")
    assert any(picks)


CONDITIONAL_FAMILIES = [f for f in FAMILIES if f != "inputs"]  # (test_inputs_are_refused_by_the_conditional_step)


def _seven_steps(family, m, ys):
    """Seven observations of each family: FAMILIES keeps four of the nonlinear
    SSM, the HMM and the slot model.  The first two go on with the simulation
    that made those four (the same seed draws the same first four); the HMM's
    four are a golden file and are followed by their first three again."""
    if family == "kitagawa":
        longer = m.simulate(7, np.random.default_rng(5))[1]
        assert np.array_equal(longer[:4], ys)
        return longer
    if family == "slots":
        longer = count_obs()[1][:7]
        assert longer[:4] == list(ys)
        return longer
    if family == "hmm":
        return list(ys) + list(ys)[:3]
    return ys[:7]


@pytest.mark.parametrize("family", CONDITIONAL_FAMILIES)
def test_bit_for_bit_of_every_family(gh_ctx, family):
    """The threshold is n + 1, not n: after a step without an observation (the
    slot models have one among their first seven) the weights are equal, the
    ESS is n exactly and maybe_resample(st, n) would not fire."""
    m, ys = FAMILIES[family]()
    n, T = 257, 7
    ys = _seven_steps(family, m, ys)
    assert len(ys) == T
    picks = _twins(m, ys, _reference(m, T, family), n, T, n + 1)
    print(f"{family}: picks {picks}")
    assert any(picks), "every pick is 0: the case shows nothing"


def test_inputs_are_refused_by_the_conditional_step(gh_ctx):
    """The one entry of FAMILIES left out above: a model with per-step inputs
    steps with new_args = (t, u_t), which the conditional step does not take."""
    m, ys, u = FAMILIES["inputs"]()
    ref = _reference(count_model(), 2, "slots")
    st = _cond(m, ys, 65, ref, ancestor_sampling=True)
    try:
        with pytest.raises(gen.GenHipError) as e:
            gen.conditional_particle_filter_step(st, (2, u[1]), (gen.UnknownChange(),) * 2, _obs_at(m, ys[1], 2), ref[1])
        assert e.value.code == INVAL and st.t == 1
    finally:
        st.close()


# ------------------------------------------------------------ 2. no resample
@pytest.mark.parametrize("n", [65, 4097])
def test_without_a_resample_nothing_changes(gh_ctx, n):
    m, ys = _model(10), _observations(10)
    assert _twins(m, ys, _reference(m, 7), n, 7, 0) == [0] * 6


# -------------------------------------------------------------- 3. genealogy
def test_genealogy_follows_the_sampled_parents(gh_ctx):
    m, ys = _model(10), _observations(10)
    n, T = 257, 7
    ref = _reference(m, T)
    st = _cond(m, ys, n, ref, ancestor_sampling=True)
    try:
        rows, par = {1: st.states()}, {}
        for t in range(2, T + 1):
            assert gen.maybe_resample(st, n)
            _step(st, m, ys, ref, t)
            rows[t], par[t] = st.states(), st.parents
        traj = gen.get_particle(st, 0)
        assert traj.shape == (T, m.d) and _bits(traj[-1], ref[-1])
        j, lineage = 0, []
        for s in range(T, 0, -1):
            assert _bits(traj[s - 1], rows[s][j]), s
            lineage.append(j)
            j = int(par[s][j]) if s > 1 else j
        print(f"particle 0's lineage, step T down to 1: {lineage}")
        assert any(lineage[1:]), "particle 0 kept itself as parent at every step: the case shows nothing"
        assert not _bits(traj, ref)  # (the plain filter's lineage of particle 0 is the reference itself)
        assert _bits(st.states(1)[0], traj[0])
    finally:
        st.close()


# ----------------------------------------------------------- 4. reproducible
def test_reproducible(gh_ctx):
    m, ys = _model(10), _observations(10)
    n, T = 4097, 7
    ref = _reference(m, T)
    runs = []
    for _ in range(2):
        st = _cond(m, ys, n, ref, ancestor_sampling=True)
        try:
            seen = []
            for t in range(2, T + 1):
                gen.maybe_resample(st, n)
                _step(st, m, ys, ref, t)
                seen.append(st.parents)
            runs.append(np.stack(seen))
        finally:
            st.close()
    assert np.array_equal(runs[0], runs[1])
    assert runs[0][:, 0].any()
    other = gen.conditional_smc(m, list(ys), n, ref, seed=SEED + 1, ess_threshold=n, ancestor_sampling=True)
    try:
        assert other.t == T  # (conditional_smc carries the keyword through a whole sweep)
    finally:
        other.close()


# --------------------------------------------------------------- 5. refusals
def _raises(f):
    with pytest.raises(gen.GenHipError) as e:
        f()
    return e.value.code, str(e.value)


def test_refusals(gh_ctx):
    m, ys = _model(2), _observations(2)
    ref = _reference(m, 3)
    lib = _lib.load()
    # a filter that is not conditional: refused by gh_pf_init and gh_pf_init_q, before any device work
    opts = _pf._opts("multinomial", True, 0, 0, False, True)
    obs, keep = _pf._step_obs(m, 1, _obs_at(m, ys[0], 1))
    h = ctypes.c_void_p()
    mh = gh_ctx.model_handle(m)
    assert lib.gh_pf_init(mh, ctypes.byref(obs), 0, 65, SEED, ctypes.byref(opts), ctypes.byref(h)) == INVAL
    assert b"ancestor_sampling" in lib.gh_last_error() and not h.value
    assert lib.gh_pf_init_q(mh, ctypes.byref(obs), 0, None, 0, 65, SEED, ctypes.byref(opts), ctypes.byref(h)) == INVAL
    assert b"conditional" in lib.gh_last_error() and not h.value
    del keep
    # a step under changed parameters
    st = _cond(m, ys, 65, ref, ancestor_sampling=True)
    try:
        m2 = gen.LinearGaussianSSM(m.A * 0.9, m.Q, m.H, m.R, m.mu0, m.P0, b=m.b, c=m.c)
        code, msg = _raises(lambda: gen.conditional_particle_filter_step(
            st, (2, m2), (gen.UnknownChange(),) * 2, _obs_at(m, ys[1], 2), ref[1]))
        assert code == STATE and "ancestor sampling" in msg and st.t == 1
        gen.maybe_resample(st, 65)
        _step(st, m, ys, ref, 2)  # (the filter goes on)
        assert st.t == 2
    finally:
        st.close()


def test_refusal_on_the_multi_rank_path(gh_ctx):
    m, ys = _model(3), _observations(3)
    ref = _reference(m, 2)
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        code, msg = _raises(lambda: _cond(m, ys, 64, ref, ctx=ctx, ancestor_sampling=True))
        assert code == STATE and "ancestor sampling" in msg
    finally:
        ctx.close()


def test_numeric_error_where_no_particle_can_precede_the_reference(gh_ctx):
    """z_t = perm(z_{t-1}) with probability 1 and z_1 = 0: every particle of
    step 1 is in class 0, the reference of step 2 is class 3, which only class
    2 precedes: every b_i is -inf, B = -inf."""
    perm = [1, 2, 3, 0]
    T_ = np.zeros((4, 4))
    for prev, new in enumerate(perm):
        T_[new, prev] = 1.0
    E = np.array([[0.4, 0.3, 0.2, 0.1], [0.1, 0.2, 0.3, 0.4], [0.5, 0.5, 0.5, 0.5]])
    E /= E.sum(axis=0)
    m = gen.DiscreteHMM([1.0, 0.0, 0.0, 0.0], T_, E)
    ys, n = [0, 1], 257
    ref = np.array([[0.0], [3.0]])
    st = _cond(m, ys, n, ref, ancestor_sampling=True)
    try:
        assert gen.maybe_resample(st, n + 1)  # (equal weights: the ESS is n)
        _step(st, m, ys, ref, 2)
        code, msg = _raises(lambda: gen.log_ml_estimate(st))
        assert code == NUMERIC and "ancestor sampling" in msg
    finally:
        st.close()


# ---------------------------------------------------------- 6. PGAS and RTS
PG_T, PG_N, PG_SWEEPS, PG_BURN = 40, 16, 600, 100


def _chain(ancestor_sampling):
    m = _lg1()
    _, ys = m.simulate(PG_T, np.random.default_rng(12))
    kw = {"ancestor_sampling": True} if ancestor_sampling else {}
    refs, lmls = gen.particle_gibbs(m, [y for y in ys], PG_N, np.zeros((PG_T, 1)), PG_SWEEPS, seed=3,
                                    ess_threshold=PG_N, **kw)
    assert np.all(np.isfinite(lmls))
    x = np.stack(refs)[:, :, 0]
    err = np.max(np.abs(np.mean(x[PG_BURN:], axis=0) - _rts_means(m, ys)))
    moved = float(np.mean(x[PG_BURN:, 0] != x[PG_BURN - 1:-1, 0]))
    return err, moved


def test_pgas_matches_the_smoother_and_moves_x1(gh_ctx):
    """Model _lg1, T = 40, 16 particles, a resample at every step, 600 sweeps
    from a zero reference, 100 of them burn-in.  The numpy restatement of the
    chain, tools/pgas_chain.py, gave with ancestor sampling a largest error of
    the smoothed means against RTS of at most 0.113 over 30 seeds and x_1
    changed in 0.86-0.92 of the sweeps; without it (5 seeds) x_1 changed in at
    most 0.008 of the sweeps and the error was 0.43-0.76.  The bounds: an error
    below 0.25, about twice the restatement's worst; x_1 moved in more than
    half of the sweeps, and in fewer than a tenth without the option.  On an
    MI355X: 0.060 and 0.892; the plain chain 0.002."""
    err, moved = _chain(True)
    print(f"PGAS: largest error of the smoothed means {err:.4f}, x_1 moved in {moved:.3f} of the sweeps")
    assert err < 0.25
    assert moved > 0.5


def test_plain_particle_gibbs_hardly_moves_x1(gh_ctx):
    err, moved = _chain(False)
    print(f"plain particle Gibbs: largest error of the smoothed means {err:.4f}, x_1 moved in {moved:.3f} of the sweeps")
    assert moved < 0.1
