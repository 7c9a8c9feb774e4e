"""elliptical_slice and map_optimize on every particle of a filter
(src/inference/elliptical_slice.jl:13-45, src/inference/map_optimize.jl:9-41).

The reference of both moves is a numpy restatement in this file: its draws are
the device's (Philox blocks of the move's window and of the shrink stream
through the oracle's philox and Box-Muller), its arithmetic is textbook
float64 (np.cos, np.sin, solve with the covariance).  Device and restatement
are compared within 1e-9.

The slice is the likelihood-only one of Murray, Adams and MacKay.  The
reference's loop slices on the whole update weight, which counts the prior of
the moved address twice; the first CPU test pins which form is implemented.

CPU: the two targets; map_optimize's fixed point; for every setting the GPU
tests use, no decision (slice test, theta < 0, s2 - s >= 0) is within 1e-9 of
its threshold, no move is exhausted, and every outcome of each move occurs.
GPU: moved states, counts, weights and trace scores against the restatement;
an unobserved step; bit-exact self-consistency; windows; the Kalman posterior
of a 1-D model; the cap; the refusals of the C ABI.

The regression's score is an exact parabola in one address, and the
benchmark LG-SSM's (lg4, lg10: Q, R, P0 multiples of the identity, H = I) an
exact paraboloid with one curvature in every direction; no particle changes
that curvature.  For a given step size every particle improves or none does
(score change = |g|^2 step (1 - curvature step / 2)), so the three outcomes of
map_optimize (improved at once, improved after backtracking, left unchanged)
cannot meet in one setting of reg1, reg2, lg4 or lg10; these cases show them
under three settings, each for every particle.  lg3 and kit show them together.
"""
import functools

import numpy as np
import pytest

import gen_amd as gen
from gen_amd.models import BayesianLinearRegression, KitagawaSSM, LinearGaussianSSM
from oracle import oracle as O
from tests import test_grad_moves as T
from tests.test_grad_moves import case, draws, gpu_filter, oracle_filter

S_SLICE = 9
SEED = T.SEED
TOL = T.TOL
MAX_SHRINKS = 64
TWO_PI = 2 * np.pi


# ------------------------------------------------------------------ draws
@functools.lru_cache(maxsize=None)
def _sblock(seed, t, w, b, n):
    """Block b of move w's window in the shrink stream, for particles 0..n-1."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    stream = S_SLICE + 16 * (w >> 12)
    out = np.empty((n, 4), dtype=np.uint32)
    for i in range(n):
        out[i] = O.philox([i & 0xFFFFFFFF, i >> 32, t, (stream << 16) | (16 * (w & 4095) + b)], key)
    return out


def first_angle(seed, t, w, n, n_draws):
    wd = T._block(seed, t, w, 15, n_draws)[:n].astype(np.uint64)
    u = (((wd[:, 2] >> np.uint64(5)) << np.uint64(26)) | (wd[:, 3] >> np.uint64(6))).astype(np.float64) * 2.0**-53
    return TWO_PI * u


# ------------------------------------- likelihoods and priors (numpy)
def loglik_of(m, y):
    """x [n, d] -> log p(y | x) per row (0 without an observation)."""
    if y is None:
        return lambda x: np.zeros(len(x))
    if isinstance(m, LinearGaussianSSM):
        return lambda x: T._mvn_sg(np.asarray(y) - (x @ m.H.T + m.c), m.R)[0]
    if isinstance(m, KitagawaSSM):
        y0 = float(np.ravel(y)[0])
        return lambda x: -0.5 * np.log(2 * np.pi * m.var_y) - (y0 - x[:, 0] ** 2 / 20) ** 2 / (2 * m.var_y)

    def reg(x):
        r = np.asarray(y)[None, :] - (x[:, :1] * m.xs[None, :] + x[:, 1:])
        with np.errstate(over="ignore"):
            return (-0.5 * np.log(2 * np.pi * m.sigma**2) - r * r / (2 * m.sigma**2)).sum(axis=1)
    return reg


def prior_of(m, t, xp, n):
    """(mu [n, d], L [d, d]): the moved address is N(mu, L L^T) given the parent."""
    if isinstance(m, LinearGaussianSSM):
        if t == 1:
            return np.broadcast_to(m.mu0, (n, m.d)), np.linalg.cholesky(m.P0)
        return xp @ m.A.T + m.b, np.linalg.cholesky(m.Q)
    if isinstance(m, KitagawaSSM):
        if t == 1:
            return np.full((n, 1), m.mu1), np.array([[m.s1]])
        return xp / 2 + 25 * xp / (1 + xp * xp) + 8 * np.cos(1.2 * t), np.array([[np.sqrt(m.var_x)]])
    return np.broadcast_to([m.mu_s, m.mu_i], (n, 2)), np.diag([m.sd_s, m.sd_i])


# ------------------------------------------------- the moves (numpy)
class SliceChain:
    """Elliptical slice sampling on particles 0..n-1.  target: the function the
    slice is on (the log-likelihood; the whole score for the reference's form)."""

    def __init__(self, target, mu, L, x, sel, seed, t, w=0, n_draws=T.N_DRAWS):
        self.target, self.mu, self.L, self.sel = target, np.asarray(mu), np.asarray(L), sel
        self.x, self.seed, self.t, self.w, self.n_draws = np.array(x, dtype=np.float64), seed, t, w, n_draws
        self.margin = np.inf       # slice tests: |delta - log u| - 1e-9 max(1, |delta|, |loglik(x)|)
        self.margin_theta = np.inf  # theta < 0 decisions: |theta| - 1e-9
        self.shrinks = 0
        self.exhausted = 0
        self.exhausted_mask = np.zeros(len(self.x), dtype=bool)  # of the last move
        self.most, self.fewest = 0, MAX_SHRINKS  # shrinks of one particle in one move
        self.first = None  # the first proposal of the last move

    def move(self, n_moves=1):
        n, d = self.x.shape
        for _ in range(n_moves):
            z, logu = draws(self.seed, self.t, self.w, d, n, self.n_draws)
            theta = first_angle(self.seed, self.t, self.w, n, self.n_draws)
            tmin, tmax = theta - TWO_PI, theta.copy()
            nu, f, base = z @ self.L.T, self.x - self.mu, self.target(self.x)
            active, k, xnew = np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64), self.x.copy()
            for i in range(MAX_SHRINKS + 1):
                y = np.where(self.sel, self.mu + f * np.cos(theta)[:, None] + nu * np.sin(theta)[:, None], self.x)
                if i == 0:
                    self.first = y
                with np.errstate(invalid="ignore", over="ignore"):
                    delta = self.target(y) - base
                    ok = delta > logu
                    mg = np.abs(delta - logu) - 1e-9 * np.maximum(np.maximum(1.0, np.abs(delta)), np.abs(base))
                mg = mg[active & np.isfinite(mg)]
                if mg.size:
                    self.margin = min(self.margin, float(mg.min()))
                take = active & ok
                xnew[take] = y[take]
                active = active & ~ok
                if i == MAX_SHRINKS or not active.any():
                    break
                self.margin_theta = min(self.margin_theta, float(np.abs(theta[active]).min()) - 1e-9)
                neg = theta < 0
                tmin = np.where(active & neg, theta, tmin)
                tmax = np.where(active & ~neg, theta, tmax)
                v = (_sblock(self.seed, self.t, self.w, i >> 2, self.n_draws)[:n, i & 3].astype(np.float64) + 0.5) * 2.0**-32
                theta = np.where(active, tmin + v * (tmax - tmin), theta)
                k += active
            self.exhausted_mask = active
            self.exhausted += int(active.sum())
            self.shrinks += int(k.sum())
            self.most, self.fewest = max(self.most, int(k.max())), min(self.fewest, int(k.min()))
            self.x = xnew
            self.w += 1
        return self.shrinks, self.exhausted


class MapChain:
    """map_optimize on particles 0..n-1: backtracking gradient ascent on sg's score."""

    def __init__(self, sg, x, sel):
        self.sg, self.x, self.sel = sg, np.array(x, dtype=np.float64), sel
        self.s, self.g = sg(self.x)
        self.margin = np.inf  # s2 - s >= 0 decisions: |s2 - s| - 1e-9 max(1, |s2 - s|)
        self.improved = self.at_once = self.after_backtracking = self.unchanged = 0

    def iterate(self, max_step, tau, min_step, n_iters=1):
        n = len(self.x)
        for _ in range(n_iters):
            step, active, tries = np.full(n, float(max_step)), np.ones(n, dtype=bool), 0
            while active.any():
                y = np.where(self.sel, self.x + step[:, None] * self.g, self.x)
                with np.errstate(invalid="ignore", over="ignore"):
                    s2, gy = self.sg(y)
                    change = s2 - self.s
                    ok = change >= 0
                    mg = np.abs(change) - 1e-9 * np.maximum(1.0, np.abs(change))
                mg = mg[active & np.isfinite(mg)]
                if mg.size:
                    self.margin = min(self.margin, float(mg.min()))
                take = active & ok
                self.x = np.where(take[:, None], y, self.x)
                self.g = np.where(take[:, None], gy, self.g)
                self.s = np.where(take, s2, self.s)
                self.improved += int(take.sum())
                if tries == 0:
                    self.at_once += int(take.sum())
                else:
                    self.after_backtracking += int(take.sum())
                active = active & ~ok
                stop = active & (step < min_step)
                self.unchanged += int(stop.sum())
                active = active & ~stop
                step = np.where(active, step * tau, step)
                tries += 1
        return self.improved


# ----------------------------------------------------------------- cases
# map_optimize per (case, step): the settings (max_step_size, tau,
# min_step_size), chosen on the CPU so that every outcome occurs (checked
# below).  The first has the reference's tau and min_step_size; the last runs
# out after three tries.
MAP_SETTINGS = {
    ("lg3", 1): [(0.5, 0.5, 1e-16), (2.0, 0.5, 0.6)],
    ("lg3", 4): [(0.25, 0.5, 1e-16), (0.5, 0.7, 0.3)],  # (critical steps within a factor 4: tau = 0.7)
    ("kit", 1): [(20.0, 0.5, 1e-16), (20.0, 0.5, 6.0)],
    ("kit", 4): [(2.0, 0.5, 1e-16), (8.0, 0.5, 2.4)],
    # one curvature for every particle (see the module's docstring): one outcome per setting
    ("lg4", 1): [(0.5, 0.5, 1e-16), (1.0, 0.5, 1e-16), (4.0, 0.5, 1.2)],
    ("lg4", 4): [(0.12, 0.5, 1e-16), (0.25, 0.5, 1e-16), (1.0, 0.5, 0.3)],
    ("lg10", 1): [(0.5, 0.5, 1e-16), (1.0, 0.5, 1e-16), (4.0, 0.5, 1.2)],
    ("lg10", 4): [(0.12, 0.5, 1e-16), (0.25, 0.5, 1e-16), (1.0, 0.5, 0.3)],
    ("reg1", 1): [(0.004, 0.5, 1e-16), (0.008, 0.5, 1e-16), (1.0, 0.5, 0.3)],
    ("reg2", 1): [(0.15, 0.5, 1e-16), (0.3, 0.5, 1e-16), (1.0, 0.5, 0.3)],
}
ONE_CURVATURE = {"lg4", "lg10", "reg1", "reg2"}
# the filter's seed where map_optimize's conditions do not hold under SEED: at
# t = 1 the nonlinear SSM's score is nearly flat around x = 0, and a particle
# there changes its score by less than 1e-9
MAP_SEED = {("kit", 1): 18}
CASES = sorted(MAP_SETTINGS)


def map_settings(cname, t):
    return MAP_SETTINGS[cname, t]


def map_start(cname, t):
    """The restatement's start for map_optimize: (x, x_parent)."""
    name, _ = T.split(cname)
    if (cname, t) not in MAP_SEED:
        return oracle_filter(name, t)[:2]
    m, ys, n = case(name)
    pf = O.OraclePF(m, n, MAP_SEED[cname, t])
    pf.init(ys[0])
    return pf.state().T.copy(), None


def map_filter(cname, t):
    name, _ = T.split(cname)
    if (cname, t) not in MAP_SEED:
        return gpu_filter(name, t)
    m, ys, n = case(name)
    return gen.initialize_particle_filter(m, (1,), ys[0], n, seed=MAP_SEED[cname, t])


def slice_chain(cname, t, x, xp, w=0, y="case", n_draws=T.N_DRAWS):
    name, mask = T.split(cname)
    m, ys, _ = case(name)
    y = ys[t - 1] if isinstance(y, str) else y
    mu, L = prior_of(m, t, xp, len(x))
    return SliceChain(loglik_of(m, y), mu, L, x, T.sel_of(m, mask), SEED, t, w=w, n_draws=n_draws)


def map_chain(cname, t, x, xp):
    name, mask = T.split(cname)
    m, _, _ = case(name)
    return MapChain(T.sg_at(name, t, xp), x, T.sel_of(m, mask))


# ------------------------------------------------------------------- CPU
Y1 = 1.3


def _lg1_chain(n=1024, seed=3):
    m = T._lg1()
    pf = O.OraclePF(m, n, seed)
    pf.init([Y1])
    return m, pf.state().T.copy()


def _check_kalman(x, n):
    mean, var = T._kalman_x1(T._lg1(), Y1)
    return abs(x.mean() - mean) < 5 * np.sqrt(var / n) + 0.01 and abs(x.var() - var) < 0.15 * var


def test_reference_slice_chains_reach_the_posterior_only_with_the_likelihood_slice():
    """1024 chains of 40 moves from the prior of the 1-D model: the likelihood
    slice reaches the Kalman x_1 | y_1 (mean 0.722, variance 0.444); the
    reference's whole-weight slice reaches prior^2 x likelihood (mean 0.5,
    variance 0.308), 0.22 away in mean against a standard error of 0.021."""
    m, x0 = _lg1_chain()
    n = len(x0)
    mu, L = prior_of(m, 1, None, n)
    lik = SliceChain(loglik_of(m, [Y1]), mu, L, x0, np.array([True]), 3, 1, n_draws=n)
    lik.move(40)
    assert lik.exhausted == 0
    assert _check_kalman(lik.x[:, 0], n), (lik.x.mean(), lik.x.var())
    full = SliceChain(lambda x: T.lg_sg(m, 1, None, x, [Y1])[0], mu, L, x0, np.array([True]), 3, 1, n_draws=n)
    full.move(40)
    assert not _check_kalman(full.x[:, 0], n)
    assert abs(full.x.mean() - 0.5) < 5 * np.sqrt(0.308 / n) + 0.01 and abs(full.x.var() - 0.308) < 0.15 * 0.308


def test_reference_map_optimize_reaches_the_posterior_mean():
    """100 iterations with the defaults: the contraction per iteration is
    1 - 0.1 * 2.25 = 0.775 (2.25 = 1/P0 + H^2/R), 0.775^100 ~ 1e-11; the floor
    is the rounding of the score difference, about 1e-8 in x."""
    m, x0 = _lg1_chain()
    c = MapChain(lambda x: T.lg_sg(m, 1, None, x, [Y1]), x0, np.array([True]))
    c.iterate(0.1, 0.5, 1e-16, 100)
    mean, _ = T._kalman_x1(m, Y1)
    assert np.abs(c.x[:, 0] - mean).max() < 1e-6


@pytest.mark.parametrize("cname,t", CASES)
def test_slice_conditions(cname, t):
    """Conditions on the inputs of the GPU comparison (5 + 2 moves from the
    filter's particles)."""
    name, _ = T.split(cname)
    x, xp, did, _ = oracle_filter(name, t)
    assert did or t < 3
    c = slice_chain(cname, t, x, xp)
    c.move(7)
    print(f"{cname} t={t}: shrinks {c.shrinks} most {c.most} margin {c.margin:.3g} theta {c.margin_theta:.3g}")
    assert c.margin > 0 and c.margin_theta > 0
    assert c.exhausted == 0
    assert c.most >= 5 and c.fewest == 0


@pytest.mark.parametrize("cname,t", CASES)
def test_map_optimize_conditions(cname, t):
    """3 iterations per setting from the filter's particles: every outcome occurs."""
    x, xp = map_start(cname, t)
    settings = map_settings(cname, t)
    seen = np.zeros(3, dtype=np.int64)
    for k, s in enumerate(settings):
        c = map_chain(cname, t, x, xp)
        c.iterate(*s, 3)
        got = [c.at_once, c.after_backtracking, c.unchanged]
        print(f"{cname} t={t} {s}: at once {got[0]} backtracked {got[1]} unchanged {got[2]} margin {c.margin:.3g}")
        assert c.margin > 0
        assert sum(got) == 3 * len(x)
        seen += got
        if cname in ONE_CURVATURE:
            assert got[k] == 3 * len(x)  # one outcome, every particle
        else:
            assert c.at_once > 0 and c.after_backtracking > 0
            if s[2] > 1e-16:
                assert c.unchanged > 0
    assert np.all(seen > 0)


def test_conditions_of_the_window_tests():
    """The window tests start from the particles after two drift moves
    (elliptical_slice at window 2) and after map_optimize (mala at window 0)."""
    m, _, n = case("lg4")
    _, xp, _, _ = oracle_filter("lg4", 4)
    pf2 = O.OraclePF(m, n, SEED)  # a fresh filter: the cached one stays unmoved
    T._replay(pf2, "lg4", 4)
    pf2.mh_drift(1, np.full(m.d, 0.3), 2)
    c = slice_chain("lg4", 4, pf2.state().T, xp, w=2)
    c.move(3)
    assert c.margin > 0 and c.margin_theta > 0 and c.exhausted == 0
    x, _, _, _ = oracle_filter("lg4", 4)
    mc = map_chain("lg4", 4, x, xp)
    mc.iterate(*map_settings("lg4", 4)[0], 2)
    ch = T.Chain(T.sg_at("lg4", 4, xp), mc.x, T.sel_of(m, 1), SEED, 4, w=0)
    ch.mala(T.SETTINGS["lg4", 4][0], 2)
    assert mc.margin > 0 and ch.margin > 0


# the cap: sigma so small that the log-likelihood of most prior draws overflows
# to -inf.  A particle whose current and proposed log-likelihoods are all -inf
# has a NaN difference at every angle, shrinks 64 times and is exhausted.
CAP_SIGMA = 5e-154
CAP_N = 1024


@functools.lru_cache(maxsize=None)
def cap_case():
    _, ys = BayesianLinearRegression.quickstart()
    m = BayesianLinearRegression(np.arange(1.0, 11.0), sigma=CAP_SIGMA)
    pf = O.OraclePF(m, CAP_N, SEED)
    pf.init(ys)
    x = pf.state().T.copy()
    mu, L = prior_of(m, 1, None, CAP_N)
    c = SliceChain(loglik_of(m, ys), mu, L, x, np.array([True, False]), SEED, 1, n_draws=CAP_N)
    c.move(1)
    return m, ys, x, c


def _cap_classes(m, ys, x):
    """log of (sum of r^2, largest r^2) / (2 sigma^2 DBL_MAX): the log-likelihood is -inf iff one is > 0."""
    r = np.asarray(ys)[None, :] - (x[:, :1] * m.xs[None, :] + x[:, 1:])
    thr = np.log(2 * m.sigma**2) + np.log(np.finfo(np.float64).max)
    return np.log((r * r).sum(axis=1)) - thr, np.log((r * r).max(axis=1)) - thr


def test_cap_conditions():
    m, ys, x, c = cap_case()
    print(f"cap: exhausted {c.exhausted} of {CAP_N}, shrinks {c.shrinks}")
    assert 0 < c.exhausted < CAP_N
    assert np.array_equal(c.x[c.exhausted_mask], x[c.exhausted_mask])
    assert np.all(c.x[~c.exhausted_mask, 0] != x[~c.exhausted_mask, 0])
    # an exhausted particle's own log-likelihood is -inf, and robustly so
    ll = loglik_of(m, ys)(x)
    assert np.all(np.isneginf(ll[c.exhausted_mask]))
    a, b = _cap_classes(m, ys, x)
    assert np.abs(a).min() > 1e-6 and np.abs(b).min() > 1e-6
    # the finite differences that decided are far from log u relative to the log-likelihoods' size
    assert c.margin > 0


# ------------------------------------------------------------------- GPU
def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("cname,t", CASES)
def test_gpu_slice_matches_the_reference(gh_ctx, cname, t):
    name, mask = T.split(cname)
    m, _, n = case(name)
    st = gpu_filter(name, t)
    sel = T.selection(m, mask, t)
    x0, lw0 = st.states(), gen.get_log_weights(st)
    tr = gen.get_traces(st)  # taken before the moves
    score0 = np.array(tr.scores(), copy=True)
    c = slice_chain(cname, t, x0, T.parents_of(st, t))
    moves0 = st.moves
    got = [gen.elliptical_slice(st, sel, k) for k in (5, 2)]
    c.move(5)
    want = [(c.shrinks, 0)]
    c.move(2)
    want.append((c.shrinks - want[0][0], 0))
    assert c.exhausted == 0
    assert st.moves == moves0 + 2
    assert got == want
    x1 = st.states()
    np.testing.assert_allclose(x1, c.x, **TOL)
    assert not np.array_equal(x1, x0)
    if name == "reg":
        assert np.array_equal(_u64(x1[:, 2 - mask]), _u64(x0[:, 2 - mask]))  # the unselected component
    assert np.array_equal(_u64(gen.get_log_weights(st)), _u64(lw0))
    # the view taken before the moves reads the moved latents and their scores
    assert np.array_equal(_u64(tr.step_states(t).reshape(n, -1)), _u64(x1))
    score1 = np.asarray(tr.scores())
    assert not np.array_equal(score1, score0)
    np.testing.assert_allclose(score1, T.numpy_total(name, st, t), **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("cname,t", CASES)
def test_gpu_map_optimize_matches_the_reference(gh_ctx, cname, t):
    name, mask = T.split(cname)
    m, _, n = case(name)
    sel = T.selection(m, mask, t)
    for setting in map_settings(cname, t):
        st = map_filter(cname, t)
        x0, lw0 = st.states(), gen.get_log_weights(st)
        tr = gen.get_traces(st)
        score0 = np.array(tr.scores(), copy=True)
        c = map_chain(cname, t, x0, T.parents_of(st, t))
        moves0 = st.moves
        got = gen.map_optimize(st, sel, *setting, n_iters=3)
        assert got == c.iterate(*setting, 3)
        assert st.moves == moves0 + 1
        x1 = st.states()
        np.testing.assert_allclose(x1, c.x, **TOL)
        assert np.array_equal(x1, x0) == (got == 0)
        if name == "reg":
            assert np.array_equal(_u64(x1[:, 2 - mask]), _u64(x0[:, 2 - mask]))
        assert np.array_equal(_u64(gen.get_log_weights(st)), _u64(lw0))
        assert np.array_equal(_u64(tr.step_states(t).reshape(n, -1)), _u64(x1))
        score1 = np.asarray(tr.scores())
        np.testing.assert_allclose(score1, T.numpy_total(name, st, t), **TOL)
        # no particle's score went down (a kept particle's score is recomputed from the same state)
        assert np.all(score1 >= score0)
        st.close()


@pytest.mark.gpu
def test_gpu_slice_of_an_unobserved_step(gh_ctx):
    """Without an observation the likelihood is 1: every move is accepted at its first angle."""
    m, ys, n = case("lg3")
    st = gpu_filter("lg3", 2, ys=[ys[0], None])
    x0 = st.states()
    c = slice_chain("lg3", 2, x0, T.parents_of(st, 2), y=None)
    assert gen.elliptical_slice(st, T.selection(m, 1, 2), 1) == (0, 0)
    assert c.move(1) == (0, 0)
    np.testing.assert_allclose(st.states(), c.first, **TOL)
    assert not np.allclose(st.states(), x0, **TOL)


@pytest.mark.gpu
def test_gpu_moves_are_reproducible_and_split(gh_ctx):
    """Same seed, same result; 5 moves = 3 moves then 2, bit for bit."""
    m, _, n = case("lg4")
    sel, setting = T.selection(m, 1, 4), map_settings("lg4", 4)[0]
    a, b, c = (gpu_filter("lg4", 4) for _ in range(3))
    ra, rb = gen.elliptical_slice(a, sel, 5), gen.elliptical_slice(b, sel, 5)
    rc = [gen.elliptical_slice(c, sel, k) for k in (3, 2)]
    assert ra == rb == (rc[0][0] + rc[1][0], 0) and ra[0] > 0
    assert np.array_equal(_u64(a.states()), _u64(b.states()))
    assert np.array_equal(_u64(a.states()), _u64(c.states()))
    ia, ib = gen.map_optimize(a, sel, *setting, n_iters=5), gen.map_optimize(b, sel, *setting, n_iters=5)
    ic = gen.map_optimize(c, sel, *setting, n_iters=3) + gen.map_optimize(c, sel, *setting, n_iters=2)
    assert ia == ib == ic and 0 < ia <= 5 * n
    assert np.array_equal(_u64(a.states()), _u64(b.states()))
    assert np.array_equal(_u64(a.states()), _u64(c.states()))


@pytest.mark.gpu
def test_gpu_windows(gh_ctx):
    """After two drift moves elliptical_slice uses window 2; map_optimize
    leaves the window where it is (a following mala uses window 0)."""
    m, _, n = case("lg4")
    st = gpu_filter("lg4", 4)
    sel = T.selection(m, 1, 4)
    gen.mh(st, gen.gaussian_drift, (sel, 0.3), n_moves=2)
    c = slice_chain("lg4", 4, st.states(), T.parents_of(st, 4), w=2)
    assert gen.elliptical_slice(st, sel, 3) == c.move(3)
    np.testing.assert_allclose(st.states(), c.x, **TOL)
    st2 = gpu_filter("lg4", 4)
    gen.map_optimize(st2, sel, *map_settings("lg4", 4)[0], n_iters=2)
    ch = T.Chain(T.sg_at("lg4", 4, T.parents_of(st2, 4)), st2.states(), T.sel_of(m, 1), SEED, 4, w=0)
    tau = T.SETTINGS["lg4", 4][0]
    assert gen.mala(st2, sel, tau, 2) == ch.mala(tau, 2)
    np.testing.assert_allclose(st2.states(), ch.x, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lg10", "kit"])
def test_gpu_moves_do_not_depend_on_the_filter_size(gh_ctx, name):
    """At t = 1 the first 64 particles of an n = 65 filter equal those of an n = 4099 one."""
    m, ys, n = case(name)
    out = []
    for k in (65, n):
        st = gpu_filter(name, 1, n=k)
        gen.elliptical_slice(st, T.selection(m, 1, 1), 3)
        out.append(st.states()[:64].copy())
        gen.map_optimize(st, T.selection(m, 1, 1), *map_settings(name, 1)[0], n_iters=2)
        out.append(st.states()[:64].copy())
    assert np.array_equal(_u64(out[0]), _u64(out[2]))
    assert np.array_equal(_u64(out[1]), _u64(out[3]))
    assert not np.array_equal(out[0], out[1])


@pytest.mark.gpu
def test_gpu_chains_reach_the_filtering_posterior_lg1(gh_ctx):
    """x_1 | y_1 of the 1-D model (Kalman): 40 slice moves reach it; 100
    map_optimize iterations put every particle on its mean."""
    m, n = T._lg1(), 1024
    sel = gen.select(m.latent_address(1))
    mean, var = T._kalman_x1(m, Y1)
    st = gen.initialize_particle_filter(m, (1,), [Y1], n, seed=3)
    shrinks, exhausted = gen.elliptical_slice(st, sel, 40)
    assert exhausted == 0 and shrinks > 0
    x = st.states()[:, 0]
    assert abs(x.mean() - mean) < 5 * np.sqrt(var / n) + 0.01
    assert abs(x.var() - var) < 0.15 * var
    assert gen.map_optimize(st, sel, n_iters=100) > 0
    assert np.abs(st.states()[:, 0] - mean).max() < 1e-6


@pytest.mark.gpu
def test_gpu_cap(gh_ctx):
    """The moves that use all 64 shrinks are counted and leave their particle bit-identical."""
    m, ys, x, c = cap_case()
    st = gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys), CAP_N, seed=SEED)
    x0 = st.states()
    assert np.array_equal(_u64(x0), _u64(x))
    shrinks, exhausted = gen.elliptical_slice(st, gen.select("slope"), 1)  # returns: GH_OK
    assert (shrinks, exhausted) == (c.shrinks, c.exhausted)
    x1 = st.states()
    same = np.all(_u64(x1) == _u64(x0), axis=1)
    assert np.array_equal(same, c.exhausted_mask)
    np.testing.assert_allclose(x1, c.x, **TOL)


@pytest.mark.gpu
def test_gpu_refusal_on_the_multirank_path(gh_ctx):
    """One rank on the multi-rank path (gh_ctx_force_multirank) stands for a sharded filter."""
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        m = T._lg1()
        st = gen.initialize_particle_filter(m, (1,), [0.1], 64, seed=1, ctx=ctx)
        sel = gen.select(m.latent_address(1))
        x0 = st.states()
        for f in (gen.elliptical_slice, gen.map_optimize):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f(st, sel)
        assert np.array_equal(_u64(st.states()), _u64(x0))
        assert gen.mh(st, gen.gaussian_drift, (sel, 0.5)) >= 0  # the filter still works
        st.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_refusals(gh_ctx):
    from gen_amd import _lib
    from tests.test_scores import hmm

    INVAL, STATE = 1, 7  # GH_E_INVAL, GH_E_STATE
    lib = _lib.load()

    def refused(code, f, *a, **k):
        with pytest.raises(gen.GenHipError) as e:
            f(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))

    def raw(st, code, fn, *args):
        assert getattr(lib, fn)(st.h, *args) == code, (fn, args, lib.gh_last_error())

    m = T._lg1()
    st = gen.initialize_particle_filter(m, (1,), [0.1], 64, seed=1)
    sel = gen.select(m.latent_address(1))
    x0 = st.states()
    refused(INVAL, gen.elliptical_slice, st, sel, -1)  # negative counts
    refused(INVAL, gen.map_optimize, st, sel, n_iters=-1)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(INVAL, gen.map_optimize, st, sel, max_step_size=bad)
        refused(INVAL, gen.map_optimize, st, sel, min_step_size=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan):
        refused(INVAL, gen.map_optimize, st, sel, tau=bad)
    refused(INVAL, gen.map_optimize, st, sel, tau=0.999999)  # more than 1100 backtracking steps
    refused(INVAL, gen.map_optimize, st, sel, max_step_size=1e300, min_step_size=1e-300)
    assert gen.map_optimize(st, sel, max_step_size=1.0, min_step_size=1e-300, n_iters=0) == 0  # within the limit
    for mask in (0, 2):  # selection 0, or outside the step's latent addresses
        raw(st, INVAL, "gh_pf_elliptical_slice", mask, 1, None, None)
        raw(st, INVAL, "gh_pf_map_optimize", mask, 0.1, 0.5, 1e-16, 1, None)
    raw(st, INVAL, "gh_pf_elliptical_slice", 1, (1 << 24) + 1, None, None)  # more than kRejuvMaxMoves moves
    # nothing was launched and the move counter did not advance: the next valid move uses window 0
    assert np.array_equal(_u64(st.states()), _u64(x0))
    mu, L = prior_of(m, 1, None, 64)
    c = SliceChain(loglik_of(m, [0.1]), mu, L, x0, np.array([True]), 1, 1, w=0, n_draws=64)
    assert gen.elliptical_slice(st, sel, 1) == c.move(1)
    np.testing.assert_allclose(st.states(), c.x, **TOL)
    assert not np.array_equal(st.states(), x0)

    gen.maybe_resample(st, 1e9)  # after maybe_resample and before the next step
    refused(STATE, gen.elliptical_slice, st, sel)
    refused(STATE, gen.map_optimize, st, sel)
    gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), [0.3])
    sel2 = gen.select(m.latent_address(2))
    assert gen.elliptical_slice(st, sel2)[1] == 0  # a following valid call still works
    assert gen.map_optimize(st, sel2) > 0

    h = hmm()  # "not lowered": the HMM and slot-described models
    sth = gen.initialize_particle_filter(h, (1,), [0], 64, seed=1)
    refused(INVAL, gen.elliptical_slice, sth, gen.select(h.latent_address(1)))
    refused(INVAL, gen.map_optimize, sth, gen.select(h.latent_address(1)))
    sl = gen.SlotSSM({"form": "affine", "A": m.A, "b": m.b, "Q": m.Q, "mu0": m.mu0, "P0": m.P0},
                     [{"name": "y", "dist": "mvnormal", "H": m.H, "c": m.c, "R": m.R}])
    sts = gen.initialize_particle_filter(sl, (1,), {sl.obs_address(1): [0.1]}, 64, seed=1)
    for a in sl.latent_addresses(1):
        refused(INVAL, gen.elliptical_slice, sts, gen.select(a))
        refused(INVAL, gen.map_optimize, sts, gen.select(a))

    r, ys = BayesianLinearRegression.quickstart()
    str_ = gen.initialize_particle_filter(r, (r.xs,), r.constraints(ys), 64, seed=1)
    xr = str_.states()
    refused(INVAL, gen.elliptical_slice, str_, gen.select("slope", "intercept"))  # the slice moves one address
    raw(str_, INVAL, "gh_pf_elliptical_slice", 4, 1, None, None)
    raw(str_, INVAL, "gh_pf_map_optimize", 4, 0.1, 0.5, 1e-16, 1, None)
    assert np.array_equal(_u64(str_.states()), _u64(xr))
    assert gen.map_optimize(str_, gen.select("slope", "intercept"), 0.004) > 0  # map_optimize moves both
    assert gen.elliptical_slice(str_, gen.select("intercept"))[1] == 0

    k = KitagawaSSM(10.0, 1.0)  # a conditional filter
    stc = gen.initialize_conditional_particle_filter(k, (1,), [0.5], 64, [0.2], seed=1)
    refused(STATE, gen.elliptical_slice, stc, gen.select(k.latent_address(1)))
    refused(STATE, gen.map_optimize, stc, gen.select(k.latent_address(1)))
