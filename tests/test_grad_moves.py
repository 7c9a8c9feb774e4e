"""choice_gradients, mala and hmc on every particle of a filter
(src/gen_fn_interface.jl:374-406, src/inference/mala.jl:11-54,
src/inference/hmc.jl:25-72).

The reference of the two moves is a numpy restatement in this file: its draws
are exactly the device's (Philox blocks of the move's window through the
oracle's philox and Box-Muller), its arithmetic is plain float64 with the
densities written as in the textbook (solve with the covariance, not the
engine's Cholesky recurrences).  Device and reference are compared within 1e-9.

CPU: the restatement's gradients equal central finite differences of scipy
log-densities; its MALA and HMC chains reach the regression's conjugate
posterior; for every setting the GPU tests use, no acceptance decision is
within 1e-9 of its threshold (so the GPU tests may demand equal counts) and
the acceptance rate lies in 0.3-0.97.
GPU: gradients, moved states, acceptance counts and trace scores against the
restatement; bit-exact self-consistency; a closed-form Kalman posterior; the
refusals of the C ABI.
"""
import functools

import numpy as np
import pytest
from scipy import stats

import gen_amd as gen
from gen_amd.models import BayesianLinearRegression, KitagawaSSM, LinearGaussianSSM
from oracle import oracle as O

S_MH = 6
SEED = 13
N_DRAWS = 4099  # the draws of particles 0..N_DRAWS-1 are generated once per (step, move)
TOL = dict(rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ draws
@functools.lru_cache(maxsize=None)
def _block(seed, t, w, b, n):
    key = [seed & 0xFFFFFFFF, seed >> 32]
    out = np.empty((n, 4), dtype=np.uint32)
    for i in range(n):
        out[i] = O.philox([i & 0xFFFFFFFF, i >> 32, t, (S_MH << 16) | (16 * w + b)], key)
    return out


@functools.lru_cache(maxsize=None)
def _pair(seed, t, w, p, n):
    """Box-Muller pair p of move w: words 3p..3p+2 of the window's concatenated blocks."""
    first, last = (3 * p) // 4, (3 * p + 2) // 4
    words = np.concatenate([_block(seed, t, w, b, n) for b in range(first, last + 1)], axis=1)
    off = 3 * p - 4 * first
    return O.box_muller_words(words[:, off:off + 3])


def draws(seed, t, w, d, n, n_draws=N_DRAWS):
    """(z [n, d], log u [n]) of move w at step t for particles 0..n-1."""
    z = np.concatenate([_pair(seed, t, w, p, n_draws) for p in range((d + 1) // 2)], axis=1)[:n, :d]
    wd = _block(seed, t, w, 15, n_draws)[:n].astype(np.uint64)
    u = (((wd[:, 0] >> np.uint64(5)) << np.uint64(26)) | (wd[:, 1] >> np.uint64(6))).astype(np.float64) * 2.0**-53
    with np.errstate(divide="ignore"):
        return z, np.log(u)


# ------------------------------------------ scores and gradients (numpy)
def _mvn_sg(r, cov):
    """log N(r; 0, cov) per row and its gradient with respect to r."""
    cov = np.atleast_2d(cov)
    sol = np.linalg.solve(cov, r.T).T
    s = -0.5 * (r.shape[1] * np.log(2 * np.pi) + np.linalg.slogdet(cov)[1] + (r * sol).sum(axis=1))
    return s, -sol


def lg_sg(m, t, xp, x, y):
    mean, cov = (m.mu0, m.P0) if t == 1 else (xp @ m.A.T + m.b, m.Q)
    s, g = _mvn_sg(x - mean, cov)
    if y is not None:
        so, ge = _mvn_sg(np.asarray(y) - (x @ m.H.T + m.c), m.R)
        s, g = s + so, g - ge @ m.H
    return s, g


def kit_sg(m, t, xp, x, y):
    if t == 1:
        mean, var = m.mu1, m.s1**2
    else:
        mean, var = xp / 2 + 25 * xp / (1 + xp * xp) + 8 * np.cos(1.2 * t), m.var_x
    s = -0.5 * np.log(2 * np.pi * var) - (x - mean) ** 2 / (2 * var)
    g = -(x - mean) / var
    if y is not None:
        r = float(np.ravel(y)[0]) - x * x / 20
        s = s - 0.5 * np.log(2 * np.pi * m.var_y) - r * r / (2 * m.var_y)
        g = g + r * x / (10 * m.var_y)
    return s[:, 0], g


def reg_sg(m, t, xp, x, y):
    sl, ic = x[:, 0], x[:, 1]
    s = (-0.5 * np.log(2 * np.pi * m.sd_s**2) - (sl - m.mu_s) ** 2 / (2 * m.sd_s**2)
         - 0.5 * np.log(2 * np.pi * m.sd_i**2) - (ic - m.mu_i) ** 2 / (2 * m.sd_i**2))
    g = np.stack([-(sl - m.mu_s) / m.sd_s**2, -(ic - m.mu_i) / m.sd_i**2], axis=1)
    if y is not None:
        r = np.asarray(y)[None, :] - (sl[:, None] * m.xs[None, :] + ic[:, None])
        s = s + (-0.5 * np.log(2 * np.pi * m.sigma**2) - r * r / (2 * m.sigma**2)).sum(axis=1)
        g = g + np.stack([(r * m.xs).sum(axis=1), r.sum(axis=1)], axis=1) / m.sigma**2
    return s, g


def model_sg(m):
    return {LinearGaussianSSM: lg_sg, KitagawaSSM: kit_sg, BayesianLinearRegression: reg_sg}[type(m)]


def sel_of(m, mask):
    """bool [d]: every component of an Unfold latent; the mask's bits for the regression."""
    if isinstance(m, BayesianLinearRegression):
        return np.array([bool(mask & 1), bool(mask & 2)])
    return np.ones(m.d if isinstance(m, LinearGaussianSSM) else 1, dtype=bool)


# ------------------------------------------------- the moves (numpy)
class Chain:
    """The moves' restatement on particles 0..n-1: state x [n, d], move counter w."""

    def __init__(self, sg, x, sel, seed, t, w=0):
        self.sg, self.x, self.sel, self.seed, self.t, self.w = sg, np.array(x, dtype=np.float64), sel, seed, t, w
        self.s, self.g = sg(self.x)
        self.margin = np.inf  # min over decisions of |log u - alpha| - 1e-9 max(1, |alpha|)
        self.accepted = 0
        self.decisions = 0

    def _decide(self, y, sy, gy, alpha, logu):
        with np.errstate(invalid="ignore"):
            ok = logu < alpha
            m = np.abs(logu - alpha) - 1e-9 * np.maximum(1.0, np.abs(alpha))
        self.margin = min(self.margin, float(np.nanmin(np.where(np.isfinite(m), m, np.inf))))
        self.x = np.where(ok[:, None], y, self.x)
        self.g = np.where(ok[:, None], gy, self.g)
        self.s = np.where(ok, sy, self.s)
        self.accepted += int(ok.sum())
        self.decisions += ok.size
        self.w += 1
        return int(ok.sum())

    def mala(self, tau, n_moves=1):
        acc, n, d = 0, *self.x.shape
        std = np.sqrt(2 * tau)
        for _ in range(n_moves):
            z, logu = draws(self.seed, self.t, self.w, d, n)
            muf = self.x + tau * self.g
            y = np.where(self.sel, muf + std * z, self.x)
            sy, gy = self.sg(y)
            mub = y + tau * gy
            fwd = stats.norm.logpdf(y, muf, std)[:, self.sel].sum(axis=1)
            bwd = stats.norm.logpdf(self.x, mub, std)[:, self.sel].sum(axis=1)
            acc += self._decide(y, sy, gy, (sy - self.s) - fwd + bwd, logu)
        return acc

    def hmc(self, L, eps, n_moves=1):
        with np.errstate(over="ignore", invalid="ignore"):
            return self._hmc(L, eps, n_moves)

    def _hmc(self, L, eps, n_moves):
        acc, n, d = 0, *self.x.shape
        for _ in range(n_moves):  # (a diverging trajectory overflows to a NaN or -Inf alpha: rejected)
            z, logu = draws(self.seed, self.t, self.w, d, n)
            p = np.where(self.sel, z, 0.0)
            k0 = -0.5 * (p * p).sum(axis=1)
            q, sq, gq = self.x.copy(), self.s, self.g
            for _ in range(L):
                p = p + (eps / 2) * np.where(self.sel, gq, 0.0)
                q = q + eps * p
                sq, gq = self.sg(q)
                p = p + (eps / 2) * np.where(self.sel, gq, 0.0)
            k1 = -0.5 * (p * p).sum(axis=1)
            acc += self._decide(q, sq, gq, sq - self.s + k1 - k0, logu)
        return acc


# ----------------------------------------------------------------- cases
def _lg1():
    return LinearGaussianSSM([[0.9]], [[0.5]], [[1.0]], [[0.8]], [0.0], [[1.0]])


def _lg3():
    """d = 3, dense Q and a 2 x 3 H: no exact-zero structure (structure 0)."""
    return LinearGaussianSSM(
        A=[[0.8, 0.1, 0.0], [-0.1, 0.7, 0.05], [0.0, 0.1, 0.9]],
        Q=[[0.3, 0.1, 0.0], [0.1, 0.2, 0.05], [0.0, 0.05, 0.25]],
        H=[[1.0, 0.5, 0.0], [0.0, 1.0, -0.5]], R=[[0.5, 0.1], [0.1, 0.4]],
        mu0=[0.1, -0.2, 0.3], P0=[[1.0, 0.2, 0.0], [0.2, 0.8, 0.1], [0.0, 0.1, 1.2]],
        b=[0.05, 0.0, -0.05], c=[0.1, -0.1])


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, per-step observations, n)."""
    if name == "reg":
        m, ys = BayesianLinearRegression.quickstart()
        return m, [ys], 3001
    m = {"lg3": _lg3, "lg4": lambda: LinearGaussianSSM.benchmark(4), "lg10": lambda: LinearGaussianSSM.benchmark(10),
         "kit": lambda: KitagawaSSM(10.0, 1.0)}[name]()
    _, ys = m.simulate(5, np.random.default_rng(4))
    return m, list(ys), 4099


# (tau of mala, eps of hmc with L = 1, eps of hmc with L = 7) per case and step;
# chosen on the CPU so that the acceptance rates lie in 0.3-0.97 (checked below)
SETTINGS = {
    ("lg3", 1): (0.15, 0.5, 0.5), ("lg3", 4): (0.08, 0.4, 0.4),
    ("lg4", 1): (0.15, 0.5, 0.8), ("lg4", 4): (0.04, 0.3, 0.3),
    ("lg10", 1): (0.15, 0.5, 0.7), ("lg10", 4): (0.04, 0.3, 0.3),
    ("kit", 1): (2.5, 2.0, 1.6), ("kit", 4): (0.6, 1.2, 0.8),
    ("reg1", 1): (0.004, 0.08, 0.08), ("reg2", 1): (0.08, 0.5, 0.6), ("reg3", 1): (0.004, 0.08, 0.085),
}
CASES = sorted(SETTINGS)
MOVES = [("mala", 0), ("hmc", 1), ("hmc", 7)]


def split(cname):
    """case name -> (model case, selection mask)"""
    return ("reg", int(cname[3])) if cname.startswith("reg") else (cname, 1)


def selection(m, mask, t):
    if isinstance(m, BayesianLinearRegression):
        return gen.select(*[a for b, a in ((1, "slope"), (2, "intercept")) if mask & b])
    return gen.select(m.latent_address(t))


def obs_at(name, t):
    m, ys, _ = case(name)
    return ys[t - 1]


def sg_at(name, t, xp):
    m, _, _ = case(name)
    f, y = model_sg(m), obs_at(name, t)
    return lambda x: f(m, t, xp, x, y)


def apply_move(obj, kind, L, setting, n_moves, sel=None, st=None):
    """One call of the move on the restatement (obj: Chain) or on the device (obj: None, st)."""
    tau, eps1, eps7 = setting
    if st is None:
        return obj.mala(tau, n_moves) if kind == "mala" else obj.hmc(L, eps1 if L == 1 else eps7, n_moves)
    if kind == "mala":
        return gen.mala(st, sel, tau, n_moves)
    return gen.hmc(st, sel, L=L, eps=eps1 if L == 1 else eps7, n_moves=n_moves)


@functools.lru_cache(maxsize=None)
def oracle_filter(name, t):
    """The CPU oracle's particles at step t (bit for bit the device's): (x, x_parent, resampled)."""
    m, ys, n = case(name)
    pf = O.OraclePF(m, n, SEED)
    pf.init(ys[0])
    did = False
    for s in range(2, t + 1):
        did |= pf.maybe_resample(1e9 if s == 3 else None)[0]
        pf.step(ys[s - 1])
    return pf.state().T.copy(), (pf.trajectory(t - 1).T.copy() if t > 1 else None), did, pf


def gpu_filter(name, t, n=None, ys=None):
    m, ys0, n0 = case(name)
    ys, n = ys or ys0, n or n0
    if name == "reg":
        return gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys[0]), n, seed=SEED)
    st = gen.initialize_particle_filter(m, (1,), ys[0], n, seed=SEED)
    for s in range(2, t + 1):
        gen.maybe_resample(st, 1e9) if s == 3 else gen.maybe_resample(st)
        gen.particle_filter_step(st, (s,), (gen.UnknownChange(),), ys[s - 1])
    if t >= 3:
        assert st.ess_history()[1][: t - 1].any()  # a resample preceded one of the steps
    return st


def parents_of(st, t):
    n = st.n_local
    return gen.get_traces(st).step_states(t - 1).reshape(n, -1) if t > 1 else None


# ------------------------------------------------------------------- CPU
def _fd(f, x, h):
    g = np.empty_like(x)
    for k in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[k] = h
        g[:, k] = (f(x + e) - f(x - e)) / (2 * h)
    return g


def test_reference_gradients_equal_finite_differences_of_scipy_densities():
    rng = np.random.default_rng(0)
    n = 8
    for m in (_lg3(), LinearGaussianSSM.benchmark(4)):
        xp, x, y = rng.normal(size=(n, m.d)), rng.normal(size=(n, m.d)), rng.normal(size=m.dy)
        for t, yy in ((1, y), (3, y), (3, None)):
            def f(x):
                mean, cov = (np.broadcast_to(m.mu0, x.shape), m.P0) if t == 1 else (xp @ m.A.T + m.b, m.Q)
                s = np.array([stats.multivariate_normal.logpdf(x[i], mean[i], cov) for i in range(len(x))])
                if yy is not None:
                    s = s + np.array([stats.multivariate_normal.logpdf(yy, m.H @ x[i] + m.c, m.R) for i in range(len(x))])
                return s
            s, g = lg_sg(m, t, xp, x, yy)
            np.testing.assert_allclose(s, f(x), rtol=1e-12)
            np.testing.assert_allclose(g, _fd(f, x, 1e-4), rtol=1e-6)
    k = KitagawaSSM(10.0, 1.0)
    xp, x = rng.normal(0, 5, size=(n, 1)), rng.normal(0, 5, size=(n, 1))
    for t, yy in ((1, 2.5), (4, 2.5), (4, None)):
        def f(x):
            mean, sd = (k.mu1, k.s1) if t == 1 else (xp / 2 + 25 * xp / (1 + xp * xp) + 8 * np.cos(1.2 * t), np.sqrt(k.var_x))
            s = stats.norm.logpdf(x, mean, sd)
            if yy is not None:
                s = s + stats.norm.logpdf(yy, x * x / 20, np.sqrt(k.var_y))
            return s[:, 0]
        s, g = kit_sg(k, t, xp, x, None if yy is None else [yy])
        np.testing.assert_allclose(s, f(x), rtol=1e-12)
        np.testing.assert_allclose(g, _fd(f, x, 1e-4), rtol=1e-6)
    r, ys = BayesianLinearRegression.quickstart()
    x = np.stack([rng.normal(-2, 0.5, n), rng.normal(10, 2, n)], axis=1)
    for yy in (ys, None):
        def f(x):
            s = stats.norm.logpdf(x[:, 0], r.mu_s, r.sd_s) + stats.norm.logpdf(x[:, 1], r.mu_i, r.sd_i)
            if yy is not None:
                s = s + stats.norm.logpdf(yy[None, :], x[:, :1] * r.xs[None, :] + x[:, 1:], r.sigma).sum(axis=1)
            return s
        s, g = reg_sg(r, 1, None, x, yy)
        np.testing.assert_allclose(s, f(x), rtol=1e-12)
        np.testing.assert_allclose(g, _fd(f, x, 1e-4), rtol=1e-6)


def _regression_chain(n=512):
    m, ys = BayesianLinearRegression.quickstart()
    rng = np.random.default_rng(5)
    x0 = np.stack([rng.normal(m.mu_s, m.sd_s, n), rng.normal(m.mu_i, m.sd_i, n)], axis=1)
    return m, ys, x0


def _check_posterior(m, ys, x, n):
    mean, cov = m.posterior(ys)
    assert np.all(np.abs(x.mean(axis=0) - mean) < 5 * np.sqrt(np.diag(cov) / n)), (x.mean(axis=0), mean)
    np.testing.assert_allclose(np.cov(x.T), cov, rtol=0.25)


def test_reference_mala_chains_reach_the_regression_posterior():
    """400 moves on each of 512 particles, alternating mala(select(:slope)) and
    mala(select(:intercept)) with tau the conditional variances: the sign of
    the drift, of the forward and of the backward term are all pinned (a wrong
    one leaves the chain biased or stuck)."""
    m, ys, x0 = _regression_chain()
    n = len(x0)
    sg = lambda x: reg_sg(m, 1, None, x, ys)
    cs = Chain(sg, x0, np.array([True, False]), 21, 1)
    ts, ti = 1 / ((m.xs**2).sum() / m.sigma**2 + 1 / m.sd_s**2), 1 / (m.xs.size / m.sigma**2 + 1 / m.sd_i**2)
    for _ in range(200):
        cs.sel = np.array([True, False])
        cs.mala(0.7 * ts)
        cs.sel = np.array([False, True])
        cs.mala(0.7 * ti)
    assert 0.3 * cs.decisions < cs.accepted < 0.97 * cs.decisions
    _check_posterior(m, ys, cs.x, n)


def test_reference_hmc_chains_reach_the_regression_posterior():
    m, ys, x0 = _regression_chain()
    n = len(x0)
    sg = lambda x: reg_sg(m, 1, None, x, ys)
    cs = Chain(sg, x0, np.array([True, True]), 21, 1)
    for i in range(400):
        cs.hmc(L=10, eps=0.03 if i % 2 else 0.08)
    assert 0.3 * cs.decisions < cs.accepted < 0.97 * cs.decisions
    _check_posterior(m, ys, cs.x, n)


@pytest.mark.parametrize("kind,L", MOVES)
@pytest.mark.parametrize("cname,t", CASES)
def test_band_and_step_size_conditions(cname, t, kind, L):
    """Conditions on the inputs of the GPU comparisons below (5 + 2 moves from
    the filter's particles): no decision within 1e-9 max(1, |alpha|) of its
    threshold, acceptance rate in 0.3-0.97."""
    name, mask = split(cname)
    m, _, n = case(name)
    x, xp, did, _ = oracle_filter(name, t)
    assert did or t < 3
    c = Chain(sg_at(name, t, xp), x, sel_of(m, mask), SEED, t)
    apply_move(c, kind, L, SETTINGS[cname, t], 7)
    rate = c.accepted / c.decisions
    print(f"{cname} t={t} {kind} L={L}: rate {rate:.3f} margin {c.margin:.3g}")
    assert c.margin > 0
    assert 0.3 <= rate <= 0.97


def test_band_condition_of_the_window_test():
    """test_gpu_mala_after_drift_moves_uses_window_2 starts from the particles after two drift moves."""
    m, _, n = case("lg4")
    _, xp, _, pf = oracle_filter("lg4", 4)
    pf2 = O.OraclePF(m, n, SEED)  # a fresh filter: the cached one stays unmoved
    _replay(pf2, "lg4", 4)
    pf2.mh_drift(1, np.full(m.d, 0.3), 2)
    c = Chain(sg_at("lg4", 4, xp), pf2.state().T, sel_of(m, 1), SEED, 4, w=2)
    c.mala(SETTINGS["lg4", 4][0], 3)
    assert c.margin > 0


def _replay(pf, name, t):
    _, ys, _ = case(name)
    pf.init(ys[0])
    for s in range(2, t + 1):
        pf.maybe_resample(1e9 if s == 3 else None)
        pf.step(ys[s - 1])


# ------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cname,t", CASES)
def test_gpu_choice_gradients(gh_ctx, cname, t):
    name, mask = split(cname)
    m, _, n = case(name)
    st = gpu_filter(name, t)
    values, grads = gen.choice_gradients(st, selection(m, mask, t))
    x = st.states()
    assert values.shape == x.shape == grads.shape == (n, x.shape[1])
    assert np.array_equal(values.view(np.uint64), x.view(np.uint64))
    _, g = sg_at(name, t, parents_of(st, t))(x)
    np.testing.assert_allclose(grads, np.where(sel_of(m, mask), g, 0.0), **TOL)
    if name == "reg" and mask != 3:
        assert np.all(grads[:, 2 - mask] == 0.0)  # the unselected component
    # the filter is unchanged
    assert np.array_equal(st.states().view(np.uint64), x.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lg3", "lg10", "kit"])
def test_gpu_choice_gradients_of_an_unobserved_step(gh_ctx, name):
    """A step without an observation: the latent term alone."""
    m, ys, n = case(name)
    st = gpu_filter(name, 2, ys=[ys[0], None])
    _, grads = gen.choice_gradients(st, selection(m, 1, 2))
    x = st.states()
    f = model_sg(m)
    _, g_lat = f(m, 2, parents_of(st, 2), x, None)
    _, g_obs = f(m, 2, parents_of(st, 2), x, ys[1])
    np.testing.assert_allclose(grads, g_lat, **TOL)
    assert not np.allclose(g_lat, g_obs, **TOL)
    st1 = gen.initialize_particle_filter(m, (1,), None, 65, seed=SEED)
    _, g1 = gen.choice_gradients(st1, selection(m, 1, 1))
    np.testing.assert_allclose(g1, f(m, 1, None, st1.states(), None)[1], **TOL)


def numpy_total(name, st, t):
    """get_score of every particle's trace by the numpy densities along its genealogy."""
    m, ys, _ = case(name)
    tr, n = gen.get_traces(st), st.n_local
    total = np.zeros(n)
    for s in range(1, t + 1):
        xs = tr.step_states(s).reshape(n, -1)
        xps = tr.step_states(s - 1).reshape(n, -1) if s > 1 else None
        total += model_sg(m)(m, s, xps, xs, ys[s - 1])[0]
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("kind,L", MOVES)
@pytest.mark.parametrize("cname,t", CASES)
def test_gpu_moves_match_the_reference(gh_ctx, cname, t, kind, L):
    name, mask = split(cname)
    m, _, n = case(name)
    st = gpu_filter(name, t)
    sel = selection(m, mask, t)
    x0, lw0 = st.states(), gen.get_log_weights(st)
    tr = gen.get_traces(st)  # taken before the moves
    score0 = np.array(tr.scores(), copy=True)
    c = Chain(sg_at(name, t, parents_of(st, t)), x0, sel_of(m, mask), SEED, t)
    moves0 = st.moves
    acc = [apply_move(None, kind, L, SETTINGS[cname, t], k, sel=sel, st=st) for k in (5, 2)]
    want = [apply_move(c, kind, L, SETTINGS[cname, t], k) for k in (5, 2)]
    assert st.moves == moves0 + 2
    assert acc == want
    x1 = st.states()
    np.testing.assert_allclose(x1, c.x, **TOL)
    assert not np.array_equal(x1, x0)
    if name == "reg" and mask != 3:
        assert np.array_equal(x1[:, 2 - mask].view(np.uint64), x0[:, 2 - mask].view(np.uint64))
    assert np.array_equal(gen.get_log_weights(st).view(np.uint64), lw0.view(np.uint64))
    # the view taken before the moves reads the moved latents and their scores
    assert np.array_equal(tr.step_states(t).reshape(n, -1).view(np.uint64), x1.view(np.uint64))
    score1 = np.asarray(tr.scores())
    assert not np.array_equal(score1, score0)
    np.testing.assert_allclose(score1, numpy_total(name, st, t), **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,L", [("mala", 0), ("hmc", 7)])
def test_gpu_moves_are_reproducible_and_split(gh_ctx, kind, L):
    """Same seed, same result; 5 moves = 3 moves then 2 (the carried score and
    gradient equal the re-evaluated ones, the windows continue)."""
    m, _, n = case("lg4")
    sel, setting = selection(m, 1, 4), SETTINGS["lg4", 4]
    a, b, c = (gpu_filter("lg4", 4) for _ in range(3))
    acc_a = apply_move(None, kind, L, setting, 5, sel=sel, st=a)
    acc_b = apply_move(None, kind, L, setting, 5, sel=sel, st=b)
    acc_c = apply_move(None, kind, L, setting, 3, sel=sel, st=c) + apply_move(None, kind, L, setting, 2, sel=sel, st=c)
    assert acc_a == acc_b == acc_c and 0 < acc_a < 5 * n
    xa = a.states().view(np.uint64)
    assert np.array_equal(xa, b.states().view(np.uint64))
    assert np.array_equal(xa, c.states().view(np.uint64))


@pytest.mark.gpu
def test_gpu_mala_after_drift_moves_uses_window_2(gh_ctx):
    m, _, n = case("lg4")
    st = gpu_filter("lg4", 4)
    sel = selection(m, 1, 4)
    gen.mh(st, gen.gaussian_drift, (sel, 0.3), n_moves=2)
    c = Chain(sg_at("lg4", 4, parents_of(st, 4)), st.states(), sel_of(m, 1), SEED, 4, w=2)
    tau = SETTINGS["lg4", 4][0]
    assert gen.mala(st, sel, tau, 3) == c.mala(tau, 3)
    np.testing.assert_allclose(st.states(), c.x, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lg10", "kit"])
def test_gpu_moves_do_not_depend_on_the_filter_size(gh_ctx, name):
    """At t = 1 the first 64 particles of an n = 65 filter equal those of an n = 4099 one."""
    m, ys, n = case(name)
    tau, _, eps7 = SETTINGS[name, 1]
    out = []
    for k in (65, n):
        st = gpu_filter(name, 1, n=k)
        gen.mala(st, selection(m, 1, 1), tau, 3)
        gen.hmc(st, selection(m, 1, 1), L=7, eps=eps7, n_moves=2)
        out.append(st.states()[:64].copy())
        _, g = gen.choice_gradients(st, selection(m, 1, 1))
        out.append(g[:64].copy())
    assert np.array_equal(out[0].view(np.uint64), out[2].view(np.uint64))
    assert np.array_equal(out[1].view(np.uint64), out[3].view(np.uint64))


def _kalman_x1(m, y1):
    P0, H, R = m.P0[0, 0], m.H[0, 0], m.R[0, 0]
    k = P0 * H / (H * P0 * H + R)
    return m.mu0[0] + k * (y1 - H * m.mu0[0]), (1 - k * H) * P0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mala", "hmc"])
def test_gpu_chains_reach_the_filtering_posterior_lg1(gh_ctx, kind):
    """x_1 | y_1 of a 1-D LG model (Kalman): 400 MALA moves, 150 HMC moves."""
    m, n = _lg1(), 1024
    st = gen.initialize_particle_filter(m, (1,), [1.3], n, seed=3)
    sel = gen.select(m.latent_address(1))
    mean, var = _kalman_x1(m, 1.3)
    if kind == "mala":
        acc, moves = gen.mala(st, sel, 0.4, 400), 400
    else:
        acc, moves = gen.hmc(st, sel, L=5, eps=0.35, n_moves=150), 150
    assert 0.3 * n * moves < acc < 0.99 * n * moves
    x = st.states()[:, 0]
    assert abs(x.mean() - mean) < 5 * np.sqrt(var / n) + 0.01
    assert abs(x.var() - var) < 0.15 * var


@pytest.mark.gpu
def test_gpu_refusal_on_the_multirank_path(gh_ctx):
    """One rank on the multi-rank path (gh_ctx_force_multirank) stands for a sharded filter."""
    ctx = gen.Context(device=0, force_multirank=True)
    try:
        m = _lg1()
        st = gen.initialize_particle_filter(m, (1,), [0.1], 64, seed=1, ctx=ctx)
        sel = gen.select(m.latent_address(1))
        x0 = st.states()
        for f, a in ((gen.mala, (0.1,)), (gen.hmc, ()), (gen.choice_gradients, ())):
            with pytest.raises(gen.GenHipError, match="GH_E_STATE"):
                f(st, sel, *a)
        assert np.array_equal(st.states().view(np.uint64), x0.view(np.uint64))
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

    m = _lg1()
    st = gen.initialize_particle_filter(m, (1,), [0.1], 64, seed=1)
    sel = gen.select(m.latent_address(1))
    x0 = st.states()
    g = np.empty((1, 64))
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(INVAL, gen.mala, st, sel, bad)
        refused(INVAL, gen.hmc, st, sel, 3, bad)
    refused(INVAL, gen.hmc, st, sel, 0, 0.1)  # L < 1
    refused(INVAL, gen.mala, st, sel, 0.1, -1)  # n_moves < 0
    refused(INVAL, gen.hmc, st, sel, 3, 0.1, -1)
    for mask in (0, 2):  # selection 0, or outside the step's latent addresses
        raw(st, INVAL, "gh_pf_mala", mask, 0.1, 1, None)
        raw(st, INVAL, "gh_pf_hmc", mask, 3, 0.1, 1, None)
        raw(st, INVAL, "gh_pf_choice_gradients", mask, None, _lib.dptr(g))
    raw(st, INVAL, "gh_pf_mala", 1, 0.1, (1 << 24) + 1, None)  # more than kRejuvMaxMoves moves at one step
    raw(st, INVAL, "gh_pf_hmc", 1, 3, 0.1, (1 << 24) + 1, None)
    # nothing was launched and the move counter did not advance: the next valid move uses window 0
    assert np.array_equal(st.states().view(np.uint64), x0.view(np.uint64))
    z, _ = draws(1, 1, 0, 1, 64, n_draws=64)
    assert gen.mala(st, sel, 0.2, 1) > 0
    y = x0 + 0.2 * lg_sg(m, 1, None, x0, [0.1])[1] + np.sqrt(0.4) * z
    x1 = st.states()
    assert np.all(np.isclose(x1, y, **TOL) | (x1 == x0)) and np.any(x1 != x0)

    gen.maybe_resample(st, 1e9)  # after maybe_resample and before the next step
    refused(STATE, gen.mala, st, sel, 0.1)
    refused(STATE, gen.hmc, st, sel)
    refused(STATE, gen.choice_gradients, st, sel)
    gen.particle_filter_step(st, (2,), (gen.UnknownChange(),), [0.3])
    assert gen.mala(st, gen.select(m.latent_address(2)), 0.1) >= 0  # a following valid call still works
    assert gen.hmc(st, gen.select(m.latent_address(2))) >= 0
    assert gen.choice_gradients(st, gen.select(m.latent_address(2)))[1].shape == (64, 1)

    h = hmm()  # "not lowered": the HMM and slot-described models
    sth = gen.initialize_particle_filter(h, (1,), [0], 64, seed=1)
    refused(INVAL, gen.mala, sth, gen.select(h.latent_address(1)), 0.1)
    refused(INVAL, gen.hmc, sth, gen.select(h.latent_address(1)))
    refused(INVAL, gen.choice_gradients, sth, gen.select(h.latent_address(1)))
    sl = gen.SlotSSM({"form": "affine", "A": m.A, "b": m.b, "Q": m.Q, "mu0": m.mu0, "P0": m.P0},
                     [{"name": "y", "dist": "mvnormal", "H": m.H, "c": m.c, "R": m.R}])
    sts = gen.initialize_particle_filter(sl, (1,), {sl.obs_address(1): [0.1]}, 64, seed=1)
    for a in sl.latent_addresses(1):
        refused(INVAL, gen.mala, sts, gen.select(a), 0.1)
        refused(INVAL, gen.hmc, sts, gen.select(a))
        refused(INVAL, gen.choice_gradients, sts, gen.select(a))

    r, ys = BayesianLinearRegression.quickstart()  # the regression at t != 1
    str_ = gen.initialize_particle_filter(r, (r.xs,), r.constraints(ys), 64, seed=1)
    assert gen.mala(str_, gen.select("slope"), 0.002) >= 0
    raw(str_, INVAL, "gh_pf_mala", 4, 0.1, 1, None)

    k = KitagawaSSM(10.0, 1.0)  # a conditional filter
    stc = gen.initialize_conditional_particle_filter(k, (1,), [0.5], 64, [0.2], seed=1)
    refused(STATE, gen.mala, stc, gen.select(k.latent_address(1)), 0.1)
    refused(STATE, gen.hmc, stc, gen.select(k.latent_address(1)))
    refused(STATE, gen.choice_gradients, stc, gen.select(k.latent_address(1)))
