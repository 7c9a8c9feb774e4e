"""Pin the bits of the seven per-particle moves (gh_rejuv.h, gh_grad.h, gh_slice.h).

The move tests compare with numpy restatements at 1e-9, which a reordered fma
or a changed draw window of one word would pass.  Here every move's result is
pinned bit for bit: tests/golden/move_pins.json holds, per case, the SHA-256 of
the state bytes after each of two calls of 3 moves (the second call starts at
window 3, so the step's move counter is pinned too) and the calls' integer
counters.  choice_gradients is pinned by the digest of its gradient array.

The pins were recorded once, in a process of its own, from the library of the
commit before the moves' shared parts (gh_move_parts.h) existed:
    GEN_HIP_LIB=<that commit's libgen_hip.so> python tests/test_move_pins.py --record
A change of any bit is a bug of the change, not a reason to record again.

n = 300: one full block and a partial one whose last wave is partial (the
counters' wave sum with idle lanes, the bounds test).  t = 1 is the INIT
instantiation; at t = 3 a forced resample precedes steps 2 and 3, so the
parent rows are read through the ancestors.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gen_amd as gen  # noqa: E402
from gen_amd.models import BayesianLinearRegression, DiscreteHMM, KitagawaSSM, LinearGaussianSSM  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "move_pins.json")
N = 300
SEED = 13
ALL = ("rejuvenate", "mh_drift", "choice_gradients", "mala", "hmc", "elliptical_slice", "map_optimize")
CAP_SIGMA = 5e-154  # test_slice_moves.py's cap: most prior draws have a log-likelihood of -inf


def _dense4():
    """d = 4, dy = 3, dense A, Q, H, R, P0: structure 0."""
    rng = np.random.default_rng(11)
    d, dy = 4, 3
    A = 0.3 * rng.standard_normal((d, d))
    G = rng.standard_normal((d, d))
    H = rng.standard_normal((dy, d))
    F = rng.standard_normal((dy, dy))
    P = rng.standard_normal((d, d))
    return LinearGaussianSSM(A, G @ G.T / d + 0.2 * np.eye(d), H, F @ F.T / dy + 0.3 * np.eye(dy),
                             rng.standard_normal(d), P @ P.T / d + 0.5 * np.eye(d), b=rng.standard_normal(d),
                             c=rng.standard_normal(dy))


def _lg1():
    return LinearGaussianSSM([[0.9]], [[0.5]], [[1.0]], [[0.8]], [0.0], [[1.0]])


def _hmm():
    prior = np.array([0.2, 0.3, 0.5])
    T = np.array([[0.1, 0.2, 0.7], [0.2, 0.7, 0.1], [0.7, 0.2, 0.1]]).T
    E = np.array([[0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]]).T
    return DiscreteHMM(prior, T, E)


def _slots():
    m = _lg1()
    return gen.SlotSSM({"form": "affine", "A": m.A, "b": m.b, "Q": m.Q, "mu0": m.mu0, "P0": m.P0},
                       [{"name": "y", "dist": "mvnormal", "H": m.H, "c": m.c, "R": m.R}])


# name -> (model, the moves pinned, their settings: drift sd, mala tau, hmc eps (L = 3), map_optimize
# max_step_size: above the stability limit, so that the first evaluations are worse and the step is halved)
MODELS = {
    "lg1": (_lg1, ALL, (0.5, 0.3, 0.4, 2.0)),
    "lg4s0": (_dense4, ALL, (0.3, 0.05, 0.2, 2.0)),
    "lg10s3": (lambda: LinearGaussianSSM.benchmark(10), ALL, (0.2, 0.04, 0.3, 1.0)),
    "kit": (lambda: KitagawaSSM(10.0, 1.0), ALL, (1.0, 0.6, 0.8, 20.0)),
    "reg": (lambda: BayesianLinearRegression.quickstart()[0], ALL, (0.05, 0.004, 0.08, 0.016)),
    "hmm": (_hmm, ("rejuvenate",), None),
    "slots": (_slots, ("rejuvenate", "mh_drift"), (0.5, None, None, None)),
}
CASES = [(name, t, mv) for name, (_, moves, _) in MODELS.items() for t in ((1,) if name == "reg" else (1, 3))
         for mv in moves]
CASES += [("cap", 1, "elliptical_slice"), ("lg4s0_multirank", 3, "rejuvenate"), ("lg4s0_multirank", 3, "mh_drift")]


def _observations(name, m):
    """The observations of steps 1..3 as initialize_particle_filter and the step take them."""
    if name == "reg":
        return [m.constraints(BayesianLinearRegression.quickstart()[1])]
    if name == "hmm":
        return [[0], [1], [2]]
    if name == "slots":
        return [{m.obs_address(t): [v]} for t, v in ((1, 0.1), (2, 0.3), (3, -0.4))]
    return list(m.simulate(3, np.random.default_rng(4))[1])


def _filter(name, t, ctx=None):
    base = name.split("_")[0]
    if base == "cap":
        m = BayesianLinearRegression(np.arange(1.0, 11.0), sigma=CAP_SIGMA)
        ys = BayesianLinearRegression.quickstart()[1]
        return m, gen.initialize_particle_filter(m, (m.xs,), m.constraints(ys), N, seed=SEED)
    m = MODELS[base][0]()
    obs = _observations(base, m)
    kw = {} if ctx is None else {"ctx": ctx}
    st = gen.initialize_particle_filter(m, (m.xs,) if base == "reg" else (1,), obs[0], N, seed=SEED, **kw)
    for s in range(2, t + 1):
        assert gen.maybe_resample(st, 1e9)  # the parent rows go through the ancestors
        gen.particle_filter_step(st, (s,), (gen.UnknownChange(),), obs[s - 1])
    return m, st


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _run(name, t, move, ctx=None):
    """What is pinned of one case: [[counter(s), digest] per call]."""
    m, st = _filter(name, t, ctx)
    base = name.split("_")[0]
    if base in ("reg", "cap"):
        sel = gen.select("slope")  # one address
    else:
        sel = gen.select(*m.latent_addresses(t))
    sd, tau, eps, step = MODELS[base][2] if base in MODELS and MODELS[base][2] else (None,) * 4
    out = []
    try:
        if move == "choice_gradients":
            x0 = st.states()
            values, grads = gen.choice_gradients(st, sel)
            assert np.array_equal(values.view(np.uint64), x0.view(np.uint64))
            return [[0, _digest(grads)]]
        for _ in range(1 if base == "cap" else 2):
            if move == "rejuvenate":
                c = gen.mh(st, sel, 3)
            elif move == "mh_drift":
                c = gen.mh(st, gen.gaussian_drift, (sel, sd), n_moves=3)
            elif move == "mala":
                c = gen.mala(st, sel, tau, 3)
            elif move == "hmc":
                c = gen.hmc(st, sel, L=3, eps=eps, n_moves=3)
            elif move == "elliptical_slice":
                c = list(gen.elliptical_slice(st, sel, 1 if base == "cap" else 3))
            else:
                c = gen.map_optimize(st, sel, step, 0.5, step / 5, n_iters=3)  # backtracks, and gives up below step / 5
            out.append([c, _digest(st.states())])
    finally:
        st.close()
    return out


def _key(name, t, move):
    return f"{name}/t{t}/{move}"


def _run_case(name, t, move):
    if not name.endswith("_multirank"):
        return _run(name, t, move)
    ctx = gen.Context(device=0, force_multirank=True)  # one rank on the multi-rank path
    try:
        return _run(name, t, move, ctx)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,t,move", CASES, ids=[_key(*c) for c in CASES])
def test_move_bits(gh_ctx, name, t, move):
    with open(PINS) as f:
        want = json.load(f)[_key(name, t, move)]
    got = _run_case(name, t, move)
    assert [c for c, _ in got] == [c for c, _ in want]  # the counters first: the more readable difference
    assert got == want


def test_pins_cover_the_cases_and_are_not_degenerate():
    with open(PINS) as f:
        pins = json.load(f)
    assert sorted(pins) == sorted(_key(*c) for c in CASES)
    for (name, t, move) in CASES:
        calls = pins[_key(name, t, move)]
        if move == "choice_gradients":
            continue
        assert len(calls) == (1 if name == "cap" else 2)
        # the second call moved particles (map_optimize may have converged in the first: kit at t = 3)
        assert calls[0][1] != calls[-1][1] or len(calls) == 1 or (move == "map_optimize" and calls[1][0] == 0)
        total = calls[0][0][0] if isinstance(calls[0][0], list) else calls[0][0]
        assert 0 < total <= (64 if move == "elliptical_slice" else 1) * 3 * N
    shrinks, exhausted = pins[_key("cap", 1, "elliptical_slice")][0][0]
    assert 0 < exhausted < N and shrinks >= 64 * exhausted


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: GEN_HIP_LIB=<library> python tests/test_move_pins.py --record")
    gen.set_default_context(gen.Context(device=0))
    pins = {}
    for case in CASES:
        pins[_key(*case)] = _run_case(*case)
        print(_key(*case), [c for c, _ in pins[_key(*case)]], flush=True)
    with open(os.environ.get("MOVE_PINS_OUT", PINS), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
