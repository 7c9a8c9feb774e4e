"""The step kernel's LDS-staged ancestor gather (k_step<LGModel<10, 3>, false>:
three of the five component pairs of x_{t-1} go through LDS-DMA)
against the CPU oracle, bit for bit after every step.

d = 10 `LinearGaussianSSM.benchmark`, resampling before every step (thr = n),
so every step gathers; both the call-by-call loop and gh_pf_run.  Sizes: a
partial wave (lanes past n do not load), a second block with one live lane,
more than one resample tile, and a size that is no multiple of anything.  The
peaked case gives nearly all 64 lanes of every wave the same ancestor; the
multi-rank context takes the paths that load x_{t-1} into registers first
(the split step's instantiation, and the general path of the waves that hold
received rows) and must agree as well.
"""
import functools

import numpy as np
import pytest

import gen_amd as gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = 10
STEPS = 6
SEED = 17
SIZES = [1, 63, 64, 65, 257, 4097, 20011]
PEAKED_N = 4133  # 64 full tiles and a partial one: the last source tile has 37 particles


@functools.lru_cache(maxsize=None)
def _model():
    return gen.LinearGaussianSSM.benchmark(D)


@functools.lru_cache(maxsize=None)
def _observations(peaked):
    _, ys = _model().simulate(STEPS + 1, np.random.default_rng(5))
    ys = np.array(ys, dtype=np.float64)
    if peaked:
        # far from every particle: the nearest one takes all the weight, and the
        # resample before the next step hands its row to every slot
        ys[2] += 400.0
        ys[4] -= 250.0
    ys.setflags(write=False)
    return ys


@functools.lru_cache(maxsize=None)
def _oracle(n, peaked):
    """(log-weights, states, parents) of the oracle after each step t = 2 .. STEPS + 1,
    and whether it resampled before it; computed once per case."""
    m, ys = _model(), _observations(peaked)
    orc = O.OraclePF(m, n, SEED, O.SYSTEMATIC)
    orc.init(ys[0])
    snaps = []
    for t in range(2, STEPS + 2):
        did, _ = orc.maybe_resample(n)
        orc.step(ys[t - 1])
        snap = (orc.log_weights(), orc.state(), orc.parents(), bool(did))
        for a in snap[:3]:
            a.setflags(write=False)
        snaps.append(snap)
    return tuple(snaps)


def _same(st, snap, what):
    lw, x, par, _ = snap
    assert np.array_equal(gen.get_log_weights(st).view(np.uint64), lw.view(np.uint64)), what
    assert np.array_equal(st.states().T.view(np.uint64), x.view(np.uint64)), what
    assert np.array_equal(st.parents, par), what


def _init(n, peaked, ctx=None):
    m, ys = _model(), _observations(peaked)
    return gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, n, seed=SEED, ctx=ctx)


def _call_by_call(n, peaked, ctx=None):
    m, ys, snaps = _model(), _observations(peaked), _oracle(n, peaked)
    st = _init(n, peaked, ctx)
    try:
        for t in range(2, STEPS + 2):
            did = gen.maybe_resample(st, n)
            assert did == snaps[t - 2][3], f"resample decision differs at t={t}"
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})
            _same(st, snaps[t - 2], f"call by call, n={n}, t={t}")
    finally:
        st.close()


def _batched(n, peaked, ctx=None):
    """gh_pf_run over the first k steps, k = 1 .. STEPS: every step's result is
    compared, each after a loop in which the earlier steps wrote block maxima
    only and the fused resample summed the weights."""
    ys, snaps = _observations(peaked), _oracle(n, peaked)
    for k in range(1, STEPS + 1):
        st = _init(n, peaked, ctx)
        try:
            gen.run_particle_filter(st, list(ys[1:k + 1]), n)
            _same(st, snaps[k - 1], f"gh_pf_run, n={n}, {k} steps")
        finally:
            st.close()


@pytest.mark.parametrize("n", SIZES)
def test_staged_gather_call_by_call(gh_ctx, n):
    _call_by_call(n, False)


@pytest.mark.parametrize("n", SIZES)
def test_staged_gather_batched_run(gh_ctx, n):
    _batched(n, False)


def test_staged_gather_peaked_weights(gh_ctx):
    snaps = _oracle(PEAKED_N, True)
    # the case is what it claims: after the far observations one parent holds
    # (nearly) every slot, later the parents spread again, up to the partial tile
    for s in (2, 4):
        assert np.bincount(snaps[s][2]).max() > PEAKED_N - 64
    assert len(np.unique(snaps[STEPS - 1][2])) > 64
    assert any(snap[2].max() >= (PEAKED_N // 64) * 64 for snap in snaps)
    _call_by_call(PEAKED_N, True)
    _batched(PEAKED_N, True)


def test_register_paths_agree_on_multirank_context(gh_ctx):
    ctx = gen.Context(device=0, force_multirank=True)  # one rank on the multi-rank path
    try:
        _call_by_call(4097, False, ctx)
        _batched(4097, False, ctx)
    finally:
        ctx.close()
