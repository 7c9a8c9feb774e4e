"""Row-tiled state slots (d = 10: a particle's components one contiguous
80-byte row, `state_rows` / `xidx` in gh_kernels.h) against the
CPU oracle, bit for bit after every step.

d = 10 `LinearGaussianSSM.benchmark`, call by call and through gh_pf_run.
With a resample before every step (thr = n) every step gathers rows by
ancestor and stores them transposed through LDS: a partial wave (rows past n
are not stored), a block with one live lane, more than one resample tile, an
odd size.  With thr = 0 no resample fires: the identity read and accumulating
log-weights.  Peaked observations give every lane of a wave the same row.
Without history the two ping-pong slots are both read and written as rows.
The multi-rank context (RCCL and peer transport at world 1) runs the split
step, whose part 2 writes its rows straight from the lanes, the general path
and the received rows.  Then every reader of the layout after three steps:
states, a trajectory, the score columns, a rejuvenation and a drift move,
choice_gradients.  d = 9 and d = 11 keep the pair tiles.
"""
import functools

import numpy as np
import pytest

import gen_amd as gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STEPS = 4
SEED = 23
SIZES = [1, 63, 64, 65, 257, 4097, 20011]
PEAKED_N = 4133  # 64 full tiles and a partial one: the last source tile has 37 particles


@functools.lru_cache(maxsize=None)
def _model(d=10):
    return gen.LinearGaussianSSM.benchmark(d)


@functools.lru_cache(maxsize=None)
def _observations(d=10, peaked=False):
    _, ys = _model(d).simulate(STEPS + 1, np.random.default_rng(5))
    ys = np.array(ys, dtype=np.float64)
    if peaked:
        # far from every particle: the nearest one takes all the weight, and the
        # resample before the next step hands its row to every slot
        ys[1] += 400.0
        ys[3] -= 250.0
    ys.setflags(write=False)
    return ys


@functools.lru_cache(maxsize=None)
def _oracle(n, thr, d=10, peaked=False):
    """(log-weights, states, parents, resampled) of the oracle after each step
    t = 2 .. STEPS + 1; computed once per case and left unchanged."""
    m, ys = _model(d), _observations(d, peaked)
    orc = O.OraclePF(m, n, SEED, O.SYSTEMATIC)
    orc.init(ys[0])
    snaps = []
    for t in range(2, STEPS + 2):
        did, _ = orc.maybe_resample(thr)
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


def _init(n, d=10, peaked=False, ctx=None, **kw):
    m, ys = _model(d), _observations(d, peaked)
    return gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, n, seed=SEED, ctx=ctx, **kw)


def _call_by_call(n, thr, d=10, peaked=False, ctx=None, **kw):
    m, ys, snaps = _model(d), _observations(d, peaked), _oracle(n, thr, d, peaked)
    st = _init(n, d, peaked, ctx, **kw)
    try:
        for t in range(2, STEPS + 2):
            did = gen.maybe_resample(st, thr)
            assert did == snaps[t - 2][3], f"resample decision differs at t={t}"
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})
            _same(st, snaps[t - 2], f"call by call, d={d}, n={n}, thr={thr}, t={t}")
    finally:
        st.close()


def _batched(n, thr, d=10, peaked=False, ctx=None, **kw):
    """gh_pf_run over the first k steps, k = 1 .. STEPS, each compared."""
    ys, snaps = _observations(d, peaked), _oracle(n, thr, d, peaked)
    for k in range(1, STEPS + 1):
        st = _init(n, d, peaked, ctx, **kw)
        try:
            gen.run_particle_filter(st, list(ys[1:k + 1]), thr)
            _same(st, snaps[k - 1], f"gh_pf_run, d={d}, n={n}, thr={thr}, {k} steps")
        finally:
            st.close()


@pytest.mark.parametrize("n", SIZES)
def test_rows_resample_every_step_call_by_call(gh_ctx, n):
    assert n == 1 or all(s[3] for s in _oracle(n, n))  # (one particle: ESS = n, no resample)
    _call_by_call(n, n)


@pytest.mark.parametrize("n", SIZES)
def test_rows_resample_every_step_batched_run(gh_ctx, n):
    _batched(n, n)


@pytest.mark.parametrize("n", SIZES)
def test_rows_no_resample_call_by_call(gh_ctx, n):
    assert not any(s[3] for s in _oracle(n, 0))
    _call_by_call(n, 0)


@pytest.mark.parametrize("n", SIZES)
def test_rows_no_resample_batched_run(gh_ctx, n):
    _batched(n, 0)


def test_rows_peaked_weights(gh_ctx):
    n = PEAKED_N
    snaps = _oracle(n, n, 10, True)
    # the case is what it claims: after a far observation one parent holds
    # (nearly) every slot, and a later resample reaches into the partial tile
    for s in (1, 3):
        assert np.bincount(snaps[s][2]).max() > n - 64
    assert any(snap[2].max() >= (n // 64) * 64 for snap in snaps)
    _call_by_call(n, n, peaked=True)
    _batched(n, n, peaked=True)


@pytest.mark.parametrize("n", [257, 4097])
def test_rows_without_history(gh_ctx, n):
    _call_by_call(n, n, record_history=False)
    _batched(n, n, record_history=False)


@pytest.mark.parametrize("transport", ["rccl", "peer"])
def test_rows_on_multirank_context(gh_ctx, transport):
    if transport == "peer":
        from gen_amd.transport import LocalTransport

        ctx = gen.Context(device=0, transport=LocalTransport(), peer=True, force_multirank=True)
    else:
        ctx = gen.Context(device=0, force_multirank=True)  # one rank on the multi-rank path
    try:
        _call_by_call(4097, 4097, ctx=ctx)
        _batched(4097, 4097, ctx=ctx)
    finally:
        ctx.close()


# ------------------------------------------------- readers of the layout
def _pair(n, steps=3):
    """A filter and the oracle after `steps` steps with a resample before each."""
    m, ys = _model(), _observations()
    st = _init(n)
    orc = O.OraclePF(m, n, SEED, O.SYSTEMATIC)
    orc.init(ys[0])
    for t in range(2, steps + 2):
        assert gen.maybe_resample(st, n) and orc.maybe_resample(n)[0]
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})
        orc.step(ys[t - 1])
    return m, ys, st, orc


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("n", [257, 4097])
def test_rows_states_trajectory_and_scores(gh_ctx, n):
    m, ys, st, orc = _pair(n)
    try:
        assert _bits_equal(st.states().T, orc.state())
        T = st.t
        for t in range(1, T + 1):  # k_traj along the genealogy, every recorded slot
            assert _bits_equal(st.states(t).T, orc.trajectory(t)), f"trajectory of step {t}"
        tot, ps = gen.get_traces(st).scores(per_step=True)
        otot, ops = orc.scores(per_step=True)
        assert _bits_equal(tot, otot) and _bits_equal(ps, ops)
    finally:
        st.close()


@pytest.mark.parametrize("n", [257, 4097])
def test_rows_rejuvenation_and_drift_moves(gh_ctx, n):
    m, ys, st, orc = _pair(n)
    try:
        T = st.t
        sel = gen.select(m.latent_address(T))
        acc = gen.rejuvenate(st, 2)
        assert acc == orc.rejuvenate(2) and 0 < acc
        assert _bits_equal(st.states().T, orc.state())
        acc = gen.mh(st, gen.gaussian_drift, (sel, 0.2), n_moves=3)
        assert acc == orc.mh_drift(1, np.full(m.d, 0.2), 3) and 0 < acc < 3 * n
        assert _bits_equal(st.states().T, orc.state())
        assert _bits_equal(gen.get_log_weights(st), orc.log_weights())
    finally:
        st.close()


@pytest.mark.parametrize("n", [257, 4097])
def test_rows_choice_gradients(gh_ctx, n):
    """values = the states, bit for bit; the gradient of the trace's score in x_T
    is Q^-1 (A x_{T-1} + b - x_T) + H' R^-1 (y_T - H x_T - c), restated in numpy
    from the oracle's states (float64 on both sides: 1e-9 of the gradient's scale)."""
    m, ys, st, orc = _pair(n)
    try:
        T = st.t
        values, grads = gen.choice_gradients(st, gen.select(m.latent_address(T)))
        x, xp = orc.state().T, orc.trajectory(T - 1).T
        assert _bits_equal(values, x)
        b = np.zeros(m.d) if getattr(m, "b", None) is None else np.asarray(m.b)
        c = np.zeros(len(ys[T - 1])) if getattr(m, "c", None) is None else np.asarray(m.c)
        A, Q, H, R = (np.asarray(v, dtype=np.float64) for v in (m.A, m.Q, m.H, m.R))
        want = np.linalg.solve(Q, (xp @ A.T + b - x).T).T + np.linalg.solve(R, (ys[T - 1] - x @ H.T - c).T).T @ H
        assert np.allclose(grads, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    finally:
        st.close()


@pytest.mark.parametrize("d", [9, 11])
def test_neighbouring_dimensions_keep_pair_tiles(gh_ctx, d):
    _call_by_call(257, 257, d=d)
    _batched(257, 257, d=d)
    _call_by_call(257, 0, d=d)
