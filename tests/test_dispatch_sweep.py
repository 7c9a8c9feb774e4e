"""Every instantiated shape through the host's dispatch (gh_api.hip: with_model,
launch_step and the dimension switches of the estimate, quantile and path
calls), one small filter per shape.

The parity tests elsewhere pin the kernels on a few shapes each; here the point
is the route: that a model of dimension d, structure S and proposal reaches
the instantiation made for it, at every d = 1..16.

1. LGSSM: d x structure x proposal {default, optimal, linear}, init and three
   steps with a resample forced before every step, n = 300 (one full block of
   256 particles and a partial one): log-weights, states and parents bit for
   bit against the oracle after every step (run_both of test_gpu_parity.py;
   the linear proposal driven as in test_lg_linear_proposal.py).
2. estimate, quantiles, estimate_path and quantiles_path: every d at n = 65,
   by the checks of test_estimates.py, test_quantiles.py and test_path.py.

The slot models' default route (with_model) is swept by test_slots_matrix.py.
Their linear proposal (SlotLinModel<d, EXT>) has no sweep: its extended
kernels of d = 2..5 are wrong on the device and must not run there until the
cause is found, and launch_step's ladder to them is the
one part of the dispatch that stays hand-written.

The structure of an LG model (LGModel<d, S>, S = 1 for a diagonal chol(Q), + 2
for a diagonal whitened observation matrix with dy = d) is chosen inside
gh_model_create and nothing in the C ABI or the Python package reports it.
structure_of restates that rule on the model's own matrices and every case
asserts that its model (test_smooth.py's _lg_shaped) has the structure it is
named for.  At d = 1 the 1 x 1 factor of Q has no off-diagonal entry, so S is
odd for every model: LGModel<1, 0> and LGModel<1, 2> cannot be reached through
the API and have no case.
"""
import functools

import numpy as np
import pytest

import gen_amd as gen
from oracle import oracle as O
from tests import test_estimates as TE
from tests import test_path as TP
from tests import test_quantiles as TQ
from tests.test_gpu_parity import assert_lml_close, run_both
from tests.test_lg_linear_proposal import _args, _flat
from tests.test_smooth import _lg_shaped

pytestmark = pytest.mark.gpu

DS = list(range(1, 17))
N = 300  # one full block of 256 particles and a partial one
T = 4
THR = N + 1  # ESS <= N: every maybe_resample fires (the optimal proposal's first weights are equal, ESS = N)
SEED = 37
PROPOSALS = ("default", "optimal", "linear")
LG_CASES = [(d, s, p) for d in DS for s in range(4) if d > 1 or s & 1 for p in PROPOSALS]


def structure_of(m):
    """gh_model_create's rule on the model's matrices: bit 0 for a diagonal
    chol(Q), bit 1 for dy = d and a diagonal chol(R)^-1 H."""
    d, dy = m.d, np.asarray(m.H).shape[0]
    LQ = np.linalg.cholesky(np.asarray(m.Q, dtype=np.float64))
    M = np.linalg.solve(np.linalg.cholesky(np.asarray(m.R, dtype=np.float64)), np.asarray(m.H, dtype=np.float64))
    lq_diag = not np.tril(LQ, -1).any()
    m_diag = dy == d and not (M - np.diag(np.diag(M))).any()
    return (1 if lq_diag else 0) | (2 if m_diag else 0)


@functools.lru_cache(maxsize=None)
def lg_case(d, s):
    """(model of structure s, observations of steps 1..T)"""
    dy = d if s & 2 else (d - 1 if d > 1 else 2)  # (d + dy <= 32: the optimal and linear proposals' limit)
    m, ys = _lg_shaped(d, dense_q=not s & 1, dy=dy)()
    return m, ys[:T]


@pytest.mark.parametrize("d,s,proposal", LG_CASES, ids=[f"d{d}-s{s}-{p}" for d, s, p in LG_CASES])
def test_lgssm_every_shape_and_proposal_bitexact(gh_ctx, d, s, proposal):
    m, ys = lg_case(d, s)
    assert structure_of(m) == s
    if proposal != "linear":
        st, orc = run_both(m, ys, N, SEED, thr=THR, proposal=gen.OptimalProposal if proposal == "optimal" else None)
    else:
        rng = np.random.default_rng(5)
        full = [_flat(*_args(m, rng, 1.0 + 0.5 * (t % 3))) for t in range(T)]
        st = gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, gen.LinearGaussianProposal,
                                            (full[0],), N, seed=SEED)
    try:
        if proposal == "linear":
            orc = O.OraclePF(m, N, SEED)
            orc.set_proposal_args(full[0])
            orc.init(ys[0], O.LINEAR)
            for t in range(2, T + 1):
                assert gen.maybe_resample(st, THR) and orc.maybe_resample(THR)[0]
                args = (full[t - 1],) if t % 2 == 0 else (full[t - 1][-d:],)  # full arguments, then u alone
                gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]},
                                         gen.LinearGaussianProposal, args)
                orc.set_proposal_args(args[0])
                orc.step(ys[t - 1], O.LINEAR)
                assert np.array_equal(gen.get_log_weights(st).view(np.uint64), orc.log_weights().view(np.uint64)), t
                assert np.array_equal(st.states().T.view(np.uint64), orc.state().view(np.uint64)), t
                assert np.array_equal(st.parents, orc.parents()), t
        assert st.ess_history()[1][: T - 1].all(), "a resample before every step"
        assert_lml_close(st, orc)
    finally:
        st.close()


@pytest.mark.parametrize("d", DS)
def test_summaries_every_dimension(gh_ctx, d):
    """k_est_mean / k_est_cov / k_qt_hist and their path forms at every d: a
    filter of 65 particles (one tile and one particle) over four steps with
    resamples before steps 3 (fires) and 2, 4 (do not)."""
    m, ys = TE._model(d), TE._observations(d)
    st = TE._init(m, ys, 65)
    try:
        TP._pattern(st, m, ys, steps=3)
        for t in (None, 1, 2):
            TE.check(st, t, what=f"d={d}")
            TQ.check(st, t, what=f"d={d}")
        path = TP.check_equal(st, what=f"d={d}")
        TP.check_diagnostics(st, path, what=f"d={d}")
    finally:
        st.close()
