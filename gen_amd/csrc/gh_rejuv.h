// gh_rejuv.h — rejuvenation moves on the particles of a filter.
//
// The reference leaves rejuvenation to the caller: after a step it applies
// an MH kernel to every trace, typically
//     state.traces[i], _ = mh(state.traces[i], select(:x => t))
// (src/inference/mh.jl:14-26, selection form: regenerate the selected choices
// from their prior; accept iff log(rand()) < weight), and the particle's log
// weight is left as it is (mh keeps the target of the trace).  Regenerating the
// current latent x_t from its prior given x_{t-1} gives
//     weight = log p(y_t | x'_t) - log p(y_t | x_t)
// because the transition density cancels between the new score and the
// proposal.  At t = 1 the prior is the initial-state distribution.  A static
// model with several latent addresses (the regression's :slope, :intercept)
// regenerates the selected ones only (mh(trace, select(:slope)),
// examples/regression/quickstart.jl:17-22): weight = the log-likelihood
// difference again (the selected choices' prior scores cancel, the
// unselected roots' are unchanged).
//
// The kernel arguments, the draw windows and the parts shared with the other
// moves are in gh_move_parts.h.
#pragma once
#include <type_traits>

#include "gh_move_parts.h"

namespace gh {

// the drift's standard deviation per state component (0: not selected)
struct DriftSd {
  double v[16];
};

template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock) void k_rejuv(const double* __restrict__ prm, typename Model::Params p0,
                                                  StepObs o, RejuvArgs a) {
  constexpr int D = Model::kD;
  const typename Model::Params p = p0.rebase(prm);
  const double* tab = move_tab();
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned acc = 0;
  if (j < a.n) {
    const uint64_t pid = (uint64_t)(a.lo + j);
    double x[D], xp[D], y[D];
    move_load<D, INIT>(a, j, x, xp);
    double ll = Model::loglik(p, o, x);
    for (int m = 0; m < a.n_moves; ++m) {
      Draw dr = rejuv_draw(a.move0 + (uint32_t)m);
      dr.tab = tab;
      // the prior proposal's weight increment is the observation log-density
      double ll2;
      if constexpr (INIT && std::is_same<Model, RegModel>::value)
        ll2 = Model::init_select(p, o, a.seed, pid, a.select, x, y, dr);
      else
        ll2 = INIT ? Model::init(p, o, a.seed, pid, 0, y, dr) : Model::step(p, o, a.seed, pid, a.t, 0, xp, y, dr);
      if (move_accept(a, pid, dr, ll2 - ll)) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = y[k];
        ll = ll2;
        ++acc;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, acc);
}

// mh(trace, drift, (sd,)) on every particle (src/inference/mh.jl:41-62, the
// proposal form): a Gaussian drift proposal — `@trace(normal(trace[a], sd), a)`
// for each selected latent address a of the current step (the LG-SSM's :x
// drifts componentwise by the sd vector, a diagonal mvnormal) — then
// update and accept iff log(rand()) < weight - fwd score + bwd score.  The
// drift is symmetric, its forward and backward scores are the same number
// ((x' - x)^2 = (x - x')^2 in floating point), so the acceptance ratio is the
// update weight: the step's latent and observation scores (Model::score, the
// trace's score columns) at x' minus those at x — the current step's latent
// has no children yet.  Draws: move w's window (normals from its first
// blocks, the uniform from its last).
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock) void k_mh_drift(const double* __restrict__ prm, typename Model::Params p0,
                                                     StepObs o, RejuvArgs a, DriftSd sd) {
  constexpr int D = Model::kD;
  const typename Model::Params p = p0.rebase(prm);
  const double* tab = move_tab();
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned acc = 0;
  if (j < a.n) {
    const uint64_t pid = (uint64_t)(a.lo + j);
    double x[D], xp[D], y[D], z[D + 1];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = a.x[xidx(j, k, D)];  // (in move_load: an SGPR spill for SlotModel<9, false>)
    move_parent<D, INIT>(a, j, xp);
    double lat, ob;
    Model::score(p, o, a.t, xp, x, &lat, &ob);
    double s = lat + ob;
    for (int m = 0; m < a.n_moves; ++m) {
      const Draw dr = rejuv_draw(a.move0 + (uint32_t)m);
      normals_n<D>(a.seed, pid, a.t, dr.stream, dr.base, z, tab);
#pragma unroll
      for (int k = 0; k < D; ++k) y[k] = sd.v[k] > 0.0 ? x[k] + sd.v[k] * z[k] : x[k];
      Model::score(p, o, a.t, xp, y, &lat, &ob);
      const double s2 = lat + ob;
      if (move_accept(a, pid, dr, s2 - s)) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = y[k];
        s = s2;
        ++acc;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, acc);
}

}  // namespace gh
