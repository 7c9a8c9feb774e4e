// gh_grad.h — choice_gradients of the current step's latent, and the two
// gradient moves built on it: mala and hmc on every particle of a filter.
//
// The reference computes choice_gradients(trace, selection, nothing) by reverse
// AD through the trace (src/gen_fn_interface.jl, static_ir/backprop.jl).  The
// engine's continuous families are hand-lowered (gh_models.h), so the gradient
// of the step's score s = lat + ob (Model::score) with respect to the current
// latent x[0..D) is a closed form over parameters the device already holds.
// The current step's latent has no children yet, so this is the whole of
// choice_gradients for a selection of that step's latent addresses.
//
// Grad<Model> gives, per family:
//   Ctx                       what does not depend on x (the prior mean), kept
//                             in registers across the moves of one launch
//   prep(p, o, t, xp, c)      fills Ctx once per particle
//   eval(p, o, t, c, x, g)    returns s and writes g[k] = ds/dx[k]
// eval's s is bit for bit Model::score's lat + ob (same operations, same
// order).  Every fused multiply-add is an fma(); evaluation order (the numeric
// specification of the gradient):
//
// LG-SSM (mean = b + A xp accumulated as Model::score does, mu0 at t = 1;
//   L = LQ, L0 at t = 1; "full" = t == 1 or chol(Q) not diagonal):
//   forward, i = 0..D-1:  r = x[i] - mean[i]; full: r = fma(-L[i][k], u[k], r), k = 0..i-1;
//                         u[i] = r / L[i][i]; quad = fma(u[i], u[i], quad)
//   lat = cst - 0.5 quad
//   back,    i = D-1..0:  r = u[i]; full: r = fma(-L[k][i], w[k], r), k = D-1..i+1 (descending);
//                         w[i] = r / L[i][i]; g[i] = -w[i]
//   observation (present): row r = 0..dy-1: acc = v[r]; acc = fma(-M[r][j], x[j], acc), j = 0..D-1;
//                         q2 = fma(acc, acc, q2); then g[j] = fma(M[r][j], acc, g[j]), j = 0..D-1
//                         (diagonal M: the one entry M[r][r] for both)
//   ob = cstR - 0.5 q2; s = lat + ob
// nonlinear SSM: d = x - mean; lat = -(d d) inv2 + cst; g = -(d (2 inv2));
//   present: diff = y - div20(x x); ob = -(diff diff) inv2vy + csty;
//            g = fma(diff x, inv2vy / 5, g)            (1 / (10 var_y) = inv2vy / 5)
// regression: ds = slope - mu_s, di = intercept - mu_i; lat as Model::score;
//   g0 = -(ds (2 inv2s)), g1 = -(di (2 inv2i));
//   present, i = 0..n-1: diff = y_i - (slope xs_i + intercept); ob += -(diff diff) inv2v + cst;
//            a0 = fma(diff, xs_i, a0); a1 = a1 + diff;
//   then g0 = fma(a0, 2 inv2v, g0), g1 = fma(a1, 2 inv2v, g1)
#pragma once
#include <type_traits>

#include "gh_rejuv.h"

namespace gh {

template <class Model>
struct Grad;

template <int D, int S>
struct Grad<LGModel<D, S>> {
  using Params = LGParams;
  struct Ctx {
    double mean[D];
  };
  __device__ __forceinline__ static void prep(const Params& p, const StepObs&, uint32_t t, const double* xp, Ctx& c) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double mean;
      if (t == 1) {
        mean = p.mu0[i];
      } else {
        mean = p.b[i];
#pragma unroll
        for (int k = 0; k < D; ++k) mean = fma(p.A[i * D + k], xp[k], mean);
      }
      c.mean[i] = mean;
    }
  }
  __device__ __forceinline__ static double eval(const Params& p, const StepObs& o, uint32_t t, const Ctx& c,
                                                const double* x, double* g) {
    const double* L = t == 1 ? p.L0 : p.LQ;
    const bool full = t == 1 || !(S & 1);
    double u[D];
    double quad = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double r = x[i] - c.mean[i];
      if (full) {
#pragma unroll
        for (int k = 0; k < i; ++k) r = fma(-L[i * D + k], u[k], r);
      }
      u[i] = r / L[i * D + i];
      quad = fma(u[i], u[i], quad);
    }
    const double lat = (t == 1 ? p.cst0 : p.cstQ) - 0.5 * quad;
    // grad lat = -L^-T u: back substitution, u overwritten by w = L^-T u
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
      double r = u[i];
      if (full) {
#pragma unroll
        for (int k = D - 1; k > i; --k) r = fma(-L[k * D + i], u[k], r);
      }
      u[i] = r / L[i * D + i];
      g[i] = -u[i];
    }
    if (!o.present) return lat + 0.0;
    double q2 = 0.0;
    if (S & 2) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        const double acc = fma(-p.M[r * D + r], x[r], o.v[r]);
        q2 = fma(acc, acc, q2);
        g[r] = fma(p.M[r * D + r], acc, g[r]);
      }
    } else {
      for (int r = 0; r < p.dy; ++r) {
        double acc = o.v[r];
#pragma unroll
        for (int j = 0; j < D; ++j) acc = fma(-p.M[r * D + j], x[j], acc);
        q2 = fma(acc, acc, q2);
#pragma unroll
        for (int j = 0; j < D; ++j) g[j] = fma(p.M[r * D + j], acc, g[j]);
      }
    }
    return lat + (p.cstR - 0.5 * q2);
  }
};

template <>
struct Grad<KitModel> {
  using Params = KitParams;
  struct Ctx {
    double mean, inv2, cst, gy;
  };
  __device__ __forceinline__ static void prep(const Params& p, const StepObs& o, uint32_t t, const double* xp, Ctx& c) {
    c.mean = p.mu1;
    c.inv2 = p.inv2v1;
    c.cst = p.cst1;
    if (t > 1) {
      const double v = xp[0];
      c.mean = ((v / 2.0) + 25.0 * (v / (1.0 + v * v))) + o.ct;
      c.inv2 = p.inv2vx;
      c.cst = p.cstx;
    }
    c.gy = p.inv2vy / 5.0;
  }
  __device__ __forceinline__ static double eval(const Params& p, const StepObs& o, uint32_t, const Ctx& c,
                                                const double* x, double* g) {
    const double d = x[0] - c.mean;
    const double lat = -(d * d) * c.inv2 + c.cst;
    g[0] = -(d * (2.0 * c.inv2));
    if (!o.present) return lat + 0.0;
    const double diff = o.v[0] - div20(x[0] * x[0]);
    g[0] = fma(diff * x[0], c.gy, g[0]);
    return lat + (-(diff * diff) * p.inv2vy + p.csty);
  }
};

template <>
struct Grad<RegModel> {
  using Params = RegParams;
  struct Ctx {};
  __device__ __forceinline__ static void prep(const Params&, const StepObs&, uint32_t, const double*, Ctx&) {}
  __device__ __forceinline__ static double eval(const Params& p, const StepObs& o, uint32_t, const Ctx&,
                                                const double* x, double* g) {
    const double ds = x[0] - p.mu_s, di = x[1] - p.mu_i;
    const double lat = (-(ds * ds) * p.inv2s + p.csts) + (-(di * di) * p.inv2i + p.csti);
    g[0] = -(ds * (2.0 * p.inv2s));
    g[1] = -(di * (2.0 * p.inv2i));
    if (!o.present) return lat + 0.0;
    double s = 0.0, a0 = 0.0, a1 = 0.0;
    for (int i = 0; i < p.n; ++i) {
      const double diff = o.v[i] - (x[0] * p.xs[i] + x[1]);
      s += -(diff * diff) * p.inv2v + p.cst;
      a0 = fma(diff, p.xs[i], a0);
      a1 = a1 + diff;
    }
    const double w = 2.0 * p.inv2v;
    g[0] = fma(a0, w, g[0]);
    g[1] = fma(a1, w, g[1]);
    return lat + s;
  }
};

// Occupancy targets (waves per SIMD) at which the gradient kernels carry no
// scratch, read off the cross-compile with tools/regs.py.
template <class Model>
struct GradWaves {
  static constexpr int kMala = 8, kHmc = 8, kGrad = 8;
};
template <>
struct GradWaves<RegModel> {
  static constexpr int kMala = 8, kHmc = 4, kGrad = 8;
};
template <int D, int S>
struct GradWaves<LGModel<D, S>> {
  static constexpr int kMala = D <= 2 ? 8 : (D <= 4 ? 4 : (D <= 9 ? 3 : (D == 10 ? 2 : 1)));
  static constexpr int kHmc = D <= 2 ? 8 : (D <= 4 ? 4 : (D <= 7 ? 3 : (D <= 10 ? 2 : 1)));
  static constexpr int kGrad = D <= 4 ? 8 : (D <= 10 ? 4 : 2);
};

// particle j's state x and what Grad keeps of its parent's
template <class Model, bool INIT>
__device__ __forceinline__ void grad_prep(const typename Model::Params& p, const StepObs& o, const RejuvArgs& a,
                                          int64_t j, double* x, typename Grad<Model>::Ctx& c) {
  double xp[Model::kD];
  move_load<Model::kD, INIT>(a, j, x, xp);
  Grad<Model>::prep(p, o, a.t, xp, c);
}

// choice_gradients(trace, selection) on every particle: the gradient of the
// step's score with respect to the selected components of the current latent
// (0 for unselected ones), written in the wave-tiled state layout.
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock, GradWaves<Model>::kGrad) void k_choice_gradients(
    const double* __restrict__ prm, typename Model::Params p0, StepObs o, RejuvArgs a, double* __restrict__ out) {
  constexpr int D = Model::kD;
  using G = Grad<Model>;
  const typename Model::Params p = p0.rebase(prm);
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.n) return;
  double x[D], g[D];
  typename G::Ctx c;
  grad_prep<Model, INIT>(p, o, a, j, x, c);
  G::eval(p, o, a.t, c, x, g);
#pragma unroll
  for (int k = 0; k < D; ++k) out[xidx(j, k, D)] = move_selected<Model>(a.select, k) ? g[k] : 0.0;
}

// mala(trace, selection, tau) on every particle (src/inference/mala.jl:11-54):
// with std = sqrt(2 tau), propose y_k ~ normal(x_k + tau g_k(x), std) for the
// selected components, accept iff
//   log(rand()) < (s(y) - s(x)) - sum logN(y_k; muf_k, std) + sum logN(x_k; mub_k, std),
// mub = y + tau g(y).  The normal densities' constants cancel: the two sums are
// (qf - qb) / (4 tau), qf = sum (y_k - muf_k)^2, qb = sum (x_k - mub_k)^2, each
// accumulated by fma over k ascending.  Draws: move w's window (z[k] for
// component k from its first blocks, the uniform from its last; move_accept).
// s and g of the accepted point are carried into the next move.
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock, GradWaves<Model>::kMala) void k_mala(const double* __restrict__ prm,
                                                                          typename Model::Params p0, StepObs o,
                                                                          RejuvArgs a, double tau, double sd) {
  constexpr int D = Model::kD;
  using G = Grad<Model>;
  const typename Model::Params p = p0.rebase(prm);
  const double* tab = move_tab();
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned acc = 0;
  if (j < a.n) {
    const uint64_t pid = (uint64_t)(a.lo + j);
    const double inv4tau = 1.0 / (4.0 * tau);
    double x[D], g[D], y[D], gy[D];
    typename G::Ctx c;
    grad_prep<Model, INIT>(p, o, a, j, x, c);
    double s = G::eval(p, o, a.t, c, x, g);
    for (int m = 0; m < a.n_moves; ++m) {
      const Draw dr = rejuv_draw(a.move0 + (uint32_t)m);
      double qf = 0.0;
      {
        double z[D + 1];
        normals_n<D>(a.seed, pid, a.t, dr.stream, dr.base, z, tab);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          if (move_selected<Model>(a.select, k)) {
            const double muf = fma(tau, g[k], x[k]);
            y[k] = fma(sd, z[k], muf);
            const double e = y[k] - muf;
            qf = fma(e, e, qf);
          } else {
            y[k] = x[k];
          }
        }
      }
      const double s2 = G::eval(p, o, a.t, c, y, gy);
      double qb = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (move_selected<Model>(a.select, k)) {
          const double e = x[k] - fma(tau, gy[k], y[k]);
          qb = fma(e, e, qb);
        }
      }
      if (move_accept(a, pid, dr, (s2 - s) + (qf - qb) * inv4tau)) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          x[k] = y[k];
          g[k] = gy[k];
        }
        s = s2;
        ++acc;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, acc);
}

// hmc(trace, selection; L, eps) on every particle (src/inference/hmc.jl:25-72):
// momenta p_k = z_k for the selected components, K0 = -0.5 sum p_k^2; L
// leapfrog steps  p = fma(eps/2, g(q), p); q = fma(eps, p, q); g(q) again;
// p = fma(eps/2, g(q), p);  accept iff log(rand()) < (s(q) - s(x)) + (K1 - K0),
// K1 = -0.5 sum p_k^2 of the final momenta (the sums by fma over k ascending).
// Draws as k_mala.
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock, GradWaves<Model>::kHmc) void k_hmc(const double* __restrict__ prm,
                                                                        typename Model::Params p0, StepObs o,
                                                                        RejuvArgs a, int L, double eps) {
  constexpr int D = Model::kD;
  using G = Grad<Model>;
  const typename Model::Params p = p0.rebase(prm);
  const double* tab = move_tab();
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned acc = 0;
  if (j < a.n) {
    const uint64_t pid = (uint64_t)(a.lo + j);
    const double heps = 0.5 * eps;
    double x[D], g[D], q[D], gq[D], mom[D];
    typename G::Ctx c;
    grad_prep<Model, INIT>(p, o, a, j, x, c);
    double s = G::eval(p, o, a.t, c, x, g);
    for (int m = 0; m < a.n_moves; ++m) {
      const Draw dr = rejuv_draw(a.move0 + (uint32_t)m);
      double k0 = 0.0;
      {
        double z[D + 1];
        normals_n<D>(a.seed, pid, a.t, dr.stream, dr.base, z, tab);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const bool sel = move_selected<Model>(a.select, k);
          mom[k] = sel ? z[k] : 0.0;
          if (sel) k0 = fma(z[k], z[k], k0);
          q[k] = x[k];
          gq[k] = g[k];
        }
      }
      double sq = s;
      for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          if (move_selected<Model>(a.select, k)) {
            mom[k] = fma(heps, gq[k], mom[k]);
            q[k] = fma(eps, mom[k], q[k]);
          }
        }
        sq = G::eval(p, o, a.t, c, q, gq);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          if (move_selected<Model>(a.select, k)) mom[k] = fma(heps, gq[k], mom[k]);
        }
      }
      double k1 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (move_selected<Model>(a.select, k)) k1 = fma(mom[k], mom[k], k1);
      }
      if (move_accept(a, pid, dr, (sq - s) + (-0.5 * k1 - -0.5 * k0))) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          x[k] = q[k];
          g[k] = gq[k];
        }
        s = sq;
        ++acc;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, acc);
}

}  // namespace gh
