// gh_slice.h — elliptical slice sampling and map_optimize on every particle
// of a filter: the two per-trace kernels of src/inference/ that have neither a
// proposal nor an acceptance ratio of the Metropolis kind.
//
//   reference                                              here
//   elliptical_slice(trace, addr, mu, cov)                 k_elliptical_slice<Model, INIT>
//     src/inference/elliptical_slice.jl:13-45                (the likelihood-only slice, below)
//   map_optimize(trace, selection; max_step_size, tau,     k_map_optimize<Model, INIT>
//     min_step_size)  src/inference/map_optimize.jl:9-41
//
// Both move the current step's latent (the address that has no children yet) of
// the LG-SSM, of the nonlinear SSM and of the regression, one particle per
// lane; the state, the prior mean (Grad<Model>::Ctx) and, for map_optimize, the
// score and its gradient stay in registers for all moves of one launch.
//
// Elliptical slice sampling (Murray, Adams, MacKay 2010) needs a Gaussian prior
// N(mu, Sigma) of the moved address and a likelihood.  mu and Sigma = L L^T are
// the model's own prior of the address given the particle's parent, so they
// are not arguments.  The slice is on the LIKELIHOOD alone: accept x' iff
//   loglik(x') - loglik(x) > log u.
// elliptical_slice.jl:32-41 compares the whole update weight, which also
// holds the prior ratio of the moved address, and so leaves prior^2 x
// likelihood invariant; this is the one place where the engine deliberately
// does not reproduce the reference's arithmetic.
//
// Numeric specification of move w of the step (dr = rejuv_draw(w); every
// multiply-add written fma is fused, nothing else is):
//   z[0..D)   normals_n<D> at (dr.stream, dr.base), as k_mala draws it
//   nu = L z  LG-SSM: L = LQ (L0 at t = 1); nu_i = 0, then nu_i = fma(L[i][k], z[k], nu_i),
//               k = 0..i ascending; chol(Q) diagonal and t > 1: k = i alone
//             nonlinear SSM: nu = sx z[0] (s1 z[0] at t = 1)
//             regression: nu = sd_s z[0] (:slope) or sd_i z[1] (:intercept), the one selected address
//   mu        LG-SSM: Grad::prep's mean; nonlinear SSM: Ctx.mean; regression: mu_s or mu_i
//   f = x - mu
//   log u = gh_log(u53(b.x, b.y)), theta = 6.283185307179586 u53(b.z, b.w) with
//           b = block dr.base + kRejuvDraws - 1 of dr.stream;
//           theta_min = theta - 6.283185307179586, theta_max = theta
//   x'_k = fma(nu_k, sin theta, fma(f_k, cos theta, mu_k))  (unselected k: x_k)
//   sin, cos  slice_sincos: k = rint(theta 2/pi), r = theta - k pi/2 by the three-part
//             reduction of gh_cos, the Taylor kernels of gh_math.h at r, the quadrant by selects
//   accept iff loglik(x') - loglik(x) > log u  (Model::loglik; the accepted
//             loglik is carried); a NaN difference shrinks
//   shrink i (from 0): theta < 0 ? theta_min = theta : theta_max = theta;
//             v = ((double)word + 0.5) 2^-32, word = word (i & 3) of block
//             dr.base + (i >> 2) of stream STREAM_SLICE + 16 (w >> 12);
//             theta = fma(v, theta_max - theta_min, theta_min)
//   cap       a move whose kSliceMaxShrinks-th shrunk angle still fails leaves
//             the particle where it is and counts as exhausted
//
// map_optimize, per iteration: s, g = Grad::eval(x) (carried from the accepted
// point); step = max_step_size; loop: y_k = fma(step, g_k, x_k) for the selected
// k; s2, gy = eval(y); s2 - s >= 0: take y (one improved), else step <
// min_step_size: keep x, else step = step tau.  A NaN difference is "worse".
#pragma once
#include "gh_grad.h"

namespace gh {

enum : uint32_t { STREAM_SLICE = 9 };  // shrink uniforms (+16 k as rejuv_draw)
constexpr uint32_t kSliceMaxShrinks = 4 * kRejuvDraws;  // the window's 16 blocks x 4 words
constexpr int kMapMaxBacktracks = 1100;                 // tau = 0.5 from 1 down to 1e-300

// sin and cos of an angle in (-2 pi, 2 pi) (any moderate |x|, as gh_cos)
__device__ __forceinline__ void slice_sincos(double x, double* s, double* c) {
  const double k = rint(x * 0x1.45f306dc9c883p-1);  // 2/pi
  double r = fma(-k, 1.57079632673412561417e+00, x);
  r = fma(-k, 6.07710050630396597660e-11, r);
  r = fma(-k, 2.02226624871116645580e-21, r);
  const double sk = sin_kernel(r), ck = cos_kernel(r);
  const int q = ((int)k) & 3;
  // q=0: (sk, ck)  q=1: (ck, -sk)  q=2: (-sk, -ck)  q=3: (-ck, sk)
  const double s0 = (q & 1) ? ck : sk;
  const double c0 = (q & 1) ? sk : ck;
  *s = (q >= 2) ? -s0 : s0;
  *c = (q == 1 || q == 2) ? -c0 : c0;
}

// The Gaussian prior of the moved address given the parent: its mean (once per
// particle) and nu = L z (once per move).
template <class Model>
struct SlicePrior;

template <int D, int S>
struct SlicePrior<LGModel<D, S>> {
  using G = Grad<LGModel<D, S>>;
  __device__ __forceinline__ static void mean(const LGParams&, const typename G::Ctx& c, double* mu) {
#pragma unroll
    for (int i = 0; i < D; ++i) mu[i] = c.mean[i];
  }
  __device__ __forceinline__ static void nu(const LGParams& p, uint32_t t, const double* z, double* v) {
    const double* L = t == 1 ? p.L0 : p.LQ;
    const bool full = t == 1 || !(S & 1);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double acc = 0.0;
      if (full) {
#pragma unroll
        for (int k = 0; k < i; ++k) acc = fma(L[i * D + k], z[k], acc);
      }
      v[i] = fma(L[i * D + i], z[i], acc);
    }
  }
};

template <>
struct SlicePrior<KitModel> {
  __device__ __forceinline__ static void mean(const KitParams&, const Grad<KitModel>::Ctx& c, double* mu) {
    mu[0] = c.mean;
  }
  __device__ __forceinline__ static void nu(const KitParams& p, uint32_t t, const double* z, double* v) {
    v[0] = (t == 1 ? p.s1 : p.sx) * z[0];
  }
};

template <>
struct SlicePrior<RegModel> {
  __device__ __forceinline__ static void mean(const RegParams& p, const Grad<RegModel>::Ctx&, double* mu) {
    mu[0] = p.mu_s;
    mu[1] = p.mu_i;
  }
  __device__ __forceinline__ static void nu(const RegParams& p, uint32_t, const double* z, double* v) {
    v[0] = p.sd_s * z[0];
    v[1] = p.sd_i * z[1];
  }
};

// Occupancy targets (waves per SIMD) at which the two kernels carry no
// scratch, read off the cross-compile with tools/regs.py.
template <class Model>
struct SliceWaves {
  static constexpr int kSlice = 8, kMap = 8;
};
template <int D, int S>
struct SliceWaves<LGModel<D, S>> {
  static constexpr int kSlice = GradWaves<LGModel<D, S>>::kMala;
  static constexpr int kMap = GradWaves<LGModel<D, S>>::kMala;
};

// elliptical_slice on every particle; a.accepted counts the shrinks,
// `exhausted` the moves that ran into the cap.
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock, SliceWaves<Model>::kSlice) void k_elliptical_slice(
    const double* __restrict__ prm, typename Model::Params p0, StepObs o, RejuvArgs a,
    unsigned long long* __restrict__ exhausted) {
  constexpr int D = Model::kD;
  using G = Grad<Model>;
  using P = SlicePrior<Model>;
  const typename Model::Params p = p0.rebase(prm);
  const double* tab = move_tab();
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned shr = 0, exh = 0;
  if (j < a.n) {
    const uint64_t pid = (uint64_t)(a.lo + j);
    constexpr double kTwoPi = 6.283185307179586;
    double x[D], mu[D], f[D], nu[D], y[D];
    {
      double xp[D];
      typename G::Ctx c;
      move_load<D, INIT>(a, j, x, xp);
      G::prep(p, o, a.t, xp, c);
      P::mean(p, c, mu);
    }
    double ll = Model::loglik(p, o, x);
    for (int m = 0; m < a.n_moves; ++m) {
      const uint32_t w = a.move0 + (uint32_t)m;
      const Draw dr = rejuv_draw(w);
      const uint32_t sstream = (uint32_t)STREAM_SLICE + ((w >> 12) << 4);
      {
        double z[D + 1];
        normals_n<D>(a.seed, pid, a.t, dr.stream, dr.base, z, tab);
        P::nu(p, a.t, z, nu);
      }
#pragma unroll
      for (int k = 0; k < D; ++k) f[k] = x[k] - mu[k];
      const u32x4 b = move_uniform_block(a, pid, dr);
      const double logu = move_logu(b);
      double theta = kTwoPi * u53(b.z, b.w);
      double tmin = theta - kTwoPi, tmax = theta;
      u32x4 sw{0, 0, 0, 0};
      uint32_t i = 0;
      for (;;) {
        double sn, cs;
        slice_sincos(theta, &sn, &cs);
#pragma unroll
        for (int k = 0; k < D; ++k)
          y[k] = move_selected<Model>(a.select, k) ? fma(nu[k], sn, fma(f[k], cs, mu[k])) : x[k];
        const double ll2 = Model::loglik(p, o, y);
        if (ll2 - ll > logu) {
#pragma unroll
          for (int k = 0; k < D; ++k) x[k] = y[k];
          ll = ll2;
          break;
        }
        if (i == kSliceMaxShrinks) {
          ++exh;
          break;
        }
        if (theta < 0.0)
          tmin = theta;
        else
          tmax = theta;
        if ((i & 3u) == 0) sw = rng_block(a.seed, pid, a.t, sstream, dr.base + (i >> 2));
        const uint32_t e = i & 3u;
        const uint32_t word = e == 0 ? sw.x : (e == 1 ? sw.y : (e == 2 ? sw.z : sw.w));
        const double v = ((double)word + 0.5) * 0x1p-32;
        theta = fma(v, tmax - tmin, tmin);
        ++i;
      }
      shr += i;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, shr);
  move_count(exhausted, exh);
}

// map_optimize on every particle, a.n_moves iterations; a.accepted counts the
// iterations that improved.  No draws, no LDS table.  The host bounds the
// backtracking by its arguments (at most kMapMaxBacktracks evaluations per
// iteration); the loop counter repeats that bound.
template <class Model, bool INIT>
__global__ __launch_bounds__(kBlock, SliceWaves<Model>::kMap) void k_map_optimize(
    const double* __restrict__ prm, typename Model::Params p0, StepObs o, RejuvArgs a, double max_step, double tau,
    double min_step) {
  constexpr int D = Model::kD;
  using G = Grad<Model>;
  const typename Model::Params p = p0.rebase(prm);
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned imp = 0;
  if (j < a.n) {
    double x[D], g[D], y[D], gy[D];
    typename G::Ctx c;
    {
      double xp[D];
      move_load<D, INIT>(a, j, x, xp);
      G::prep(p, o, a.t, xp, c);
    }
    double s = G::eval(p, o, a.t, c, x, g);
    for (int m = 0; m < a.n_moves; ++m) {
      double step = max_step;
      for (int b = 0; b < kMapMaxBacktracks; ++b) {
#pragma unroll
        for (int k = 0; k < D; ++k) y[k] = move_selected<Model>(a.select, k) ? fma(step, g[k], x[k]) : x[k];
        const double s2 = G::eval(p, o, a.t, c, y, gy);
        if (s2 - s >= 0.0) {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            x[k] = y[k];
            g[k] = gy[k];
          }
          s = s2;
          ++imp;
          break;
        }
        if (step < min_step) break;
        step *= tau;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) a.x[xidx(j, k, D)] = x[k];
  }
  move_count(a.accepted, imp);
}

}  // namespace gh
