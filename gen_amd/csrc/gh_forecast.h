// gh_forecast.h — h-step-ahead predictive moments and draws of a filter
// (gh_pf_forecast): x_{T+k} and y_{T+k}, k = 1..H, given the data up to T.
//
// In Gen: particle_filter_step!(copy, (T+k,), (UnknownChange(),), EmptyChoiceMap())
// (particle_filter.jl:139-160) — the Unfold extended by update with no
// constraints (unfold/update.jl:54-78), weight increment exactly 0 — and :y
// drawn as simulate draws it (static_ir/simulate.jl:23-34).
//
//   x_{T+k}^i = Model::step(p, o_{T+k} unobserved, seed, lo + i, T+k, proposal 0,
//               x_{T+k-1}^i, ., Draw{STREAM_STEP, 0})      the filter's own counters
//   y_{T+k}^i = Model::sim_obs(p, seed, lo + i, T+k, x_{T+k}^i, ...)   simulate's noise
//
//   k_forecast<Model, 0>  per block and horizon: sum w, sum w x_k, sum w y_r; with
//                         samples, x stored as [H][d][n] and y as [H][dy][n]
//   k_forecast<Model, 1>  the same propagation again (the draws are counter-based),
//                         the upper triangles of sum w (x - m)(x - m)^T and
//                         sum w (y - m)(y - m)^T with their delta terms, m the
//                         pass-0 means read from device memory
//   k_fc_fold             a block per horizon: the partial rows summed in block
//                         order, then the division (k_est_fold's formulas)
//
// One lane per particle: est_tiles (gh_moments.h) loads the state and the
// weight once, the state stays in registers for the H transitions.  After each
// transition the wave's sums (DPP) are added by lane 0 into the wave's own LDS
// accumulators [hc][sums]; the block's waves are added in wave order at the
// end.  y has a run-time length: it lives in a column of the wave's LDS region
// at stride 64 (the region est_tiles stages a row tile in — free once the
// state is in registers).  The horizon is split over blockIdx.y into chunks of
// hc steps so that the accumulators fit (fc_plan); a chunk's blocks propagate
// from T+1 to their first horizon without accumulating.  Without samples the
// traffic to HBM does not depend on H.  No atomics, a grid that depends on
// (n, H) and the model's sizes only, every sum in a fixed order.
#pragma once
#include "gh_moments.h"
#include "gh_slots.h"
#include "gh_shapes.h"

namespace gh {

constexpr int kFcMaxHorizon = 64;          // the interface's limit (bounds the partials buffer)
constexpr int kFcMaxBlocks = 1024;         // blocks of a pass along x at most
constexpr int kFcLdsBytes = 64 * 1024;     // dynamic LDS of a block at most

// sums per horizon: pass 0 (W, x, y), pass 1 (est_entries of x, then of y)
__host__ __device__ constexpr int fc_sums(int D, int dy, int pass) {
  return pass ? est_entries(D) + est_entries(dy) : 1 + D + dy;
}
// doubles of a horizon's result block: W, mean x, mean y, cov x, cov y
__host__ __device__ constexpr int fc_result_doubles(int D, int dy) { return 1 + D + dy + D * D + dy * dy; }
// a wave's LDS region: the staged row tile while loading, the y column after
__host__ __device__ constexpr int fc_stage_bytes(int D) { return state_rows(D) ? kTileP * D * 8 : 0; }
__host__ __device__ constexpr int fc_wave_bytes(int D, int dy) {
  return fc_stage_bytes(D) > dy * kTileP * 8 ? fc_stage_bytes(D) : dy * kTileP * 8;
}
__host__ __device__ constexpr int fc_lds_bytes(int D, int dy, int pass, int nw, int hc) {
  return kMathTabDoubles * 8 + nw * (fc_wave_bytes(D, dy) + hc * fc_sums(D, dy, pass) * 8);
}

// The launch shape of a pass: the most waves per block (4, 2, 1) whose
// accumulators of at least one horizon fit, the fewest chunks at that width,
// and the chunks evened out.
struct FcPlan {
  int nw, hc, chunks, lds;
};
inline FcPlan fc_plan(int D, int dy, int pass, int H) {
  FcPlan pl{};
  for (int nw = kBlock / 64; nw >= 1; nw /= 2) {
    const int room = kFcLdsBytes - fc_lds_bytes(D, dy, pass, nw, 0);
    const int fit = room / (nw * fc_sums(D, dy, pass) * 8);
    if (room < 0 || fit < 1) continue;
    pl.nw = nw;
    pl.chunks = (H + fit - 1) / fit;
    pl.hc = (H + pl.chunks - 1) / pl.chunks;
    pl.lds = fc_lds_bytes(D, dy, pass, nw, pl.hc);
    break;
  }
  return pl;
}

struct FcArgs {
  EstArgs e;            // the particles and their weights (t_target = t_cur = T; e.part: [H][sums][gridDim.x])
  const StepObs* obs;   // [H] the unobserved steps' constants (Kitagawa ct, slot inputs)
  uint64_t seed;
  int64_t lo;           // global id of the first particle
  int H, hc, dy;
  const double* res;    // [H][fc_result_doubles]: pass 1 reads the means
  double* sx;           // pass 0: [H][D][n] latent draws, or null
  double* sy;           //         [H][dy][n] observation draws, or null
};

// The observation draw into the wave's LDS column (y_r at y[r * kTileP]).
template <class Model>
struct FcObs {
  __device__ __forceinline__ static void run(const typename Model::Params& p, uint64_t seed, uint64_t pid, uint32_t t,
                                             const double* x, double* y, const double* tab) {
    Model::sim_obs(p, seed, pid, t, x, y, kTileP, tab);
  }
};
// LGModel::sim_obs keeps z and L_R^{-1}(y - c) in private arrays of kMaxObs
// indexed at run time (scratch), for a score nobody reads here.  The same y,
// operation for operation — acc = c_r, fma over H_r x ascending, then over
// L_R[r][k] z_k, k ascending — with the normals consumed pair by pair as
// normals_rt generates them and y_r accumulated in the column.
template <int D, int S>
struct FcObs<LGModel<D, S>> {
  __device__ __forceinline__ static void run(const LGParams& p, uint64_t seed, uint64_t pid, uint32_t t,
                                             const double* x, double* y, const double* tab) {
    const int dy = p.dy;
    for (int r = 0; r < dy; ++r) {
      double acc = p.cv[r];
#pragma unroll
      for (int j = 0; j < D; ++j) acc = fma(p.H[r * D + j], x[j], acc);
      y[r * kTileP] = acc;
    }
    u32x4 w{0, 0, 0, 0};
    int cur = -1;
    for (int q = 0; 2 * q < dy; ++q) {
      uint32_t wd[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k = 3 * q + i;
        if ((k >> 2) != cur) {
          cur = k >> 2;
          w = rng_block(seed, pid, t, STREAM_SIM, kSimObsDraw + (uint32_t)cur);
        }
        const int e = k & 3;
        wd[i] = e == 0 ? w.x : (e == 1 ? w.y : (e == 2 ? w.z : w.w));
      }
      double z0, z1;
      box_muller(wd[0], wd[1], wd[2], &z0, &z1, tab);
      const int k = 2 * q;
      for (int r = k; r < dy; ++r) {
        double acc = fma(p.LR[r * dy + k], z0, y[r * kTileP]);
        if (r > k) acc = fma(p.LR[r * dy + k + 1], z1, acc);
        y[r * kTileP] = acc;
      }
    }
  }
};

template <class Model, int PASS>
__global__ __launch_bounds__(kBlock) void k_forecast(const double* __restrict__ prm, typename Model::Params p0,
                                                     FcArgs a) {
  constexpr int D = Model::kD;
  // a model whose step makes out-of-line calls: the wave index in a scalar
  // register, the lane counted again after every call (gh_kernels.h makes_calls)
  constexpr bool CALLS = makes_calls<Model>::value;
  const typename Model::Params p = p0.rebase(prm);
  extern __shared__ __attribute__((aligned(16))) char fc_lds[];  // (no static LDS: the base stays 16-byte aligned)
  const int nw = (int)blockDim.x >> 6;
  const int ws = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int dy = a.dy, hc = a.hc;
  const int E = fc_sums(D, dy, PASS);
  const int wbytes = fc_wave_bytes(D, dy);
  double* const tab = (double*)fc_lds;
  char* const region = fc_lds + kMathTabDoubles * 8;
  double* const acc_all = (double*)(region + nw * wbytes);
  double* const ycol = (double*)(region + ws * wbytes);
  double* const acc = acc_all + ws * hc * E;
  // est_tiles stages wave w at stage + w * (a row tile): that is this wave's region
  est_d2* const stage = (est_d2*)(region + ws * (wbytes - fc_stage_bytes(D)));
  load_math_tab(tab);
  for (int i = threadIdx.x; i < nw * hc * E; i += blockDim.x) acc_all[i] = 0.0;
  lds_barrier();
  const int k0 = (int)blockIdx.y * hc;  // this chunk's horizons: k0 < k <= k1
  const int k1 = k0 + hc < a.H ? k0 + hc : a.H;
  const int64_t n = a.e.n;
  const Draw dr{STREAM_STEP, 0, tab};
  const int R = fc_result_doubles(D, dy);

  est_tiles<D>(a.e, stage, [&](double wt, const double* x0, int64_t j0) {
    const int tile = CALLS ? __builtin_amdgcn_readfirstlane((int)(j0 >> 6)) : (int)(j0 >> 6);
    int lane = threadIdx.x & 63;
    double x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = j0 < n ? x0[i] : 0.0;  // (a tail lane steps a valid state; its weight is 0)
#pragma unroll 1
    for (int k = 1; k <= k1; ++k) {
      const StepObs& o = a.obs[k - 1];
      const uint32_t t = (uint32_t)(a.e.t_cur + k);
      {
        const uint64_t pid = (uint64_t)(a.lo + ((int64_t)tile * kTileP + lane));
        double xn[D];
        Model::step(p, o, a.seed, pid, t, 0, x, xn, dr);
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = xn[i];
      }
      if (k <= k0) continue;
      if constexpr (CALLS) lane = lane_now();
      double* const y = ycol + lane;
      FcObs<Model>::run(p, a.seed, (uint64_t)(a.lo + ((int64_t)tile * kTileP + lane)), t, x, y, tab);
      if constexpr (CALLS) lane = lane_now();
      const int64_t j = (int64_t)tile * kTileP + lane;
      double* const ak = acc + (k - 1 - k0) * E;
      const bool first = lane == 0;
      if constexpr (PASS == 0) {
        {
          const double s = wave_sum(wt);
          if (first) ak[0] += s;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const double s = wave_sum(wt * (wt == 0.0 ? 0.0 : x[i]));
          if (first) ak[1 + i] += s;
        }
        for (int r = 0; r < dy; ++r) {
          const double s = wave_sum(wt * (wt == 0.0 ? 0.0 : y[r * kTileP]));
          if (first) ak[1 + D + r] += s;
        }
        if (a.sx && j < n) {  // (both or neither: one buffer on the host's side)
          double* const xk = a.sx + ((int64_t)(k - 1) * D) * n + j;
#pragma unroll
          for (int i = 0; i < D; ++i) xk[(int64_t)i * n] = x[i];
          double* const yk = a.sy + ((int64_t)(k - 1) * dy) * n + j;
          for (int r = 0; r < dy; ++r) yk[(int64_t)r * n] = y[r * kTileP];
        }
      } else {
        const double* const m = a.res + (int64_t)(k - 1) * R + 1;  // mean x [D], mean y [dy]
        double dx[D], wd[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          dx[i] = wt == 0.0 ? 0.0 : x[i] - m[i];
          wd[i] = wt * dx[i];
        }
        if constexpr (CALLS) {  // rolled
          int e = 0;
#pragma unroll 1
          for (int i = 0; i < D; ++i) {
#pragma unroll 1
            for (int l = i; l <= D; ++l, ++e) {
              const double s = wave_sum(l < D ? wd[i] * dx[l] : wd[i]);
              if (first) ak[e] += s;
            }
          }
        } else {
          int e = 0;  // (a constant at every use once the loops are unrolled)
#pragma unroll
          for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int l = i; l <= D; ++l, ++e) {
              const double s = wave_sum(l < D ? wd[i] * dx[l] : wd[i]);
              if (first) ak[e] += s;
            }
          }
        }
        double* const ay = ak + est_entries(D);
        int e = 0;
        for (int r = 0; r < dy; ++r) {
          const double wr = wt * (wt == 0.0 ? 0.0 : y[r * kTileP] - m[D + r]);
          for (int l = r; l <= dy; ++l, ++e) {
            const double s = wave_sum(l < dy ? wr * (wt == 0.0 ? 0.0 : y[l * kTileP] - m[D + l]) : wr);
            if (first) ay[e] += s;
          }
        }
      }
    }
  }, nw);

  // the block's partials: the waves' accumulators added in wave order
  lds_barrier();
  const int tid = CALLS ? ws * 64 + lane_now() : (int)threadIdx.x;
  for (int i = tid; i < (k1 - k0) * E; i += nw * 64) {
    double s = acc_all[i];
    for (int w = 1; w < nw; ++w) s += acc_all[w * hc * E + i];
    a.e.part[((int64_t)k0 * E + i) * gridDim.x + blockIdx.x] = s;
  }
}

// A block per horizon: fold the nb partial rows in block order (k_est_fold's
// style) and divide.  pass 0: W and the means of x and y; pass 1: the two
// covariances, cov = C / W - (delta / W)(delta / W)^T, mirrored to full matrices.
// W is stored as NaN where k_est_ess would report one: weights that are not
// uniform (no resample pending) under a maximum that is not finite.
static __global__ __launch_bounds__(1024) void k_fc_fold(const double* part, int nb, int D, int dy, int pass,
                                                         const double* stats, const DevScalars* dev, int live,
                                                         double* res) {
  __shared__ double sums[est_entries(16) + est_entries(kMaxObs)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int E = fc_sums(D, dy, pass);
  const double* pk = part + (int64_t)blockIdx.x * E * nb;
  double* rk = res + (int64_t)blockIdx.x * fc_result_doubles(D, dy);
  for (int e = w; e < E; e += 16) {
    double s = 0.0;
    for (int b = lane; b < nb; b += 64) s += pk[(int64_t)e * nb + b];
    s = wave_sum(s);
    if (lane == 0) sums[e] = s;
  }
  __syncthreads();
  if (!pass) {
    const double W = sums[0];
    if (threadIdx.x == 0) {
      const double M = stats[0];
      const bool ok = (live && (dev->pending | dev->fire)) || (M > -INFINITY && M < INFINITY);
      rk[0] = ok ? W : NAN;
    }
    for (int i = threadIdx.x; i < D + dy; i += 1024) rk[1 + i] = sums[1 + i] / W;
    return;
  }
  const double W = rk[0];
  for (int q = threadIdx.x; q < D * D + dy * dy; q += 1024) {
    const bool isx = q < D * D;
    const int m = isx ? D : dy, i = isx ? q : q - D * D;
    const double* sm = isx ? sums : sums + est_entries(D);
    const int r = i / m, c = i % m, k = r < c ? r : c, l = r < c ? c : r;
    const double dk = sm[est_entry(k, m, m)] / W, dl = sm[est_entry(l, m, m)] / W;
    rk[1 + D + dy + q] = sm[est_entry(k, l, m)] / W - dk * dl;
  }
}

}  // namespace gh

// X is `extern template` (declaration) or `template` (definition), as in gh_inst.h
#define GH_FC_KERNELS(X, M, P)                                              \
  X __global__ void gh::k_forecast<M, 0>(const double*, P, gh::FcArgs);     \
  X __global__ void gh::k_forecast<M, 1>(const double*, P, gh::FcArgs);
