// gh_path.h — every step's summary in one backward walk of the genealogy
// (gh_pf_estimate_path, gh_pf_quantiles_path): what gh_pf_estimate and
// gh_pf_quantiles return for t = t0..t1, and per step how much of the
// genealogy still stands behind it.
//
// gh_pf_estimate(pf, t) walks every current particle from step T back to t
// inside each of its passes: over a path that is n T (T - 1) / 2 hops per
// pass.  Here the walk is kept between the steps as a cursor, cur[i] = a_t(i),
// the index among step t's particles of the ancestor of current particle i:
//
//   k_path_cursor  the first launch composes the pending resample's ancestors
//                  (or the identity) with the hops from T down to t1; every
//                  later one takes cur one step boundary further down, a hop
//                  through that step's ancestor array if a resample preceded
//                  it (res_before, read here as est_tiles reads it).  Every
//                  ancestor array is read once per call.  With m given it
//                  then adds the particle's integer weight q_i (gh_quantiles.h)
//                  to m[cur[i]]: u64 atomic adds, exact in any order.
//   k_path_diag    m_t(j) = sum of the q_i with a_t(i) = j, reduced per block
//                  to (# m > 0, sum m, sum m^2) and cleared for the next step
//   k_path_diag_fold  the blocks' partials in block order: distinct, and
//                  ess = S^2 / sum m^2 with S = sum m
//
// and the moment and quantile kernels run in est_tiles' index-array mode
// (k_est_mean<D, true>, k_est_cov<D, true>, k_qt_hist<D, true>): the lane of
// current particle i reads row cur[i] of the step's states.  Weights, grids
// and the order of every sum are those of the per-step calls, so the mean,
// the covariance and the quantiles carry the same bits.  No floating-point
// atomics: two calls return the same bits.
#pragma once
#include "gh_quantiles.h"

namespace gh {

constexpr int kPathCursorBlocks = 4096;  // blocks of k_path_cursor at most (a grid-stride loop)
constexpr int kPathDiagBlocks = 256;     // blocks of k_path_diag at most: its partials, [3][blocks] words

struct PathArgs {
  int32_t* cur;                // [n] the cursor
  const int32_t* const* ancs;  // device array of per-step ancestor arrays (index t-1)
  const int32_t* res_before;   // res_before[t]: a resample preceded step t
  const int32_t* anc_pending;  // ancestors of a resample pending after the last step
  const double* logw;
  const double* stats;         // the rank's (M, S, S2)
  const DevScalars* dev;
  unsigned long long* m;       // [n] zero on entry; null: no weights are scattered
  int64_t n;
  int s_hi, s_lo;              // the boundaries crossed: steps s_hi, s_hi - 1, .., s_lo + 1
  int init;                    // cur is formed here (else read)
  int live;                    // the device resample flags are current
  double qscale;               // 2^shift
};

static __global__ __launch_bounds__(kBlock) void k_path_cursor(PathArgs a) {
  const bool uniform = a.live && (a.dev->pending | a.dev->fire);
  const double M = a.stats[0];
  // (clamped at every hop: a broken record reads a wrong particle, never outside the arrays)
  const auto clamp = [&](int64_t i) { return i < 0 ? 0 : (i >= a.n ? a.n - 1 : i); };
  const int lane = threadIdx.x & 63;
  // (a wave's 64 particles per trip, the trip count uniform over the wave: lane 0 is always inside n)
  for (int64_t j0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63); j0 < a.n; j0 += (int64_t)gridDim.x * kBlock) {
    const int64_t j = j0 + lane;
    const bool in = j < a.n;
    int64_t idx = 0;
    if (in) {
      if (a.init)
        idx = (uniform && a.anc_pending) ? clamp(a.anc_pending[j]) : j;
      else
        idx = clamp(a.cur[j]);
      for (int s = a.s_hi; s > a.s_lo; --s)
        if (a.res_before[s]) idx = clamp(a.ancs[s - 1][idx]);
      a.cur[j] = (int32_t)idx;
    }
    if (a.m) {
      // est_tiles' weight, k_qt_hist's integer
      double wt = 0.0;
      if (uniform) {
        wt = in ? 1.0 : 0.0;
      } else {
        const double lw = in ? a.logw[j] : -INFINITY;
        if (lw > -INFINITY) wt = gh_exp_nonpos(lw - M);
        if (lw != lw) wt = lw;
      }
      const uint64_t q = wt == wt ? f64_to_u52(wt * a.qscale) : 0;
      // Far enough back the genealogy has coalesced and whole waves stand on
      // one ancestor: their weights are summed in the wave and added once
      // (integer sums: the same m whichever way they are added).
      const int first = __builtin_amdgcn_readfirstlane((int)idx);
      if (__builtin_amdgcn_ballot_w64(in && (int)idx != first) == 0) {
        const uint64_t s = wave_sum_u64(q);
        if (lane == 0 && s) atomicAdd(a.m + first, (unsigned long long)s);
      } else if (q) {
        atomicAdd(a.m + idx, (unsigned long long)q);
      }
    }
  }
}

// part[0][b] = # slots of block b with m > 0, part[1][b] = their sum,
// part[2][b] = the bits of sum (double)m^2: a thread's slots at the grid's
// stride, DPP wave sums, the four waves in wave order
static __global__ __launch_bounds__(kBlock) void k_path_diag(unsigned long long* m, int64_t n, uint64_t* part) {
  __shared__ uint64_t rc[kBlock / 64], rs[kBlock / 64];
  __shared__ double r2[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t cnt = 0, sum = 0;
  double ss = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    const uint64_t v = m[j];
    if (v) {
      const double f = (double)v;
      cnt += 1;
      sum += v;
      ss += f * f;
      m[j] = 0;
    }
  }
  cnt = wave_sum_u64(cnt);
  sum = wave_sum_u64(sum);
  ss = wave_sum(ss);
  if (lane == 0) {
    rc[w] = cnt;
    rs[w] = sum;
    r2[w] = ss;
  }
  lds_barrier();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = (rc[0] + rc[1]) + (rc[2] + rc[3]);
    part[gridDim.x + blockIdx.x] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
    part[2 * gridDim.x + blockIdx.x] = as_u64((r2[0] + r2[1]) + (r2[2] + r2[3]));
  }
}

// one wave: its lanes stride the blocks, then the DPP sums.  res[0] = ess,
// res[slot_distinct] = the bits of the count.
static __global__ __launch_bounds__(64) void k_path_diag_fold(const uint64_t* part, int nb, double* res, int slot_distinct) {
  const int lane = threadIdx.x;
  uint64_t cnt = 0, sum = 0;
  double ss = 0.0;
  for (int b = lane; b < nb; b += 64) {
    cnt += part[b];
    sum += part[nb + b];
    ss += as_f64(part[2 * nb + b]);
  }
  cnt = wave_sum_u64(cnt);
  sum = wave_sum_u64(sum);
  ss = wave_sum(ss);
  if (lane == 0) {
    const double S = (double)sum;
    res[0] = (S * S) / ss;
    res[slot_distinct] = as_f64(cnt);
  }
}

}  // namespace gh

#define GH_PATH_KERNELS(X, D)                               \
  X __global__ void gh::k_est_mean<D, true>(gh::EstArgs);   \
  X __global__ void gh::k_est_cov<D, true>(gh::EstArgs);    \
  X __global__ void gh::k_qt_hist<D, true>(gh::QtArgs);
