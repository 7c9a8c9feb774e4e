// gh_moments.h — weighted moments of a filter's particles, reduced on the
// device (gh_pf_estimate): the effective sample size, the weighted mean and
// the weighted population covariance of the latent of one step along the
// current particles' genealogy.  effective_sample_size / normalize_weights
// (particle_filter.jl:3-14) and the expectation callers take over get_traces
// with get_log_weights.
//
//   k_est_ess    ESS from the rank's (max, sum e, sum e^2) — no particle pass
//   k_est_mean   pass 1: per block, sum w and sum w x_k           (D + 1 sums)
//   k_est_cov    pass 2: per block, the upper triangle of
//                sum w (x - m)(x - m)^T and delta = sum w (x - m), m the
//                pass-1 mean read from device memory             (est_entries(D) sums)
//   k_est_fold   the blocks' partial rows summed in block order, then the
//                division: mean = sum w x / W, cov = C / W - (delta / W)(delta / W)^T
//
// The corrected two-pass algorithm: raw second moments in one pass lose
// |mean|^2 / var digits to cancellation; centred on the pass-1 mean the
// correction term is of the order of that mean's rounding error.  No atomics,
// a grid that depends on n only and a fixed order of every sum: two calls
// return the same bits.
//
// w_i = exp(lw_i - M), M the rank's maximum (stats_all[0], ensure_stats), or 1
// for every particle while a resample is pending (the particles are then the
// resampled ones, anc_pending).  A particle of weight exactly 0 adds nothing,
// whatever its state holds.  A tile's lanes past n have weight 0.
#pragma once
#include "gh_kernels.h"
#include "gh_shapes.h"

namespace gh {

typedef double est_d2 __attribute__((ext_vector_type(2)));  // a 16-byte word: a component pair

// blocks of a pass at most; a wave walks its tiles at the grid's stride.  Pass 1:
// 4 blocks of 4 waves per CU.  Pass 2 holds up to kEstPanelMax sums per lane
// (2-3 waves per SIMD) and ends in as many wave reductions: 2 blocks per CU,
// all resident at once, each wave with twice the tiles before that epilogue.
constexpr int kEstMaxBlocks = 1024;
constexpr int kEstCovBlocks = 512;
constexpr int kEstPanelMax = 68;     // fp64 accumulators of one k_est_cov panel (136 VGPRs)

// sums of pass 2: rows k = 0..D-1 of the upper triangle, each followed by its
// delta_k (column D stands for the constant 1)
__host__ __device__ constexpr int est_entries(int D) { return D * (D + 1) / 2 + D; }
__host__ __device__ constexpr int est_entry(int k, int l, int D) { return k * (D + 1) - k * (k - 1) / 2 + (l - k); }
__host__ __device__ constexpr int est_panels(int D) { return (est_entries(D) + kEstPanelMax - 1) / kEstPanelMax; }
// doubles of the result block: ess, mean[D], cov[D][D], then W (stays on the device)
__host__ __device__ constexpr int est_result_doubles(int D) { return 1 + D + D * D; }

struct EstArgs {
  const double* x;             // wave-tiled states of the target step (xidx)
  const int32_t* const* ancs;  // device array of per-step ancestor arrays (index t-1); read when t_target < t_cur
  const int32_t* res_before;   // res_before[t]: a resample preceded step t
  const int32_t* anc_pending;  // ancestors of a resample pending after the last step; index-array mode
                               // (est_tiles<D, true>): the cursor, a_t(i) of every current particle i
  const double* logw;
  const double* stats;         // the rank's (M, S, S2)
  const DevScalars* dev;
  int64_t n;
  int t_target, t_cur;
  int live;                    // the device resample flags are current
  double* part;                // [sums][gridDim.x] block partials
  double* res;                 // the result block (est_result_doubles)
};

static __global__ void k_est_ess(const double* stats, const DevScalars* dev, int live, int64_t n, double* res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ess;
  if (live && (dev->pending | dev->fire)) {
    ess = (double)n;  // every weight is 1
  } else {
    const double M = stats[0];
    ess = (M > -INFINITY && M < INFINITY) ? (stats[1] * stats[1]) / stats[2] : NAN;
  }
  res[0] = ess;
}

// Between a wave's LDS accesses that hand data from lane to lane: the earlier
// ones have completed (lgkmcnt(0), as store_rows_staged waits), and the
// wavefront-scope fences keep the compiler from moving accesses across.
__device__ __forceinline__ void est_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Every tile of this wave, each lane with its particle's weight and D
// components: f(w, x).  Identity path (the target step is the current one and
// no resample is pending): a wave reads its tile as whole lines — a pair
// tile as 16-byte pair words per lane; a row tile's 640 contiguous doubles
// spread over the lanes and turned into one row per lane through `stage`
// (5 KiB of LDS private to the wave; lane l's row starts 20 banks after lane
// l-1's, so the 16-lane groups of a 16-byte read meet no conflict).  The
// gather paths index by xidx along the genealogy, as k_traj does.
// nw: the block's waves (k_forecast launches fewer than kBlock / 64 when its
// LDS asks for it); an f that takes a third argument gets the lane's particle
// index, which is past n in the last tile's tail (weight 0, state unspecified).
// IDX, the index-array mode (gh_path.h): the genealogy has been walked already
// and a.anc_pending holds its result, the lane's particle index among a.x's
// step for every current particle (a pending resample included: it is not
// applied again); ancs, res_before, t_target and t_cur are not read.
template <int D, bool IDX = false, class F>
__device__ __forceinline__ void est_tiles(const EstArgs& a, est_d2* stage, F&& f, const int nw = kBlock / 64) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool uniform = a.live && (a.dev->pending | a.dev->fire);
  const bool walk = !IDX && a.t_target != a.t_cur;
  const bool gather = IDX || walk || (uniform && a.anc_pending);
  const double M = a.stats[0];
  const int64_t tiles = (a.n + kTileP - 1) / kTileP;
  for (int64_t tile = (int64_t)blockIdx.x * nw + w; tile < tiles; tile += (int64_t)gridDim.x * nw) {
    const int64_t j = tile * kTileP + lane;
    const bool in = j < a.n;
    double wt = 0.0;
    if (uniform) {
      wt = in ? 1.0 : 0.0;
    } else {
      const double lw = in ? a.logw[j] : -INFINITY;
      if (lw > -INFINITY) wt = gh_exp_nonpos(lw - M);
      if (lw != lw) wt = lw;
    }
    double x[D];
    if (gather) {
      // (clamped at every hop: a broken record reads a wrong particle, never outside the arrays)
      const auto clamp = [&](int64_t i) { return i < 0 ? 0 : (i >= a.n ? a.n - 1 : i); };
      int64_t idx = in ? j : 0;
      if constexpr (IDX) {
        if (in) idx = clamp(a.anc_pending[idx]);
      } else {
        if (in && uniform && a.anc_pending) idx = clamp(a.anc_pending[idx]);
        if (in && walk)
          for (int s = a.t_cur; s > a.t_target; --s)
            if (a.res_before[s]) idx = clamp(a.ancs[s - 1][idx]);
      }
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = a.x[xidx(idx, k, D)];
    } else if constexpr (state_rows(D)) {
      const est_d2* tb = (const est_d2*)(a.x + tile * (kTileP * D));
      est_d2* st = stage + w * (kTileP * D / 2);
      est_d2 v[D / 2];
#pragma unroll
      for (int c = 0; c < D / 2; ++c) v[c] = tb[c * kTileP + lane];
      est_lds_order();  // after the previous tile's reads of the region
#pragma unroll
      for (int c = 0; c < D / 2; ++c) st[c * kTileP + lane] = v[c];
      est_lds_order();
#pragma unroll
      for (int c = 0; c < D / 2; ++c) {
        const est_d2 r = st[lane * (D / 2) + c];
        x[2 * c] = r.x;
        x[2 * c + 1] = r.y;
      }
    } else {
      const double* tb = a.x + tile * (kTileP * D);
#pragma unroll
      for (int c = 0; c < D / 2; ++c) {
        const est_d2 r = ((const est_d2*)tb)[c * kTileP + lane];
        x[2 * c] = r.x;
        x[2 * c + 1] = r.y;
      }
      if constexpr ((D & 1) != 0) x[D - 1] = tb[(D - 1) * kTileP + lane];
    }
    if constexpr (std::is_invocable_v<F&, double, const double*, int64_t>)
      f(wt, x, j);
    else
      f(wt, x);
  }
}

// The block's E sums from its lanes' accumulators: DPP wave sums, the four
// waves through LDS in wave order, one partial per sum at part[e][block].
template <int E>
__device__ __forceinline__ void est_block_partial(const double* acc, double (*red)[E], double* part, int e0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const double v = wave_sum(acc[e]);
    if (lane == 0) red[w][e] = v;
  }
  lds_barrier();
  for (int e = threadIdx.x; e < E; e += kBlock)
    part[(int64_t)(e0 + e) * gridDim.x + blockIdx.x] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// (IDX: est_tiles' index-array mode, instantiated by gh_inst_path.hip; it always gathers and stages nothing)
template <int D, bool IDX = false>
__global__ __launch_bounds__(kBlock) void k_est_mean(EstArgs a) {
  __shared__ est_d2 stage[state_rows(D) && !IDX ? (kBlock / 64) * kTileP * D / 2 : 1];
  __shared__ double red[kBlock / 64][D + 1];
  double acc[D + 1];
#pragma unroll
  for (int e = 0; e <= D; ++e) acc[e] = 0.0;
  est_tiles<D, IDX>(a, stage, [&](double w, const double* x) {
    acc[0] += w;
#pragma unroll
    for (int k = 0; k < D; ++k) acc[1 + k] = fma(w, w == 0.0 ? 0.0 : x[k], acc[1 + k]);
  });
  est_block_partial<D + 1>(acc, red, a.part, 0);
}

// One panel of pass 2: entries [PANEL * EP, (PANEL + 1) * EP) of the sums, so
// that the accumulators stay a register array (D = 16: 152 sums in 3 panels).
template <int D, int PANEL, bool IDX>
__device__ __forceinline__ void est_cov_panel(const EstArgs& a, est_d2* stage) {
  constexpr int E = est_entries(D), P = est_panels(D), EP = (E + P - 1) / P;
  constexpr int E0 = PANEL * EP, E1 = E0 + EP < E ? E0 + EP : E;
  __shared__ double red[kBlock / 64][EP];
  double m[D];
#pragma unroll
  for (int k = 0; k < D; ++k) m[k] = a.res[1 + k];
  double acc[EP];
#pragma unroll
  for (int e = 0; e < EP; ++e) acc[e] = 0.0;
  est_tiles<D, IDX>(a, stage, [&](double w, const double* x) {
    double dx[D], wd[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      dx[k] = w == 0.0 ? 0.0 : x[k] - m[k];
      wd[k] = w * dx[k];
    }
    int e = 0;  // (a constant at every use once the loops are unrolled)
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int l = k; l <= D; ++l, ++e)
        if (e >= E0 && e < E1) acc[e - E0] = l < D ? fma(wd[k], dx[l], acc[e - E0]) : acc[e - E0] + wd[k];
    }
  });
  est_block_partial<E1 - E0>(acc, (double(*)[E1 - E0]) red, a.part, E0);
}

template <int D, bool IDX = false>
__global__ __launch_bounds__(kBlock) void k_est_cov(EstArgs a) {
  __shared__ est_d2 stage[state_rows(D) && !IDX ? (kBlock / 64) * kTileP * D / 2 : 1];
  static_assert(est_panels(D) <= 3, "one case per panel");
  if (blockIdx.y == 0) est_cov_panel<D, 0, IDX>(a, stage);
  if constexpr (est_panels(D) > 1)
    if (blockIdx.y == 1) est_cov_panel<D, 1, IDX>(a, stage);
  if constexpr (est_panels(D) > 2)
    if (blockIdx.y == 2) est_cov_panel<D, 2, IDX>(a, stage);
}

// Fold the nb partial rows in block order (k_fold's style: one 1024-thread
// block; a wave per sum, its lanes striding the blocks, then the DPP sum) and
// divide.  cov = 0: the D + 1 sums of pass 1 -> W and the mean; cov = 1: the
// est_entries(D) sums of pass 2 -> the covariance, mirrored to the full matrix.
static __global__ __launch_bounds__(1024) void k_est_fold(const double* part, int nb, int D, int cov, double* res) {
  __shared__ double sums[est_entries(16)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int E = cov ? est_entries(D) : D + 1;
  for (int e = w; e < E; e += 16) {
    double s = 0.0;
    for (int b = lane; b < nb; b += 64) s += part[(int64_t)e * nb + b];
    s = wave_sum(s);
    if (lane == 0) sums[e] = s;
  }
  __syncthreads();
  double* rw = res + est_result_doubles(D);
  if (!cov) {
    const double W = sums[0];
    if (threadIdx.x == 0) *rw = W;
    if ((int)threadIdx.x < D) res[1 + threadIdx.x] = sums[1 + threadIdx.x] / W;
    return;
  }
  const double W = *rw;
  for (int i = threadIdx.x; i < D * D; i += 1024) {
    const int r = i / D, c = i % D, k = r < c ? r : c, l = r < c ? c : r;
    const double dk = sums[est_entry(k, D, D)] / W, dl = sums[est_entry(l, D, D)] / W;
    res[1 + D + i] = sums[est_entry(k, l, D)] / W - dk * dl;
  }
}

}  // namespace gh

// per dimension (GH_FOR_D of gh_shapes.h); X is `extern template` or `template`, as in gh_inst.h
#define GH_EST_KERNELS(X, D)                          \
  X __global__ void gh::k_est_mean<D>(gh::EstArgs);   \
  X __global__ void gh::k_est_cov<D>(gh::EstArgs);
