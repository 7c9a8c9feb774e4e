// gh_move_parts.h — the parts every per-particle move is assembled from
// (gh_rejuv.h, gh_grad.h, gh_slice.h), one definition each, as
// gh_resample_parts.h has for the resample kernels.  The accept/reject kernels
// keep their own loop over the moves, all of one shape: dr = rejuv_draw(w);
// candidate y and alpha; if move_accept: take y, count.  (Why no shared loop
// and no function for the write-back or the copy: DESIGN.md §7n.)
//
// One particle per lane; the current state and its parent's state live in
// registers for all moves of one launch.  Move w (counted from the step) draws
// its proposal from draw window (w mod 4096) * kRejuvDraws of stream
// STREAM_MH + 16 (w / 4096) and its acceptance uniform from the last draw of
// that window; the first 4096 moves use the MH stream itself.
#pragma once
#include <type_traits>

#include "gh_kernels.h"

namespace gh {

constexpr uint32_t kRejuvDraws = 16;           // draw window per move (LG d <= 16 uses 8)
constexpr uint32_t kRejuvMaxMoves = 1u << 24;  // 4096 windows x 4096 stream blocks

__device__ __host__ __forceinline__ Draw rejuv_draw(uint32_t w) {
  return Draw{(uint32_t)STREAM_MH + ((w >> 12) << 4), (w & 4095u) * kRejuvDraws};
}

struct RejuvArgs {
  const double* xprev;    // wave-tiled states of step t-1 (t >= 2)
  const int32_t* anc;     // ancestors consumed by step t (valid when *res)
  const int32_t* res;     // res_hist + t: a resample preceded step t
  const double* remote;   // multi-rank rows received by the last exchange
  int64_t ld_remote;
  double* x;              // wave-tiled states of step t, rewritten in place
  int64_t n, lo;
  uint64_t seed;
  uint32_t t;
  uint32_t move0;         // moves already applied at this step
  uint32_t select;        // selected latent addresses of the step (the regression: bit 0 :slope, bit 1 :intercept)
  int n_moves;
  unsigned long long* accepted;  // accepted moves (summed over particles)
};

// The block's copy of the Box–Muller tables (LDS reads), loaded and fenced.
// Every thread of the block calls it, before any bounds test.
__device__ __forceinline__ const double* move_tab() {
  __shared__ double tab[kMathTabDoubles];
  load_math_tab(tab);
  lds_barrier();
  return tab;
}

// The parent's state xp of particle j (0 at t = 1, where nothing reads it):
// the previous slot through the step's ancestors, or a row received from
// another rank.
template <int D, bool INIT>
__device__ __forceinline__ void move_parent(const RejuvArgs& a, int64_t j, double* xp) {
#pragma unroll
  for (int k = 0; k < D; ++k) xp[k] = 0.0;
  if (!INIT) {
    const int64_t src = *a.res ? (int64_t)a.anc[j] : j;
    if (src >= 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) xp[k] = a.xprev[xidx(src, k, D)];
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) xp[k] = ld_sys(&a.remote[(-1 - src) * a.ld_remote + k]);
    }
  }
}

// particle j's state x and its parent's
template <int D, bool INIT>
__device__ __forceinline__ void move_load(const RejuvArgs& a, int64_t j, double* x, double* xp) {
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = a.x[xidx(j, k, D)];
  move_parent<D, INIT>(a, j, xp);
}

// bit k of the selection for the regression's two addresses; an Unfold latent
// moves as a whole (gh_pf_mh_drift's rule)
template <class Model>
__device__ __forceinline__ bool move_selected(uint32_t select, int k) {
  if constexpr (std::is_same<Model, RegModel>::value) return ((select >> k) & 1u) != 0;
  return true;
}

// the last Philox block of the move's window; its words x, y make the accept
// uniform (z, w: the slice's first angle)
__device__ __forceinline__ u32x4 move_uniform_block(const RejuvArgs& a, uint64_t pid, const Draw& dr) {
  return rng_block(a.seed, pid, a.t, dr.stream, dr.base + kRejuvDraws - 1);
}
__device__ __forceinline__ double move_logu(const u32x4& b) { return gh_log(u53(b.x, b.y)); }

// counter += the wave's sum of n, one atomic per wave.  Every lane of every
// wave calls it (idle lanes with n = 0): it stays outside the bounds test.
__device__ __forceinline__ void move_count(unsigned long long* counter, unsigned n) {
  const uint64_t tot = wave_sum_u64((uint64_t)n);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(counter, (unsigned long long)tot);
}

// The accept test of a Metropolis move with log acceptance ratio alpha: log u <
// alpha, u from the last block of the move's window (a NaN alpha rejects).
__device__ __forceinline__ bool move_accept(const RejuvArgs& a, uint64_t pid, const Draw& dr, double alpha) {
  return move_logu(move_uniform_block(a, pid, dr)) < alpha;
}

}  // namespace gh
