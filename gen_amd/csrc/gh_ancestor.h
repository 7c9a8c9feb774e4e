// gh_ancestor.h — ancestor sampling in conditional SMC (gh_pf_opts.ancestor_sampling;
// particle Gibbs with ancestor sampling, PGAS: Lindsten, Jordan & Schön, JMLR
// 2014).  At a conditional step t >= 2 whose resample fired, the distinguished
// particle's parent is drawn among all n particles of step t - 1 with
// probability proportional to
//
//   exp(b_i),  b_i = lw_{t-1}[i] + logpdf(ref_t | x_{t-1}^i)    one fp64 add
//
// lw_{t-1} the filter's log-weights as step t - 1 left them (a pending resample
// does not rewrite them: only the step kernels store logw), ref_t the state the
// caller pins at step t and the score the model's own (Model::score, called as
// k_bs_weights calls it): the bits of gh_pf_backward_weights(pf, t - 1, ref_t).
// The selection is gh_pf_smooth's integer rule (gh_smooth.h) under the uniform
// of stream STREAM_ANCESTOR, counter (0, 0, t); the pick replaces the 0 that
// gh_pf_maybe_resample wrote to the step's ancestor array.
//
// One trajectory through k_bs_max / k_bs_fold / k_bs_sum / k_bs_pick reads
// every row of step t - 1 twice; here a row is read once:
//
//   k_as_score  a lane loads its row and weight, computes b, stores it to the
//               filter's n-double scratch (allocated by gh_pf_init_conditional
//               with the option); the block maximum to pmax[block]
//   k_as_sum    every block folds the maxima (the same bits in each: an fp64
//               maximum does not depend on its order), then its 256-particle
//               chunks of b give q and bsum[chunk]; block 0 keeps B and flags a
//               maximum that is not finite
//   k_as_pick   one block: the crossing chunk (bs_cross), its 256 q from the
//               stored b again, the pick inside it, one int32
//
// Where the device flags say that no resample fired the parent is not a random
// variable (particle 0 continues itself): every kernel returns before it loads
// a row.  Plain launches in stream order before the step kernel; no atomics, no
// grid barrier; the index that comes from device memory is clamped.
#pragma once
#include "gh_smooth.h"

namespace gh {

constexpr int kAsSumBlocks = 512;  // k_as_sum's grid at most: each block folds all of pmax (8 nblk bytes from L2)

__device__ __forceinline__ uint64_t as_uniform(uint64_t seed, uint32_t t) {
  const u32x4 w = rng_block(seed, 0, t, STREAM_ANCESTOR, 0);
  return u53_bits(w.x, w.y);
}

// BsArgs as these kernels read it: x, lw the rows and weights of step t - 1 (a.t
// = t - 1), xt = ref_t [D], bw = b [n], pmax / bsum [nblk], B [1], io = the
// ancestor array of step t, err = the filter's device error
template <class Model>
__global__ __launch_bounds__(kBlock) void k_as_score(const double* __restrict__ prm, typename Model::Params p0,
                                                     StepObs o, BsArgs a) {
  if (!sm_uniform(a)) return;  // (no resample fired)
  constexpr int D = Model::kD;
  constexpr bool CALLS = makes_calls<Model>::value;
  const typename Model::Params p = p0.rebase(prm);
  __shared__ double red[kBlock / 64];
  const int tid = threadIdx.x;
  const int ws = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t j = (int64_t)blockIdx.x * kBlock + tid;
  double x[D], xn[D], lw, lat, ob;
  bs_load<D>(a, j, x, &lw);
#pragma unroll
  for (int k = 0; k < D; ++k) xn[k] = a.xt[k];
  Model::score(p, o, a.t + 1, x, xn, &lat, &ob);
  const double b = lw + lat;
  const int lane = CALLS ? lane_now() : (tid & 63);
  const int64_t js = CALLS ? (int64_t)blockIdx.x * kBlock + ws * 64 + lane : j;
  const bool in = js < a.n;
  if (in) a.bw[js] = b;
  const double v = wave_max(bs_for_max(b, in));
  if (lane == 0) red[ws] = v;
  __syncthreads();
  if (ws == 0 && lane == 0) a.pmax[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

static __global__ __launch_bounds__(kBlock) void k_as_sum(BsArgs a) {
  if (!sm_uniform(a)) return;
  __shared__ double smd[kBlock / 64];
  __shared__ uint64_t sm[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, ws = tid >> 6;
  double v = -INFINITY;
  for (int i = tid; i < a.nblk; i += kBlock) v = fmax(v, a.pmax[i]);
  v = wave_max(v);
  if (lane == 0) smd[ws] = v;
  __syncthreads();
  const double B = fmax(fmax(smd[0], smd[1]), fmax(smd[2], smd[3]));
  if (blockIdx.x == 0 && tid == 0) {
    a.B[0] = B;
    if (!(B > -INFINITY && B < INFINITY) && !*a.err) *a.err = kErrAncestor;  // (an earlier error stays)
  }
  for (int c = blockIdx.x; c < a.nblk; c += gridDim.x) {
    const int64_t j = (int64_t)c * kBlock + tid;
    const bool in = j < a.n;
    const uint64_t s = wave_sum_u64(bs_q(in ? a.bw[j] : -INFINITY, B, a.qscale, in));
    __syncthreads();  // (the readers of the chunk before)
    if (lane == 0) sm[ws] = s;
    __syncthreads();
    if (tid == 0) a.bsum[c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  }
}

static __global__ __launch_bounds__(kBlock) void k_as_pick(BsArgs a) {
  if (!sm_uniform(a)) return;
  __shared__ uint64_t sm[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, ws = tid >> 6;
  uint64_t target, before;
  int blk;
  bs_cross(a.bsum, a.nblk, as_uniform(a.seed, a.t + 1), sm, tid, lane, ws, &target, &blk, &before);
  if (blk >= a.nblk) {  // (no chunk crosses: S = 0 under a maximum that is not finite)
    blk = a.nblk - 1;
    if (tid == 0 && !*a.err) *a.err = kErrAncestor;
  }
  const int64_t j = (int64_t)blk * kBlock + tid;
  const bool in = j < a.n;
  const int c = bs_pick_in_block(bs_q(in ? a.bw[j] : -INFINITY, a.B[0], a.qscale, in), before, target, sm, lane, ws);
  int64_t pick = (int64_t)blk * kBlock + c;
  pick = pick >= a.n ? a.n - 1 : pick;
  if (tid == 0) a.io[0] = (int32_t)pick;
}

}  // namespace gh

// X is `extern template` (declaration) or `template` (definition), as in gh_inst.h
#define GH_AS_KERNELS(X, M, P) X __global__ void gh::k_as_score<M>(const double*, P, gh::StepObs, gh::BsArgs);
