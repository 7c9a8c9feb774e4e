// gh_smooth.h — backward simulation over a filter's history (gh_pf_smooth,
// gh_pf_backward_weights): draws from p(x_1:T | y_1:T) whose diversity does not
// collapse at early steps (FFBSi: Godsill, Doucet & West 2004).  The filter
// kept every step's states (record_history) and weights (record_weights); a
// trajectory starts from a draw of the current particles and goes back one
// step at a time, picking particle i of step t with probability proportional to
//
//   exp(b_i),  b_i = lw_t[i] + logpdf(x~ | x_t^i)     one fp64 add of the recorded
//                                                     weight and the latent score
//
// x~ the state already drawn for step t + 1 and the score the model's own
// (Model::score, called as k_scores calls it for step t + 1).  The selection
// is on integers (include/gen_hip.h states it): B = max b_i, q_i = floor(exp(b_i
// - B) 2^shift) (gh_pf_quantiles' weights and shift), S = sum q_i, target =
// floor(u S / 2^53) and the first i whose inclusive sum exceeds the target.
// Integer sums and the fp64 maximum do not depend on their order, so a pick is
// the same bits whatever the grid.
//
// A backward step of G trajectories over n particles, 256 particles per block:
//
//   k_bs_max    grid (blocks, chunks of kBsChunk trajectories): a lane loads its
//               particle's row and lw_t once, the chunk's x~ rows sit in LDS and
//               are read as broadcasts; per trajectory the wave maximum (DPP),
//               then the block's, one partial at pmax[m][block].  A NaN or +inf
//               among the b_i enters the maximum as +inf.
//   k_bs_fold   a block per trajectory: B_m, the error flag when it is not finite
//   k_bs_sum    the same tiling: b again, q, the wave's u64 sum, bsum[m][block]
//   k_bs_pick   a block per trajectory: S and the target from bsum[m][.], the
//               crossing block by a scan in block order, that block's 256 q's
//               again and their inclusive scan; the row of the pick goes to the
//               output, where the next backward step reads it as its x~.
//
// The start (step T) is the same selection over the current log-weights — every
// q_i = 2^shift and the row anc_pending[i] while a resample is pending — whose
// q's do not depend on the trajectory: k_sm_start_max / k_sm_start_sum run once
// per call, k_sm_start_pick per trajectory.
//
// Plain launches in stream order; no atomics; every index that comes from
// device memory is clamped into its array.  A model whose score makes
// out-of-line calls (makes_calls) gets its lane counted again after them.
#pragma once
#include "gh_kernels.h"
#include "gh_slots.h"
#include "gh_shapes.h"

namespace gh {

constexpr int kBsChunk = 64;      // trajectories of one block: their x~ rows in LDS (8 KiB at d = 16)
constexpr int kBsMaxTraj = 65536; // the interface's limit (gh_pf_smooth)
constexpr int kBsMaxGroup = 1024; // trajectories of one launch at most (a multiple of kBsChunk)
// pmax + bsum of one group stay within this while a group of kBsChunk fits it
// (n <= 2^24); above that the group is one chunk and the scratch is (kBsChunk
// + 1) x n / 256 x 16 bytes = 4.1 n bytes, half of one step's weight slot
constexpr size_t kBsScratchBytes = (size_t)64 << 20;

// trajectories of one launch: a multiple of kBsChunk, at least one chunk, whose
// partials fit kBsScratchBytes when one chunk's do
inline int bs_group(int64_t nblk) {
  int64_t g = (int64_t)(kBsScratchBytes / 16) / (nblk > 0 ? nblk : 1);
  g = g / kBsChunk * kBsChunk;
  if (g > kBsMaxGroup) g = kBsMaxGroup;
  if (g < kBsChunk) g = kBsChunk;
  return (int)g;
}

struct BsArgs {
  const double* x;         // the states of step t (tiled)
  const double* lw;        // the recorded log-weights of step t (the start: the current ones)
  const double* xt;        // [G][D] the trajectories' rows at step t + 1
  double* pmax;            // [G][nblk] block maxima
  double* B;               // [G]
  uint64_t* bsum;          // [G][nblk] block sums of q
  double* xo;              // [G][D] out: the picked rows of step t
  int32_t* io;             // [G] out: the picks (nullable)
  double* bw;              // k_bs_weights: [n] out
  int* err;                // set when a maximum is not finite (or no sum crosses its target)
  const int32_t* anc;      // the start: ancestors of a pending resample
  const DevScalars* dev;
  int live;                //   the device resample flags are current
  int64_t n;
  int nblk, G, D;
  uint64_t seed;
  int64_t m0;              // the first trajectory's index (the uniform's counter)
  uint32_t t;              // the step picked at (the uniform's counter); the score is step t + 1's
  double qscale;           // 2^shift
};

// (b as the maximum sees it: +inf marks a NaN or +inf; a tail lane adds nothing)
__device__ __forceinline__ double bs_for_max(double b, bool in) {
  return in ? ((b != b || b == INFINITY) ? INFINITY : b) : -INFINITY;
}
// q = floor(exp(b - B) 2^shift); 0 for b = -inf, a tail lane and whatever the flagged cases hold
__device__ __forceinline__ uint64_t bs_q(double b, double B, double qscale, bool in) {
  return in && b > -INFINITY && b <= B ? f64_to_u52(gh_exp_nonpos(b - B) * qscale) : 0ull;
}

// the block's inclusive scan of v in thread order and its total (sm: 4 words)
__device__ __forceinline__ uint64_t bs_block_incl(uint64_t v, uint64_t* sm, int lane, int ws, uint64_t* total) {
  v = wave_incl_sum_u64(v);
  __syncthreads();  // (the readers of the scan before)
  if (lane == 63) sm[ws] = v;
  __syncthreads();
  uint64_t off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) {
    const uint64_t s = sm[k];
    off += k < ws ? s : 0ull;
    tot += s;
  }
  *total = tot;
  return v + off;
}

// S, the target and the crossing block of one trajectory's block sums: the
// first block whose inclusive sum, in block order, exceeds the target, and the
// sum of the blocks before it.  The inclusive sums do not decrease, so the
// blocks at or below the target are exactly those before the crossing one:
// their count is its index, their sum its offset.
__device__ __forceinline__ void bs_cross(const uint64_t* bs, int nblk, uint64_t u, uint64_t* sm, int tid, int lane,
                                         int ws, uint64_t* target, int* block, uint64_t* before) {
  uint64_t s = 0, S;
  for (int i = tid; i < nblk; i += kBlock) s += bs[i];
  bs_block_incl(s, sm, lane, ws, &S);
  const uint64_t tg = scale_u53(u, S);
  uint64_t run = 0, cnt = 0, pre = 0;
  for (int base = 0; base < nblk; base += kBlock) {
    const bool have = base + tid < nblk;
    const uint64_t v = have ? bs[base + tid] : 0ull;
    uint64_t tot;
    const uint64_t incl = bs_block_incl(v, sm, lane, ws, &tot) + run;
    if (have && incl <= tg) {
      cnt += 1;
      pre += v;
    }
    run += tot;
  }
  uint64_t c, p;
  bs_block_incl(cnt, sm, lane, ws, &c);
  bs_block_incl(pre, sm, lane, ws, &p);
  *target = tg;
  *block = (int)c;
  *before = p;
}

// the pick inside the crossing block from its lanes' q (thread order = index
// order): the count of inclusive sums at or below the target
__device__ __forceinline__ int bs_pick_in_block(uint64_t q, uint64_t before, uint64_t target, uint64_t* sm, int lane,
                                                int ws) {
  uint64_t tot, c;
  const uint64_t incl = bs_block_incl(q, sm, lane, ws, &tot) + before;
  bs_block_incl(incl <= target ? 1ull : 0ull, sm, lane, ws, &c);
  return (int)c;
}

__device__ __forceinline__ uint64_t bs_uniform(uint64_t seed, int64_t m, uint32_t t) {
  const u32x4 w = rng_block(seed, (uint64_t)m, t, STREAM_SMOOTH, 0);
  return u53_bits(w.x, w.y);
}

// the block's maxima of `red` ([wave][kBsChunk]) to pmax[m][block]
__device__ __forceinline__ void bs_store_max(const double (*red)[kBsChunk], int nm, int c0, int tid, const BsArgs& a) {
  __syncthreads();
  for (int mm = tid; mm < nm; mm += kBlock)
    a.pmax[(int64_t)(c0 + mm) * a.nblk + blockIdx.x] = fmax(fmax(red[0][mm], red[1][mm]), fmax(red[2][mm], red[3][mm]));
}

// a lane's particle of step t: its row and its recorded weight (a tail lane: the last particle's row, -inf)
template <int D>
__device__ __forceinline__ void bs_load(const BsArgs& a, int64_t j, double* x, double* lw) {
  const bool in = j < a.n;
  const int64_t jj = in ? j : a.n - 1;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = a.x[xidx(jj, k, D)];
  *lw = in ? a.lw[jj] : -INFINITY;
}

template <class Model>
__global__ __launch_bounds__(kBlock) void k_bs_max(const double* __restrict__ prm, typename Model::Params p0, StepObs o,
                                                   BsArgs a) {
  constexpr int D = Model::kD;
  constexpr bool CALLS = makes_calls<Model>::value;
  const typename Model::Params p = p0.rebase(prm);
  __shared__ double xt[kBsChunk * D];
  __shared__ double red[kBlock / 64][kBsChunk];
  const int tid = threadIdx.x;
  const int ws = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = (int)blockIdx.y * kBsChunk;
  const int nm = a.G - c0 < kBsChunk ? a.G - c0 : kBsChunk;
  for (int i = tid; i < nm * D; i += kBlock) xt[i] = a.xt[(int64_t)c0 * D + i];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * kBlock + tid;
  const bool in = j < a.n;
  double x[D], lw;
  bs_load<D>(a, j, x, &lw);
#pragma unroll 1
  for (int mm = 0; mm < nm; ++mm) {
    double xn[D], lat, ob;
#pragma unroll
    for (int k = 0; k < D; ++k) xn[k] = xt[mm * D + k];
    Model::score(p, o, a.t + 1, x, xn, &lat, &ob);
    const double v = wave_max(bs_for_max(lw + lat, in));
    const int lane = CALLS ? lane_now() : (tid & 63);
    if (lane == 0) red[ws][mm] = v;
  }
  bs_store_max(red, nm, c0, CALLS ? ws * 64 + lane_now() : tid, a);
}

static __global__ __launch_bounds__(kBlock) void k_bs_fold(const double* pmax, int nblk, double* B, int* err) {
  __shared__ double sm[kBlock / 64];
  const double* pm = pmax + (int64_t)blockIdx.x * nblk;
  double v = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += kBlock) v = fmax(v, pm[i]);
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
    B[blockIdx.x] = v;
    if (!(v > -INFINITY && v < INFINITY)) *err = 1;
  }
}

template <class Model>
__global__ __launch_bounds__(kBlock) void k_bs_sum(const double* __restrict__ prm, typename Model::Params p0, StepObs o,
                                                   BsArgs a) {
  constexpr int D = Model::kD;
  constexpr bool CALLS = makes_calls<Model>::value;
  const typename Model::Params p = p0.rebase(prm);
  __shared__ double xt[kBsChunk * D];
  __shared__ double Bs[kBsChunk];
  __shared__ uint64_t red[kBlock / 64][kBsChunk];
  const int tid = threadIdx.x;
  const int ws = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = (int)blockIdx.y * kBsChunk;
  const int nm = a.G - c0 < kBsChunk ? a.G - c0 : kBsChunk;
  for (int i = tid; i < nm * D; i += kBlock) xt[i] = a.xt[(int64_t)c0 * D + i];
  for (int i = tid; i < nm; i += kBlock) Bs[i] = a.B[c0 + i];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * kBlock + tid;
  const bool in = j < a.n;
  double x[D], lw;
  bs_load<D>(a, j, x, &lw);
#pragma unroll 1
  for (int mm = 0; mm < nm; ++mm) {
    double xn[D], lat, ob;
#pragma unroll
    for (int k = 0; k < D; ++k) xn[k] = xt[mm * D + k];
    Model::score(p, o, a.t + 1, x, xn, &lat, &ob);
    const uint64_t s = wave_sum_u64(bs_q(lw + lat, Bs[mm], a.qscale, in));
    const int lane = CALLS ? lane_now() : (tid & 63);
    if (lane == 0) red[ws][mm] = s;
  }
  __syncthreads();
  const int t2 = CALLS ? ws * 64 + lane_now() : tid;
  for (int mm = t2; mm < nm; mm += kBlock)
    a.bsum[(int64_t)(c0 + mm) * a.nblk + blockIdx.x] = (red[0][mm] + red[1][mm]) + (red[2][mm] + red[3][mm]);
}

template <class Model>
__global__ __launch_bounds__(kBlock) void k_bs_pick(const double* __restrict__ prm, typename Model::Params p0, StepObs o,
                                                    BsArgs a) {
  constexpr int D = Model::kD;
  constexpr bool CALLS = makes_calls<Model>::value;
  const typename Model::Params p = p0.rebase(prm);
  __shared__ uint64_t sm[kBlock / 64];
  const int m = blockIdx.x;
  int tid = threadIdx.x, lane = tid & 63;
  const int ws = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint64_t target, before;
  int blk;
  bs_cross(a.bsum + (int64_t)m * a.nblk, a.nblk, bs_uniform(a.seed, a.m0 + m, a.t), sm, tid, lane, ws, &target, &blk,
           &before);
  if (blk >= a.nblk) {  // (no block crosses: S = 0 under a maximum that is not finite; the flag is set)
    blk = a.nblk - 1;
    if (tid == 0) *a.err = 1;
  }
  const int64_t j = (int64_t)blk * kBlock + tid;
  const bool in = j < a.n;
  double x[D], xn[D], lw, lat, ob;
  bs_load<D>(a, j, x, &lw);
#pragma unroll
  for (int k = 0; k < D; ++k) xn[k] = a.xt[(int64_t)m * D + k];
  const double B = a.B[m];
  Model::score(p, o, a.t + 1, x, xn, &lat, &ob);
  if constexpr (CALLS) {
    lane = lane_now();
    tid = ws * 64 + lane;
  }
  const int c = bs_pick_in_block(bs_q(lw + lat, B, a.qscale, in), before, target, sm, lane, ws);
  int64_t pick = (int64_t)blk * kBlock + c;
  pick = pick >= a.n ? a.n - 1 : pick;
  if (tid < D) a.xo[(int64_t)m * D + tid] = a.x[xidx(pick, tid, D)];
  if (tid == 0 && a.io) a.io[m] = (int32_t)pick;
}

// gh_pf_backward_weights: b_i of every particle of step t for one x~ (a.xt: [D])
template <class Model>
__global__ __launch_bounds__(kBlock) void k_bs_weights(const double* __restrict__ prm, typename Model::Params p0,
                                                       StepObs o, BsArgs a) {
  constexpr int D = Model::kD;
  const typename Model::Params p = p0.rebase(prm);
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double x[D], xn[D], lw, lat, ob;
  bs_load<D>(a, j, x, &lw);
#pragma unroll
  for (int k = 0; k < D; ++k) xn[k] = a.xt[k];
  Model::score(p, o, a.t + 1, x, xn, &lat, &ob);
  if (j < a.n) a.bw[j] = lw + lat;
}

// ---- the start: the current particles under the current weights
__device__ __forceinline__ bool sm_uniform(const BsArgs& a) { return a.live && (a.dev->pending | a.dev->fire); }
__device__ __forceinline__ double sm_start_b(const BsArgs& a, int64_t j, bool uniform) {
  return j < a.n ? (uniform ? 0.0 : a.lw[j]) : -INFINITY;
}

static __global__ __launch_bounds__(kBlock) void k_sm_start_max(BsArgs a) {
  __shared__ double sm[kBlock / 64];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double v = wave_max(bs_for_max(sm_start_b(a, j, sm_uniform(a)), j < a.n));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) a.pmax[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

__device__ __forceinline__ uint64_t sm_start_q(const BsArgs& a, int64_t j, bool uniform, double B) {
  if (uniform) return j < a.n ? (uint64_t)a.qscale : 0ull;
  return bs_q(sm_start_b(a, j, false), B, a.qscale, j < a.n);
}

static __global__ __launch_bounds__(kBlock) void k_sm_start_sum(BsArgs a) {
  __shared__ uint64_t sm[kBlock / 64];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t s = wave_sum_u64(sm_start_q(a, j, sm_uniform(a), a.B[0]));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

static __global__ __launch_bounds__(kBlock) void k_sm_start_pick(BsArgs a) {
  __shared__ uint64_t sm[kBlock / 64];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, ws = tid >> 6;
  const bool uniform = sm_uniform(a);
  uint64_t target, before;
  int blk;
  bs_cross(a.bsum, a.nblk, bs_uniform(a.seed, a.m0 + m, a.t), sm, tid, lane, ws, &target, &blk, &before);
  if (blk >= a.nblk) {
    blk = a.nblk - 1;
    if (tid == 0) *a.err = 1;
  }
  const int64_t j = (int64_t)blk * kBlock + tid;
  const int c = bs_pick_in_block(sm_start_q(a, j, uniform, a.B[0]), before, target, sm, lane, ws);
  int64_t pick = (int64_t)blk * kBlock + c;
  pick = pick >= a.n ? a.n - 1 : pick;
  if (uniform && a.anc) {  // the resampled particle stands on its ancestor's row (clamped: never outside the slot)
    const int64_t r = a.anc[pick];
    pick = r < 0 ? 0 : (r >= a.n ? a.n - 1 : r);
  }
  if (tid < a.D) a.xo[(int64_t)m * a.D + tid] = a.x[xidx(pick, tid, a.D)];
  if (tid == 0 && a.io) a.io[m] = (int32_t)pick;
}

}  // namespace gh

// X is `extern template` (declaration) or `template` (definition), as in gh_inst.h
#define GH_BS_KERNELS(X, M, P)                                                       \
  X __global__ void gh::k_bs_max<M>(const double*, P, gh::StepObs, gh::BsArgs);      \
  X __global__ void gh::k_bs_sum<M>(const double*, P, gh::StepObs, gh::BsArgs);      \
  X __global__ void gh::k_bs_pick<M>(const double*, P, gh::StepObs, gh::BsArgs);     \
  X __global__ void gh::k_bs_weights<M>(const double*, P, gh::StepObs, gh::BsArgs);
