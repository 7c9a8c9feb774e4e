// gh_quantiles.h — weighted quantiles of a filter's particles, selected on the
// device (gh_pf_quantiles): for every component k of the latent of one step
// along the current particles' genealogy and every probability p_j, the
// inverse CDF (type 1) of the particles under the resampler's integer weights.
//
// Definition (include/gen_hip.h states it for callers): q_i = floor(exp(lw_i -
// M) 2^shift), M the maximum log-weight, shift = quant_shift(n) — tile_quantise's
// value; 2^shift for every particle while a resample is pending.  S = sum q_i,
// u = floor(p 2^53), r = max(1, ceil(u S / 2^53)).  Doubles ordered by the
// total-order key (qt_key).  Q_k(p) = the smallest x_ik with q_i > 0 whose
// cumulative weight sum_{x_lk <= x_ik} q_l reaches r.  Integer sums do not
// depend on their order, so the result is the same bits on every run, whatever
// the grid and the arrival order of the atomics.
//
// A most-significant-digit radix select over the 64-bit keys, kQtBits bits per
// pass, all d components and all probabilities (a "pair" = (j, k), index
// j d + k) at once:
//
//   k_qt_hist    per pass: every particle whose key k carries pair (j, k)'s
//                prefix so far adds its q to the pair's bin of the next digit.
//                Bins are u64 in LDS (ds_add_u64), the block's non-zero bins
//                go to the global histogram by u64 atomic adds.  blockIdx.y
//                takes qt_chunk_probs(D) probabilities: at most kQtChunkPairs
//                pairs = 32 KiB of bins per block.  In pass 0 no pair has a
//                prefix yet: one histogram per component serves every
//                probability, so only the first chunk's blocks run.
//                A pass that few particles can still match (k_qt_select's
//                verdict on the pass before) is a sparse one: no bins in
//                LDS, the blocks of the first chunk take every probability
//                and a matching lane adds to the global histogram itself.
//   k_qt_select  per pass, one block: per pair, the first bin whose running sum
//                reaches the pair's remaining rank; its digit joins the
//                prefix, the sum of the bins before it leaves the rank, the
//                bins are cleared for the next pass.  Pass 0's bins sum to S:
//                the ranks are formed there and S never leaves the device.
//                The sums are exact, so a crossing bin always exists.
//
// In the first passes many particles of a wave share the digit (sign and high
// exponent bits; class indices share all of them) and their lanes add to one
// LDS address.  A wave-aggregated path for that case (a ballot per shared
// digit, wave_sum_u64 of the lanes' q, one add) was built and measured: the
// same bits and 4-10 % slower on every model tried, class indices included,
// so every matching lane adds for itself (DESIGN.md §7q has the figures).
// Probabilities of one component whose prefixes still coincide share their
// match and ballot.  In the last passes nearly no lane matches: one ballot per
// distinct prefix and nothing else.
#pragma once
#include "gh_moments.h"

namespace gh {

constexpr int kQtBits = 8;                    // digit width: 8 passes of 256 bins
constexpr int kQtBins = 1 << kQtBits;
constexpr int kQtPasses = 64 / kQtBits;
constexpr int kQtMaxProbs = 16;               // interface limit (gh_pf_quantiles)
constexpr int kQtMaxPairs = 16 * kQtMaxProbs; // d <= 16
constexpr int kQtChunkPairs = 16;             // pairs of one block, 2 KiB of bins each
__host__ __device__ constexpr int qt_chunk_probs(int D) {  // probabilities of one block
  return kQtChunkPairs / D > kQtMaxProbs ? kQtMaxProbs : (kQtChunkPairs / D > 0 ? kQtChunkPairs / D : 1);
}

// after a pass whose chosen bins each hold at most S >> kQtSparseShift, few
// particles still match a prefix: the next pass is a sparse one
constexpr int kQtSparseShift = 6;

// scratch of one filter (u64 words): the histogram, then per pair the prefix
// and the remaining rank, the control words (per pass: the next pass is a
// dense one; then S), then the result block (marker, out[pairs]) as doubles
constexpr size_t kQtHistWords = (size_t)kQtMaxPairs * kQtBins;
constexpr int kQtCtlWords = kQtPasses + 1;
constexpr size_t kQtScratchWords = kQtHistWords + 2 * kQtMaxPairs + kQtCtlWords + 1 + kQtMaxPairs;

// the total-order key: all bits flipped for negatives, the sign bit otherwise
// (-nan < -inf < ... < -0.0 < +0.0 < ... < +inf < +nan, by the bits)
__host__ __device__ __forceinline__ uint64_t qt_key(uint64_t b) { return b ^ ((b >> 63) ? ~0ull : 1ull << 63); }
__host__ __device__ __forceinline__ uint64_t qt_unkey(uint64_t k) { return k ^ ((k >> 63) ? 1ull << 63 : ~0ull); }

// r = max(1, ceil(u S / 2^53)), u <= 2^53, S < 2^63 (scale_u53's hi/lo form)
__device__ __forceinline__ uint64_t qt_rank(uint64_t u, uint64_t S) {
  const uint64_t lo = u * S, hi = __umul64hi(u, S);
  const uint64_t c = ((hi << 11) | (lo >> 53)) + ((lo & ((1ull << 53) - 1)) != 0 ? 1 : 0);
  return c ? c : 1;
}

struct QtArgs {
  EstArgs e;               // (part, res unused)
  uint64_t* hist;          // [pairs][kQtBins], zero on entry
  const uint64_t* prefix;  // [pairs]: the digits chosen so far, in place (pass > 0)
  const uint64_t* ctl;     // ctl[p] != 0: pass p + 1 is a dense one
  double qscale;           // 2^shift
  int n_probs, pass;
};

// (IDX: est_tiles' index-array mode, instantiated by gh_inst_path.hip)
template <int D, bool IDX = false>
__global__ __launch_bounds__(kBlock) void k_qt_hist(QtArgs a) {
  constexpr int JC = qt_chunk_probs(D);
  __shared__ est_d2 stage[state_rows(D) && !IDX ? (kBlock / 64) * kTileP * D / 2 : 1];
  __shared__ unsigned long long bins[JC * D * kQtBins];
  const int lo = 64 - kQtBits * (a.pass + 1);  // the digit's position
  const bool first_pass = a.pass == 0;
  if (!first_pass && a.ctl[a.pass - 1] == 0) {
    // A sparse pass: hardly a lane matches, so the blocks of the first chunk
    // take every probability (the state is read once, not once per chunk) and
    // a matching lane adds to the global histogram itself.
    if (blockIdx.y != 0) return;
    unsigned long long* g = (unsigned long long*)a.hist;
    est_tiles<D, IDX>(a.e, stage, [&](double w, const double* x) {
      const uint64_t q = w == w ? f64_to_u52(w * a.qscale) : 0;
      const bool live = q != 0;
      if (!__builtin_amdgcn_ballot_w64(live)) return;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const uint64_t key = qt_key(as_u64(x[k]));
        uint64_t ppre = 0, mask = 0;
        bool have = false, match = false;
        for (int j = 0; j < a.n_probs; ++j) {
          const uint64_t pre = a.prefix[j * D + k];
          if (!have || pre != ppre) {
            have = true;
            ppre = pre;
            match = live && ((key ^ pre) >> (lo + kQtBits)) == 0;
            mask = __builtin_amdgcn_ballot_w64(match);
          }
          if (mask && match)
            atomicAdd(g + (size_t)(j * D + k) * kQtBins + ((key >> lo) & (kQtBins - 1)), (unsigned long long)q);
        }
      }
    });
    return;
  }
  // (pass 0: no prefix yet, so the probabilities share one histogram per
  // component, pair (0, k)'s, which the first chunk's blocks fill)
  if (first_pass && blockIdx.y != 0) return;
  const int j0 = blockIdx.y * JC;
  const int nj = first_pass ? 1 : (a.n_probs - j0 < JC ? a.n_probs - j0 : JC);
  for (int i = threadIdx.x; i < JC * D * kQtBins; i += kBlock) bins[i] = 0;
  lds_barrier();
  est_tiles<D, IDX>(a.e, stage, [&](double w, const double* x) {
    const uint64_t q = w == w ? f64_to_u52(w * a.qscale) : 0;
    const bool live = q != 0;
    if (!__builtin_amdgcn_ballot_w64(live)) return;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t key = qt_key(as_u64(x[k]));
      const int digit = (int)((key >> lo) & (kQtBins - 1));
      // the last distinct prefix of this component (wave-uniform but `match`)
      uint64_t ppre = 0, mask = 0;
      bool have = false, match = false;
      for (int jj = 0; jj < nj; ++jj) {
        const uint64_t pre = first_pass ? 0 : a.prefix[(j0 + jj) * D + k];
        if (!have || pre != ppre) {
          have = true;
          ppre = pre;
          match = live && (first_pass || ((key ^ pre) >> (lo + kQtBits)) == 0);
          mask = __builtin_amdgcn_ballot_w64(match);
        }
        if (mask && match) atomicAdd(bins + (jj * D + k) * kQtBins + digit, (unsigned long long)q);
      }
    }
  });
  lds_barrier();
  unsigned long long* g = (unsigned long long*)a.hist + (size_t)j0 * D * kQtBins;
  for (int i = threadIdx.x; i < nj * D * kQtBins; i += kBlock) {
    const unsigned long long v = bins[i];
    if (v) atomicAdd(g + i, v);
  }
}

struct QtSel {
  uint64_t* hist;
  uint64_t* prefix;
  uint64_t* rank;
  uint64_t* ctl;           // ctl[pass]: a chosen bin holds more than S >> kQtSparseShift; ctl[kQtPasses]: S
  double* res;             // res[0]: NaN when S = 0; res[1 + pair]: the quantile (last pass)
  int pairs, D, pass;
  uint64_t u[kQtMaxProbs]; // floor(p_j 2^53)
};

// a wave per pair: lane l holds bins 4l..4l+3, the running sums by a wave scan
static __global__ __launch_bounds__(1024) void k_qt_select(QtSel s) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lo = 64 - kQtBits * (s.pass + 1);
  __shared__ int dense;
  if (threadIdx.x == 0) dense = 0;
  __syncthreads();
  for (int pair = w; pair < s.pairs; pair += 16) {
    // (pass 0: the component's one histogram, cleared below once every wave has read it)
    uint64_t* h = s.hist + (size_t)(s.pass == 0 ? pair % s.D : pair) * kQtBins + 4 * lane;
    uint64_t b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = h[i];
    if (s.pass != 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = 0;
    }
    const uint64_t local = (b[0] + b[1]) + (b[2] + b[3]);
    const uint64_t incl = wave_incl_sum_u64(local);
    uint64_t r, pre = 0, S;
    if (s.pass == 0) {
      S = readlane63_u64(incl);
      r = qt_rank(s.u[pair / s.D], S);
      if (S == 0 && lane == 0) s.res[0] = NAN;
      if (pair == 0 && lane == 0) s.ctl[kQtPasses] = S;
    } else {
      S = s.ctl[kQtPasses];
      r = s.rank[pair];
      pre = s.prefix[pair];
    }
    const uint64_t cross = __builtin_amdgcn_ballot_w64(incl >= r);
    const int L = cross ? (int)__builtin_ctzll(cross) : 63;  // (S = 0: no crossing; the marker is set)
    if (lane == L) {
      uint64_t run = incl - local;
      int i = 0;  // the first of the lane's bins that reaches r (the last one if none before it does)
      uint64_t held = b[0];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (i == c && run + b[c] < r) {
          run += b[c];
          i = c + 1;
          held = b[c + 1];
        }
      if (held > (S >> kQtSparseShift)) dense = 1;
      pre |= (uint64_t)(4 * L + i) << lo;
      s.prefix[pair] = pre;
      s.rank[pair] = r - run;
      if (s.pass == kQtPasses - 1) s.res[1 + pair] = as_f64(qt_unkey(pre));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) s.ctl[s.pass] = (uint64_t)dense;
  if (s.pass == 0)
    for (int i = threadIdx.x; i < s.D * kQtBins; i += 1024) s.hist[i] = 0;
}

}  // namespace gh

// per dimension (GH_FOR_D of gh_shapes.h); X is `extern template` or `template`, as in gh_inst.h
#define GH_QT_KERNELS(X, D) X __global__ void gh::k_qt_hist<D>(gh::QtArgs);
