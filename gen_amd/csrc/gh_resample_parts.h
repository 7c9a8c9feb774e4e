// gh_resample_parts.h — the pieces the systematic resample kernels share
// (DESIGN.md §6, §7): k_resample1 (one rank), k_rank_a2 + k_rank_b (multi-rank,
// two launches) and k_rank_ab (gh_rank_ab.h: the peer transport's one launch).
// The multi-rank paths must reproduce the one-rank tile totals, records,
// decision, marks and rows bit for bit, so each piece exists once: the tile
// quantisation, the tagged tile words and their polling barrier, the
// systematic constants, the marks loop, and the rank records with the
// decision and the receivers' coverage taken from them.
//
// Included by gh_kernels.h (not on its own) below the primitives it builds
// on.  Everything is inlined into the calling kernel: the kernels are tuned to
// their register budgets (two 1024-thread blocks per CU at IT = 4), so a part
// takes kernel arguments by value or const reference (SGPRs) and keeps no
// state of its own.
#pragma once

namespace gh {

// ---------------------------------------------------------- tile quantisation
// q_k = floor(exp(w_k - M) 2^shift) of the thread's IT consecutive particles
// (qscale = 2^shift; = quantize_weight: the branch-free exp, the 3-instruction
// conversion, e 2^shift <= 2^52), their sum, and with SUMS the thread's sums of
// e and e^2 from the same exps (a NaN log-weight quantises to 0 and poisons
// the sums).  Particles past n weigh nothing.  A caller that does not use q[]
// (k_rank_a2) pays nothing for it.
template <int IT, bool SUMS>
__device__ __forceinline__ void tile_quantise(const double (&lw)[IT], int64_t i0, int64_t n, double M, double qscale,
                                              uint64_t (&q)[IT], uint64_t& tsum, double& s1, double& s2) {
  tsum = 0;
  s1 = 0.0;
  s2 = 0.0;
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const bool in = i0 + k < n;
    const double e = in ? gh_exp_nonpos(lw[k] - M) : 0.0;
    q[k] = e == e ? f64_to_u52(e * qscale) : 0;
    tsum += q[k];
    if (SUMS) {
      const double ee = lw[k] != lw[k] ? lw[k] : e;  // NaN poisons the statistics
      s1 += ee;
      s2 += ee * ee;
    }
  }
}

// ------------------------------------------------------------- the tile words
// The grid barrier of the resample: each tile total (< 2^62) is published as
// ONE 8-byte agent-scope store tagged in bit 63 with the parity of the barrier
// generation, and read back with agent-scope loads until every tag matches
// (the payload is its own flag: no counter, no fence).  The tile sums of e and
// e^2 (>= 0, so their sign bit is free) are published and polled the same way.
// All three words are published on EVERY generation (sums of 0 when the pass
// takes none), so each word alternates its tag strictly and a matching tag
// always means this generation's value: a poller can never pair a fresh tile
// total with sums left over from two generations back.
constexpr uint64_t kTileTag = 1ull << 63;
__device__ __forceinline__ uint64_t tile_parity(unsigned gen) { return (gen & 1u) ? kTileTag : 0ull; }

// (r: the kernel's arguments, with the word arrays tsum, ts1, ts2 [grid])
// incl: the block's inclusive scan (the tile total in its last thread); s1, s2:
// the tile sums (thread 0's)
template <class Args>
__device__ __forceinline__ void tile_publish(const Args& r, uint64_t par, uint64_t incl, double s1, double s2) {
  if (threadIdx.x == kRsBlock - 1) st_sc1(&r.tsum[blockIdx.x], incl | par);
  if (threadIdx.x == 0) {
    st_sc1(&r.ts1[blockIdx.x], (as_u64(s1) & ~kTileTag) | par);
    st_sc1(&r.ts2[blockIdx.x], (as_u64(s2) & ~kTileTag) | par);
  }
}

// Waves 0..7 read the tile words, 64 tiles each (grid <= 512, host-checked):
// one poll in flight per lane, so the caller's register budget stays at two
// resident 1024-thread blocks per CU.  Each wave leaves its sums in LDS: the
// tiles' total (spa) and the total of the tiles before this block (spb) with
// TOTALS, the sums of e and e^2 (spg, zeros without SUMS); the integer totals
// in any order, the weight sums by the DPP tree, and the caller's thread 0
// combines the eight in wave order — the same arithmetic in every block.
// With TOTALS the totals are polled alone while the grid publishes, then
// (wait_sums, wave-uniform) the tile sums published with them until their tags
// match too: a third of the polling traffic while lagging blocks still load
// their tiles (C4, 512 tiles: barrier 2.2 us sooner, 39.7 -> 37.8 us per step;
// C2 -0.9 us).  Without TOTALS (a block that crossed the barrier before and
// now wants the sums) only the sums are polled.
// The waits are bounded (~0.5 s each): a grid that is not co-resident times
// out with partial sums and *sfail set — REPORT: by the polling wave, with
// kErrBarrier in dev->error; otherwise by the wave's lane 0 after its sums, the
// caller reporting the error.  Called by every thread of the block; the caller
// crosses an LDS barrier before it reads the arrays.
template <bool TOTALS, bool SUMS, bool REPORT, class Args>
__device__ __forceinline__ void tile_poll(const Args& r, uint64_t par, bool wait_sums, uint64_t* spa, uint64_t* spb,
                                          double (*spg)[8], int* sfail) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w < 8) {
    const unsigned b = (unsigned)(w * 64 + lane);
    const bool mine = b < gridDim.x;
    uint64_t v = par, v1 = par, v2 = par;
    bool ok = !mine, timed_out = false;  // (wave-uniform)
    if (TOTALS) {
      for (unsigned spins = 0;; ++spins) {
        if (!ok) v = ld_sc1(&r.tsum[b]);
        ok = ok || (v & kTileTag) == par;
        if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
        if (spins == (1u << 22)) {
          if (REPORT) {
            r.dev->error = kErrBarrier;
            *sfail = 1;
          }
          timed_out = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    ok = !mine || !wait_sums || timed_out;  // (a timed-out wave does not wait a second time)
    for (unsigned spins = 0;; ++spins) {
      if (!ok) {
        v1 = ld_sc1(&r.ts1[b]);
        v2 = ld_sc1(&r.ts2[b]);
      }
      ok = ok || ((v1 & kTileTag) == par && (v2 & kTileTag) == par);
      if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
      if (spins == (1u << 22)) {
        if (REPORT) {
          r.dev->error = kErrBarrier;
          *sfail = 1;
        }
        timed_out = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    uint64_t all = 0, before = 0;
    if (TOTALS) {
      const uint64_t x = mine ? (v & ~kTileTag) : 0ull;
      all = wave_sum_u64(x);
      before = wave_sum_u64(b < blockIdx.x ? x : 0ull);
    }
    double g1 = 0.0, g2 = 0.0;
    if (SUMS) {
      g1 = wave_sum(mine ? as_f64(v1 & ~kTileTag) : 0.0);
      g2 = wave_sum(mine ? as_f64(v2 & ~kTileTag) : 0.0);
    }
    if (lane == 0) {
      if (TOTALS) {
        spa[w] = all;
        spb[w] = before;
      }
      spg[0][w] = g1;
      spg[1][w] = g2;
      if (!REPORT && timed_out) *sfail = 1;
    }
  }
}

// ------------------------------------------------- the systematic constants
// Thread 0's plan of a resample that fires: the global total S, this rank's
// base (the totals of the ranks before it) and own total, the offset
// o = floor(u S) of the systematic comb from the step's uniform (su53), and
// the constants of sys_target / sys_count.
__device__ __forceinline__ void sys_constants(DevScalars& sd, uint64_t S, uint64_t base, uint64_t local, uint64_t su53,
                                              uint64_t N, double inv_n) {
  sd.S = S;
  sd.base = base;
  sd.local = local;
  sd.o = scale_u53(su53, S);
  sd.invN = inv_n;
  sd.Qs = udiv_n(S, N, sd.invN);
  sd.Rs = S - sd.Qs * N;
  sd.invS = recip_est((double)S);
}
// block 0's copy for the kernels that follow (local, ra, rb: the caller's)
__device__ __forceinline__ void sys_constants_mirror(DevScalars* dev, const DevScalars& sd) {
  dev->S = sd.S;
  dev->base = sd.base;
  dev->o = sd.o;
  dev->Qs = sd.Qs;
  dev->Rs = sd.Rs;
  dev->invN = sd.invN;
  dev->invS = sd.invS;
}

// --------------------------------------------------------------- the marks
// The thread's IT particles, the CDF before them `run`: particle i owns the
// global slots [s_i, e_i) = [count(C_{i-1}), count(C_i)).  The part of the
// range inside the caller's slot space — local(s): the slot's index there, the
// identity on one rank, clamped to the rank's block on several — gets a tagged
// mark at its start and the carry of every 64-slot group that starts inside
// it; a lane writes up to two carries itself, a longer range (a particle with
// > 128 offspring) gets its carries from the whole wave (one wave-wide store
// loop per such particle: no LDS copy of the range ends, no block barrier).
// Then each(k, i, s_i, e_i, run) sees the particle (the rows other ranks take).
//
// The slot counts count(X) = ceil(v), v = (X N - o) / S, as sys_count, but
// v advances by q N / S per particle (one FMA on the quantised weight, exact
// as a double) instead of being re-derived from the 64-bit X.  Error: v_0 is
// within 8 N 2^-53 + 2^-53 of the exact quotient (sys_count); ns = N / S to
// within 6 units of 2^-53 (1/S within 2 ulp, one product), so the tile's
// increments q ns add at most 6 N 2^-53 (their exact sum is <= N); each FMA
// rounds by at most N 2^-53: |v - v*| <= (14 + IT) N 2^-53 + 2^-53 <=
// 31 N 2^-53 + 2^-53 for IT <= 16, a quarter of count_window(N), so ceil(v)
// is exact outside the window and the count is taken exactly inside it.  No
// clamps or edge tests: for 0 < X < S, v* lies in (-1, N); X = 0 and X = S
// give v* = -o/S and N - o/S, whose ceilings are 0 and N (o small: inside
// the window, so the exact count).  Slots and groups are 32-bit (N < 2^31, as
// gh_pf_init enforces).
template <int IT, class Local, class Each>
__device__ __forceinline__ void marks_loop(const DevScalars* sd, const MarkArgs& mk, uint32_t N, uint64_t run,
                                           const uint64_t (&q)[IT], int64_t i0, Local local, Each each) {
  static_assert(IT <= 16, "the error bound of the incremental slot counts");
  uint32_t* const mark = mk.mark;  // (read once: SGPRs through the loop)
  uint32_t* const cmark = mk.cmark;
  const uint32_t tag = mk.tag;
  const double ns = as_f64(readfirstlane_u64(as_u64((double)N * sd->invS)));  // (uniform: SGPRs)
  // near the integers: |fr - 1/2| >= 1/2 - w (1/2 - w is a double, so the
  // rounding of fr - 1/2 never takes a near value out; it may take a value
  // just outside the window in, which only costs an exact count)
  const double hw = as_f64(readfirstlane_u64(as_u64(0.5 - count_window(N))));
  double v = fma((double)run, (double)N, -(double)sd->o) * sd->invS;
  auto count = [&](uint64_t X) {
    const double fl = floor(v);
    const double fr = v - fl;
    int32_t j = (int32_t)fl + 1;
    const bool near = fabs(fr - 0.5) >= hw;
    if (near) j = sys_count_exact_call(sd, N, X);  // (exec-masked call, skipped when no lane is near)
    return j;
  };
  int32_t s_i = count(run);
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    run += q[k];
    v = fma(u52_to_f64(q[k]), ns, v);
    const int64_t i = i0 + k;
    // (a particle past n or of zero weight leaves run, v, hence the count, unchanged)
    const int32_t e_i = count(run);
    const uint32_t l0 = local(s_i), l1 = local(e_i);
    const uint32_t tagged = tag | (uint32_t)i;
    if (l1 > l0) mark[l0] = tagged;
    const uint32_t g0 = (l0 + 63u) >> 6, g1 = (l1 + 63u) >> 6;  // groups g with 64 g in [l0, l1)
    const bool many = g1 - g0 > 2u;
    if (!many) {
      if (g1 > g0) cmark[g0] = tagged;
      if (g1 > g0 + 1u) cmark[g0 + 1u] = tagged;
    }
    uint64_t bm = __builtin_amdgcn_ballot_w64(many);
    while (bm) {
      const int L = __builtin_ctzll(bm);
      bm &= bm - 1;
      const int32_t a0 = __builtin_amdgcn_readlane((int32_t)g0, L), a1 = __builtin_amdgcn_readlane((int32_t)g1, L);
      const uint32_t tg = tag | (uint32_t)__builtin_amdgcn_readlane((int32_t)i, L);
      for (int32_t g = a0 + (threadIdx.x & 63); g < a1; g += 64) cmark[g] = tg;
    }
    each(k, i, s_i, e_i, run);
    s_i = e_i;
  }
}

// the slot mappers: one rank owns every slot; rank q owns [own_lo, own_hi)
// (32-bit, so the clamp is one v_med3_i32, not 64-bit compares and selects)
struct AllSlots {
  __device__ __forceinline__ uint32_t operator()(int32_t s) const { return (uint32_t)s; }
};
struct OwnSlots {
  int32_t own_lo, own_hi;
  __device__ __forceinline__ uint32_t operator()(int32_t s) const {
    return (uint32_t)(min(max(s, own_lo), own_hi) - own_lo);
  }
};

// ------------------------------------------------------- the rank records
// One wave: the R rank records (k_rank_a2's: integer total, S_r, S2_r, M) from
// the own mailbox into srecs, once every rank has published its record for
// this use; block 0 then empties the shards the records' maximum was read
// from.  A rank that never publishes (bounded wait): NaN records, so the
// decision raises, and kErrPeer; false is returned.
__device__ __forceinline__ bool poll_records(const PeerBox& pb, uint64_t use_rec, uint64_t* srecs, DevScalars* dev,
                                             uint64_t* amax_reset) {
  const int lane = threadIdx.x & 63, par = (int)(use_rec & 1);
  const uint64_t* own = pb.peer[pb.rank];
  const bool ok = peer_poll(own, mb_rec_tag(pb.R, par, 0), pb.R, use_rec, pb.wait_ticks);
  if (lane < pb.R)
    for (int k = 0; k < kRecWords; ++k)
      srecs[lane * kRecWords + k] = ok ? ld_sys(own + mb_rec(pb.R, par, lane) + k) : (k == 3 ? as_u64(NAN) : 0ull);
  if (!ok && lane == 0) dev->error = kErrPeer;  // a rank never published its record
  if (blockIdx.x == 0 && lane < kAmaxShards) amax_reset[lane * kAmaxStride] = kAmaxEmpty;
  return ok;
}

// Block 0's thread 0 commits the decision taken from the records, and hands
// the host its copy of them (the plan mailbox hplan, when there is one): the
// R records, then the tag behind a system-scope release.
__device__ __forceinline__ void commit_records(const DecideArgs& d, const Decision& dec, DevScalars* dev,
                                               const uint64_t* recs, int R, uint64_t* hplan, uint64_t htag) {
  dev->pending = 0;
  commit_decision(d, dec, dev, 0);
  if (hplan) {
    for (int w = 0; w < R * kRecWords; ++w) hplan[1 + w] = recs[w];
    __threadfence_system();
    __hip_atomic_store(&hplan[0], htag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Thread 0: every receiving rank's split of its slot block [dlo_k, dlo_k+1)
// into the slots other ranks cover, [0, ra_k) and [rb_k, n_k) (local), from
// the rank totals (rank k's at totals[k * stride]): the layout of the rows
// sent to it (send_rows_peer).  dst_lo (optional) takes the block starts.
__device__ __forceinline__ void recv_coverage(const DevScalars* sd, uint64_t N, int R, const uint64_t* totals,
                                              int stride, const int64_t* dlo, int64_t* ra_all, int64_t* rb_all,
                                              int64_t* dst_lo) {
  uint64_t bk = 0;
  for (int k = 0; k < R; ++k) {
    const uint64_t tk = totals[k * stride];
    const int64_t dl = dlo[k], dh = dlo[k + 1];
    const int64_t lo_k = sys_count_exact(sd, N, bk), hi_k = sys_count_exact(sd, N, bk + tk);
    if (dst_lo) dst_lo[k] = dl;
    ra_all[k] = (lo_k < dl ? dl : (lo_k > dh ? dh : lo_k)) - dl;
    rb_all[k] = (hi_k < dl ? dl : (hi_k > dh ? dh : hi_k)) - dl;
    bk += tk;
  }
}

}  // namespace gh
