// gh_rank_ab.h — the batched loop's multi-rank resample on the peer transport
// in ONE launch.
//
// maybe_resample! (particle_filter.jl:189-213) on R ranks after a max-only
// step was two launches: k_rank_a2 (the global maximum through the mailboxes,
// quantisation and the weight sums, tile totals behind one grid barrier that
// only block 0 waited on, the rank record published to every rank) and
// k_rank_b (every block polls the R records, takes the decision, re-reads its
// log-weights, quantises them AGAIN, re-sums the tile totals before it, and
// writes the range marks and the rows other ranks take).  On the peer
// transport every exchange is a device-side poll, so nothing forces the
// launch boundary: k_rank_ab keeps each thread's quantised weights in
// registers from the quantisation to the marks, every block reads the tile
// totals it needs in the barrier it crosses anyway (as k_resample1 does), and
// the marks loop is the one k_resample1 runs (32-bit slots, incremental slot
// counts, exact recount near integers) on the global CDF: the kernel is
// phases calling the parts of gh_resample_parts.h.  The values — tile
// totals, records, decision, marks, rows — are the two-kernel path's bit for
// bit (tests/test_multirank.py peer cases against the single-rank oracle).
#pragma once
#include "gh_kernels.h"

namespace gh {

struct RankABArgs {
  RankA2Args a;  // the fold, quantisation, tile words and record (pb, amax_own, use_sh, use_rec)
  RankBArgs b;   // the decision, marks and rows (pb, use_rec, prow, amax_reset, hplan / htag, d)
};

template <int IT>
__global__ __launch_bounds__(kRsBlock, IT <= 4 ? 8 : 1) void k_rank_ab(RankABArgs args) {
  const RankA2Args& ra = args.a;
  const RankBArgs& rb = args.b;
  __shared__ double smd[32];
  __shared__ uint64_t smu[32];
  __shared__ unsigned sgen;
  __shared__ int sfail, sfire;
  __shared__ uint64_t spa[8], spb[8];
  __shared__ double spg[2][8];
  __shared__ double sM;
  __shared__ uint64_t su53, sbefore;
  __shared__ uint64_t srec[kRecWords];
  __shared__ uint64_t srecs[kPeerMaxRanks * kRecWords];
  __shared__ DevScalars sd;
  __shared__ int64_t sdst_lo[kPeerMaxRanks], sra_all[kPeerMaxRanks], srb_all[kPeerMaxRanks];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int R = ra.pb.R;
  if (threadIdx.x == 0) {
    sgen = ra.dev->bar_gen + 1;  // (read before this block publishes)
    sfail = 0;
  }
  const int64_t i0 = (int64_t)blockIdx.x * (kRsBlock * IT) + (int64_t)threadIdx.x * IT;
  double lw[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) lw[k] = (i0 + k < ra.n) ? ra.logw[i0 + k] : -INFINITY;
  // ---- the global maximum: this rank's shards (every block), published to
  // every rank by block 0, the R ranks' polled from the own mailbox
  {
    const uint64_t k0 = threadIdx.x < kAmaxShards ? ra.amax_own[threadIdx.x * kAmaxStride] : kAmaxEmpty;
    const double Ml = blk16_max1(amax_value(k0), smd);
    if (w == 0) {
      const int par = (int)(ra.use_sh & 1);
      const uint64_t* own = ra.pb.peer[ra.pb.rank];
      if (blockIdx.x == 0)
        peer_publish(ra.pb, mb_sh(R, par, ra.pb.rank), mb_sh_tag(R, par, ra.pb.rank), amax_key(Ml), 1, ra.use_sh);
      const bool ok = peer_poll(own, mb_sh_tag(R, par, 0), R, ra.use_sh, ra.pb.wait_ticks);
      uint64_t kk = ok && lane < R ? ld_sys(own + mb_sh(R, par, lane)) : kAmaxEmpty;
      kk = readlane63_u64(wave_incl_max_u64(kk));
      if (lane == 0) {
        sM = ok ? amax_value(kk) : NAN;
        if (!ok) {
          sfail = 1;
          ra.dev->error = kErrPeer;  // a rank never published
        }
      }
    }
    if (threadIdx.x == 8 * 64) {  // a non-polling wave draws the systematic offset's uniform meanwhile
      const u32x4 wr = rng_block(rb.seed, ~0ull, rb.t, STREAM_RESAMPLE, 0);
      su53 = u53_bits(wr.x, wr.y);
    }
    lds_barrier();
  }
  const double M = sM;
  const bool m_ok = M > -INFINITY && M != INFINITY && M == M;  // (uniform over every rank's grid)
  // ---- quantise the tile (the weights stay in registers for the marks), the
  // tile's sums, one tagged word each, and the grid barrier every block
  // crosses: its tile offset (the totals before it), the rank total and sums
  const double qscale = as_f64((uint64_t)(ra.shift + 1023) << 52);
  uint64_t q[IT];
  uint64_t tsum = 0, incl = 0;
  if (m_ok) {
    double s1, s2;
    tile_quantise<IT, true>(lw, i0, ra.n, M, qscale, q, tsum, s1, s2);
    incl = blk16_scan<true>(tsum, &s1, &s2, smu, smd);
    const uint64_t par = tile_parity(sgen);
    tile_publish(ra, par, incl, s1, s2);
    tile_poll<true, true, false>(ra, par, true, spa, spb, spg, &sfail);
    lds_barrier();
    if (threadIdx.x == 0) {  // (k_rank_a2's record: the same sums in the same order)
      uint64_t all = 0, before = 0;
      double g1 = 0.0, g2 = 0.0;
#pragma unroll 1
      for (int k = 0; k < 8; ++k) {  // (not unrolled: 32 LDS values at once would spill the kept weights)
        all += spa[k];
        before += spb[k];
        g1 += spg[0][k];
        g2 += spg[1][k];
      }
      if (sfail) {
        ra.dev->error = kErrBarrier;  // partial totals
        g1 = NAN;
      }
      sbefore = before;
      srec[0] = all;
      srec[1] = as_u64(g1);
      srec[2] = as_u64(g2);
      srec[3] = as_u64(M);
      if (blockIdx.x == 0) {
        ra.dev->local = all;
        ra.dev->bar_gen = sgen;  // every block has published, so has read the old value
      }
    }
  } else if (threadIdx.x == 0) {  // no tile publishes: the record carries M, the decision raises GH_E_NUMERIC
    sbefore = 0;
    srec[0] = 0;
    srec[1] = 0;
    srec[2] = 0;
    srec[3] = as_u64(M);
    if (blockIdx.x == 0) ra.dev->local = 0;
  }
  lds_barrier();
  // ---- the rank records: block 0 publishes this rank's to every mailbox,
  // every block polls the R records from its own
  if (w == 0) {
    const int par = (int)(ra.use_rec & 1);
    if (blockIdx.x == 0) {
      if (lane < kRecWords) ra.rec[lane] = srec[lane];  // (the host's copy: the plan mailbox below)
      peer_publish(ra.pb, mb_rec(R, par, ra.pb.rank), mb_rec_tag(R, par, ra.pb.rank),
                   lane < kRecWords ? srec[lane] : 0ull, kRecWords, ra.use_rec);
    }
    const bool ok = poll_records(ra.pb, ra.use_rec, srecs, ra.dev, rb.amax_reset);  // (the shards: read above)
    if (!ok && lane == 0) sfail = 1;
  }
  lds_barrier();
  // ---- the decision from the R records (every block the same), committed by block 0
  if (threadIdx.x == 0) {
    const Decision dec = decide_records(srecs, R, rb.d.thr);
    sfire = dec.fire && !sfail;
    if (blockIdx.x == 0) commit_records(rb.d, dec, rb.dev, srecs, R, rb.hplan, rb.htag);
  }
  lds_barrier();
  if (!sfire) return;
  // ---- the plan (thread 0): the global systematic constants, every rank's
  // slot block and the part of it other ranks cover (the rows' layout there)
  const uint32_t N = (uint32_t)rb.mk.n_global;  // < 2^31 (host-checked): 32-bit slots
  if (threadIdx.x == 0) {
    uint64_t S = 0, base = 0;
    for (int k = 0; k < R; ++k) {
      if (k < rb.rank) base += srecs[k * kRecWords];
      S += srecs[k * kRecWords];
    }
    sys_constants(sd, S, base, srecs[rb.rank * kRecWords], su53, N, rb.d.inv_n);
    recv_coverage(&sd, N, R, srecs, kRecWords, rb.dlo, sra_all, srb_all, sdst_lo);
    if (blockIdx.x == 0) {
      sys_constants_mirror(rb.dev, sd);
      rb.dev->ra = sra_all[rb.rank];
      rb.dev->rb = srb_all[rb.rank];
    }
  }
  lds_barrier();
  // ---- the marks on the global CDF, clamped to this rank's slots, and the
  // rows of slots other ranks own (only a range that crosses this rank's block
  // edge has any), stored into their buffers
  const int32_t own_lo = (int32_t)rb.lo, own_hi = (int32_t)(rb.lo + rb.n);
  marks_loop<IT>(&sd, rb.mk, N, sd.base + sbefore + incl - tsum, q, i0, OwnSlots{own_lo, own_hi},
                 [&](int, int64_t i, int32_t s_i, int32_t e_i, uint64_t) {
                   if (e_i > s_i && (s_i < own_lo || e_i > own_hi))
                     send_rows_peer(s_i, e_i, i, own_lo, own_hi, R, N, sdst_lo, sra_all, srb_all, rb.prow, rb.xprev,
                                    rb.D, rb.lo);
                 });
}

}  // namespace gh
