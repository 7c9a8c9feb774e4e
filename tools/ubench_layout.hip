// State-layout microbenchmark (timing-only tool, not part of the product):
// the C2 step's HBM skeleton (range marks -> DPP prefix max -> gather of the
// ancestor's D=10 fp64 components -> store of the new state, logw, ancestor)
// in record_history mode (16 rotating slots: every launch writes fresh lines)
// under different placements of the D components of one particle.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_layout.hip -o tools/ubench_layout
//   tools/ubench_layout [ANC.bin] [--pmc]
//
// Layouts:
//   soa_pP     column k of slot s at s*SP + k*(N+P) doubles (P = pad)
//   tile_B     [N/B][D][B] per slot: a B-particle tile's components contiguous
//   pair_64    [N/64][D/2][64][2]: the product's wave tiles, 16-byte pair words
//   row        particle i at doubles [i*D, i*D + D): five 16-byte loads per lane,
//              stores straight from the lanes (80-byte lane stride)
//   row_lds3   row, the stores transposed through 3 KiB of wave-private LDS:
//              components 0-5 as [64][3] words (contiguous 48-byte runs per
//              store instruction), then 6-9 as [64][2] words
//   row_lds5   row, the stores transposed through 5 KiB of wave-private LDS:
//              every store instruction writes 1 KiB contiguous
//   row_ldsh   row, the stores transposed through 2.5 KiB of wave-private LDS in
//              two passes of 32 rows: every store instruction writes whole
//              lines (1 KiB, 1 KiB, 512 B per pass)
//   chunk_32   [N/64]{[64][4], [64][4], [64][2]}: components 0-3 and 4-7 as
//              32-byte chunks per particle, 8-9 as a pair word; no transposition
//   copy_* / rd / wr   halves of the skeleton without marks / gather
// Ancestor patterns (the suffix of a variant's name):
//   c2   ANC.bin when given (int32 ancestors, S steps of N each, written by
//        tools/parent_stats.py from the product's own parents on the bench's
//        C2 run; launch i gathers by step i mod S), else systematic ancestors
//        of iid lognormal weights, sigma 2.16 (28 % survivors, ESS/N 0.009)
//   u4   systematic ancestors of iid weights u^4 (46 % survivors): the
//        pattern of the round-2 layout study
//   id   anc = j (a step without a resample), no marks
// --pmc: three launches per variant and no timing (for a counter run: the
// kernel name carries the layout and the pattern, k_lay<layout, pattern>).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

constexpr int D = 10;
constexpr int64_t N = 1 << 20;
constexpr int kBlock = 256;
constexpr int kSlots = 16;

template <int CTRL>
__device__ __forceinline__ uint64_t dppmv(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo;
}
__device__ __forceinline__ uint64_t wave_incl_max_u64(uint64_t v) {
  const int lane = threadIdx.x & 63, rl = lane & 15;
  uint64_t t;
  t = dppmv<0x111>(v); if (rl >= 1 && t > v) v = t;
  t = dppmv<0x112>(v); if (rl >= 2 && t > v) v = t;
  t = dppmv<0x114>(v); if (rl >= 4 && t > v) v = t;
  t = dppmv<0x118>(v); if (rl >= 8 && t > v) v = t;
  t = dppmv<0x142>(v); if ((lane & 31) >= 16 && t > v) v = t;
  t = dppmv<0x143>(v); if (lane >= 32 && t > v) v = t;
  return v;
}

struct Args {
  const double* x;
  double* y;
  const uint64_t* mark;
  const uint64_t* carry;
  int32_t* anc;
  double* logw;
};

// ------------------------------------------------- 16-byte-word layouts
enum { PAIR = 0, ROW = 1, ROW_LDS3 = 2, ROW_LDS5 = 3, CHUNK32 = 4, ROW_LDSH = 5 };
enum { ID = 0, C2 = 1, U4 = 2 };

// index (in doubles) of 16-byte word c of particle i (components 2c, 2c+1);
// every layout keeps a 64-particle tile in 64*D contiguous doubles
template <int LAY>
__device__ __forceinline__ int64_t at_word(int64_t i, int c) {
  if (LAY == PAIR) return (i >> 6) * (64 * D) + c * 128 + (i & 63) * 2;
  if (LAY == CHUNK32)
    return (i >> 6) * (64 * D) + (c < 4 ? (c >> 1) * 256 + (i & 63) * 4 + (c & 1) * 2 : 512 + (i & 63) * 2);
  return i * D + 2 * c;  // rows
}

// wave-private LDS hand-off between a lane's writes and other lanes' reads
// (one wave's LDS operations execute in order; the compiler must keep it)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <int LAY, int PAT>  // PAT only names the kernel: ID has no gather, C2 and U4 differ in the marks
__global__ __launch_bounds__(kBlock) void k_lay(Args a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t tile = (int64_t)blockIdx.x * 4 + w;
  const int64_t j = tile * 64 + lane;
  int64_t src = j;
  if (PAT != ID) {
    uint64_t v = a.mark[j];
    const uint64_t c = a.carry[tile];
    v = wave_incl_max_u64(v > c ? v : c);
    src = (int64_t)(uint32_t)v;
    a.anc[j] = (int32_t)src;
  }
  double2 y[D / 2];
#pragma unroll
  for (int c = 0; c < D / 2; ++c) y[c] = *reinterpret_cast<const double2*>(&a.x[at_word<LAY>(src, c)]);
#pragma unroll
  for (int c = 0; c < D / 2; ++c) {
    y[c].x += 1.0;
    y[c].y += 1.0;
  }
  double* const yt = a.y + tile * (64 * D);  // this wave's tile of the output slot
  if constexpr (LAY == ROW_LDS3) {
    __shared__ double2 stg[kBlock / 64][192];
    double2* const s = stg[w];
#pragma unroll
    for (int q = 0; q < 3; ++q) s[lane * 3 + q] = y[q];
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 3; ++m) {  // word W = 64 m + lane is word W % 3 of row W / 3
      const int W = m * 64 + lane, r = W / 3;
      *reinterpret_cast<double2*>(&yt[r * D + (W - 3 * r) * 2]) = s[W];
    }
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 2; ++q) s[lane * 2 + q] = y[3 + q];
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int W = m * 64 + lane;
      *reinterpret_cast<double2*>(&yt[(W >> 1) * D + 6 + (W & 1) * 2]) = s[W];
    }
  } else if constexpr (LAY == ROW_LDS5) {
    __shared__ double2 stg5[kBlock / 64][320];
    double2* const s = stg5[w];
#pragma unroll
    for (int c = 0; c < 5; ++c) s[lane * 5 + c] = y[c];
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 5; ++m) *reinterpret_cast<double2*>(&yt[(m * 64 + lane) * 2]) = s[m * 64 + lane];
  } else if constexpr (LAY == ROW_LDSH) {
    __shared__ double2 stgh[kBlock / 64][160];
    double2* const s = stgh[w];
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // rows 32 h .. 32 h + 31: 160 words, 2.5 KiB = 20 whole lines
      if (h) wave_lds_sync();
      if ((lane >> 5) == h) {
#pragma unroll
        for (int c = 0; c < 5; ++c) s[(lane & 31) * 5 + c] = y[c];
      }
      wave_lds_sync();
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const int W = m * 64 + lane;
        if (W < 160) *reinterpret_cast<double2*>(&yt[(h * 160 + W) * 2]) = s[W];
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < D / 2; ++c) *reinterpret_cast<double2*>(&a.y[at_word<LAY>(j, c)]) = y[c];
  }
  a.logw[j] = 1.0;
}

// -------------------------------------------------- 8-byte-word layouts
template <int L, int P>
__device__ __forceinline__ int64_t at(int64_t i, int k) {
  if (L == 0) return (int64_t)k * (N + P) + i;                       // SoA, padded pitch
  return (i / L) * (D * L + P) + (int64_t)k * L + (i % L);           // tiles of L particles, P doubles of tile padding
}

template <int L, int P, bool GATHER, int MODE>  // MODE 0 rw, 1 read-only, 2 write-only
__global__ __launch_bounds__(kBlock) void k_skel(Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t j = tile * 64 + lane;
  int64_t src = j;
  if (GATHER) {
    uint64_t v = a.mark[j];
    const uint64_t c = a.carry[tile];
    v = wave_incl_max_u64(v > c ? v : c);
    src = (int64_t)(uint32_t)v;
    a.anc[j] = (int32_t)src;
  }
  double x[D];
  double s = 0.0;
  if (MODE != 2) {
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = a.x[at<L, P>(src, k)];
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = (double)(k + j);
  }
  if (MODE != 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) a.y[at<L, P>(j, k)] = x[k] + 1.0;
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) s += x[k];
  }
  a.logw[j] = s;
}

// ------------------------------------------------------------ host side
static double* g_hist = nullptr;
static int64_t g_slot_pitch = 0;
static int g_slot = 0;

// an ancestor pattern on the device: S steps of marks[N] and carry[N/64]
struct Pattern {
  uint64_t* mark = nullptr;
  uint64_t* carry = nullptr;
  int steps = 0;
};
static Pattern g_pat[3];

static Args next_args(Args a, int pat) {
  a.x = g_hist + (size_t)(g_slot % kSlots) * g_slot_pitch;
  a.y = g_hist + (size_t)((g_slot + 1) % kSlots) * g_slot_pitch;
  if (pat != ID) {
    const int s = g_slot % g_pat[pat].steps;
    a.mark = g_pat[pat].mark + (size_t)s * N;
    a.carry = g_pat[pat].carry + (size_t)s * (N / 64);
  }
  ++g_slot;
  return a;
}

template <int L, int P, bool GATHER, int MODE>
static void launch(Args a) {
  hipLaunchKernelGGL((k_skel<L, P, GATHER, MODE>), dim3(N / kBlock), dim3(kBlock), 0, 0, next_args(a, GATHER ? U4 : ID));
}
template <int LAY, int PAT>
static void launch_lay(Args a) {
  hipLaunchKernelGGL((k_lay<LAY, PAT>), dim3(N / kBlock), dim3(kBlock), 0, 0, next_args(a, PAT));
}

// systematic ancestors of the weights w (offset 0.37)
static std::vector<int32_t> systematic(const std::vector<double>& w) {
  double S = 0;
  for (double v : w) S += v;
  double cum = 0;
  int64_t i = 0;
  std::vector<int32_t> anc(N);
  for (int64_t j = 0; j < N; ++j) {
    const double tgt = (j + 0.37) * S / N;
    while (i < N - 1 && cum + w[i] <= tgt) cum += w[i++];
    anc[j] = (int32_t)i;
  }
  return anc;
}

// uploads the marks of `steps` ancestor vectors (anc: steps * N, sorted within
// a step or not: a mark at every change) and prints what the pattern touches
static bool make_pattern(Pattern& p, const char* name, const std::vector<int32_t>& anc, int steps) {
  std::vector<uint64_t> mark((size_t)steps * N, 0), carry((size_t)steps * (N / 64), 0);
  const uint64_t ep = 5ull << 32;
  double alive = 0, l8 = 0, l4 = 0, rl = 0, rs = 0;
  std::vector<uint8_t> live(N);
  for (int s = 0; s < steps; ++s) {
    const int32_t* a = anc.data() + (size_t)s * N;
    std::fill(live.begin(), live.end(), 0);
    for (int64_t j = 0; j < N; ++j) {
      if (a[j] < 0 || a[j] >= N) {  // (the kernels index the slots by these)
        fprintf(stderr, "%s: ancestor %d of step %d, slot %lld is outside [0, N)\n", name, a[j], s, (long long)j);
        return false;
      }
      live[a[j]] = 1;
      if (j == 0 || a[j] != a[j - 1]) mark[(size_t)s * N + j] = ep | (uint64_t)a[j];
    }
    for (int64_t g = 0; g < N / 64; ++g) carry[(size_t)s * (N / 64) + g] = ep | (uint64_t)a[g * 64];
    int64_t na = 0, n8 = 0, n4 = 0, nrl = 0, nrs = 0, lastl = -1, lasts = -1;
    for (int64_t i = 0; i < N; ++i) {
      if ((i & 7) == 0 && (*reinterpret_cast<const uint64_t*>(&live[i]) != 0)) ++n8;
      if ((i & 3) == 0 && (*reinterpret_cast<const uint32_t*>(&live[i]) != 0)) ++n4;
      if (!live[i]) continue;
      ++na;
      for (int64_t l = i * 80 / 128; l <= (i * 80 + 79) / 128; ++l)
        if (l > lastl) ++nrl, lastl = l;
      for (int64_t l = i * 80 / 64; l <= (i * 80 + 79) / 64; ++l)
        if (l > lasts) ++nrs, lasts = l;
    }
    alive += (double)na / N;
    l8 += (double)n8 / (N / 8);
    l4 += (double)n4 / (N / 4);
    rl += nrl * 128.0 / (80.0 * N);
    rs += nrs * 64.0 / (80.0 * N);
  }
  printf("pattern %-3s %2d step(s): survivors %.3f  pair 128-B lines %.3f  (64-B sectors %.3f)  "
         "row lines %.3f  (sectors %.3f)  chunk_32 lines %.3f\n",
         name, steps, alive / steps, l8 / steps, l4 / steps, rl / steps, rs / steps,
         (0.8 * l4 + 0.2 * l8) / steps);
  hipMalloc(&p.mark, sizeof(uint64_t) * mark.size());
  hipMalloc(&p.carry, sizeof(uint64_t) * carry.size());
  hipMemcpy(p.mark, mark.data(), sizeof(uint64_t) * mark.size(), hipMemcpyHostToDevice);
  hipMemcpy(p.carry, carry.data(), sizeof(uint64_t) * carry.size(), hipMemcpyHostToDevice);
  p.steps = steps;
  return true;
}

int main(int argc, char** argv) {
  const char* anc_file = nullptr;
  bool pmc = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--pmc")) pmc = true;
    else anc_file = argv[i];
  }
  printf("N=%lld D=%d slots=%d\n", (long long)N, D, kSlots);
  {  // u4: the round-2 study's weights
    srand(1);
    std::vector<double> w(N);
    for (auto& v : w) { const double u = (rand() + 0.5) / (RAND_MAX + 1.0); v = u * u * u * u; }
    if (!make_pattern(g_pat[U4], "u4", systematic(w), 1)) return 1;
  }
  if (anc_file) {  // c2: the product's own parents
    FILE* f = fopen(anc_file, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", anc_file); return 1; }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    const int steps = (int)(sz / (long)(sizeof(int32_t) * N));
    if (steps < 1 || (long)steps * (long)(sizeof(int32_t) * N) != sz) {
      fprintf(stderr, "%s: not a whole number of steps of %lld int32 ancestors\n", anc_file, (long long)N);
      return 1;
    }
    std::vector<int32_t> anc((size_t)steps * N);
    const size_t got = fread(anc.data(), sizeof(int32_t), anc.size(), f);
    fclose(f);
    if (got != anc.size()) { fprintf(stderr, "%s: short read\n", anc_file); return 1; }
    printf("c2 ancestors from %s\n", anc_file);
    if (!make_pattern(g_pat[C2], "c2", anc, steps)) return 1;
  } else {
    std::mt19937_64 g(2);
    std::normal_distribution<double> z;
    std::vector<double> w(N);
    for (auto& v : w) v = exp(2.16 * z(g));
    printf("c2 ancestors synthetic (iid lognormal weights, sigma 2.16)\n");
    if (!make_pattern(g_pat[C2], "c2", systematic(w), 1)) return 1;
  }
  Args a{};
  hipMalloc(&a.anc, sizeof(int32_t) * N);
  hipMalloc(&a.logw, sizeof(double) * N);
  constexpr int64_t kMaxPad = 8192;
  g_slot_pitch = (int64_t)D * (N + kMaxPad) + (N / 32) * 256 + 4096;  // slots never alias, fixed pitch for every variant
  hipMalloc(&g_hist, sizeof(double) * g_slot_pitch * kSlots);
  hipMemset(g_hist, 0, sizeof(double) * g_slot_pitch * kSlots);
  const double bytes = (double)N * (16.0 * D + 8.0 + 8.0 + 4.0), cbytes = (double)N * (16.0 * D + 8.0);
  struct V {
    const char* name;
    double bytes;
    void (*f)(Args);
    std::vector<double> us;
  };
  std::vector<V> vs = {
      {"pair_64.c2", bytes, launch_lay<PAIR, C2>, {}},
      {"row.c2", bytes, launch_lay<ROW, C2>, {}},
      {"row_lds3.c2", bytes, launch_lay<ROW_LDS3, C2>, {}},
      {"row_lds5.c2", bytes, launch_lay<ROW_LDS5, C2>, {}},
      {"row_ldsh.c2", bytes, launch_lay<ROW_LDSH, C2>, {}},
      {"chunk_32.c2", bytes, launch_lay<CHUNK32, C2>, {}},
      {"pair_64.u4", bytes, launch_lay<PAIR, U4>, {}},
      {"row.u4", bytes, launch_lay<ROW, U4>, {}},
      {"row_lds3.u4", bytes, launch_lay<ROW_LDS3, U4>, {}},
      {"row_lds5.u4", bytes, launch_lay<ROW_LDS5, U4>, {}},
      {"row_ldsh.u4", bytes, launch_lay<ROW_LDSH, U4>, {}},
      {"chunk_32.u4", bytes, launch_lay<CHUNK32, U4>, {}},
      {"pair_64.id", cbytes, launch_lay<PAIR, ID>, {}},
      {"row.id", cbytes, launch_lay<ROW, ID>, {}},
      {"row_lds3.id", cbytes, launch_lay<ROW_LDS3, ID>, {}},
      {"row_lds5.id", cbytes, launch_lay<ROW_LDS5, ID>, {}},
      {"row_ldsh.id", cbytes, launch_lay<ROW_LDSH, ID>, {}},
      {"chunk_32.id", cbytes, launch_lay<CHUNK32, ID>, {}},
  };
  if (!pmc) {
    const V old[] = {
        {"soa_p0.u4", bytes, launch<0, 0, true, 0>, {}},
        {"soa_p512.u4", bytes, launch<0, 512, true, 0>, {}},
        {"tile_64.u4", bytes, launch<64, 0, true, 0>, {}},
        {"tile_256.u4", bytes, launch<256, 0, true, 0>, {}},
        {"tile_32.u4", bytes, launch<32, 0, true, 0>, {}},
        {"tile_128.u4", bytes, launch<128, 0, true, 0>, {}},
        {"copy_p0", cbytes, launch<0, 0, false, 0>, {}},
        {"copy_t256", cbytes, launch<256, 0, false, 0>, {}},
        {"copy_t64", cbytes, launch<64, 0, false, 0>, {}},
        {"rd_t64", (double)N * (8.0 * D + 8.0), launch<64, 0, false, 1>, {}},
        {"wr_t64", (double)N * (8.0 * D + 8.0), launch<64, 0, false, 2>, {}},
    };
    vs.insert(vs.end(), std::begin(old), std::end(old));
  }
  if (pmc) {
    for (auto& v : vs)
      for (int i = 0; i < 3; ++i) v.f(a);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
  }
  const int reps = 5;
  for (int rep = 0; rep < reps; ++rep)
    for (auto& v : vs) {
      for (int i = 0; i < 4; ++i) v.f(a);
      hipDeviceSynchronize();
      hipEvent_t e0, e1;
      hipEventCreate(&e0);
      hipEventCreate(&e1);
      const int it = 32;
      hipEventRecord(e0);
      for (int i = 0; i < it; ++i) v.f(a);
      hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "%s failed\n", v.name); return 1; }
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      hipEventDestroy(e0);
      hipEventDestroy(e1);
      v.us.push_back(ms * 1e3 / it);
    }
  // per variant: every repeat (interleaved across variants), then min / median / max
  printf("%-14s %s   %7s %7s %7s   %s\n", "variant", "us per launch, repeats 1..5", "min", "median", "max",
         "GB/s algorithmic at the median");
  for (auto& v : vs) {
    printf("%-14s", v.name);
    for (double u : v.us) printf(" %6.2f", u);
    std::vector<double> s = v.us;
    std::sort(s.begin(), s.end());
    printf("   %7.2f %7.2f %7.2f   %6.0f\n", s.front(), s[s.size() / 2], s.back(), v.bytes / (s[s.size() / 2] * 1e-6) / 1e9);
  }
  return 0;
}
