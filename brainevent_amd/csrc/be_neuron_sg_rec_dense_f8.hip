// be_neuron_sg_rec_dense_f8.hip — the fused recurrent spiking layer with a dense recurrence whose matrix is kept in
// OCP FP8 CODES, e4m3 or e5m2, with one f32 scale: step t's input is
//     xin[t][j] = x[t][j] + fl32( fl32( sum over the rows i with sp[i] of decode(codes[i, j]) ) * scale ),
// codes [N, N] row-major, rows = presynaptic neurons — Float8Dense's product contract with the inner sum EXACT.  Every finite e4m3
// value is a multiple of 2^-9 (|v| <= 448), every finite e5m2 value a multiple of 2^-16 (|v| <= 57344): a decoded weight times 2^9 /
// 2^16 is an integer, a column's sum over at most 8192 rows is an integer in that unit — known at compile time, so there is no
// exponent argument — and it is rounded to f32 once.  For e4m3 the sum fits 32 bits (8192 * 448 * 512 < 2^31), for e5m2 it takes 64.
// One workgroup of kF8Threads threads owns one sample for the whole launch.  The kernels are templated on the format (E4M3 / E5M2:
// how a code pair becomes two f32, v_cvt_pk_f32_fp8 / _bf8 — OCP on gfx950 —, the unit and the accumulator); the codes travel as raw
// uint8_t / uint32_t / uint4.  The neuron is be_sg_lane.h's; the time loops' scaffolding is be_neuron_sg_rec_dense_half.hip's,
// restated (that file keeps its kernels to itself).  The caller guarantees finite codes.
//
// Forwards (k_lif_rec_dense_f8_forward).  A thread owns ADJACENT COLUMN QUADS: thread tid has the neurons 4 * tid + h + k * kF8Span,
// h < 4, k < kF8Quads, state and integer sums in registers whose indices are compile-time constants.  One 4-byte load then brings
// the four weights of a quad, a wave reads 256 contiguous bytes of a row — 256 columns — and N <= 4096 needs ONE load per lane and
// active row.  The previous step's spikes are a bit mask in LDS, double-buffered, one barrier per step; it is not in neuron order:
// wave w's ballot of its neurons h of quad k is word 4 * (16 * k + w) + h, so
//     bit b of word q is row (q >> 2) * 256 + 4 * b + (q & 3)
// — scalar arithmetic in the wave-uniform walk.  The walk gathers kF8RowBatch row ids in two scalars, 16 bits each, and issues the
// loads of all of them before the first is used.  For N <= kF8GroupN the threads form G = 1024 / P row groups, P = the power of two
// >= max(N / 4, 64) threads: group g takes the active rows whose ordinal in the mask is g modulo G, the partial sums meet in an LDS
// array of N accumulators (ds_add_u32 / ds_add_u64).  The 4-byte loads need N % 4 == 0 and 4-byte aligned codes; otherwise the same
// thread loads the same four codes a byte at a time (the later ones only below N).  Integer sums: every such split gives the same bits.
//
// Backwards (k_lif_rec_dense_f8_backward).  g_rec[i] = fl32( (sum_j decode(codes[i, j]) * G[j]) * scale ), G = g_x[t+1] of the sample
// in LDS.  A 16-byte chunk holds 16 weights; lane l of a row's L lanes (a power of two chosen from N, up to a wave) takes the chunks
// l, l + L, ... and the four float4 of G that go with each.  G is stored SPLIT in LDS — one array per quarter of a chunk — so
// consecutive lanes read consecutive 16 bytes in each of the four reads (the half kernel's split, carried to four).  kF8Chunks
// chunks of kF8Rows rows are in flight, the weights are decoded in registers, every product is rounded on its own, one f32 partial
// sum per row runs in ascending j within a lane, then one butterfly, then * scale once per row: an order N alone fixes.  The 16-byte
// path needs N % 16 == 0 and 16-byte aligned codes; otherwise the same lanes load the same elements a byte at a time, in the same
// order.
//
// No global atomics, no spin waits, nothing between workgroups; every barrier sits in uniform control flow and every loop is bounded
// by T and N.
#include "be_sg_lane.h"
#include <cmath>

typedef float f8r_v2f __attribute__((ext_vector_type(2)));

namespace {

namespace lane = be_sg_lane;

constexpr int kF8Threads = 1024;
constexpr int kF8MaxN = 8192;
constexpr int kF8Span = 4 * kF8Threads;                // the columns one quad per thread covers
constexpr int kF8Quads = kF8MaxN / kF8Span;            // column quads a thread owns
constexpr int kF8PerThread = 4 * kF8Quads;             // its neurons: n = 4 * k + h is neuron 4 * tid + h + k * kF8Span
constexpr int kF8Waves = kF8Threads / kWave;
constexpr int kF8MaxWords = kF8MaxN / 64;
// at most this many neurons are served by row groups (their partial sums: one accumulator each in LDS)
constexpr int kF8GroupN = 2048;
// rows whose loads a thread issues before it uses the first (their ids: 16 bits each in two 64-bit scalars)
constexpr int kF8RowBatch = 8;
static_assert(kF8RowBatch <= 8, "two 64-bit scalars hold eight 16-bit row ids");
// backwards: rows and 16-byte chunks per row a lane has in flight, and the neurons a thread owns there (tid + k * kF8Threads)
constexpr int kF8Rows = 8, kF8Chunks = 1;
constexpr int kF8BackPerThread = kF8MaxN / kF8Threads;
// the neurons of a thread whose step inputs are loaded before the walk / the row product, not after it
constexpr int kF8EarlyFwd = 4;                         // (forwards: the first quad, every N <= 4096)
constexpr int kF8Early = 2;                            // (backwards: every N <= 2048)

// A format: two codes of a word -> two f32 (exactly), the unit 2^-kUnit every finite value is a multiple of, and the accumulator a
// column's sum of at most kF8MaxN values in that unit fits.
struct E4M3 {
  using acc_t = uint32_t;                                  // (wrapping; read back as int32_t)
  static constexpr int kUnit = 9;
  static_assert((long long)kF8MaxN * 448 * (1 << kUnit) < (1ll << 31), "an e4m3 column sum fits 32 bits");
  template <bool HI> __device__ static __forceinline__ f8r_v2f pair(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI); }
  __device__ static __forceinline__ acc_t units(float v) { return (uint32_t)(int)(v * 512.0f); }   // exact: |v * 512| <= 229376
  __device__ static __forceinline__ double value(acc_t r) { return (double)(int)r * 0x1p-9; }
};
struct E5M2 {
  using acc_t = unsigned long long;                        // (wrapping; read back as int64_t)
  static constexpr int kUnit = 16;
  static_assert((long long)kF8MaxN * 57344 * (1ll << kUnit) < (1ll << 53), "an e5m2 column sum is exact in f64");
  template <bool HI> __device__ static __forceinline__ f8r_v2f pair(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI); }
  // |v * 65536| <= 57344 * 65536 < 2^32: the magnitude is one v_cvt_u32_f32, the sign a 64-bit negation
  __device__ static __forceinline__ acc_t units(float v) {
    const float t = v * 65536.0f;
    const unsigned long long m = (unsigned long long)(uint32_t)fabsf(t);
    return t < 0.f ? 0ull - m : m;
  }
  __device__ static __forceinline__ double value(acc_t r) { return (double)(long long)r * 0x1p-16; }
};

__device__ __forceinline__ unsigned long long f8r_uniform64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// A new value at every step for the lane's index (no instruction): addresses derived from it are formed where they are used, a
// scalar base plus a 32-bit offset, not hoisted out of the time loop as a 64-bit register pair per array and owned neuron.
__device__ __forceinline__ uint32_t f8r_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the codes of columns j .. j + 3 of a row, the lowest byte first; j % 4 == 0.  QUAD: one load (N % 4 == 0, codes 4-byte aligned)
template <bool QUAD>
__device__ __forceinline__ uint32_t f8r_quad(const uint8_t* __restrict__ row, int N, int j) {
  if (QUAD) return *reinterpret_cast<const uint32_t*>(row + (uint32_t)j);
  uint32_t r = row[(uint32_t)j];                           // j < N: the column exists
#pragma unroll
  for (int h = 1; h < 4; ++h)
    if (j + h < N) r |= (uint32_t)row[(uint32_t)(j + h)] << (8 * h);   // (code 0: the weight 0, the integer 0)
  return r;
}

// the n <= kF8RowBatch rows whose ids sit in the low 16-bit fields of lo (then hi):
// acc[4 * k + h] += units(decode(codes[row, col + h + k * kF8Span]))
template <class FT, bool QUAD, int KQ>
__device__ __forceinline__ void f8r_add_rows(const uint8_t* __restrict__ codes, int N, int col, unsigned long long lo,
                                             unsigned long long hi, int n, typename FT::acc_t (&acc)[4 * KQ]) {
#pragma unroll
  for (int k = 0; k < KQ; ++k) {
    const int j = col + k * kF8Span;
    if (k * kF8Span < N && j < N) {
      uint32_t wv[kF8RowBatch];
#pragma unroll
      for (int q = 0; q < kF8RowBatch; ++q) {                  // in flight together
        const uint32_t row = (uint32_t)((q < 4 ? lo >> (16 * q) : hi >> (16 * (q - 4))) & 0xffffull);
        wv[q] = 0u;                                            // four codes +0: an absent row adds the integer 0
        if (q < n) wv[q] = f8r_quad<QUAD>(codes + (size_t)row * (size_t)N, N, j);   // a scalar row base + a 32-bit lane offset
      }
#pragma unroll
      for (int q = 0; q < kF8RowBatch; ++q) {
        const f8r_v2f a = FT::template pair<false>(wv[q]), b = FT::template pair<true>(wv[q]);
        acc[4 * k] += FT::units(a.x);
        acc[4 * k + 1] += FT::units(a.y);
        acc[4 * k + 2] += FT::units(b.x);
        acc[4 * k + 3] += FT::units(b.y);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                     // one quad's loads at a time: kF8RowBatch registers, not KQ times that
  }
}

// the rows the mask lists whose ordinal is g modulo G (G a power of two; G = 1: all of them), kF8RowBatch at a time.  Bit b of
// word q is row (q >> 2) * 256 + 4 * b + (q & 3): a wave's 256 neurons are four words, one per place in the quad.
template <class FT, bool QUAD, int KQ>
__device__ __forceinline__ void f8r_walk(const uint8_t* __restrict__ codes, int N, const unsigned long long* mask, int words, int col,
                                         uint32_t g, uint32_t G, typename FT::acc_t (&acc)[4 * KQ]) {
  unsigned long long lo = 0ull, hi = 0ull, m = 0ull;
  uint32_t ord = 0;
  int q = -1;
  for (;;) {                                             // one batch per turn: a single call site keeps the registers in bounds
    int n = 0;
    while (n < kF8RowBatch) {
      if (m == 0ull) {
        if (++q >= words) break;
        m = f8r_uniform64(mask[q]);
        continue;
      }
      const uint32_t row = (uint32_t)((q >> 2) * 256 + 4 * __builtin_ctzll(m) + (q & 3));
      m &= m - 1ull;
      if ((ord++ & (G - 1u)) != g) continue;
      hi = (hi << 16) | (lo >> 48);
      lo = (lo << 16) | row;
      ++n;
    }
    if (n == 0) break;
    f8r_add_rows<FT, QUAD, KQ>(codes, N, col, lo, hi, n, acc);
    if (n < kF8RowBatch) break;                          // the mask is exhausted
  }
}

template <class FT, int KQ>
__device__ __forceinline__ void f8r_walk(bool quad, const uint8_t* __restrict__ codes, int N, const unsigned long long* mask,
                                         int words, int col, uint32_t g, uint32_t G, typename FT::acc_t (&acc)[4 * KQ]) {
  if (quad) f8r_walk<FT, true, KQ>(codes, N, mask, words, col, g, G, acc);
  else f8r_walk<FT, false, KQ>(codes, N, mask, words, col, g, G, acc);
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N]; codes [N, N] bytes.  s0 / c0 / v0 /
// a0 NULL = 0; v_seq / h_save / th_save may be NULL.  Static LDS only: the two masks and the row groups' sums.
template <class FT, bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kF8Threads)
k_lif_rec_dense_f8_forward(const float* __restrict__ x, const uint8_t* __restrict__ codes, const float* __restrict__ s0,
                           const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ a0,
                           float* __restrict__ s_out, float* __restrict__ v_seq, float* __restrict__ h_save,
                           float* __restrict__ th_save, float* __restrict__ c_last, float* __restrict__ v_last,
                           float* __restrict__ a_last, int64_t T, int64_t B, int N, int quad, float w_scale, lane::LifP p) {
#pragma clang fp contract(off)
  using acc_t = typename FT::acc_t;
  __shared__ unsigned long long mask[2][kF8MaxWords];
  __shared__ acc_t part[kF8GroupN];
  const int tid = threadIdx.x, wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  const int words = 4 * ((N + 255) / 256);               // four per 256 neurons: a wave's neurons by their place in the quad
  // the row groups: P threads = 4 * P columns each (N <= kF8GroupN), or one group over all the columns
  int P = kF8Threads;
  if (N <= kF8GroupN) {
    P = kWave;
    while (4 * P < N) P <<= 1;
  }
  const uint32_t G = (uint32_t)(kF8Threads / P);
  const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane(tid / P);   // whole waves: P >= kWave
  float c[kF8PerThread], v[kF8PerThread], a[kF8PerThread];
  uint32_t sbits = 0;                                    // bit n: the thread's neuron n spiked at the previous step
#pragma unroll
  for (int n = 0; n < kF8PerThread; ++n) {
    const int i = 4 * tid + (n & 3) + (n >> 2) * kF8Span;
    c[n] = v[n] = a[n] = 0.f;
    if (i < N) {
      if (c0 != nullptr) c[n] = (c0 + base)[(uint32_t)i];
      if (v0 != nullptr) v[n] = (v0 + base)[(uint32_t)i];
      if (ADAPT && a0 != nullptr) a[n] = (a0 + base)[(uint32_t)i];
      if (s0 != nullptr && (s0 + base)[(uint32_t)i] != 0.f) sbits |= 1u << n;
    }
  }
  for (int i = tid; i < kF8GroupN; i += kF8Threads) part[i] = (acc_t)0;
  int cur = 0;
  for (int64_t t = 0; t < T; ++t) {
    const int64_t at = t * step + base;
    const int ft = (int)f8r_fresh((uint32_t)tid);
    // the previous step's spikes -> the mask: wave w's ballot of its neurons n = 4 * k + h is word 4 * (16 * k + w) + h (the other
    // buffer is still being read)
#pragma unroll
    for (int n = 0; n < kF8PerThread; ++n) {
      if ((n >> 2) * kF8Span < N) {
        const unsigned long long m = __ballot((sbits >> n) & 1u);
        const int word = 4 * (kF8Waves * (n >> 2) + wave) + (n & 3);
        if ((tid & (kWave - 1)) == 0 && word < words) mask[cur][word] = m;
      }
    }
    // x does not depend on the chain: that of a thread's first quad (every N <= 4096) is in flight during the walk, the rest is
    // loaded after it (the walk's sums and loads need the registers)
    float xv[kF8PerThread];
    auto load_x = [&](int n) {
      const int i = 4 * ft + (n & 3) + (n >> 2) * kF8Span;
      xv[n] = 0.f;
      if (i < N) xv[n] = (x + at)[(uint32_t)i];
    };
#pragma unroll
    for (int n = 0; n < kF8EarlyFwd; ++n) load_x(n);
    __syncthreads();
    acc_t R[kF8PerThread];
#pragma unroll
    for (int n = 0; n < kF8PerThread; ++n) R[n] = (acc_t)0;
    if (G == 1u) {
      f8r_walk<FT, kF8Quads>(quad != 0, codes, N, mask[cur], words, 4 * ft, 0u, 1u, R);
    } else {
      acc_t one[4] = {(acc_t)0, (acc_t)0, (acc_t)0, (acc_t)0};
      const int col = 4 * (ft & (P - 1));
      f8r_walk<FT, 1>(quad != 0, codes, N, mask[cur], words, col, g, G, one);
#pragma unroll
      for (int h = 0; h < 4; ++h)
        if (col + h < N && one[h] != (acc_t)0) atomicAdd(&part[col + h], one[h]);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        if (4 * tid + h < N) {
          R[h] = part[4 * tid + h];
          part[4 * tid + h] = (acc_t)0;                  // read and cleared by its owner only; the next adds come after a barrier
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = kF8EarlyFwd; n < kF8PerThread; ++n) load_x(n);
    cur ^= 1;
    sbits = 0;
#pragma unroll
    for (int n = 0; n < kF8PerThread; ++n) {
      const int i = 4 * ft + (n & 3) + (n >> 2) * kF8Span;
      if (i < N) {
        const float sum = (float)FT::value(R[n]);        // the exact sum, rounded once
        const float r = sum * w_scale;
        const lane::Fired f = lane::forward_step<HARD, true, ADAPT>(xv[n] + r, c[n], v[n], a[n], p.beta, p.v_th, p);
        if (f.s) sbits |= 1u << n;
        (s_out + at)[(uint32_t)i] = f.s ? 1.0f : 0.0f;
        if (v_seq != nullptr) (v_seq + at)[(uint32_t)i] = v[n];
        if (h_save != nullptr) {
          (h_save + at)[(uint32_t)i] = f.h;
          if (ADAPT) (th_save + at)[(uint32_t)i] = f.th;
        }
      }
      __builtin_amdgcn_sched_barrier(0);                 // one neuron's step at a time: interleaving eight costs registers
    }
  }
#pragma unroll
  for (int n = 0; n < kF8PerThread; ++n) {
    const int i = 4 * tid + (n & 3) + (n >> 2) * kF8Span;
    if (i < N) {
      (c_last + base)[(uint32_t)i] = c[n];
      (v_last + base)[(uint32_t)i] = v[n];
      if (ADAPT) (a_last + base)[(uint32_t)i] = a[n];
    }
  }
}

// the 16-byte chunk `chunk` of row `row`, 16 codes: one load (VEC: N % 16 == 0, codes 16-byte aligned), or its elements below N one
// by one (an absent one: code 0)
template <bool VEC>
__device__ __forceinline__ uint4 f8r_chunk(const uint8_t* __restrict__ codes, int N, int row, int chunk) {
  const uint8_t* at = codes + (size_t)row * (size_t)N + (size_t)chunk * 16u;
  if (VEC) return *reinterpret_cast<const uint4*>(at);
  const int j = chunk * 16;
  uint32_t e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (j + q < N) e[q >> 2] |= (uint32_t)at[q] << (8 * (q & 3));   // j < N: the chunk exists
  return make_uint4(e[0], e[1], e[2], e[3]);
}

// where G[i] lies in LDS: quarter (i >> 2) & 3 of every chunk of 16 in an array of its own (`chunks` float4 each)
__device__ __forceinline__ int f8r_g_index(int i, int chunks) { return ((i >> 2) & 3) * 4 * chunks + (i >> 4) * 4 + (i & 3); }

// s + the four rounded products of word w's codes with g, in ascending j; only the elements j + h < N (ALL: all four)
template <class FT, bool ALL>
__device__ __forceinline__ float f8r_dot4(float s, uint32_t w, const float4& g, int j, int N) {
#pragma clang fp contract(off)
  const f8r_v2f a = FT::template pair<false>(w), b = FT::template pair<true>(w);
  const float t0 = a.x * g.x, t1 = a.y * g.y, t2 = b.x * g.z, t3 = b.y * g.w;
  if (ALL) return (((s + t0) + t1) + t2) + t3;
  s = j < N ? s + t0 : s;
  s = j + 1 < N ? s + t1 : s;
  s = j + 2 < N ? s + t2 : s;
  s = j + 3 < N ? s + t3 : s;
  return s;
}

// out[i] = (sum_j decode(codes[i, j]) * G[j]) * w_scale for every row i < N, G split in LDS as f8r_g_index says (its tail up to a
// multiple of 16 is zero).  Lane `sub` of a row's L = 1 << lsh takes the chunks sub, sub + L, ... in order, every product rounded,
// then a butterfly over the L partial sums, then the scale: an order N alone fixes.  kF8Rows rows (kF8Threads / L apart) and
// kF8Chunks chunks of each are loaded before the first is used.
template <class FT, bool VEC>
__device__ __forceinline__ void f8r_rows(const uint8_t* __restrict__ codes, const float* G, int N, int lsh, float w_scale, float* out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, L = 1 << lsh, sub = tid & (L - 1), apart = kF8Threads >> lsh;
  const int chunks = (N + 15) >> 4;
  const float4* Gq = reinterpret_cast<const float4*>(G);
  for (int row0 = tid >> lsh; row0 < N; row0 += kF8Rows * apart) {       // a row's lanes share row0: they leave the loop together
    float sum[kF8Rows];
#pragma unroll
    for (int r = 0; r < kF8Rows; ++r) sum[r] = 0.f;
    for (int ch = sub; ch < chunks; ch += kF8Chunks * L) {
      uint4 wv[kF8Rows][kF8Chunks];
      float4 gq[kF8Chunks][4];
#pragma unroll
      for (int u = 0; u < kF8Chunks; ++u) {
        const int cu = ch + u * L;
        const bool in = cu < chunks;
#pragma unroll
        for (int quarter = 0; quarter < 4; ++quarter) gq[u][quarter] = Gq[quarter * chunks + (in ? cu : 0)];
#pragma unroll
        for (int r = 0; r < kF8Rows; ++r) {
          const int row = row0 + r * apart;
          wv[r][u] = make_uint4(0u, 0u, 0u, 0u);
          if (in && row < N) wv[r][u] = f8r_chunk<VEC>(codes, N, row, cu);
        }
      }
#pragma unroll
      for (int u = 0; u < kF8Chunks; ++u) {
        const int j = (ch + u * L) * 16;                                 // (past the row: j >= N, nothing is added)
#pragma unroll
        for (int r = 0; r < kF8Rows; ++r) {
          const uint4 q = wv[r][u];
          float s = sum[r];
          if (VEC) {                                                     // N % 16 == 0: a chunk lies below N whole or not at all
            float f = f8r_dot4<FT, true>(s, q.x, gq[u][0], j, N);
            f = f8r_dot4<FT, true>(f, q.y, gq[u][1], j + 4, N);
            f = f8r_dot4<FT, true>(f, q.z, gq[u][2], j + 8, N);
            f = f8r_dot4<FT, true>(f, q.w, gq[u][3], j + 12, N);
            sum[r] = j < N ? f : s;
            continue;
          }
          s = f8r_dot4<FT, false>(s, q.x, gq[u][0], j, N);
          s = f8r_dot4<FT, false>(s, q.y, gq[u][1], j + 4, N);
          s = f8r_dot4<FT, false>(s, q.z, gq[u][2], j + 8, N);
          s = f8r_dot4<FT, false>(s, q.w, gq[u][3], j + 12, N);
          sum[r] = s;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kF8Rows; ++r) {
      float s = sum[r];
      for (int off = L >> 1; off > 0; off >>= 1) s = s + __shfl_xor(s, off);   // within the row's aligned group of L lanes
      const int row = row0 + r * apart;
      if (sub == 0 && row < N) out[row] = s * w_scale;
    }
  }
}

template <class FT>
__device__ __forceinline__ void f8r_rows(bool vec, const uint8_t* __restrict__ codes, const float* G, int N, int lsh, float w_scale,
                                         float* out) {
  if (vec) f8r_rows<FT, true>(codes, G, N, lsh, w_scale, out);
  else f8r_rows<FT, false>(codes, G, N, lsh, w_scale, out);
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; the others [B, N]; codes [N, N] bytes.  g_s / g_vseq / g_clast /
// g_vlast / g_alast NULL = 0; g_c0 / g_v0 / g_a0 / g_s0 may be NULL.  Dynamic LDS: g_x[t+1] of the sample (N floats rounded up to a
// multiple of 16, the tail zero, split as f8r_g_index says), then g_rec (N floats).  Thread tid owns neurons tid + k * kF8Threads.
template <class FT, bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kF8Threads)
k_lif_rec_dense_f8_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const uint8_t* __restrict__ codes,
                            const float* __restrict__ g_s, const float* __restrict__ g_vseq, const float* __restrict__ g_clast,
                            const float* __restrict__ g_vlast, const float* __restrict__ g_alast, float* __restrict__ g_x,
                            float* __restrict__ g_c0, float* __restrict__ g_v0, float* __restrict__ g_a0, float* __restrict__ g_s0,
                            int64_t T, int64_t B, int N, int vec, int detach_reset, float w_scale, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* G = reinterpret_cast<float*>(smem_raw);
  const int chunks = (N + 15) >> 4, padded = 16 * chunks;
  float* grec = G + padded;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  // lanes per row: the power of two that leaves a lane at most kF8Chunks chunks, up to a wave
  int lsh = 0;
  while ((1 << lsh) < kWave && (kF8Chunks << lsh) < chunks) ++lsh;
  if (tid < padded - N) G[f8r_g_index(N + tid, chunks)] = 0.f;           // written once: the steps write G of i < N only
  float cc[kF8BackPerThread], cv[kF8BackPerThread], ca[kF8BackPerThread];
#pragma unroll
  for (int k = 0; k < kF8BackPerThread; ++k) {
    const int i = tid + k * kF8Threads;
    cc[k] = cv[k] = ca[k] = 0.f;
    if (i < N) {
      if (g_clast != nullptr) cc[k] = (g_clast + base)[(uint32_t)i];
      if (g_vlast != nullptr) cv[k] = (g_vlast + base)[(uint32_t)i];
      if (ADAPT && g_alast != nullptr) ca[k] = (g_alast + base)[(uint32_t)i];
    }
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t at = t * step + base;
    const int ft = (int)f8r_fresh((uint32_t)tid);
    const bool rec = t < T - 1;
    // the step's inputs: those of a thread's first kF8Early neurons (every N <= 2048) are in flight during the row product, the
    // others are loaded after it (32 more registers across the product would not fit beside its loads)
    float hv[kF8BackPerThread], tv[kF8BackPerThread], gsv[kF8BackPerThread], gvv[kF8BackPerThread];
    auto load_inputs = [&](int k) {
      const int i = ft + k * kF8Threads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = (h_save + at)[(uint32_t)i];
        if (ADAPT) tv[k] = (th_save + at)[(uint32_t)i];
        if (g_s != nullptr) gsv[k] = (g_s + at)[(uint32_t)i];
        if (g_vseq != nullptr) gvv[k] = (g_vseq + at)[(uint32_t)i];
      }
    };
#pragma unroll
    for (int k = 0; k < kF8Early; ++k) load_inputs(k);
    if (rec) {
      f8r_rows<FT>(vec != 0, codes, G, N, lsh, w_scale, grec);
      __syncthreads();
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = kF8Early; k < kF8BackPerThread; ++k) load_inputs(k);
#pragma unroll
    for (int k = 0; k < kF8BackPerThread; ++k) {
      const int i = ft + k * kF8Threads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const float th = ADAPT ? tv[k] : p.v_th;         // the threshold h was compared with
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        (g_x + at)[(uint32_t)i] = g_c;
        G[f8r_g_index(i, chunks)] = g_c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kF8BackPerThread; ++k) {
    const int i = tid + k * kF8Threads;
    if (i < N) {
      if (g_c0 != nullptr) (g_c0 + base)[(uint32_t)i] = cc[k];
      if (g_v0 != nullptr) (g_v0 + base)[(uint32_t)i] = cv[k];
      if (ADAPT && g_a0 != nullptr) (g_a0 + base)[(uint32_t)i] = ca[k];
    }
  }
  if (g_s0 != nullptr) f8r_rows<FT>(vec != 0, codes, G, N, lsh, w_scale, g_s0 + base);    // from g_x[0]
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int f8r_check_common(const char* who, int64_t T, int64_t B, int64_t N, int reset_mode, int fmt_code, double w_scale) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : (fmt_code != BE_F8_E4M3 && fmt_code != BE_F8_E5M2)                   ? ": fmt_code must be BE_F8_E4M3 or BE_F8_E5M2"
                    : !std::isfinite((float)w_scale)                                       ? ": w_scale must be a finite f32"
                                                                                           : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kF8MaxN || B > 0x7fffffffll) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons (limit: " + std::to_string(kF8MaxN) +
                 ", one workgroup holds a sample's neurons in its registers), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

// E4M3 or E5M2 as a tag (fmt_code was checked)
template <typename F>
inline int f8r_dispatch_format(int fmt_code, F&& f) {
  return fmt_code == BE_F8_E4M3 ? f(be_type_tag<E4M3>{}) : f(be_type_tag<E5M2>{});
}

}  // namespace

extern "C" {

int be_lif_rec_dense_f8_sg_forward(const float* x, const void* codes, int fmt_code, double w_scale, const float* s0, const float* c0,
                                   const float* v0, const float* a0, float* s_out, float* v_seq, float* h_save, float* th_save,
                                   float* c_last, float* v_last, float* a_last, int64_t T, int64_t B, int64_t N, double syn_decay,
                                   double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode, int adaptive,
                                   be_stream_t stream) {
  if (const int rc = f8r_check_common(__func__, T, B, N, reset_mode, fmt_code, w_scale)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(codes, BE_ERR_INVALID, "null pointer (codes is required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const int quad = N % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0;
  const uint8_t* cp = static_cast<const uint8_t*>(codes);
  const float scale = (float)w_scale;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  f8r_dispatch_format(fmt_code, [&](auto S) {
    using FT = typename decltype(S)::type;
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        hipLaunchKernelGGL((k_lif_rec_dense_f8_forward<FT, decltype(H)::value, decltype(A)::value>), dim3((unsigned)B),
                           dim3(kF8Threads), 0, st, x, cp, s0, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, B,
                           (int)N, quad, scale, p);
        return BE_OK;
      });
    });
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_dense_f8_sg_backward(const float* h_save, const float* th_save, const void* codes, int fmt_code, double w_scale,
                                    const float* g_s, const float* g_vseq, const float* g_clast, const float* g_vlast,
                                    const float* g_alast, float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0, int64_t T,
                                    int64_t B, int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho,
                                    double kappa, int reset_mode, int surrogate, double alpha, int adaptive, int detach_reset,
                                    be_stream_t stream) {
  if (const int rc = f8r_check_common(__func__, T, B, N, reset_mode, fmt_code, w_scale)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(codes, BE_ERR_INVALID, "null pointer (codes is required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int vec = N % 16 == 0 && reinterpret_cast<uintptr_t>(codes) % 16 == 0;
  const int lds = (int)be_align_up((be_align_up(N, 16) + N) * 4, 16);
  const int detach = (int)(detach_reset != 0);
  const uint8_t* cp = static_cast<const uint8_t*>(codes);
  const float scale = (float)w_scale;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  f8r_dispatch_format(fmt_code, [&](auto S) {
    using FT = typename decltype(S)::type;
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
          auto kern = k_lif_rec_dense_f8_backward<FT, decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
          allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
          if (allowed == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kF8Threads), lds, st, h_save, th_save, cp, g_s, g_vseq, g_clast, g_vlast,
                               g_alast, g_x, g_c0, g_v0, g_a0, g_s0, T, B, (int)N, vec, detach, scale, p);
          return BE_OK;
        });
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
