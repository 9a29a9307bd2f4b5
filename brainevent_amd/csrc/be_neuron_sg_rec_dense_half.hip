// be_neuron_sg_rec_dense_half.hip — the fused recurrent spiking layer with a dense recurrence whose matrix is kept
// in TWO-BYTE weights, f16 or bf16: step t's input is x[t] + s[t-1] @ W, W [N, N] row-major, rows = presynaptic
// neurons.  The layer is the f32 layer on the up-converted matrix: every weight becomes an f32 exactly (f16: v_cvt_f32_f16, bf16: a
// 16-bit shift), the recurrent sums are the 64-bit integers of fixed_from_f32 at the given exponent, scaled back in f64 and rounded
// once — so the forward outputs are those of be_lif_rec_dense_sg_forward on float(W), bit for bit, however the work is split.
// One workgroup of kHalfThreads threads owns one sample for the whole launch.  The kernels are templated on the storage (F16 / BF16:
// how 16 bits become an f32); the weights travel as raw uint16_t / uint32_t / uint4.  The neuron is be_sg_lane.h's; the time loops'
// scaffolding is be_neuron_sg_rec_dense.hip's, restated (that file keeps its kernels to itself).
//
// Forwards (k_lif_rec_dense_half_forward).  A thread owns ADJACENT COLUMN PAIRS: thread tid has the neurons 2 * tid + h + k *
// kHalfSpan, h < 2, k < kHalfPairs, state and int64 sums in registers whose indices are compile-time constants.  One 4-byte load
// then brings both weights of a pair, a wave reads 256 contiguous bytes of a row — 128 columns, where the f32 kernel's 256 bytes are
// 64 — and N <= 2048 needs ONE load per lane and active row.  The previous step's spikes are a bit mask in LDS, double-buffered,
// one barrier per step; it is not in neuron order: wave w's ballot of its EVEN neurons of pair k is word 2 * (16 * k + w), that of
// its ODD neurons word 2 * (16 * k + w) + 1, so bit b of word q is row (q >> 1) * 128 + 2 * b + (q & 1) — scalar arithmetic in the
// wave-uniform walk.  The walk gathers kHalfRowBatch row ids in two scalars, 16 bits each, and issues the loads of all of them
// before the first is used.  For N <= kHalfGroupN the threads form G = 1024 / P row groups, P = the power of two >= max(N / 2, 64)
// threads: group g takes the active rows whose ordinal in the mask is g modulo G, the partial sums meet in an N x 8-byte LDS array
// (ds_add_u64).  The 4-byte loads need an even N and a 4-byte aligned W; otherwise the same thread loads the same two weights
// 2 bytes at a time (the second only below N).  Integer sums: every such split gives the same bits.
//
// Backwards (k_lif_rec_dense_half_backward).  g_rec[i] = sum_j float(W[i, j]) * G[j], G = g_x[t+1] of the sample in LDS.  A 16-byte
// chunk holds 8 weights; lane l of a row's L lanes (a power of two chosen from N, up to a wave) takes the chunks l, l + L, ... and
// the two float4 of G that go with each.  G is stored SPLIT in LDS — the first float4 of every chunk in one array, the second in
// another — so consecutive lanes read consecutive 16 bytes in each of the two reads (the conflict-free pattern of the f32 kernel;
// reading 16 of every 32 bytes would not be).  kHalfChunks chunks of kHalfRows rows are in flight, the weights are up-converted in
// registers, every product is rounded on its own, one f32 partial sum per row runs in ascending j within a lane, then one butterfly:
// an order N alone fixes.  The 16-byte path needs N % 8 == 0 and a 16-byte aligned W; otherwise the same lanes load the same
// elements 2 bytes at a time, in the same order.
//
// No global atomics, no spin waits, nothing between workgroups; every barrier sits in uniform control flow and every loop is bounded
// by T and N.
#include "be_sg_lane.h"

namespace {

namespace lane = be_sg_lane;

constexpr int kHalfThreads = 1024;
constexpr int kHalfMaxN = 8192;
constexpr int kHalfSpan = 2 * kHalfThreads;              // the columns one pair per thread covers
constexpr int kHalfPairs = kHalfMaxN / kHalfSpan;        // column pairs a thread owns
constexpr int kHalfPerThread = 2 * kHalfPairs;           // its neurons: n = 2 * k + h is neuron 2 * tid + h + k * kHalfSpan
constexpr int kHalfWaves = kHalfThreads / kWave;
constexpr int kHalfMaxWords = kHalfMaxN / 64;
// at most this many neurons are served by row groups (their partial sums: kHalfGroupN * 8 bytes of LDS)
constexpr int kHalfGroupN = 1024;
// rows whose loads a thread issues before it uses the first (their ids: 16 bits each in two 64-bit scalars)
constexpr int kHalfRowBatch = 8;
static_assert(kHalfRowBatch <= 8, "two 64-bit scalars hold eight 16-bit row ids");
// backwards: rows and 16-byte chunks per row a lane has in flight, and the neurons a thread owns there (tid + k * kHalfThreads)
constexpr int kHalfRows = 4, kHalfChunks = 2;
constexpr int kHalfBackPerThread = kHalfMaxN / kHalfThreads;
// the neurons of a thread whose step inputs are loaded before the walk / the row product, not after it (every N <= 2048)
constexpr int kHalfEarly = 2;
// the exponents be_fixed_point_exponent returns (2^(e - 32) must be a normal f32)
constexpr int kHalfMinExp = -90, kHalfMaxExp = 150;

// how the low 16 bits of a register become an f32, exactly
struct F16 {
  __device__ static __forceinline__ float up(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
};
struct BF16 {
  __device__ static __forceinline__ float up(uint32_t bits) { return __uint_as_float(bits << 16); }
};

__device__ __forceinline__ unsigned long long half_uniform64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// A new value at every step for the lane's index (no instruction): addresses derived from it are formed where they are used, a
// scalar base plus a 32-bit offset, not hoisted out of the time loop as a 64-bit register pair per array and owned neuron.
__device__ __forceinline__ uint32_t half_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the weights of columns j (low half) and j + 1 (high half) of a row; j is even.  PAIR: one load (N even, w 4-byte aligned)
template <bool PAIR>
__device__ __forceinline__ uint32_t half_pair(const uint16_t* __restrict__ row, int N, int j) {
  if (PAIR) return *reinterpret_cast<const uint32_t*>(row + (uint32_t)j);
  uint32_t r = row[(uint32_t)j];                           // j < N: the column exists
  if (j + 1 < N) r |= (uint32_t)row[(uint32_t)j + 1u] << 16;   // (bits 0: the weight 0, the integer 0)
  return r;
}

// the n <= kHalfRowBatch rows whose ids sit in the low 16-bit fields of lo (then hi):
// acc[2 * k + h] += fixed(float(W[row, col + h + k * kHalfSpan]))
template <class ST, bool PAIR, int KP>
__device__ __forceinline__ void half_add_rows(const uint16_t* __restrict__ w, int N, int col, unsigned long long lo,
                                              unsigned long long hi, int n, float scale, unsigned long long (&acc)[2 * KP]) {
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int j = col + k * kHalfSpan;
    if (k * kHalfSpan < N && j < N) {
      uint32_t wv[kHalfRowBatch];
#pragma unroll
      for (int q = 0; q < kHalfRowBatch; ++q) {                // in flight together
        const uint32_t row = (uint32_t)((q < 4 ? lo >> (16 * q) : hi >> (16 * (q - 4))) & 0xffffull);
        wv[q] = 0u;                                            // fixed(0) = 0: an absent row adds the integer 0
        if (q < n) wv[q] = half_pair<PAIR>(w + (size_t)row * (size_t)N, N, j);   // a scalar row base + a 32-bit lane offset
      }
#pragma unroll
      for (int q = 0; q < kHalfRowBatch; ++q) {
        acc[2 * k] += fixed_from_f32(ST::up(wv[q] & 0xffffu), scale);
        acc[2 * k + 1] += fixed_from_f32(ST::up(wv[q] >> 16), scale);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                     // one pair's loads at a time: kHalfRowBatch registers, not KP times that
  }
}

// the rows the mask lists whose ordinal is g modulo G (G a power of two; G = 1: all of them), kHalfRowBatch at a time.  Bit b of
// word q is row (q >> 1) * 128 + 2 * b + (q & 1): the even and the odd neurons of a wave's 128 are a word each.
template <class ST, bool PAIR, int KP>
__device__ __forceinline__ void half_walk(const uint16_t* __restrict__ w, int N, const unsigned long long* mask, int words, int col,
                                          uint32_t g, uint32_t G, float scale, unsigned long long (&acc)[2 * KP]) {
  unsigned long long lo = 0ull, hi = 0ull, m = 0ull;
  uint32_t ord = 0;
  int q = -1;
  for (;;) {                                             // one batch per turn: a single call site keeps the registers in bounds
    int n = 0;
    while (n < kHalfRowBatch) {
      if (m == 0ull) {
        if (++q >= words) break;
        m = half_uniform64(mask[q]);
        continue;
      }
      const uint32_t row = (uint32_t)((q >> 1) * 128 + 2 * __builtin_ctzll(m) + (q & 1));
      m &= m - 1ull;
      if ((ord++ & (G - 1u)) != g) continue;
      hi = (hi << 16) | (lo >> 48);
      lo = (lo << 16) | row;
      ++n;
    }
    if (n == 0) break;
    half_add_rows<ST, PAIR, KP>(w, N, col, lo, hi, n, scale, acc);
    if (n < kHalfRowBatch) break;                        // the mask is exhausted
  }
}

template <class ST, int KP>
__device__ __forceinline__ void half_walk(bool pair, const uint16_t* __restrict__ w, int N, const unsigned long long* mask, int words,
                                          int col, uint32_t g, uint32_t G, float scale, unsigned long long (&acc)[2 * KP]) {
  if (pair) half_walk<ST, true, KP>(w, N, mask, words, col, g, G, scale, acc);
  else half_walk<ST, false, KP>(w, N, mask, words, col, g, G, scale, acc);
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N]; w [N, N] of 2-byte weights.  s0 /
// c0 / v0 / a0 NULL = 0; v_seq / h_save / th_save may be NULL.  Static LDS only: the two masks and the row groups' sums.
template <class ST, bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kHalfThreads)
k_lif_rec_dense_half_forward(const float* __restrict__ x, const uint16_t* __restrict__ w, const float* __restrict__ s0,
                             const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ a0,
                             float* __restrict__ s_out, float* __restrict__ v_seq, float* __restrict__ h_save,
                             float* __restrict__ th_save, float* __restrict__ c_last, float* __restrict__ v_last,
                             float* __restrict__ a_last, int64_t T, int64_t B, int N, int pair, float scale, double inv, lane::LifP p) {
#pragma clang fp contract(off)
  __shared__ unsigned long long mask[2][kHalfMaxWords];
  __shared__ unsigned long long part[kHalfGroupN];
  const int tid = threadIdx.x, wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  const int words = 2 * ((N + 127) / 128);               // two per 128 neurons: a wave's even and odd ones
  // the row groups: P threads = 2 * P columns each (N <= kHalfGroupN), or one group over all the columns
  int P = kHalfThreads;
  if (N <= kHalfGroupN) {
    P = kWave;
    while (2 * P < N) P <<= 1;
  }
  const uint32_t G = (uint32_t)(kHalfThreads / P);
  const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane(tid / P);   // whole waves: P >= kWave
  float c[kHalfPerThread], v[kHalfPerThread], a[kHalfPerThread];
  uint32_t sbits = 0;                                    // bit n: the thread's neuron n spiked at the previous step
#pragma unroll
  for (int n = 0; n < kHalfPerThread; ++n) {
    const int i = 2 * tid + (n & 1) + (n >> 1) * kHalfSpan;
    c[n] = v[n] = a[n] = 0.f;
    if (i < N) {
      if (c0 != nullptr) c[n] = (c0 + base)[(uint32_t)i];
      if (v0 != nullptr) v[n] = (v0 + base)[(uint32_t)i];
      if (ADAPT && a0 != nullptr) a[n] = (a0 + base)[(uint32_t)i];
      if (s0 != nullptr && (s0 + base)[(uint32_t)i] != 0.f) sbits |= 1u << n;
    }
  }
  if (tid < kHalfGroupN) part[tid] = 0ull;
  int cur = 0;
  for (int64_t t = 0; t < T; ++t) {
    const int64_t at = t * step + base;
    const int ft = (int)half_fresh((uint32_t)tid);
    // the previous step's spikes -> the mask: wave w's ballot of its neurons n = 2 * k + h is word 2 * (16 * k + w) + h (the other
    // buffer is still being read)
#pragma unroll
    for (int n = 0; n < kHalfPerThread; ++n) {
      if ((n >> 1) * kHalfSpan < N) {
        const unsigned long long m = __ballot((sbits >> n) & 1u);
        const int word = 2 * (kHalfWaves * (n >> 1) + wave) + (n & 1);
        if ((tid & (kWave - 1)) == 0 && word < words) mask[cur][word] = m;
      }
    }
    // x does not depend on the chain: that of a thread's first kHalfEarly neurons (every N <= 2048) is in flight during the walk,
    // the rest is loaded after it (the walk's sums and loads need the registers)
    float xv[kHalfPerThread];
    auto load_x = [&](int n) {
      const int i = 2 * ft + (n & 1) + (n >> 1) * kHalfSpan;
      xv[n] = 0.f;
      if (i < N) xv[n] = (x + at)[(uint32_t)i];
    };
#pragma unroll
    for (int n = 0; n < kHalfEarly; ++n) load_x(n);
    __syncthreads();
    unsigned long long R[kHalfPerThread];
#pragma unroll
    for (int n = 0; n < kHalfPerThread; ++n) R[n] = 0ull;
    if (G == 1u) {
      half_walk<ST, kHalfPairs>(pair != 0, w, N, mask[cur], words, 2 * ft, 0u, 1u, scale, R);
    } else {
      unsigned long long one[2] = {0ull, 0ull};
      const int col = 2 * (ft & (P - 1));
      half_walk<ST, 1>(pair != 0, w, N, mask[cur], words, col, g, G, scale, one);
      if (col < N && one[0] != 0ull) atomicAdd(&part[col], one[0]);
      if (col + 1 < N && one[1] != 0ull) atomicAdd(&part[col + 1], one[1]);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (2 * tid + h < N) {
          R[h] = part[2 * tid + h];
          part[2 * tid + h] = 0ull;                      // read and cleared by its owner only; the next adds come after a barrier
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = kHalfEarly; n < kHalfPerThread; ++n) load_x(n);
    cur ^= 1;
    sbits = 0;
#pragma unroll
    for (int n = 0; n < kHalfPerThread; ++n) {
      const int i = 2 * ft + (n & 1) + (n >> 1) * kHalfSpan;
      if (i < N) {
        const float r = (float)((double)(long long)R[n] * inv);
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
  for (int n = 0; n < kHalfPerThread; ++n) {
    const int i = 2 * tid + (n & 1) + (n >> 1) * kHalfSpan;
    if (i < N) {
      (c_last + base)[(uint32_t)i] = c[n];
      (v_last + base)[(uint32_t)i] = v[n];
      if (ADAPT) (a_last + base)[(uint32_t)i] = a[n];
    }
  }
}

// the 16-byte chunk `chunk` of row `row`, 8 weights: one load (VEC: N % 8 == 0, w 16-byte aligned), or its elements below N one by
// one (an absent one: bits 0)
template <bool VEC>
__device__ __forceinline__ uint4 half_chunk(const uint16_t* __restrict__ w, int N, int row, int chunk) {
  const uint16_t* at = w + (size_t)row * (size_t)N + (size_t)chunk * 8u;
  if (VEC) return *reinterpret_cast<const uint4*>(at);
  const int j = chunk * 8;
  uint32_t e[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) e[q] = j + q < N ? (uint32_t)at[q] : 0u;   // j < N: the chunk exists
  return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// where G[i] lies in LDS: the first four columns of every chunk of 8 in one array (`chunks` float4), the last four in a second
__device__ __forceinline__ int half_g_index(int i, int chunks) { return ((i >> 2) & 1) * 4 * chunks + (i >> 3) * 4 + (i & 3); }

// out[i] = sum_j float(W[i, j]) * G[j] for every row i < N, G split in LDS as half_g_index says (its tail up to a multiple of 8 is
// zero).  Lane `sub` of a row's L = 1 << lsh takes the chunks sub, sub + L, ... in order, every product rounded, then a butterfly
// over the L partial sums: an order N alone fixes.  kHalfRows rows (kHalfThreads / L apart) and kHalfChunks chunks of each are
// loaded before the first is used.
template <class ST, bool VEC>
__device__ __forceinline__ void half_rows(const uint16_t* __restrict__ w, const float* G, int N, int lsh, float* out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, L = 1 << lsh, sub = tid & (L - 1), apart = kHalfThreads >> lsh;
  const int chunks = (N + 7) >> 3;
  const float4* Ga = reinterpret_cast<const float4*>(G);
  const float4* Gb = Ga + chunks;
  for (int row0 = tid >> lsh; row0 < N; row0 += kHalfRows * apart) {     // a row's lanes share row0: they leave the loop together
    float sum[kHalfRows];
#pragma unroll
    for (int r = 0; r < kHalfRows; ++r) sum[r] = 0.f;
    for (int ch = sub; ch < chunks; ch += kHalfChunks * L) {
      uint4 wv[kHalfRows][kHalfChunks];
      float4 ga[kHalfChunks], gb[kHalfChunks];
#pragma unroll
      for (int u = 0; u < kHalfChunks; ++u) {
        const int cu = ch + u * L;
        const bool in = cu < chunks;
        ga[u] = Ga[in ? cu : 0];
        gb[u] = Gb[in ? cu : 0];
#pragma unroll
        for (int r = 0; r < kHalfRows; ++r) {
          const int row = row0 + r * apart;
          wv[r][u] = make_uint4(0u, 0u, 0u, 0u);
          if (in && row < N) wv[r][u] = half_chunk<VEC>(w, N, row, cu);
        }
      }
#pragma unroll
      for (int u = 0; u < kHalfChunks; ++u) {
        const int j = (ch + u * L) * 8;                                  // (past the row: j >= N, nothing is added)
#pragma unroll
        for (int r = 0; r < kHalfRows; ++r) {
          const uint4 q = wv[r][u];
          const float t0 = ST::up(q.x & 0xffffu) * ga[u].x, t1 = ST::up(q.x >> 16) * ga[u].y;
          const float t2 = ST::up(q.y & 0xffffu) * ga[u].z, t3 = ST::up(q.y >> 16) * ga[u].w;
          const float t4 = ST::up(q.z & 0xffffu) * gb[u].x, t5 = ST::up(q.z >> 16) * gb[u].y;
          const float t6 = ST::up(q.w & 0xffffu) * gb[u].z, t7 = ST::up(q.w >> 16) * gb[u].w;
          float s = sum[r];
          if (VEC) {                                                     // N % 8 == 0: a chunk lies below N whole or not at all
            sum[r] = j < N ? (((((((s + t0) + t1) + t2) + t3) + t4) + t5) + t6) + t7 : s;
            continue;
          }
          s = j < N ? s + t0 : s;
          s = j + 1 < N ? s + t1 : s;
          s = j + 2 < N ? s + t2 : s;
          s = j + 3 < N ? s + t3 : s;
          s = j + 4 < N ? s + t4 : s;
          s = j + 5 < N ? s + t5 : s;
          s = j + 6 < N ? s + t6 : s;
          s = j + 7 < N ? s + t7 : s;
          sum[r] = s;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kHalfRows; ++r) {
      float s = sum[r];
      for (int off = L >> 1; off > 0; off >>= 1) s = s + __shfl_xor(s, off);   // within the row's aligned group of L lanes
      const int row = row0 + r * apart;
      if (sub == 0 && row < N) out[row] = s;
    }
  }
}

template <class ST>
__device__ __forceinline__ void half_rows(bool vec, const uint16_t* __restrict__ w, const float* G, int N, int lsh, float* out) {
  if (vec) half_rows<ST, true>(w, G, N, lsh, out);
  else half_rows<ST, false>(w, G, N, lsh, out);
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; the others [B, N]; w [N, N] of 2-byte weights.  g_s / g_vseq / g_clast
// / g_vlast / g_alast NULL = 0; g_c0 / g_v0 / g_a0 / g_s0 may be NULL.  Dynamic LDS: g_x[t+1] of the sample (N floats rounded up to
// a multiple of 8, the tail zero, split as half_g_index says), then g_rec (N floats).  Thread tid owns neurons tid + k * kHalfThreads.
template <class ST, bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kHalfThreads)
k_lif_rec_dense_half_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const uint16_t* __restrict__ w,
                              const float* __restrict__ g_s, const float* __restrict__ g_vseq, const float* __restrict__ g_clast,
                              const float* __restrict__ g_vlast, const float* __restrict__ g_alast, float* __restrict__ g_x,
                              float* __restrict__ g_c0, float* __restrict__ g_v0, float* __restrict__ g_a0, float* __restrict__ g_s0,
                              int64_t T, int64_t B, int N, int vec, int detach_reset, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* G = reinterpret_cast<float*>(smem_raw);
  const int chunks = (N + 7) >> 3, padded = 8 * chunks;
  float* grec = G + padded;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  // lanes per row: the power of two that leaves a lane at most kHalfChunks chunks, up to a wave
  int lsh = 0;
  while ((1 << lsh) < kWave && (kHalfChunks << lsh) < chunks) ++lsh;
  if (tid < padded - N) G[half_g_index(N + tid, chunks)] = 0.f;          // written once: the steps write G of i < N only
  float cc[kHalfBackPerThread], cv[kHalfBackPerThread], ca[kHalfBackPerThread];
#pragma unroll
  for (int k = 0; k < kHalfBackPerThread; ++k) {
    const int i = tid + k * kHalfThreads;
    cc[k] = cv[k] = ca[k] = 0.f;
    if (i < N) {
      if (g_clast != nullptr) cc[k] = (g_clast + base)[(uint32_t)i];
      if (g_vlast != nullptr) cv[k] = (g_vlast + base)[(uint32_t)i];
      if (ADAPT && g_alast != nullptr) ca[k] = (g_alast + base)[(uint32_t)i];
    }
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t at = t * step + base;
    const int ft = (int)half_fresh((uint32_t)tid);
    const bool rec = t < T - 1;
    // the step's inputs: those of a thread's first kHalfEarly neurons (every N <= 2048) are in flight during the row product, the
    // others are loaded after it (32 more registers across the product would not fit beside its loads)
    float hv[kHalfBackPerThread], tv[kHalfBackPerThread], gsv[kHalfBackPerThread], gvv[kHalfBackPerThread];
    auto load_inputs = [&](int k) {
      const int i = ft + k * kHalfThreads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = (h_save + at)[(uint32_t)i];
        if (ADAPT) tv[k] = (th_save + at)[(uint32_t)i];
        if (g_s != nullptr) gsv[k] = (g_s + at)[(uint32_t)i];
        if (g_vseq != nullptr) gvv[k] = (g_vseq + at)[(uint32_t)i];
      }
    };
#pragma unroll
    for (int k = 0; k < kHalfEarly; ++k) load_inputs(k);
    if (rec) {
      half_rows<ST>(vec != 0, w, G, N, lsh, grec);
      __syncthreads();
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = kHalfEarly; k < kHalfBackPerThread; ++k) load_inputs(k);
#pragma unroll
    for (int k = 0; k < kHalfBackPerThread; ++k) {
      const int i = ft + k * kHalfThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const float th = ADAPT ? tv[k] : p.v_th;         // the threshold h was compared with
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        (g_x + at)[(uint32_t)i] = g_c;
        G[half_g_index(i, chunks)] = g_c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kHalfBackPerThread; ++k) {
    const int i = tid + k * kHalfThreads;
    if (i < N) {
      if (g_c0 != nullptr) (g_c0 + base)[(uint32_t)i] = cc[k];
      if (g_v0 != nullptr) (g_v0 + base)[(uint32_t)i] = cv[k];
      if (ADAPT && g_a0 != nullptr) (g_a0 + base)[(uint32_t)i] = ca[k];
    }
  }
  if (g_s0 != nullptr) half_rows<ST>(vec != 0, w, G, N, lsh, g_s0 + base);    // from g_x[0]
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int half_check_common(const char* who, int64_t T, int64_t B, int64_t N, int reset_mode, int wdtype) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : (wdtype != BE_F16 && wdtype != BE_BF16) ? ": wdtype must be BE_F16 or BE_BF16 (f32 weights: be_lif_rec_dense_sg_*)"
                                                              : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kHalfMaxN || B > 0x7fffffffll) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons (limit: " + std::to_string(kHalfMaxN) +
                 ", one workgroup holds a sample's neurons in its registers), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

// F16 or BF16 as a tag (wdtype was checked)
template <typename F>
inline int half_dispatch_storage(int wdtype, F&& f) {
  return wdtype == BE_F16 ? f(be_type_tag<F16>{}) : f(be_type_tag<BF16>{});
}

}  // namespace

extern "C" {

int be_lif_rec_dense_half_sg_forward(const float* x, const void* w, int wdtype, const float* s0, const float* c0, const float* v0,
                                     const float* a0, float* s_out, float* v_seq, float* h_save, float* th_save, float* c_last,
                                     float* v_last, float* a_last, int64_t T, int64_t B, int64_t N, double syn_decay, double beta,
                                     double v_th, double v_reset, double rho, double kappa, int reset_mode, int adaptive,
                                     int scale_exp, be_stream_t stream) {
  if (const int rc = half_check_common(__func__, T, B, N, reset_mode, wdtype)) return rc;
  BE_REQUIRE(scale_exp >= kHalfMinExp && scale_exp <= kHalfMaxExp, BE_ERR_INVALID,
             "scale_exp outside the exponents be_fixed_point_exponent returns (-90 .. 150)");
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(w, BE_ERR_INVALID, "null pointer (w is required)");
  BE_REQUIRE(reinterpret_cast<uintptr_t>(w) % 2 == 0, BE_ERR_INVALID, "w must be 2-byte aligned");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const float scale = ldexpf(1.0f, scale_exp - 32);   // see fixed_from_f32
  const double inv = ldexp(1.0, -scale_exp);
  const int pair = N % 2 == 0 && reinterpret_cast<uintptr_t>(w) % 4 == 0;
  const uint16_t* wp = static_cast<const uint16_t*>(w);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  half_dispatch_storage(wdtype, [&](auto S) {
    using ST = typename decltype(S)::type;
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        hipLaunchKernelGGL((k_lif_rec_dense_half_forward<ST, decltype(H)::value, decltype(A)::value>), dim3((unsigned)B),
                           dim3(kHalfThreads), 0, st, x, wp, s0, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, B,
                           (int)N, pair, scale, inv, p);
        return BE_OK;
      });
    });
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_dense_half_sg_backward(const float* h_save, const float* th_save, const void* w, int wdtype, const float* g_s,
                                      const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                                      float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0, int64_t T, int64_t B, int64_t N,
                                      double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa,
                                      int reset_mode, int surrogate, double alpha, int adaptive, int detach_reset,
                                      be_stream_t stream) {
  if (const int rc = half_check_common(__func__, T, B, N, reset_mode, wdtype)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(w, BE_ERR_INVALID, "null pointer (w is required)");
  BE_REQUIRE(reinterpret_cast<uintptr_t>(w) % 2 == 0, BE_ERR_INVALID, "w must be 2-byte aligned");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int vec = N % 8 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
  const int lds = (int)be_align_up((be_align_up(N, 8) + N) * 4, 16);
  const int detach = (int)(detach_reset != 0);
  const uint16_t* wp = static_cast<const uint16_t*>(w);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  half_dispatch_storage(wdtype, [&](auto S) {
    using ST = typename decltype(S)::type;
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
          auto kern = k_lif_rec_dense_half_backward<ST, decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
          allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
          if (allowed == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kHalfThreads), lds, st, h_save, th_save, wp, g_s, g_vseq, g_clast,
                               g_vlast, g_alast, g_x, g_c0, g_v0, g_a0, g_s0, T, B, (int)N, vec, detach, p);
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
