// be_neuron_sg_rec_dense.hip — the fused recurrent spiking layer with a DENSE recurrence: step t's
// input is x[t] + s[t-1] @ W with W [N, N] f32 row-major, rows = presynaptic neurons.  The function is the CSR layer's on the matrix
// that stores all N * N entries: the recurrent sums are the 64-bit fixed-point integers of fixed_from_f32 at the given exponent,
// scaled back and rounded once — so the forward outputs are those of be_lif_rec_sg_forward bit for bit, however the work is split.
// One workgroup of kDenThreads threads owns one sample for the whole launch; thread tid owns neurons tid + k * kDenThreads,
// k < kDenPerThread, their state in registers whose indices are compile-time constants (no scratch).  The time loop's scaffolding
// is be_neuron_sg_rec.hip's, restated; the neuron is be_sg_lane.h's.
//
// Forwards (k_lif_rec_dense_forward).  No id list, no LDS atomics on the main path.  The previous step's spikes are a bit mask in LDS,
// ceil(N / 64) 64-bit words, double-buffered: with the ownership above wave w's ballot for chunk k IS word 16 * k + w.  After ONE
// barrier every wave scans the words (LDS broadcasts, wave-uniform control flow: the words go through readfirstlane), gathers
// kDenRowBatch row ids in two scalars, 16 bits each, and for such a batch loads W[i, j] of its own columns j — a wave reads 256
// contiguous bytes of each row, all rows of the batch in flight before the first is used (the walk is bound by L2 latency, not
// bytes) — converts each value with fixed_from_f32 and adds it to an int64 sum per owned column, in registers.  For N <= 512 the
// threads form G = 1024 / P row groups, P = the power of two >= max(N, 64): thread tid has column tid % P and group tid / P, group
// g takes the active rows whose ordinal in the mask is g modulo G (so the groups share the work whatever words it sits in), and the
// groups' partial sums meet in an N x 8-byte LDS array through ds_add_u64; the neuron's owner reads and clears its entry.
// Integer sums: every such split gives the same bits.
//
// Backwards (k_lif_rec_dense_backward).  The CSR kernel's loop with the gather replaced by a dense row product: G = g_x[t+1] of the
// sample is in LDS, g_rec[i] = sum_j W[i, j] * G[j].  L lanes work per row (a power of two chosen from N, up to a wave), lane l
// takes the 16-byte chunks l, l + L, ... of the row and the matching float4 of G (consecutive lanes, consecutive 16 bytes:
// conflict-free), kDenChunks chunks of kDenRows rows in flight, an f32 partial sum per row in ascending j, then one butterfly.
// The 16-byte path needs N % 4 == 0 and a 16-byte aligned W; otherwise the same lanes load the same elements 4 bytes at a time: the
// order of the additions is a function of N alone.  Every operation is rounded on its own (no FMA contraction).
//
// No global atomics, no spin waits, nothing between workgroups; every barrier sits in uniform control flow and every loop is bounded
// by T and N.  Matrix instructions are not used: a sample's steps are one dependent chain of 1 x N by N x N products.
#include "be_sg_lane.h"

namespace {

namespace lane = be_sg_lane;

constexpr int kDenThreads = 1024;
constexpr int kDenMaxN = 8192;
constexpr int kDenPerThread = kDenMaxN / kDenThreads;
constexpr int kDenWaves = kDenThreads / kWave;
constexpr int kDenMaxWords = kDenMaxN / 64;
// at most this many neurons are served by row groups (their partial sums: kDenGroupN * 8 bytes of LDS)
constexpr int kDenGroupN = 512;
// rows whose loads a thread issues before it uses the first (their ids: 16 bits each in two 64-bit scalars)
constexpr int kDenRowBatch = 6;
static_assert(kDenRowBatch <= 8, "two 64-bit scalars hold eight 16-bit row ids");
// backwards: rows and 16-byte chunks per row a lane has in flight
constexpr int kDenRows = 4, kDenChunks = 2;
// the neurons of a thread whose step inputs are loaded before the walk / the row product, not after it
constexpr int kDenEarly = 2;
// the exponents be_fixed_point_exponent returns (2^(e - 32) must be a normal f32)
constexpr int kDenMinExp = -90, kDenMaxExp = 150;

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// A new value at every step for the lane's index (no instruction): addresses derived from it are formed where they are used, a
// scalar base plus a 32-bit offset, not hoisted out of the time loop as a 64-bit register pair per array and owned neuron.
__device__ __forceinline__ uint32_t dense_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the n <= kDenRowBatch rows whose ids sit in the low 16-bit fields of lo (then hi): acc[k] += fixed(W[row, col + k * kDenThreads])
template <int KP>
__device__ __forceinline__ void dense_add_rows(const float* __restrict__ w, int N, int col, unsigned long long lo,
                                               unsigned long long hi, int n, float scale, unsigned long long (&acc)[KP]) {
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int j = col + k * kDenThreads;
    if (k * kDenThreads < N && j < N) {
      float wv[kDenRowBatch];
#pragma unroll
      for (int q = 0; q < kDenRowBatch; ++q) {                 // in flight together
        const uint32_t row = (uint32_t)((q < 4 ? lo >> (16 * q) : hi >> (16 * (q - 4))) & 0xffffull);
        wv[q] = 0.f;                                           // fixed(0) = 0: an absent row adds the integer 0
        if (q < n) wv[q] = (w + (size_t)row * (size_t)N)[(uint32_t)j];   // a scalar row base + a 32-bit lane offset
      }
#pragma unroll
      for (int q = 0; q < kDenRowBatch; ++q) acc[k] += fixed_from_f32(wv[q], scale);
    }
    __builtin_amdgcn_sched_barrier(0);                     // one chunk's loads at a time: kDenRowBatch registers, not KP times that
  }
}

// the rows the mask lists whose ordinal is g modulo G (G a power of two; G = 1: all of them), kDenRowBatch at a time
template <int KP>
__device__ __forceinline__ void dense_walk(const float* __restrict__ w, int N, const unsigned long long* mask, int words, int col,
                                           uint32_t g, uint32_t G, float scale, unsigned long long (&acc)[KP]) {
  unsigned long long lo = 0ull, hi = 0ull, m = 0ull;
  uint32_t ord = 0;
  int q = -1;
  for (;;) {                                             // one batch per turn: a single call site keeps the registers in bounds
    int n = 0;
    while (n < kDenRowBatch) {
      if (m == 0ull) {
        if (++q >= words) break;
        m = uniform64(mask[q]);
        continue;
      }
      const uint32_t row = (uint32_t)(q * 64 + __builtin_ctzll(m));
      m &= m - 1ull;
      if ((ord++ & (G - 1u)) != g) continue;
      hi = (hi << 16) | (lo >> 48);
      lo = (lo << 16) | row;
      ++n;
    }
    if (n == 0) break;
    dense_add_rows<KP>(w, N, col, lo, hi, n, scale, acc);
    if (n < kDenRowBatch) break;                         // the mask is exhausted
  }
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N]; w [N, N].  s0 / c0 / v0 / a0
// NULL = 0; v_seq / h_save / th_save may be NULL.  Static LDS only: the two masks and the row groups' sums.
template <bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kDenThreads)
k_lif_rec_dense_forward(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ s0,
                        const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ a0,
                        float* __restrict__ s_out, float* __restrict__ v_seq, float* __restrict__ h_save, float* __restrict__ th_save,
                        float* __restrict__ c_last, float* __restrict__ v_last, float* __restrict__ a_last, int64_t T, int64_t B, int N,
                        float scale, double inv, lane::LifP p) {
#pragma clang fp contract(off)
  __shared__ unsigned long long mask[2][kDenMaxWords];
  __shared__ unsigned long long part[kDenGroupN];
  const int tid = threadIdx.x, wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  const int words = (N + 63) / 64;
  // the row groups: P columns each (N <= kDenGroupN), or one group over all the columns
  int P = kDenThreads;
  if (N <= kDenGroupN) {
    P = kWave;
    while (P < N) P <<= 1;
  }
  const uint32_t G = (uint32_t)(kDenThreads / P);
  const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane(tid / P);   // whole waves: P >= kWave
  const int col = tid & (P - 1);
  float c[kDenPerThread], v[kDenPerThread], a[kDenPerThread];
  uint32_t sbits = 0;                                    // bit k: neuron tid + k * kDenThreads spiked at the previous step
#pragma unroll
  for (int k = 0; k < kDenPerThread; ++k) {
    const int i = tid + k * kDenThreads;
    c[k] = v[k] = a[k] = 0.f;
    if (i < N) {
      if (c0 != nullptr) c[k] = (c0 + base)[(uint32_t)i];
      if (v0 != nullptr) v[k] = (v0 + base)[(uint32_t)i];
      if (ADAPT && a0 != nullptr) a[k] = (a0 + base)[(uint32_t)i];
      if (s0 != nullptr && (s0 + base)[(uint32_t)i] != 0.f) sbits |= 1u << k;
    }
  }
  if (tid < kDenGroupN) part[tid] = 0ull;
  int cur = 0;
  for (int64_t t = 0; t < T; ++t) {
    const int64_t at = t * step + base;
    const int ft = (int)dense_fresh((uint32_t)tid);
    // the previous step's spikes -> the mask: wave w's ballot for chunk k is word 16 * k + w (the other buffer is still being read)
#pragma unroll
    for (int k = 0; k < kDenPerThread; ++k) {
      if (k * kDenThreads < N) {
        const unsigned long long m = __ballot((sbits >> k) & 1u);
        if ((tid & (kWave - 1)) == 0 && kDenWaves * k + wave < words) mask[cur][kDenWaves * k + wave] = m;
      }
    }
    // x does not depend on the chain: that of a thread's first kDenEarly neurons (every N <= 2048) is in flight during the walk,
    // the rest is loaded after it (the walk's sums and loads need the registers)
    float xv[kDenPerThread];
    auto load_x = [&](int k) {
      const int i = ft + k * kDenThreads;
      xv[k] = 0.f;
      if (i < N) xv[k] = (x + at)[(uint32_t)i];
    };
#pragma unroll
    for (int k = 0; k < kDenEarly; ++k) load_x(k);
    __syncthreads();
    unsigned long long R[kDenPerThread];
#pragma unroll
    for (int k = 0; k < kDenPerThread; ++k) R[k] = 0ull;
    if (G == 1u) {
      dense_walk<kDenPerThread>(w, N, mask[cur], words, ft, 0u, 1u, scale, R);
    } else {
      unsigned long long one[1] = {0ull};
      dense_walk<1>(w, N, mask[cur], words, ft & (P - 1), g, G, scale, one);
      if (col < N && one[0] != 0ull) atomicAdd(&part[col], one[0]);
      __syncthreads();
      if (tid < N) {
        R[0] = part[tid];
        part[tid] = 0ull;                                // read and cleared by its owner only; the next adds come after a barrier
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = kDenEarly; k < kDenPerThread; ++k) load_x(k);
    cur ^= 1;
    sbits = 0;
#pragma unroll
    for (int k = 0; k < kDenPerThread; ++k) {
      const int i = ft + k * kDenThreads;
      if (i < N) {
        const float r = (float)((double)(long long)R[k] * inv);
        const lane::Fired f = lane::forward_step<HARD, true, ADAPT>(xv[k] + r, c[k], v[k], a[k], p.beta, p.v_th, p);
        if (f.s) sbits |= 1u << k;
        (s_out + at)[(uint32_t)i] = f.s ? 1.0f : 0.0f;
        if (v_seq != nullptr) (v_seq + at)[(uint32_t)i] = v[k];
        if (h_save != nullptr) {
          (h_save + at)[(uint32_t)i] = f.h;
          if (ADAPT) (th_save + at)[(uint32_t)i] = f.th;
        }
      }
      __builtin_amdgcn_sched_barrier(0);                 // one neuron's step at a time: interleaving eight costs registers
    }
  }
#pragma unroll
  for (int k = 0; k < kDenPerThread; ++k) {
    const int i = tid + k * kDenThreads;
    if (i < N) {
      (c_last + base)[(uint32_t)i] = c[k];
      (v_last + base)[(uint32_t)i] = v[k];
      if (ADAPT) (a_last + base)[(uint32_t)i] = a[k];
    }
  }
}

// the 16-byte chunk `chunk` of row `row`: one load (VEC: N % 4 == 0, w 16-byte aligned), or its elements below N one by one
template <bool VEC>
__device__ __forceinline__ float4 dense_chunk(const float* __restrict__ w, int N, int row, int chunk) {
  const float* at = w + (size_t)row * (size_t)N + (size_t)chunk * 4u;
  if (VEC) return *reinterpret_cast<const float4*>(at);
  const int j = chunk * 4;
  float4 r;
  r.x = at[0];                                            // j < N: the chunk exists
  r.y = j + 1 < N ? at[1] : 0.f;
  r.z = j + 2 < N ? at[2] : 0.f;
  r.w = j + 3 < N ? at[3] : 0.f;
  return r;
}

// out[i] = sum_j W[i, j] * G[j] for every row i < N, G in LDS (its tail up to a multiple of 4 is zero).  Lane `sub` of a row's
// L = 1 << lsh takes the chunks sub, sub + L, ... in order, every product rounded, then a butterfly over the L partial sums: an
// order N alone fixes.  kDenRows rows (kDenThreads / L apart) and kDenChunks chunks of each are loaded before the first is used.
template <bool VEC>
__device__ __forceinline__ void dense_rows(const float* __restrict__ w, const float* G, int N, int lsh, float* out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, L = 1 << lsh, sub = tid & (L - 1), apart = kDenThreads >> lsh;
  const int chunks = (N + 3) >> 2;
  const float4* G4 = reinterpret_cast<const float4*>(G);
  for (int row0 = tid >> lsh; row0 < N; row0 += kDenRows * apart) {      // a row's lanes share row0: they leave the loop together
    float sum[kDenRows];
#pragma unroll
    for (int r = 0; r < kDenRows; ++r) sum[r] = 0.f;
    for (int ch = sub; ch < chunks; ch += kDenChunks * L) {
      float4 wv[kDenRows][kDenChunks], gv[kDenChunks];
#pragma unroll
      for (int u = 0; u < kDenChunks; ++u) {
        const int cu = ch + u * L;
        const bool in = cu < chunks;
        gv[u] = G4[in ? cu : 0];
#pragma unroll
        for (int r = 0; r < kDenRows; ++r) {
          const int row = row0 + r * apart;
          wv[r][u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (in && row < N) wv[r][u] = dense_chunk<VEC>(w, N, row, cu);
        }
      }
#pragma unroll
      for (int u = 0; u < kDenChunks; ++u) {
        const int j = (ch + u * L) * 4;                                  // (past the row: j >= N, nothing is added)
#pragma unroll
        for (int r = 0; r < kDenRows; ++r) {
          const float t0 = wv[r][u].x * gv[u].x, t1 = wv[r][u].y * gv[u].y, t2 = wv[r][u].z * gv[u].z, t3 = wv[r][u].w * gv[u].w;
          float s = sum[r];
          s = j < N ? s + t0 : s;
          s = j + 1 < N ? s + t1 : s;
          s = j + 2 < N ? s + t2 : s;
          s = j + 3 < N ? s + t3 : s;
          sum[r] = s;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kDenRows; ++r) {
      float s = sum[r];
      for (int off = L >> 1; off > 0; off >>= 1) s = s + __shfl_xor(s, off);   // within the row's aligned group of L lanes
      const int row = row0 + r * apart;
      if (sub == 0 && row < N) out[row] = s;
    }
  }
}

__device__ __forceinline__ void dense_rows(bool vec, const float* __restrict__ w, const float* G, int N, int lsh, float* out) {
  if (vec) dense_rows<true>(w, G, N, lsh, out);
  else dense_rows<false>(w, G, N, lsh, out);
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; the others [B, N]; w [N, N].  g_s / g_vseq / g_clast / g_vlast /
// g_alast NULL = 0; g_c0 / g_v0 / g_a0 / g_s0 may be NULL.  Dynamic LDS: g_x[t+1] of the sample (N floats rounded up to a multiple
// of 4, the tail zero), then g_rec (N floats).
template <bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kDenThreads)
k_lif_rec_dense_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ w,
                         const float* __restrict__ g_s, const float* __restrict__ g_vseq, const float* __restrict__ g_clast,
                         const float* __restrict__ g_vlast, const float* __restrict__ g_alast, float* __restrict__ g_x,
                         float* __restrict__ g_c0, float* __restrict__ g_v0, float* __restrict__ g_a0, float* __restrict__ g_s0,
                         int64_t T, int64_t B, int N, int vec, int detach_reset, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* G = reinterpret_cast<float*>(smem_raw);
  const int padded = (N + 3) & ~3;
  float* grec = G + padded;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  // lanes per row: the power of two that leaves a lane at most kDenChunks chunks, up to a wave
  int lsh = 0;
  while ((1 << lsh) < kWave && (kDenChunks << lsh) < ((N + 3) >> 2)) ++lsh;
  if (tid < padded - N) G[N + tid] = 0.f;                // written once: the steps write G[i] for i < N only
  float cc[kDenPerThread], cv[kDenPerThread], ca[kDenPerThread];
#pragma unroll
  for (int k = 0; k < kDenPerThread; ++k) {
    const int i = tid + k * kDenThreads;
    cc[k] = cv[k] = ca[k] = 0.f;
    if (i < N) {
      if (g_clast != nullptr) cc[k] = (g_clast + base)[(uint32_t)i];
      if (g_vlast != nullptr) cv[k] = (g_vlast + base)[(uint32_t)i];
      if (ADAPT && g_alast != nullptr) ca[k] = (g_alast + base)[(uint32_t)i];
    }
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t at = t * step + base;
    const int ft = (int)dense_fresh((uint32_t)tid);
    const bool rec = t < T - 1;
    // the step's inputs: those of a thread's first kDenEarly neurons (every N <= 2048) are in flight during the row product, the
    // others are loaded after it (32 more registers across the product would not fit beside its loads)
    float hv[kDenPerThread], tv[kDenPerThread], gsv[kDenPerThread], gvv[kDenPerThread];
    auto load_inputs = [&](int k) {
      const int i = ft + k * kDenThreads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = (h_save + at)[(uint32_t)i];
        if (ADAPT) tv[k] = (th_save + at)[(uint32_t)i];
        if (g_s != nullptr) gsv[k] = (g_s + at)[(uint32_t)i];
        if (g_vseq != nullptr) gvv[k] = (g_vseq + at)[(uint32_t)i];
      }
    };
#pragma unroll
    for (int k = 0; k < kDenEarly; ++k) load_inputs(k);
    if (rec) {
      dense_rows(vec != 0, w, G, N, lsh, grec);
      __syncthreads();
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = kDenEarly; k < kDenPerThread; ++k) load_inputs(k);
#pragma unroll
    for (int k = 0; k < kDenPerThread; ++k) {
      const int i = ft + k * kDenThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const float th = ADAPT ? tv[k] : p.v_th;         // the threshold h was compared with
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        (g_x + at)[(uint32_t)i] = g_c;
        G[i] = g_c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kDenPerThread; ++k) {
    const int i = tid + k * kDenThreads;
    if (i < N) {
      if (g_c0 != nullptr) (g_c0 + base)[(uint32_t)i] = cc[k];
      if (g_v0 != nullptr) (g_v0 + base)[(uint32_t)i] = cv[k];
      if (ADAPT && g_a0 != nullptr) (g_a0 + base)[(uint32_t)i] = ca[k];
    }
  }
  if (g_s0 != nullptr) dense_rows(vec != 0, w, G, N, lsh, g_s0 + base);      // from g_x[0]
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int dense_check_common(const char* who, int64_t T, int64_t B, int64_t N, int reset_mode) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode" : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kDenMaxN || B > 0x7fffffffll) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons (limit: " + std::to_string(kDenMaxN) +
                 ", one workgroup holds a sample's neurons in its registers), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

}  // namespace

extern "C" {

int be_lif_rec_dense_sg_forward(const float* x, const float* w, const float* s0, const float* c0, const float* v0, const float* a0,
                                float* s_out, float* v_seq, float* h_save, float* th_save, float* c_last, float* v_last,
                                float* a_last, int64_t T, int64_t B, int64_t N, double syn_decay, double beta, double v_th,
                                double v_reset, double rho, double kappa, int reset_mode, int adaptive, int scale_exp,
                                be_stream_t stream) {
  if (const int rc = dense_check_common(__func__, T, B, N, reset_mode)) return rc;
  BE_REQUIRE(scale_exp >= kDenMinExp && scale_exp <= kDenMaxExp, BE_ERR_INVALID,
             "scale_exp outside the exponents be_fixed_point_exponent returns (-90 .. 150)");
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(w, BE_ERR_INVALID, "null pointer (w is required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const float scale = ldexpf(1.0f, scale_exp - 32);   // see fixed_from_f32
  const double inv = ldexp(1.0, -scale_exp);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      hipLaunchKernelGGL((k_lif_rec_dense_forward<decltype(H)::value, decltype(A)::value>), dim3((unsigned)B), dim3(kDenThreads), 0, st,
                         x, w, s0, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, B, (int)N, scale, inv, p);
      return BE_OK;
    });
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_dense_sg_backward(const float* h_save, const float* th_save, const float* w, const float* g_s, const float* g_vseq,
                                 const float* g_clast, const float* g_vlast, const float* g_alast, float* g_x, float* g_c0,
                                 float* g_v0, float* g_a0, float* g_s0, int64_t T, int64_t B, int64_t N, double syn_decay,
                                 double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode, int surrogate,
                                 double alpha, int adaptive, int detach_reset, be_stream_t stream) {
  if (const int rc = dense_check_common(__func__, T, B, N, reset_mode)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(w, BE_ERR_INVALID, "null pointer (w is required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int vec = N % 4 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
  const int lds = (int)be_align_up((be_align_up(N, 4) + N) * 4, 16);
  const int detach = (int)(detach_reset != 0);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        auto kern = k_lif_rec_dense_backward<decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
        allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
        if (allowed == hipSuccess)
          hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kDenThreads), lds, st, h_save, th_save, w, g_s, g_vseq, g_clast, g_vlast,
                             g_alast, g_x, g_c0, g_v0, g_a0, g_s0, T, B, (int)N, vec, detach, p);
        return BE_OK;
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
