// be_neuron_sg_param.hip — the differentiable LIF neuron of be_neuron_sg.hip with beta and v_th read from DEVICE memory, one
// value per slot with a period: slot i of the N slots of a step uses beta[i % beta_period] and
// v_th[i % vth_period] (period 1: one shared value; period N / R: one value per neuron under R batch rows).  Nothing crosses to
// the host, so a Parameter an optimiser updates in place is seen by the next call and by the next replay of a captured graph.
//
// Forward (k_lif_sgp_forward) and backward (k_lif_sgp_backward) are §2.19's passes with beta_i, th_i in place of the two
// constants: the same lane layout (a lane keeps its S slots for the whole launch, the time loop runs inside it, the loads the
// chain does not depend on run kSgpPrefetch steps ahead in a register ring with compile-time indices), the same operations in
// the same order, every one rounded separately.  The backward pass also keeps, per slot, the two f32 accumulators of the
// parameters' gradients — a_b += g_h * v_prev and a_th -= g_sp * sg (+ the soft reset's direct term) — where v_prev is the
// membrane the step started from, recomputed from h[t-1], which the ring already holds (v0 at t = 0).  They are written per slot
// (g_beta_slot, g_vth_slot [N]); be_lif_sg_reduce_slots then sums the N / P slots of each parameter element in f64, in an order
// the shape alone fixes, and rounds to f32 once.  No float atomics anywhere: two calls give identical bits.
//
// S = kSgpVec with 16-byte accesses where N, every base and every period allow it (a period is 1, or a multiple of kSgpVec with
// an aligned base: then i % period is a multiple of kSgpVec too and the S values are consecutive), S = 1 otherwise.
#include "be_common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kSgpThreads = 256;
constexpr int kSgpGridCap = 2048;
constexpr int kSgpVec = 4;
constexpr int kSgpPrefetch = 4;
// the reduce: blocks of kSgpRedThreads; period 1 runs at most kSgpRedGridCap blocks over tiles of kSgpRedTile slots, then one
// block over their partials; a longer period runs kSgpRedCols columns by kSgpRedThreads / kSgpRedCols row lanes a block
constexpr int kSgpRedThreads = 256;
constexpr int kSgpRedTile = 4096;
constexpr int kSgpRedGridCap = 256;
constexpr int kSgpRedCols = 64;
static_assert(kSgpRedGridCap <= kSgpRedThreads && kSgpRedThreads % kSgpRedCols == 0, "the reduce's second stage is one block");

template <int S> struct SgpPack;
template <> struct SgpPack<1> { using type = float; };
template <> struct SgpPack<4> { using type = float4; };

template <int S>
struct SgpVals {
  float f[S];
};

template <int S>
__device__ __forceinline__ SgpVals<S> sgp_load(const float* __restrict__ p) {
  using P = typename SgpPack<S>::type;
  const P raw = *reinterpret_cast<const P*>(p);
  SgpVals<S> out;
  __builtin_memcpy(out.f, &raw, sizeof(P));
  return out;
}

template <int S>
__device__ __forceinline__ void sgp_store(float* __restrict__ p, const SgpVals<S>& v) {
  using P = typename SgpPack<S>::type;
  P raw;
  __builtin_memcpy(&raw, v.f, sizeof(P));
  *reinterpret_cast<P*>(p) = raw;
}

template <int S>
__device__ __forceinline__ SgpVals<S> sgp_fill(float c) {
  SgpVals<S> out;
#pragma unroll
  for (int j = 0; j < S; ++j) out.f[j] = c;
  return out;
}

// the S parameter values of the slots i .. i + S - 1 (i % S == 0; period 1, or period % S == 0)
template <int S>
__device__ __forceinline__ SgpVals<S> sgp_load_param(const float* __restrict__ p, int64_t period, int64_t i) {
  if (period == 1) return sgp_fill<S>(p[0]);
  return sgp_load<S>(p + i % period);
}

// a parameter array and its period
struct SgpArr {
  const float* p;
  int64_t period;
};

struct SgpConsts {
  float v_reset, alpha, atan_c, atan_half;
};

// the membrane a step leaves behind, from its h
template <bool HARD>
__device__ __forceinline__ float sgp_reset(float h, float th, float v_reset) {
#pragma clang fp contract(off)
  const bool s = h >= th;
  return HARD ? (s ? v_reset : h) : (s ? h - th : h);
}

// Forward: v_seq / h_save may be NULL (uniform branches outside the arithmetic), v0 NULL = 0.
template <int S, bool HARD>
__global__ void __launch_bounds__(kSgpThreads) k_lif_sgp_forward(const float* __restrict__ x, const float* __restrict__ v0,
                                                                 SgpArr beta, SgpArr vth, float* __restrict__ s_out,
                                                                 float* __restrict__ v_seq, float* __restrict__ h_save,
                                                                 float* __restrict__ v_last, int64_t T, int64_t N, SgpConsts c) {
#pragma clang fp contract(off)
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    const SgpVals<S> bv = sgp_load_param<S>(beta.p, beta.period, i);
    const SgpVals<S> tv = sgp_load_param<S>(vth.p, vth.period, i);
    SgpVals<S> v = v0 != nullptr ? sgp_load<S>(v0 + i) : sgp_fill<S>(0.f);
    SgpVals<S> ring[kSgpPrefetch];
#pragma unroll
    for (int r = 0; r < kSgpPrefetch; ++r)
      if (r < T) ring[r] = sgp_load<S>(x + (int64_t)r * N + i);
    for (int64_t t0 = 0; t0 < T; t0 += kSgpPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgpPrefetch; ++r) {
        const int64_t t = t0 + r;
        if (t < T) {
          const SgpVals<S> xv = ring[r];
          if (t + kSgpPrefetch < T) ring[r] = sgp_load<S>(x + (t + kSgpPrefetch) * N + i);
          SgpVals<S> sv, hv;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float h = (bv.f[j] * v.f[j]) + xv.f[j];
            const bool s = h >= tv.f[j];
            v.f[j] = HARD ? (s ? c.v_reset : h) : (s ? h - tv.f[j] : h);
            sv.f[j] = s ? 1.0f : 0.0f;
            hv.f[j] = h;
          }
          sgp_store<S>(s_out + t * N + i, sv);
          if (v_seq != nullptr) sgp_store<S>(v_seq + t * N + i, v);
          if (h_save != nullptr) sgp_store<S>(h_save + t * N + i, hv);
        }
      }
    }
    sgp_store<S>(v_last + i, v);
  }
}

// the surrogate's derivative at u = h - v_th (SG: BE_LIF_SG_*)
template <int SG>
__device__ __forceinline__ float sgp_derivative(float u, const SgpConsts& c) {
#pragma clang fp contract(off)
  if (SG == 0) {                    // fast sigmoid
    const float d = 1.0f + c.alpha * fabsf(u);
    return 1.0f / (d * d);
  }
  if (SG == 1) {                    // arctangent
    const float q = c.atan_c * u;
    return c.atan_half / (1.0f + q * q);
  }
  const float a = 1.0f - c.alpha * fabsf(u);     // triangle; a NaN compares false: 0, as fmaxf(0, NaN)
  return c.alpha * (a > 0.0f ? a : 0.0f);
}

// Backward: g_s / g_vseq / g_vlast / g_v0 / g_beta_slot / g_vth_slot may be NULL; v0 (NULL = 0) is read only for g_beta_slot.
template <int S, bool HARD, int SG>
__global__ void __launch_bounds__(kSgpThreads) k_lif_sgp_backward(const float* __restrict__ h_save, const float* __restrict__ v0,
                                                                  const float* __restrict__ g_s, const float* __restrict__ g_vseq,
                                                                  const float* __restrict__ g_vlast, SgpArr beta, SgpArr vth,
                                                                  float* __restrict__ g_x, float* __restrict__ g_v0,
                                                                  float* __restrict__ g_beta_slot, float* __restrict__ g_vth_slot,
                                                                  int64_t T, int64_t N, int detach_reset, SgpConsts c) {
#pragma clang fp contract(off)
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    const SgpVals<S> bv = sgp_load_param<S>(beta.p, beta.period, i);
    const SgpVals<S> tv = sgp_load_param<S>(vth.p, vth.period, i);
    SgpVals<S> carry = g_vlast != nullptr ? sgp_load<S>(g_vlast + i) : sgp_fill<S>(0.f);
    SgpVals<S> acc_b = sgp_fill<S>(0.f), acc_t = sgp_fill<S>(0.f);
    SgpVals<S> ring_h[kSgpPrefetch], ring_s[kSgpPrefetch], ring_v[kSgpPrefetch];
#pragma unroll
    for (int r = 0; r < kSgpPrefetch; ++r) {
      ring_s[r] = sgp_fill<S>(0.f);
      ring_v[r] = sgp_fill<S>(0.f);
      if (r < T) {
        const int64_t off = (T - 1 - r) * N + i;
        ring_h[r] = sgp_load<S>(h_save + off);
        if (g_s != nullptr) ring_s[r] = sgp_load<S>(g_s + off);
        if (g_vseq != nullptr) ring_v[r] = sgp_load<S>(g_vseq + off);
      }
    }
    for (int64_t k0 = 0; k0 < T; k0 += kSgpPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgpPrefetch; ++r) {
        const int64_t k = k0 + r;        // the k-th step from the end: t = T - 1 - k
        if (k < T) {
          const SgpVals<S> hv = ring_h[r], gsv = ring_s[r], gvv = ring_v[r];
          if (k + kSgpPrefetch < T) {
            const int64_t off = (T - 1 - k - kSgpPrefetch) * N + i;
            ring_h[r] = sgp_load<S>(h_save + off);
            if (g_s != nullptr) ring_s[r] = sgp_load<S>(g_s + off);
            if (g_vseq != nullptr) ring_v[r] = sgp_load<S>(g_vseq + off);
          }
          // the membrane step t started from: step t - 1 is the next one of the ring (loaded at the start, or, for the
          // ring's last place, refilled at this block's first step); t = 0 started from v0
          SgpVals<S> vp = sgp_fill<S>(0.f);
          if (g_beta_slot != nullptr) {
            if (k + 1 < T) {
              const SgpVals<S> hp = ring_h[(r + 1) % kSgpPrefetch];
#pragma unroll
              for (int j = 0; j < S; ++j) vp.f[j] = sgp_reset<HARD>(hp.f[j], tv.f[j], c.v_reset);
            } else if (v0 != nullptr) {
              vp = sgp_load<S>(v0 + i);
            }
          }
          SgpVals<S> gx;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float h = hv.f[j];
            const float th = tv.f[j];
            const bool s = h >= th;
            const float u = h - th;
            float g_vo = carry.f[j];
            if (g_vseq != nullptr) g_vo = g_vo + gvv.f[j];
            const float sg = sgp_derivative<SG>(u, c);
            float g_sp = gsv.f[j];                       // 0 when g_s is NULL
            if (!detach_reset) g_sp = HARD ? g_sp + g_vo * (c.v_reset - h) : g_sp - g_vo * th;
            const float gs = g_sp * sg;
            const float g_h = gs + (HARD ? (s ? 0.0f : g_vo) : g_vo);
            gx.f[j] = g_h;
            carry.f[j] = bv.f[j] * g_h;
            if (g_beta_slot != nullptr) acc_b.f[j] = acc_b.f[j] + (g_h * vp.f[j]);
            if (g_vth_slot != nullptr) {
              float d = gs;
              if (!HARD) d = d + (s ? g_vo : 0.0f);
              acc_t.f[j] = acc_t.f[j] - d;
            }
          }
          sgp_store<S>(g_x + (T - 1 - k) * N + i, gx);
        }
      }
    }
    if (g_v0 != nullptr) sgp_store<S>(g_v0 + i, carry);
    if (g_beta_slot != nullptr) sgp_store<S>(g_beta_slot + i, acc_b);
    if (g_vth_slot != nullptr) sgp_store<S>(g_vth_slot + i, acc_t);
  }
}

// ---------------------------------------------------------------------------------------------- the reduce
// the block's sum of one f64 per thread, in a fixed tree; valid in thread 0
__device__ __forceinline__ double sgp_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int half = kSgpRedThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) lds[threadIdx.x] += lds[threadIdx.x + half];
    __syncthreads();
  }
  return lds[0];
}

// period 1, first stage: block b sums the tiles b, b + gridDim.x, ... (a thread: its strided slots of each tile, in order)
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_tiles(const float* __restrict__ slot, int64_t N,
                                                                         double* __restrict__ partial) {
  __shared__ double lds[kSgpRedThreads];
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * kSgpRedTile; base < N; base += (int64_t)gridDim.x * kSgpRedTile) {
    const int64_t end = std::min<int64_t>(base + kSgpRedTile, N);
    for (int64_t i = base + threadIdx.x; i < end; i += kSgpRedThreads) acc += (double)slot[i];
  }
  const double sum = sgp_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// period 1, second stage: one block over the at most kSgpRedGridCap (<= kSgpRedThreads) partials; rounds to f32 once
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_final(const double* __restrict__ partial, int count,
                                                                         float* __restrict__ out) {
  __shared__ double lds[kSgpRedThreads];
  const double sum = sgp_block_sum((int)threadIdx.x < count ? partial[threadIdx.x] : 0.0, lds);
  if (threadIdx.x == 0) out[0] = (float)sum;
}

// period P > 1: a block owns kSgpRedCols consecutive elements p; row lane q sums the rows q, q + kRows, ... of its column in
// order, then the kRows partials of a column are added in order of q and rounded to f32 once
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_columns(const float* __restrict__ slot, int64_t R, int64_t P,
                                                                           float* __restrict__ out) {
  constexpr int kRows = kSgpRedThreads / kSgpRedCols;
  __shared__ double lds[kRows][kSgpRedCols];
  const int col = threadIdx.x % kSgpRedCols, q = threadIdx.x / kSgpRedCols;
  const int64_t p = (int64_t)blockIdx.x * kSgpRedCols + col;
  double acc = 0.0;
  if (p < P)
    for (int64_t r = q; r < R; r += kRows) acc += (double)slot[r * P + p];
  lds[q][col] = acc;
  __syncthreads();
  if (q == 0 && p < P) {
    double sum = lds[0][col];
#pragma unroll
    for (int k = 1; k < kRows; ++k) sum += lds[k][col];
    out[p] = (float)sum;
  }
}

inline int sgp_reduce_blocks(int64_t N) {
  return (int)std::min<int64_t>((N + kSgpRedTile - 1) / kSgpRedTile, kSgpRedGridCap);
}

// ---------------------------------------------------------------------------------------------- host side
inline bool sgp_aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

// a parameter array allows the 16-byte kernel: one shared value, or groups of kSgpVec that never wrap
inline bool sgp_param_vec(const float* p, int64_t period) {
  return period == 1 || (period % kSgpVec == 0 && sgp_aligned16(p));
}

inline int sgp_grid(int64_t N, int S) {
  const int64_t groups = N / S;
  return (int)std::min<int64_t>((groups + kSgpThreads - 1) / kSgpThreads, kSgpGridCap);
}

// the checks the two passes share (BE_REQUIRE would name this function, not the entry point)
inline int sgp_check_common(const char* who, int64_t T, int64_t N, int reset_mode, int64_t beta_period, int64_t vth_period) {
  const char* msg = (T < 0 || N < 0) ? ": T < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : (beta_period < 1 || vth_period < 1) ? ": a period must be >= 1"
                    : (N % beta_period != 0 || N % vth_period != 0) ? ": a period must divide N" : nullptr;
  if (msg == nullptr) return BE_OK;
  be_set_error(std::string(who) + msg);
  return BE_ERR_INVALID;
}

template <int S, bool HARD>
void sgp_launch_backward(int surrogate, int grid, hipStream_t st, const float* h_save, const float* v0, const float* g_s,
                         const float* g_vseq, const float* g_vlast, SgpArr beta, SgpArr vth, float* g_x, float* g_v0,
                         float* g_beta_slot, float* g_vth_slot, int64_t T, int64_t N, int detach_reset, const SgpConsts& c) {
  if (surrogate == BE_LIF_SG_FAST_SIGMOID)
    hipLaunchKernelGGL((k_lif_sgp_backward<S, HARD, 0>), dim3(grid), dim3(kSgpThreads), 0, st, h_save, v0, g_s, g_vseq, g_vlast, beta,
                       vth, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach_reset, c);
  else if (surrogate == BE_LIF_SG_ATAN)
    hipLaunchKernelGGL((k_lif_sgp_backward<S, HARD, 1>), dim3(grid), dim3(kSgpThreads), 0, st, h_save, v0, g_s, g_vseq, g_vlast, beta,
                       vth, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach_reset, c);
  else
    hipLaunchKernelGGL((k_lif_sgp_backward<S, HARD, 2>), dim3(grid), dim3(kSgpThreads), 0, st, h_save, v0, g_s, g_vseq, g_vlast, beta,
                       vth, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach_reset, c);
}

}  // namespace

extern "C" {

int be_lif_sg_forward_params(const float* x, const float* v0, const float* beta, int64_t beta_period, const float* v_th,
                             int64_t vth_period, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T, int64_t N,
                             double v_reset, int reset_mode, be_stream_t stream) {
  if (const int rc = sgp_check_common(__func__, T, N, reset_mode, beta_period, vth_period)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && beta && v_th && s_out && v_last, BE_ERR_INVALID, "null pointer (x, beta, v_th, s_out and v_last are required)");
  const SgpConsts c{(float)v_reset, 0.f, 0.f, 0.f};
  const SgpArr b{beta, beta_period}, th{v_th, vth_period};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  const bool vec = (N % kSgpVec == 0) && sgp_aligned16(x) && sgp_aligned16(v0) && sgp_aligned16(s_out) && sgp_aligned16(v_seq) &&
                   sgp_aligned16(h_save) && sgp_aligned16(v_last) && sgp_param_vec(beta, beta_period) && sgp_param_vec(v_th, vth_period);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = sgp_grid(N, vec ? kSgpVec : 1);
  if (vec && hard)
    hipLaunchKernelGGL((k_lif_sgp_forward<kSgpVec, true>), dim3(grid), dim3(kSgpThreads), 0, st, x, v0, b, th, s_out, v_seq, h_save, v_last, T, N, c);
  else if (vec)
    hipLaunchKernelGGL((k_lif_sgp_forward<kSgpVec, false>), dim3(grid), dim3(kSgpThreads), 0, st, x, v0, b, th, s_out, v_seq, h_save, v_last, T, N, c);
  else if (hard)
    hipLaunchKernelGGL((k_lif_sgp_forward<1, true>), dim3(grid), dim3(kSgpThreads), 0, st, x, v0, b, th, s_out, v_seq, h_save, v_last, T, N, c);
  else
    hipLaunchKernelGGL((k_lif_sgp_forward<1, false>), dim3(grid), dim3(kSgpThreads), 0, st, x, v0, b, th, s_out, v_seq, h_save, v_last, T, N, c);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_sg_backward_params(const float* h_save, const float* v0, const float* g_s, const float* g_vseq, const float* g_vlast,
                              const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period, float* g_x, float* g_v0,
                              float* g_beta_slot, float* g_vth_slot, int64_t T, int64_t N, double v_reset, int reset_mode,
                              int surrogate, double alpha, int detach_reset, be_stream_t stream) {
  if (const int rc = sgp_check_common(__func__, T, N, reset_mode, beta_period, vth_period)) return rc;
  BE_REQUIRE(surrogate == BE_LIF_SG_FAST_SIGMOID || surrogate == BE_LIF_SG_ATAN || surrogate == BE_LIF_SG_TRIANGLE, BE_ERR_INVALID,
             "unknown surrogate");
  BE_REQUIRE(alpha > 0., BE_ERR_INVALID, "alpha must be positive");
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && beta && v_th && g_x, BE_ERR_INVALID, "null pointer (h_save, beta, v_th and g_x are required)");
  // derived constants in double, rounded to f32 once
  const SgpConsts c{(float)v_reset, (float)alpha, (float)(M_PI / 2 * alpha), (float)(alpha / 2)};
  const SgpArr b{beta, beta_period}, th{v_th, vth_period};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  const float* v0_read = g_beta_slot != nullptr ? v0 : nullptr;        // read for the beta gradient alone
  const bool vec = (N % kSgpVec == 0) && sgp_aligned16(h_save) && sgp_aligned16(v0_read) && sgp_aligned16(g_s) && sgp_aligned16(g_vseq) &&
                   sgp_aligned16(g_vlast) && sgp_aligned16(g_x) && sgp_aligned16(g_v0) && sgp_aligned16(g_beta_slot) &&
                   sgp_aligned16(g_vth_slot) && sgp_param_vec(beta, beta_period) && sgp_param_vec(v_th, vth_period);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = sgp_grid(N, vec ? kSgpVec : 1);
  const int detach = detach_reset != 0;
  if (vec && hard)
    sgp_launch_backward<kSgpVec, true>(surrogate, grid, st, h_save, v0_read, g_s, g_vseq, g_vlast, b, th, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach, c);
  else if (vec)
    sgp_launch_backward<kSgpVec, false>(surrogate, grid, st, h_save, v0_read, g_s, g_vseq, g_vlast, b, th, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach, c);
  else if (hard)
    sgp_launch_backward<1, true>(surrogate, grid, st, h_save, v0_read, g_s, g_vseq, g_vlast, b, th, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach, c);
  else
    sgp_launch_backward<1, false>(surrogate, grid, st, h_save, v0_read, g_s, g_vseq, g_vlast, b, th, g_x, g_v0, g_beta_slot, g_vth_slot, T, N, detach, c);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int64_t be_lif_sg_reduce_slots_workspace_bytes(int64_t N, int64_t P) {
  if (N <= 0 || P != 1) return 0;
  return (int64_t)sgp_reduce_blocks(N) * (int64_t)sizeof(double);
}

int be_lif_sg_reduce_slots(const float* slot, int64_t N, int64_t P, float* out, void* workspace, int64_t workspace_bytes,
                           be_stream_t stream) {
  BE_REQUIRE(N >= 0, BE_ERR_INVALID, "N < 0");
  BE_REQUIRE(P >= 1, BE_ERR_INVALID, "the period must be >= 1");
  BE_REQUIRE(N % P == 0, BE_ERR_INVALID, "the period must divide N");
  if (N == 0) return BE_OK;
  BE_REQUIRE(slot && out, BE_ERR_INVALID, "null pointer (slot and out are required)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (P == 1) {
    const int blocks = sgp_reduce_blocks(N);
    BE_REQUIRE(workspace != nullptr && workspace_bytes >= be_lif_sg_reduce_slots_workspace_bytes(N, P), BE_ERR_INVALID,
               "workspace too small (be_lif_sg_reduce_slots_workspace_bytes)");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, BE_ERR_INVALID, "workspace must be 8-byte aligned");
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_lif_sgp_reduce_tiles, dim3(blocks), dim3(kSgpRedThreads), 0, st, slot, N, partial);
    hipLaunchKernelGGL(k_lif_sgp_reduce_final, dim3(1), dim3(kSgpRedThreads), 0, st, partial, blocks, out);
  } else {
    const int64_t blocks = (P + kSgpRedCols - 1) / kSgpRedCols;
    BE_REQUIRE(blocks <= 0x7fffffff, BE_ERR_INVALID, "the period is too long for one grid");
    hipLaunchKernelGGL(k_lif_sgp_reduce_columns, dim3((unsigned)blocks), dim3(kSgpRedThreads), 0, st, slot, N / P, P, out);
  }
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
