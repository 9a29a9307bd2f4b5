// be_neuron_sg.hip — the differentiable leaky integrate-and-fire neuron: one launch runs T time steps of N
// neuron slots forwards (k_lif_sg_forward) and one runs them backwards with a surrogate gradient (k_lif_sg_backward).  The
// single step is T = 1 of the same kernels.  Everything is f32; every operation is rounded separately (no FMA contraction),
// in the order include/brainevent_amd.h states, so the result equals the same formulas written as elementwise f32 array
// operations bit for bit.
//
// A slot's T steps form one dependent chain, so a lane keeps its slots for the whole launch and the time loop runs inside
// it.  What the chain does not depend on — x[t] forwards; h[t], g_s[t], g_vseq[t] backwards — is loaded kSgPrefetch steps
// ahead into a register ring whose indices are compile-time constants (the loop over the ring is unrolled: no scratch).
// A lane owns S consecutive slots: S = kSgVec with one 16-byte load / store per array and step where N and every base
// allow it (then every row t * N of a [T, N] array is 16-byte aligned too), S = 1 with 4-byte accesses otherwise.  Plain
// vector stores only; no atomics, no LDS.
#include "be_common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kSgThreads = 256;
constexpr int kSgGridCap = 2048;
constexpr int kSgVec = 4;
constexpr int kSgPrefetch = 4;

template <int S> struct SgPack;
template <> struct SgPack<1> { using type = float; };
template <> struct SgPack<4> { using type = float4; };

template <int S>
struct SgVals {
  float f[S];
};

template <int S>
__device__ __forceinline__ SgVals<S> sg_load(const float* __restrict__ p) {
  using P = typename SgPack<S>::type;
  const P raw = *reinterpret_cast<const P*>(p);
  SgVals<S> out;
  __builtin_memcpy(out.f, &raw, sizeof(P));
  return out;
}

template <int S>
__device__ __forceinline__ void sg_store(float* __restrict__ p, const SgVals<S>& v) {
  using P = typename SgPack<S>::type;
  P raw;
  __builtin_memcpy(&raw, v.f, sizeof(P));
  *reinterpret_cast<P*>(p) = raw;
}

template <int S>
__device__ __forceinline__ SgVals<S> sg_zero() {
  SgVals<S> out;
#pragma unroll
  for (int j = 0; j < S; ++j) out.f[j] = 0.f;
  return out;
}

struct LifSgP {
  float beta, v_th, v_reset, alpha, atan_c, atan_half;
};

// Forward: v_seq / h_save may be NULL (uniform branches outside the arithmetic), v0 NULL = 0.
template <int S, bool HARD>
__global__ void __launch_bounds__(kSgThreads) k_lif_sg_forward(const float* __restrict__ x, const float* __restrict__ v0,
                                                               float* __restrict__ s_out, float* __restrict__ v_seq,
                                                               float* __restrict__ h_save, float* __restrict__ v_last,
                                                               int64_t T, int64_t N, LifSgP p) {
#pragma clang fp contract(off)
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    SgVals<S> v = v0 != nullptr ? sg_load<S>(v0 + i) : sg_zero<S>();
    SgVals<S> ring[kSgPrefetch];
#pragma unroll
    for (int r = 0; r < kSgPrefetch; ++r)
      if (r < T) ring[r] = sg_load<S>(x + (int64_t)r * N + i);
    for (int64_t t0 = 0; t0 < T; t0 += kSgPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgPrefetch; ++r) {
        const int64_t t = t0 + r;
        if (t < T) {
          const SgVals<S> xv = ring[r];
          if (t + kSgPrefetch < T) ring[r] = sg_load<S>(x + (t + kSgPrefetch) * N + i);
          SgVals<S> sv, hv;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float h = (p.beta * v.f[j]) + xv.f[j];
            const bool s = h >= p.v_th;
            v.f[j] = HARD ? (s ? p.v_reset : h) : (s ? h - p.v_th : h);
            sv.f[j] = s ? 1.0f : 0.0f;
            hv.f[j] = h;
          }
          sg_store<S>(s_out + t * N + i, sv);
          if (v_seq != nullptr) sg_store<S>(v_seq + t * N + i, v);
          if (h_save != nullptr) sg_store<S>(h_save + t * N + i, hv);
        }
      }
    }
    sg_store<S>(v_last + i, v);
  }
}

// the surrogate's derivative at u = h - v_th (SG: BE_LIF_SG_*)
template <int SG>
__device__ __forceinline__ float sg_derivative(float u, const LifSgP& p) {
#pragma clang fp contract(off)
  if (SG == 0) {                    // fast sigmoid
    const float d = 1.0f + p.alpha * fabsf(u);
    return 1.0f / (d * d);
  }
  if (SG == 1) {                    // arctangent
    const float q = p.atan_c * u;
    return p.atan_half / (1.0f + q * q);
  }
  const float a = 1.0f - p.alpha * fabsf(u);     // triangle; a NaN compares false: 0, as fmaxf(0, NaN)
  return p.alpha * (a > 0.0f ? a : 0.0f);
}

// Backward: g_s / g_vseq / g_vlast / g_v0 may be NULL.
template <int S, bool HARD, int SG>
__global__ void __launch_bounds__(kSgThreads) k_lif_sg_backward(const float* __restrict__ h_save, const float* __restrict__ g_s,
                                                                const float* __restrict__ g_vseq, const float* __restrict__ g_vlast,
                                                                float* __restrict__ g_x, float* __restrict__ g_v0, int64_t T,
                                                                int64_t N, int detach_reset, LifSgP p) {
#pragma clang fp contract(off)
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    SgVals<S> carry = g_vlast != nullptr ? sg_load<S>(g_vlast + i) : sg_zero<S>();
    SgVals<S> ring_h[kSgPrefetch], ring_s[kSgPrefetch], ring_v[kSgPrefetch];
#pragma unroll
    for (int r = 0; r < kSgPrefetch; ++r) {
      ring_s[r] = sg_zero<S>();
      ring_v[r] = sg_zero<S>();
      if (r < T) {
        const int64_t off = (T - 1 - r) * N + i;
        ring_h[r] = sg_load<S>(h_save + off);
        if (g_s != nullptr) ring_s[r] = sg_load<S>(g_s + off);
        if (g_vseq != nullptr) ring_v[r] = sg_load<S>(g_vseq + off);
      }
    }
    for (int64_t k0 = 0; k0 < T; k0 += kSgPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgPrefetch; ++r) {
        const int64_t k = k0 + r;        // the k-th step from the end: t = T - 1 - k
        if (k < T) {
          const SgVals<S> hv = ring_h[r], gsv = ring_s[r], gvv = ring_v[r];
          if (k + kSgPrefetch < T) {
            const int64_t off = (T - 1 - k - kSgPrefetch) * N + i;
            ring_h[r] = sg_load<S>(h_save + off);
            if (g_s != nullptr) ring_s[r] = sg_load<S>(g_s + off);
            if (g_vseq != nullptr) ring_v[r] = sg_load<S>(g_vseq + off);
          }
          SgVals<S> gx;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float h = hv.f[j];
            const bool s = h >= p.v_th;
            const float u = h - p.v_th;
            float g_vo = carry.f[j];
            if (g_vseq != nullptr) g_vo = g_vo + gvv.f[j];
            const float sg = sg_derivative<SG>(u, p);
            float g_sp = gsv.f[j];                       // 0 when g_s is NULL
            if (!detach_reset) g_sp = HARD ? g_sp + g_vo * (p.v_reset - h) : g_sp - g_vo * p.v_th;
            const float g_h = g_sp * sg + (HARD ? (s ? 0.0f : g_vo) : g_vo);
            gx.f[j] = g_h;
            carry.f[j] = p.beta * g_h;
          }
          sg_store<S>(g_x + (T - 1 - k) * N + i, gx);
        }
      }
    }
    if (g_v0 != nullptr) sg_store<S>(g_v0 + i, carry);
  }
}

inline bool sg_aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

inline int sg_grid(int64_t N, int S) {
  const int64_t groups = N / S;
  return (int)std::min<int64_t>((groups + kSgThreads - 1) / kSgThreads, kSgGridCap);
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int sg_check_common(const char* who, int64_t T, int64_t N, int reset_mode) {
  const char* msg = (T < 0 || N < 0) ? ": T < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode" : nullptr;
  if (msg == nullptr) return BE_OK;
  be_set_error(std::string(who) + msg);
  return BE_ERR_INVALID;
}

template <int S, bool HARD>
void sg_launch_backward(int surrogate, int grid, hipStream_t st, const float* h_save, const float* g_s, const float* g_vseq,
                        const float* g_vlast, float* g_x, float* g_v0, int64_t T, int64_t N, int detach_reset, const LifSgP& p) {
  if (surrogate == BE_LIF_SG_FAST_SIGMOID)
    hipLaunchKernelGGL((k_lif_sg_backward<S, HARD, 0>), dim3(grid), dim3(kSgThreads), 0, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0,
                       T, N, detach_reset, p);
  else if (surrogate == BE_LIF_SG_ATAN)
    hipLaunchKernelGGL((k_lif_sg_backward<S, HARD, 1>), dim3(grid), dim3(kSgThreads), 0, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0,
                       T, N, detach_reset, p);
  else
    hipLaunchKernelGGL((k_lif_sg_backward<S, HARD, 2>), dim3(grid), dim3(kSgThreads), 0, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0,
                       T, N, detach_reset, p);
}

}  // namespace

extern "C" {

int be_lif_sg_forward(const float* x, const float* v0, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T,
                      int64_t N, double beta, double v_th, double v_reset, int reset_mode, be_stream_t stream) {
  if (const int rc = sg_check_common(__func__, T, N, reset_mode)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && v_last, BE_ERR_INVALID, "null pointer (x, s_out and v_last are required)");
  const LifSgP p{(float)beta, (float)v_th, (float)v_reset, 0.f, 0.f, 0.f};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  const bool vec = (N % kSgVec == 0) && sg_aligned16(x) && sg_aligned16(v0) && sg_aligned16(s_out) && sg_aligned16(v_seq) &&
                   sg_aligned16(h_save) && sg_aligned16(v_last);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = sg_grid(N, vec ? kSgVec : 1);
  if (vec && hard)
    hipLaunchKernelGGL((k_lif_sg_forward<kSgVec, true>), dim3(grid), dim3(kSgThreads), 0, st, x, v0, s_out, v_seq, h_save, v_last, T, N, p);
  else if (vec)
    hipLaunchKernelGGL((k_lif_sg_forward<kSgVec, false>), dim3(grid), dim3(kSgThreads), 0, st, x, v0, s_out, v_seq, h_save, v_last, T, N, p);
  else if (hard)
    hipLaunchKernelGGL((k_lif_sg_forward<1, true>), dim3(grid), dim3(kSgThreads), 0, st, x, v0, s_out, v_seq, h_save, v_last, T, N, p);
  else
    hipLaunchKernelGGL((k_lif_sg_forward<1, false>), dim3(grid), dim3(kSgThreads), 0, st, x, v0, s_out, v_seq, h_save, v_last, T, N, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_sg_backward(const float* h_save, const float* g_s, const float* g_vseq, const float* g_vlast, float* g_x, float* g_v0,
                       int64_t T, int64_t N, double beta, double v_th, double v_reset, int reset_mode, int surrogate, double alpha,
                       int detach_reset, be_stream_t stream) {
  if (const int rc = sg_check_common(__func__, T, N, reset_mode)) return rc;
  BE_REQUIRE(surrogate == BE_LIF_SG_FAST_SIGMOID || surrogate == BE_LIF_SG_ATAN || surrogate == BE_LIF_SG_TRIANGLE, BE_ERR_INVALID,
             "unknown surrogate");
  BE_REQUIRE(alpha > 0., BE_ERR_INVALID, "alpha must be positive");
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  // derived constants in double, rounded to f32 once
  const LifSgP p{(float)beta, (float)v_th, (float)v_reset, (float)alpha, (float)(M_PI / 2 * alpha), (float)(alpha / 2)};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  const bool vec = (N % kSgVec == 0) && sg_aligned16(h_save) && sg_aligned16(g_s) && sg_aligned16(g_vseq) && sg_aligned16(g_vlast) &&
                   sg_aligned16(g_x) && sg_aligned16(g_v0);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = sg_grid(N, vec ? kSgVec : 1);
  const int detach = detach_reset != 0;
  if (vec && hard) sg_launch_backward<kSgVec, true>(surrogate, grid, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0, T, N, detach, p);
  else if (vec) sg_launch_backward<kSgVec, false>(surrogate, grid, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0, T, N, detach, p);
  else if (hard) sg_launch_backward<1, true>(surrogate, grid, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0, T, N, detach, p);
  else sg_launch_backward<1, false>(surrogate, grid, st, h_save, g_s, g_vseq, g_vlast, g_x, g_v0, T, N, detach, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
