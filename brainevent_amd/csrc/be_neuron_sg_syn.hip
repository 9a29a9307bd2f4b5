// be_neuron_sg_syn.hip — the differentiable LIF neuron with a synaptic current and an optional adaptive threshold (DESIGN.md
// §2.21): one launch runs T time steps of N slots forwards (k_lif_syn_forward), one runs them backwards with a surrogate
// gradient (k_lif_syn_backward).  Per slot a current c, a membrane v and — ADAPT — a spike trace a that raises the threshold.
// Everything is f32; every operation is rounded separately (no FMA contraction), in the order include/brainevent_amd.h states,
// so the result equals the same formulas written as elementwise f32 array operations bit for bit.
//
// The layout is be_neuron_sg.hip's: a slot's T steps form one dependent chain, so a lane keeps its slots for the whole launch
// and the time loop runs inside it.  What the chain does not depend on — x[t] forwards; h[t], th[t], g_s[t], g_vseq[t]
// backwards — is loaded a ring's depth ahead into registers whose indices are compile-time constants (the loop over the ring is
// unrolled: no scratch).  A lane owns S consecutive slots: S = kSynVec with one 16-byte access per array and step where N and
// every given base allow it, S = 1 with 4-byte accesses otherwise.  Reset mode, surrogate and ADAPT are template parameters: the
// instantiation without adaptation holds no a / ca / th registers and moves no th_save.  Plain vector stores only; no atomics,
// no LDS.
#include "be_sg_lane.h"
#include <algorithm>

namespace {

namespace lane = be_sg_lane;

constexpr int kSynThreads = 256;
constexpr int kSynGridCap = 2048;
constexpr int kSynVec = 4;
// One depth for every kernel.  The adaptive 16-byte backward kernel holds the most — four rings (h, th, g_s, g_vseq) and three
// carries of 4 slots each — and at depth 4 stays within 128 VGPRs (4 waves per SIMD) without scratch: DESIGN.md §2.21 has the table.
constexpr int kSynPrefetch = 4;

struct LifSynP {
  float syn_decay, beta, v_th, v_reset, rho, kappa;
  lane::Surrogate sur;
};

// Forward: c0 / v0 / a0 NULL = 0; v_seq / h_save / th_save may be NULL (uniform branches outside the arithmetic).  Without ADAPT
// a0, th_save and a_last are not touched.
template <int S, bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kSynThreads) k_lif_syn_forward(const float* __restrict__ x, const float* __restrict__ c0,
                                                                 const float* __restrict__ v0, const float* __restrict__ a0,
                                                                 float* __restrict__ s_out, float* __restrict__ v_seq,
                                                                 float* __restrict__ h_save, float* __restrict__ th_save,
                                                                 float* __restrict__ c_last, float* __restrict__ v_last,
                                                                 float* __restrict__ a_last, int64_t T, int64_t N, LifSynP p) {
#pragma clang fp contract(off)
  using V = lane::Vals<S>;
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    V c = lane::load_or_zero<S>(c0, i);
    V v = lane::load_or_zero<S>(v0, i);
    V a = lane::zero<S>();
    if (ADAPT) a = lane::load_or_zero<S>(a0, i);
    V ring[kSynPrefetch];
#pragma unroll
    for (int r = 0; r < kSynPrefetch; ++r)
      if (r < T) ring[r] = lane::load<S>(x + (int64_t)r * N + i);
    for (int64_t t0 = 0; t0 < T; t0 += kSynPrefetch) {
#pragma unroll
      for (int r = 0; r < kSynPrefetch; ++r) {
        const int64_t t = t0 + r;
        if (t < T) {
          const V xv = ring[r];
          if (t + kSynPrefetch < T) ring[r] = lane::load<S>(x + (t + kSynPrefetch) * N + i);
          V sv, hv, thv;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            c.f[j] = (p.syn_decay * c.f[j]) + xv.f[j];
            const float h = (p.beta * v.f[j]) + c.f[j];
            const float th = ADAPT ? p.v_th + (p.kappa * a.f[j]) : p.v_th;
            const bool s = h >= th;
            v.f[j] = HARD ? (s ? p.v_reset : h) : (s ? h - p.v_th : h);
            if (ADAPT) a.f[j] = (p.rho * a.f[j]) + (s ? 1.0f : 0.0f);
            sv.f[j] = s ? 1.0f : 0.0f;
            hv.f[j] = h;
            thv.f[j] = th;
          }
          lane::store<S>(s_out + t * N + i, sv);
          if (v_seq != nullptr) lane::store<S>(v_seq + t * N + i, v);
          if (h_save != nullptr) {
            lane::store<S>(h_save + t * N + i, hv);
            if (ADAPT) lane::store<S>(th_save + t * N + i, thv);
          }
        }
      }
    }
    lane::store<S>(c_last + i, c);
    lane::store<S>(v_last + i, v);
    if (ADAPT) lane::store<S>(a_last + i, a);
  }
}

// Backward: g_s / g_vseq / g_clast / g_vlast / g_alast NULL = 0; g_c0 / g_v0 / g_a0 may be NULL.  Without ADAPT th_save, g_alast
// and g_a0 are not touched.
template <int S, bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kSynThreads)
k_lif_syn_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ g_s,
                   const float* __restrict__ g_vseq, const float* __restrict__ g_clast, const float* __restrict__ g_vlast,
                   const float* __restrict__ g_alast, float* __restrict__ g_x, float* __restrict__ g_c0, float* __restrict__ g_v0,
                   float* __restrict__ g_a0, int64_t T, int64_t N, int detach_reset, LifSynP p) {
#pragma clang fp contract(off)
  using V = lane::Vals<S>;
  constexpr int P = kSynPrefetch;
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    V cc = lane::load_or_zero<S>(g_clast, i);
    V cv = lane::load_or_zero<S>(g_vlast, i);
    V ca = lane::zero<S>();
    if (ADAPT) ca = lane::load_or_zero<S>(g_alast, i);
    V ring_h[P], ring_t[ADAPT ? P : 1], ring_s[P], ring_v[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
      ring_s[r] = lane::zero<S>();
      ring_v[r] = lane::zero<S>();
      if (r < T) {
        const int64_t off = (T - 1 - r) * N + i;
        ring_h[r] = lane::load<S>(h_save + off);
        if (ADAPT) ring_t[r] = lane::load<S>(th_save + off);
        if (g_s != nullptr) ring_s[r] = lane::load<S>(g_s + off);
        if (g_vseq != nullptr) ring_v[r] = lane::load<S>(g_vseq + off);
      }
    }
    for (int64_t k0 = 0; k0 < T; k0 += P) {
#pragma unroll
      for (int r = 0; r < P; ++r) {
        const int64_t k = k0 + r;        // the k-th step from the end: t = T - 1 - k
        if (k < T) {
          const V hv = ring_h[r], gsv = ring_s[r], gvv = ring_v[r];
          V tv;
          if (ADAPT) tv = ring_t[r];
          if (k + P < T) {
            const int64_t off = (T - 1 - k - P) * N + i;
            ring_h[r] = lane::load<S>(h_save + off);
            if (ADAPT) ring_t[r] = lane::load<S>(th_save + off);
            if (g_s != nullptr) ring_s[r] = lane::load<S>(g_s + off);
            if (g_vseq != nullptr) ring_v[r] = lane::load<S>(g_vseq + off);
          }
          V gx;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float h = hv.f[j];
            const float th = ADAPT ? tv.f[j] : p.v_th;
            const bool s = h >= th;
            const float u = h - th;
            float g_vo = cv.f[j];
            if (g_vseq != nullptr) g_vo = g_vo + gvv.f[j];
            const float sg = lane::derivative<SG>(u, p.sur);
            float g_sp = gsv.f[j];                       // 0 when g_s is NULL
            if (ADAPT) g_sp = g_sp + ca.f[j];
            if (!detach_reset) g_sp = HARD ? g_sp + g_vo * (p.v_reset - h) : g_sp - g_vo * p.v_th;
            const float g_u = g_sp * sg;
            const float g_h = g_u + (HARD ? (s ? 0.0f : g_vo) : g_vo);
            const float g_c = cc.f[j] + g_h;
            gx.f[j] = g_c;
            cc.f[j] = p.syn_decay * g_c;
            cv.f[j] = p.beta * g_h;
            if (ADAPT) ca.f[j] = (p.rho * ca.f[j]) - (p.kappa * g_u);
          }
          lane::store<S>(g_x + (T - 1 - k) * N + i, gx);
        }
      }
    }
    if (g_c0 != nullptr) lane::store<S>(g_c0 + i, cc);
    if (g_v0 != nullptr) lane::store<S>(g_v0 + i, cv);
    if (ADAPT && g_a0 != nullptr) lane::store<S>(g_a0 + i, ca);
  }
}

inline int syn_grid(int64_t N, int S) {
  const int64_t groups = N / S;
  return (int)std::min<int64_t>((groups + kSynThreads - 1) / kSynThreads, kSynGridCap);
}

template <typename... Ptr>
inline bool syn_all_aligned16(Ptr... ptrs) {
  return (lane::aligned16(ptrs) && ...);
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int syn_check_common(const char* who, int64_t T, int64_t N, int reset_mode) {
  const char* msg = (T < 0 || N < 0) ? ": T < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode" : nullptr;
  if (msg == nullptr) return BE_OK;
  be_set_error(std::string(who) + msg);
  return BE_ERR_INVALID;
}

template <int S, typename... Args>
void syn_launch_forward(bool hard, bool adaptive, int grid, hipStream_t st, Args... args) {
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adaptive, [&](auto A) {
      hipLaunchKernelGGL((k_lif_syn_forward<S, decltype(H)::value, decltype(A)::value>), dim3(grid), dim3(kSynThreads), 0, st, args...);
      return BE_OK;
    });
  });
}

template <int S, typename... Args>
void syn_launch_backward(bool hard, int surrogate, bool adaptive, int grid, hipStream_t st, Args... args) {
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adaptive, [&](auto A) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        hipLaunchKernelGGL((k_lif_syn_backward<S, decltype(H)::value, decltype(SG)::value, decltype(A)::value>), dim3(grid),
                           dim3(kSynThreads), 0, st, args...);
        return BE_OK;
      });
    });
  });
}

}  // namespace

extern "C" {

int be_lif_syn_sg_forward(const float* x, const float* c0, const float* v0, const float* a0, float* s_out, float* v_seq,
                          float* h_save, float* th_save, float* c_last, float* v_last, float* a_last, int64_t T, int64_t N,
                          double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                          int adaptive, be_stream_t stream) {
  if (const int rc = syn_check_common(__func__, T, N, reset_mode)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const LifSynP p{(float)syn_decay, (float)beta, (float)v_th, (float)v_reset, (float)rho, (float)kappa, lane::make_surrogate(1.0)};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const bool vec = (N % kSynVec == 0) && syn_all_aligned16(x, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = syn_grid(N, vec ? kSynVec : 1);
  if (vec) syn_launch_forward<kSynVec>(hard, adapt, grid, st, x, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, N, p);
  else syn_launch_forward<1>(hard, adapt, grid, st, x, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, N, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_syn_sg_backward(const float* h_save, const float* th_save, const float* g_s, const float* g_vseq, const float* g_clast,
                           const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0, float* g_a0, int64_t T,
                           int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa,
                           int reset_mode, int surrogate, double alpha, int adaptive, int detach_reset, be_stream_t stream) {
  if (const int rc = syn_check_common(__func__, T, N, reset_mode)) return rc;
  BE_REQUIRE(surrogate == BE_LIF_SG_FAST_SIGMOID || surrogate == BE_LIF_SG_ATAN || surrogate == BE_LIF_SG_TRIANGLE, BE_ERR_INVALID,
             "unknown surrogate");
  BE_REQUIRE(alpha > 0., BE_ERR_INVALID, "alpha must be positive");
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  // derived constants in double, rounded to f32 once
  const LifSynP p{(float)syn_decay, (float)beta, (float)v_th, (float)v_reset, (float)rho, (float)kappa, lane::make_surrogate(alpha)};
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const bool vec = (N % kSynVec == 0) && syn_all_aligned16(h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = syn_grid(N, vec ? kSynVec : 1);
  const int detach = detach_reset != 0;
  if (vec)
    syn_launch_backward<kSynVec>(hard, surrogate, adapt, grid, st, h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0,
                                 g_v0, g_a0, T, N, detach, p);
  else
    syn_launch_backward<1>(hard, surrogate, adapt, grid, st, h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0,
                           g_a0, T, N, detach, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
