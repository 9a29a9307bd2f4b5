// be_neuron_sg.hip — the differentiable leaky integrate-and-fire neuron in every feed-forward model (DESIGN.md §2.19 – §2.21,
// §2.23, §2.24): one launch runs T time steps of N neuron slots forwards (k_lif_lane_forward) and one runs them backwards with a
// surrogate gradient (k_lif_lane_backward).  The single step is T = 1 of the same kernels.  One kernel pair serves every
// model, chosen at compile time: the plain LIF (beta, v_th constants), PARAMS (beta[i % beta_period], v_th[i % vth_period] read
// from DEVICE memory, and the per-slot accumulators of their gradients, which be_neuron_sg_reduce.hip sums), SYN (a synaptic
// current c per slot) and SYN + ADAPT (a spike trace a per slot that raises the threshold); SYN (+ ADAPT) with PARAMS reads
// syn_decay (rho, kappa) from device memory as well and keeps their accumulators (§2.24).  What a model does not have costs its
// instantiation nothing: no register, no load, no store.  Everything is f32; every operation is rounded separately (no FMA
// contraction), in the order include/brainevent_amd.h states — the arithmetic itself is be_sg_lane.h's — so the result equals
// the same formulas written as elementwise f32 array operations bit for bit.
//
// A slot's T steps form one dependent chain, so a lane keeps its slots for the whole launch and the time loop runs inside
// it.  What the chain does not depend on — x[t] forwards; h[t], th[t], g_s[t], g_vseq[t] backwards — is loaded kSgPrefetch steps
// ahead into a register ring whose indices are compile-time constants (the loop over the ring is unrolled: no scratch).
// A lane owns S consecutive slots: S = kSgVec with one 16-byte load / store per array and step where N, every given base and
// every period allow it (then every row t * N of a [T, N] array is 16-byte aligned too; a period is 1, or a multiple of kSgVec
// with an aligned base: then i % period is a multiple of kSgVec and the S values are consecutive), S = 1 with 4-byte accesses
// otherwise.  Plain vector stores only; no atomics, no LDS.
#include "be_sg_lane.h"
#include <algorithm>

namespace {

namespace lane = be_sg_lane;

constexpr int kSgThreads = 256;
constexpr int kSgGridCap = 2048;
constexpr int kSgVec = 4;
// One depth for every kernel.  Without PARAMS the adaptive 16-byte backward kernel holds the most — four rings (h, th, g_s, g_vseq)
// and three carries of 4 slots each — and at depth 4 stays within 128 VGPRs (4 waves per SIMD) without scratch: DESIGN.md §2.23 has
// the table.  With PARAMS it adds a ring (c_save), five parameter vectors and five accumulators: 206 – 208 VGPRs, 2 waves, no
// scratch, and still faster than its 4-byte kernel (measured: §2.24).
constexpr int kSgPrefetch = 4;

// what a slot carries and where beta / v_th come from
template <bool SYN_, bool ADAPT_, bool PARAMS_>
struct Model {
  static constexpr bool SYN = SYN_, ADAPT = ADAPT_, PARAMS = PARAMS_;
  static_assert(!ADAPT || SYN, "the adaptive threshold exists for the synaptic neuron");
  // with PARAMS the synaptic neuron reads syn_decay too, the adaptive one rho and kappa, each with a period of its own
  static constexpr bool PSYN = PARAMS && SYN, PADAPT = PARAMS && ADAPT;
};
using Plain = Model<false, false, false>;
using PerSlot = Model<false, false, true>;
template <bool ADAPT>
using Synaptic = Model<true, ADAPT, false>;
template <bool ADAPT>
using SynapticPerSlot = Model<true, ADAPT, true>;

// the constants a slot's step reads: the kernel's, with the slot's own syn_decay, rho and kappa where the model has them in memory
// (no arithmetic; everything else passes p through untouched)
template <class M>
__device__ __forceinline__ lane::LifP slot_constants(const lane::LifP& p, float syn_decay, float rho, float kappa) {
  lane::LifP q = p;
  if (M::PSYN) q.syn_decay = syn_decay;
  if (M::PADAPT) q.rho = rho, q.kappa = kappa;
  return q;
}

// Forward: c0 / v0 / a0 NULL = 0; v_seq / h_save / th_save / c_save may be NULL (uniform branches outside the arithmetic).  Without
// SYN c0 and c_last, without ADAPT a0, th_save and a_last, without PARAMS beta and vth, without PARAMS and SYN sd and c_save,
// without PARAMS and ADAPT rho and kappa are not touched.  With PARAMS and ADAPT th_save takes the trace a the step STARTED from
// (the entry point's a_save) in the threshold's place: the backward pass forms th from it with the same two operations.
template <int S, bool HARD, class M>
__global__ void __launch_bounds__(kSgThreads)
k_lif_lane_forward(const float* __restrict__ x, const float* __restrict__ c0, const float* __restrict__ v0,
                   const float* __restrict__ a0, lane::ParamArr sd, lane::ParamArr beta, lane::ParamArr vth, lane::ParamArr rho,
                   lane::ParamArr kappa, float* __restrict__ s_out, float* __restrict__ v_seq, float* __restrict__ h_save,
                   float* __restrict__ th_save, float* __restrict__ c_save, float* __restrict__ c_last, float* __restrict__ v_last,
                   float* __restrict__ a_last, int64_t T, int64_t N, lane::LifP p) {
#pragma clang fp contract(off)
  using V = lane::Vals<S>;
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    // beta and the base threshold of the lane's slots: the slot's own, or the uniform kernel argument (no register of its own)
    const V bv = M::PARAMS ? lane::load_param<S>(beta, i) : lane::fill<S>(p.beta);
    const V tv = M::PARAMS ? lane::load_param<S>(vth, i) : lane::fill<S>(p.v_th);
    const V sdv = M::PSYN ? lane::load_param<S>(sd, i) : lane::fill<S>(p.syn_decay);
    const V rv = M::PADAPT ? lane::load_param<S>(rho, i) : lane::fill<S>(p.rho);
    const V kv = M::PADAPT ? lane::load_param<S>(kappa, i) : lane::fill<S>(p.kappa);
    V c = lane::zero<S>(), a = lane::zero<S>();
    if (M::SYN) c = lane::load_or_zero<S>(c0, i);
    V v = lane::load_or_zero<S>(v0, i);
    if (M::ADAPT) a = lane::load_or_zero<S>(a0, i);
    V ring[kSgPrefetch];
#pragma unroll
    for (int r = 0; r < kSgPrefetch; ++r)
      if (r < T) ring[r] = lane::load<S>(x + (int64_t)r * N + i);
    for (int64_t t0 = 0; t0 < T; t0 += kSgPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgPrefetch; ++r) {
        const int64_t t = t0 + r;
        if (t < T) {
          const V xv = ring[r];
          if (t + kSgPrefetch < T) ring[r] = lane::load<S>(x + (t + kSgPrefetch) * N + i);
          V sv, hv, thv;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const lane::LifP q = slot_constants<M>(p, sdv.f[j], rv.f[j], kv.f[j]);
            const float a_in = a.f[j];
            const lane::Fired f = lane::forward_step<HARD, M::SYN, M::ADAPT>(xv.f[j], c.f[j], v.f[j], a.f[j], bv.f[j], tv.f[j], q);
            sv.f[j] = f.s ? 1.0f : 0.0f;
            hv.f[j] = f.h;
            thv.f[j] = M::PADAPT ? a_in : f.th;
          }
          lane::store<S>(s_out + t * N + i, sv);
          if (v_seq != nullptr) lane::store<S>(v_seq + t * N + i, v);
          if (h_save != nullptr) {
            lane::store<S>(h_save + t * N + i, hv);
            if (M::ADAPT) lane::store<S>(th_save + t * N + i, thv);
          }
          if (M::PSYN && c_save != nullptr) lane::store<S>(c_save + t * N + i, c);
        }
      }
    }
    if (M::SYN) lane::store<S>(c_last + i, c);
    lane::store<S>(v_last + i, v);
    if (M::ADAPT) lane::store<S>(a_last + i, a);
  }
}

// Backward: g_s / g_vseq / g_clast / g_vlast / g_alast NULL = 0; g_c0 / g_v0 / g_a0 and the five slot arrays may be NULL.
// Without SYN g_clast and g_c0, without ADAPT th_save, g_alast and g_a0, without PARAMS beta, vth, v0 and the slot arrays are
// not touched; v0 (NULL = 0) is read only for g_beta_slot.  PARAMS keeps, per slot, the two f32 accumulators of the parameters'
// gradients — a_b += g_h * v_prev and a_th -= g_u (+ the soft reset's direct term) — where v_prev is the membrane the step
// started from, recomputed from h[t-1], which the ring already holds (v0 at t = 0).  PARAMS and SYN adds a_sd += g_c * c_prev
// (c_prev: c_save[t-1] from a ring of its own, c0 at t = 0; both read only for g_sd_slot); PARAMS and ADAPT has th_save hold the
// trace a_in each step started from, forms th = vth_i + (kappa_i * a_in) from it — for step t and, to decide v_prev, for step
// t - 1 — and adds a_k -= g_u * a_in and a_r += ca * a_in with the carry ca that ARRIVES at the step.
template <int S, bool HARD, int SG, class M>
__global__ void __launch_bounds__(kSgThreads)
k_lif_lane_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ c_save,
                    const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ g_s,
                    const float* __restrict__ g_vseq, const float* __restrict__ g_clast, const float* __restrict__ g_vlast,
                    const float* __restrict__ g_alast, lane::ParamArr sd, lane::ParamArr beta, lane::ParamArr vth, lane::ParamArr rho,
                    lane::ParamArr kappa, float* __restrict__ g_x, float* __restrict__ g_c0, float* __restrict__ g_v0,
                    float* __restrict__ g_a0, float* __restrict__ g_sd_slot, float* __restrict__ g_beta_slot,
                    float* __restrict__ g_vth_slot, float* __restrict__ g_rho_slot, float* __restrict__ g_kappa_slot, int64_t T, int64_t N,
                    int detach_reset, lane::LifP p) {
#pragma clang fp contract(off)
  using V = lane::Vals<S>;
  const int64_t groups = N / S;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i = g * S;
    // beta and the base threshold of the lane's slots: the slot's own, or the uniform kernel argument (no register of its own)
    const V bv = M::PARAMS ? lane::load_param<S>(beta, i) : lane::fill<S>(p.beta);
    const V tv = M::PARAMS ? lane::load_param<S>(vth, i) : lane::fill<S>(p.v_th);
    const V sdv = M::PSYN ? lane::load_param<S>(sd, i) : lane::fill<S>(p.syn_decay);
    const V rv = M::PADAPT ? lane::load_param<S>(rho, i) : lane::fill<S>(p.rho);
    const V kv = M::PADAPT ? lane::load_param<S>(kappa, i) : lane::fill<S>(p.kappa);
    V cc = lane::zero<S>(), ca = lane::zero<S>();
    if (M::SYN) cc = lane::load_or_zero<S>(g_clast, i);
    V cv = lane::load_or_zero<S>(g_vlast, i);
    if (M::ADAPT) ca = lane::load_or_zero<S>(g_alast, i);
    V acc_b = lane::zero<S>(), acc_t = lane::zero<S>(), acc_sd = lane::zero<S>(), acc_r = lane::zero<S>(), acc_k = lane::zero<S>();
    V ring_h[kSgPrefetch], ring_t[M::ADAPT ? kSgPrefetch : 1], ring_s[kSgPrefetch], ring_v[kSgPrefetch];
    V ring_c[M::PSYN ? kSgPrefetch : 1];     // c_save, for g_sd_slot alone
#pragma unroll
    for (int r = 0; r < kSgPrefetch; ++r) {
      ring_s[r] = lane::zero<S>();
      ring_v[r] = lane::zero<S>();
      if (r < T) {
        const int64_t off = (T - 1 - r) * N + i;
        ring_h[r] = lane::load<S>(h_save + off);
        if (M::ADAPT) ring_t[r] = lane::load<S>(th_save + off);
        if (g_s != nullptr) ring_s[r] = lane::load<S>(g_s + off);
        if (g_vseq != nullptr) ring_v[r] = lane::load<S>(g_vseq + off);
        if (M::PSYN && g_sd_slot != nullptr) ring_c[r] = lane::load<S>(c_save + off);
      }
    }
    for (int64_t k0 = 0; k0 < T; k0 += kSgPrefetch) {
#pragma unroll
      for (int r = 0; r < kSgPrefetch; ++r) {
        const int64_t k = k0 + r;        // the k-th step from the end: t = T - 1 - k
        if (k < T) {
          const V hv = ring_h[r], gsv = ring_s[r], gvv = ring_v[r];
          V thv = tv;                    // the threshold h was compared with
          if (M::ADAPT) thv = ring_t[r];
          V av = lane::zero<S>();        // PARAMS: the ring holds the trace the step started from, and th is formed as forwards
          if (M::PADAPT) {
            av = thv;
#pragma unroll
            for (int j = 0; j < S; ++j) thv.f[j] = tv.f[j] + (kv.f[j] * av.f[j]);
          }
          if (k + kSgPrefetch < T) {
            const int64_t off = (T - 1 - k - kSgPrefetch) * N + i;
            ring_h[r] = lane::load<S>(h_save + off);
            if (M::ADAPT) ring_t[r] = lane::load<S>(th_save + off);
            if (g_s != nullptr) ring_s[r] = lane::load<S>(g_s + off);
            if (g_vseq != nullptr) ring_v[r] = lane::load<S>(g_vseq + off);
            if (M::PSYN && g_sd_slot != nullptr) ring_c[r] = lane::load<S>(c_save + off);
          }
          // the membrane step t started from: step t - 1 is the next one of the ring (loaded at the start, or, for the
          // ring's last place, refilled at this block's first step); t = 0 started from v0
          V vp = lane::zero<S>();
          if (M::PARAMS && g_beta_slot != nullptr) {
            if (k + 1 < T) {
              const V hp = ring_h[(r + 1) % kSgPrefetch];
              V tp = tv;                 // the threshold step t - 1 compared with: the adaptive one, from its own a_in
              if (M::PADAPT) {
                const V ap = ring_t[(r + 1) % kSgPrefetch];
#pragma unroll
                for (int j = 0; j < S; ++j) tp.f[j] = tv.f[j] + (kv.f[j] * ap.f[j]);
              }
#pragma unroll
              for (int j = 0; j < S; ++j) vp.f[j] = lane::membrane_after<HARD>(hp.f[j], tp.f[j], tv.f[j], p.v_reset);
            } else if (v0 != nullptr) {
              vp = lane::load<S>(v0 + i);
            }
          }
          // the current step t started from, the same way: c_save[t - 1], or c0
          V cp = lane::zero<S>();
          if (M::PSYN && g_sd_slot != nullptr) {
            if (k + 1 < T) {
              cp = ring_c[(r + 1) % kSgPrefetch];
            } else if (c0 != nullptr) {
              cp = lane::load<S>(c0 + i);
            }
          }
          V gx;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            float g_vo = cv.f[j];
            if (g_vseq != nullptr) g_vo = g_vo + gvv.f[j];
            // gsv: 0 when g_s is NULL
            const lane::LifP q = slot_constants<M>(p, sdv.f[j], rv.f[j], kv.f[j]);
            const float ca_in = ca.f[j];
            const lane::Grad d = lane::backward_step<HARD, SG, M::ADAPT>(hv.f[j], thv.f[j], tv.f[j], gsv.f[j], g_vo, ca.f[j], detach_reset, q);
            gx.f[j] = lane::backward_carry<M::SYN, M::ADAPT>(d, cc.f[j], cv.f[j], ca.f[j], bv.f[j], q);
            if (M::PSYN && g_sd_slot != nullptr) acc_sd.f[j] = acc_sd.f[j] + (gx.f[j] * cp.f[j]);
            if (M::PADAPT && g_kappa_slot != nullptr) acc_k.f[j] = acc_k.f[j] - (d.g_u * av.f[j]);
            if (M::PADAPT && g_rho_slot != nullptr) acc_r.f[j] = acc_r.f[j] + (ca_in * av.f[j]);
            if (M::PARAMS && g_beta_slot != nullptr) acc_b.f[j] = acc_b.f[j] + (d.g_h * vp.f[j]);
            if (M::PARAMS && g_vth_slot != nullptr) {
              float direct = d.g_u;
              if (!HARD) direct = direct + (d.s ? g_vo : 0.0f);
              acc_t.f[j] = acc_t.f[j] - direct;
            }
          }
          lane::store<S>(g_x + (T - 1 - k) * N + i, gx);
        }
      }
    }
    if (M::SYN && g_c0 != nullptr) lane::store<S>(g_c0 + i, cc);
    if (g_v0 != nullptr) lane::store<S>(g_v0 + i, cv);
    if (M::ADAPT && g_a0 != nullptr) lane::store<S>(g_a0 + i, ca);
    if (M::PARAMS && g_beta_slot != nullptr) lane::store<S>(g_beta_slot + i, acc_b);
    if (M::PARAMS && g_vth_slot != nullptr) lane::store<S>(g_vth_slot + i, acc_t);
    if (M::PSYN && g_sd_slot != nullptr) lane::store<S>(g_sd_slot + i, acc_sd);
    if (M::PADAPT && g_rho_slot != nullptr) lane::store<S>(g_rho_slot + i, acc_r);
    if (M::PADAPT && g_kappa_slot != nullptr) lane::store<S>(g_kappa_slot + i, acc_k);
  }
}

// ---------------------------------------------------------------------------------------------- host side
// a parameter array allows the 16-byte kernel: one shared value, or groups of kSgVec that never wrap
inline bool param_vec(const float* p, int64_t period) {
  return period == 1 || (period % kSgVec == 0 && lane::aligned16(p));
}

inline int lane_grid(int64_t N, int S) {
  const int64_t groups = N / S;
  return (int)std::min<int64_t>((groups + kSgThreads - 1) / kSgThreads, kSgGridCap);
}

// what stands in a kernel's argument list for an array the model does not have
constexpr const float* kNoIn = nullptr;
constexpr float* kNoOut = nullptr;
constexpr lane::ParamArr kNoParam{nullptr, 1};

// args: the kernel's, in its order
template <class M, typename... Args>
void launch_forward(bool vec, bool hard, int64_t N, hipStream_t st, Args... args) {
  be_dispatch_bool(vec, [&](auto V) {
    return be_dispatch_bool(hard, [&](auto H) {
      constexpr int S = decltype(V)::value ? kSgVec : 1;
      hipLaunchKernelGGL((k_lif_lane_forward<S, decltype(H)::value, M>), dim3(lane_grid(N, S)), dim3(kSgThreads), 0, st, args...);
      return BE_OK;
    });
  });
}

template <class M, typename... Args>
void launch_backward(bool vec, bool hard, int surrogate, int64_t N, hipStream_t st, Args... args) {
  be_dispatch_bool(vec, [&](auto V) {
    return be_dispatch_bool(hard, [&](auto H) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        constexpr int S = decltype(V)::value ? kSgVec : 1;
        hipLaunchKernelGGL((k_lif_lane_backward<S, decltype(H)::value, decltype(SG)::value, M>), dim3(lane_grid(N, S)),
                           dim3(kSgThreads), 0, st, args...);
        return BE_OK;
      });
    });
  });
}

}  // namespace

extern "C" {

int be_lif_sg_forward(const float* x, const float* v0, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T,
                      int64_t N, double beta, double v_th, double v_reset, int reset_mode, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && v_last, BE_ERR_INVALID, "null pointer (x, s_out and v_last are required)");
  const lane::LifP p = lane::make_params(0., beta, v_th, v_reset, 0., 0., 1.);
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, v0, s_out, v_seq, h_save, v_last);
  launch_forward<Plain>(vec, reset_mode == BE_LIF_RESET_HARD, N, static_cast<hipStream_t>(stream), x, kNoIn, v0, kNoIn, kNoParam,
                        kNoParam, kNoParam, kNoParam, kNoParam, s_out, v_seq, h_save, kNoOut, kNoOut, kNoOut, v_last, kNoOut, T, N, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_sg_backward(const float* h_save, const float* g_s, const float* g_vseq, const float* g_vlast, float* g_x, float* g_v0,
                       int64_t T, int64_t N, double beta, double v_th, double v_reset, int reset_mode, int surrogate, double alpha,
                       int detach_reset, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  const lane::LifP p = lane::make_params(0., beta, v_th, v_reset, 0., 0., alpha);
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, g_s, g_vseq, g_vlast, g_x, g_v0);
  launch_backward<Plain>(vec, reset_mode == BE_LIF_RESET_HARD, surrogate, N, static_cast<hipStream_t>(stream), h_save, kNoIn, kNoIn,
                         kNoIn, kNoIn, g_s, g_vseq, kNoIn, g_vlast, kNoIn, kNoParam, kNoParam, kNoParam, kNoParam, kNoParam, g_x, kNoOut,
                         g_v0, kNoOut, kNoOut, kNoOut, kNoOut, kNoOut, kNoOut, T, N, (int)(detach_reset != 0), p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_sg_forward_params(const float* x, const float* v0, const float* beta, int64_t beta_period, const float* v_th,
                             int64_t vth_period, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T, int64_t N,
                             double v_reset, int reset_mode, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode, beta_period, vth_period)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && beta && v_th && s_out && v_last, BE_ERR_INVALID, "null pointer (x, beta, v_th, s_out and v_last are required)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., 1.);
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, v0, s_out, v_seq, h_save, v_last) && param_vec(beta, beta_period) &&
                   param_vec(v_th, vth_period);
  launch_forward<PerSlot>(vec, reset_mode == BE_LIF_RESET_HARD, N, static_cast<hipStream_t>(stream), x, kNoIn, v0, kNoIn,
                          kNoParam, lane::ParamArr{beta, beta_period}, lane::ParamArr{v_th, vth_period}, kNoParam, kNoParam, s_out, v_seq,
                          h_save, kNoOut, kNoOut, kNoOut, v_last, kNoOut, T, N, p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_sg_backward_params(const float* h_save, const float* v0, const float* g_s, const float* g_vseq, const float* g_vlast,
                              const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period, float* g_x, float* g_v0,
                              float* g_beta_slot, float* g_vth_slot, int64_t T, int64_t N, double v_reset, int reset_mode,
                              int surrogate, double alpha, int detach_reset, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode, beta_period, vth_period)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && beta && v_th && g_x, BE_ERR_INVALID, "null pointer (h_save, beta, v_th and g_x are required)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., alpha);
  const float* v0_read = g_beta_slot != nullptr ? v0 : nullptr;        // read for the beta gradient alone
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, v0_read, g_s, g_vseq, g_vlast, g_x, g_v0, g_beta_slot, g_vth_slot) &&
                   param_vec(beta, beta_period) && param_vec(v_th, vth_period);
  launch_backward<PerSlot>(vec, reset_mode == BE_LIF_RESET_HARD, surrogate, N, static_cast<hipStream_t>(stream), h_save, kNoIn,
                           kNoIn, kNoIn, v0_read, g_s, g_vseq, kNoIn, g_vlast, kNoIn, kNoParam, lane::ParamArr{beta, beta_period},
                           lane::ParamArr{v_th, vth_period}, kNoParam, kNoParam, g_x, kNoOut, g_v0, kNoOut, kNoOut, g_beta_slot,
                           g_vth_slot, kNoOut, kNoOut, T, N, (int)(detach_reset != 0), p);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_syn_sg_forward(const float* x, const float* c0, const float* v0, const float* a0, float* s_out, float* v_seq,
                          float* h_save, float* th_save, float* c_last, float* v_last, float* a_last, int64_t T, int64_t N,
                          double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                          int adaptive, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last);
  be_dispatch_bool(adapt, [&](auto A) {
    launch_forward<Synaptic<decltype(A)::value>>(vec, reset_mode == BE_LIF_RESET_HARD, N, static_cast<hipStream_t>(stream), x, c0, v0,
                                                 a0, kNoParam, kNoParam, kNoParam, kNoParam, kNoParam, s_out, v_seq, h_save, th_save,
                                                 kNoOut, c_last, v_last, a_last, T, N, p);
    return BE_OK;
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_syn_sg_backward(const float* h_save, const float* th_save, const float* g_s, const float* g_vseq, const float* g_clast,
                           const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0, float* g_a0, int64_t T,
                           int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa,
                           int reset_mode, int surrogate, double alpha, int adaptive, int detach_reset, be_stream_t stream) {
  if (const int rc = lane::check_common(__func__, T, N, reset_mode)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0);
  be_dispatch_bool(adapt, [&](auto A) {
    launch_backward<Synaptic<decltype(A)::value>>(vec, reset_mode == BE_LIF_RESET_HARD, surrogate, N, static_cast<hipStream_t>(stream),
                                                  h_save, th_save, kNoIn, kNoIn, kNoIn, g_s, g_vseq, g_clast, g_vlast, g_alast, kNoParam,
                                                  kNoParam, kNoParam, kNoParam, kNoParam, g_x, g_c0, g_v0, g_a0, kNoOut, kNoOut, kNoOut,
                                                  kNoOut, kNoOut, T, N, (int)(detach_reset != 0), p);
    return BE_OK;
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_syn_sg_forward_params(const float* x, const float* c0, const float* v0, const float* a0, const float* syn_decay,
                                 int64_t sd_period, const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period,
                                 const float* rho, int64_t rho_period, const float* kappa, int64_t kappa_period, float* s_out,
                                 float* v_seq, float* h_save, float* c_save, float* a_save, float* c_last, float* v_last,
                                 float* a_last, int64_t T, int64_t N, double v_reset, int reset_mode, int adaptive,
                                 be_stream_t stream) {
  const bool adapt = adaptive != 0;
  if (!adapt) rho_period = 1, kappa_period = 1;                            // the adaptation's arguments are not looked at
  if (const int rc = lane::check_common(__func__, T, N, reset_mode, beta_period, vth_period, sd_period, rho_period, kappa_period)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(syn_decay && beta && v_th, BE_ERR_INVALID, "null pointer (syn_decay, beta and v_th are required)");
  BE_REQUIRE(!adapt || (rho && kappa), BE_ERR_INVALID, "null pointer (adaptive: rho and kappa are required)");
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || a_save, BE_ERR_INVALID, "null pointer (adaptive: a_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., 1.);
  if (!adapt) a0 = nullptr, a_save = nullptr, a_last = nullptr, rho = nullptr, kappa = nullptr;   // neither read nor written
  if (!h_save) a_save = nullptr;                                           // written beside h_save alone
  const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, c0, v0, a0, s_out, v_seq, h_save, c_save, a_save, c_last, v_last, a_last) &&
                   param_vec(syn_decay, sd_period) && param_vec(beta, beta_period) && param_vec(v_th, vth_period) &&
                   (!adapt || (param_vec(rho, rho_period) && param_vec(kappa, kappa_period)));
  be_dispatch_bool(adapt, [&](auto A) {
    launch_forward<SynapticPerSlot<decltype(A)::value>>(
        vec, reset_mode == BE_LIF_RESET_HARD, N, static_cast<hipStream_t>(stream), x, c0, v0, a0, lane::ParamArr{syn_decay, sd_period},
        lane::ParamArr{beta, beta_period}, lane::ParamArr{v_th, vth_period}, lane::ParamArr{rho, rho_period},
        lane::ParamArr{kappa, kappa_period}, s_out, v_seq, h_save, a_save, c_save, c_last, v_last, a_last, T, N, p);
    return BE_OK;
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_syn_sg_backward_params(const float* h_save, const float* c_save, const float* a_save, const float* c0, const float* v0,
                                  const float* g_s, const float* g_vseq, const float* g_clast, const float* g_vlast,
                                  const float* g_alast, const float* syn_decay, int64_t sd_period, const float* beta,
                                  int64_t beta_period, const float* v_th, int64_t vth_period, const float* rho, int64_t rho_period,
                                  const float* kappa, int64_t kappa_period, float* g_x, float* g_c0, float* g_v0, float* g_a0,
                                  float* g_sd_slot, float* g_beta_slot, float* g_vth_slot, float* g_rho_slot, float* g_kappa_slot,
                                  int64_t T, int64_t N, double v_reset, int reset_mode, int surrogate, double alpha, int adaptive,
                                  int detach_reset, be_stream_t stream) {
  const bool adapt = adaptive != 0;
  if (!adapt) rho_period = 1, kappa_period = 1;                            // the adaptation's arguments are not looked at
  if (const int rc = lane::check_common(__func__, T, N, reset_mode, beta_period, vth_period, sd_period, rho_period, kappa_period)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(syn_decay && beta && v_th, BE_ERR_INVALID, "null pointer (syn_decay, beta and v_th are required)");
  BE_REQUIRE(!adapt || (rho && kappa), BE_ERR_INVALID, "null pointer (adaptive: rho and kappa are required)");
  BE_REQUIRE(!adapt || a_save, BE_ERR_INVALID, "null pointer (adaptive: a_save is required)");
  BE_REQUIRE(!g_sd_slot || c_save, BE_ERR_INVALID, "null pointer (c_save is required where g_sd_slot is given)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., alpha);
  if (!adapt)                                                              // neither read nor written, whatever was passed
    a_save = nullptr, g_alast = nullptr, g_a0 = nullptr, rho = nullptr, kappa = nullptr, g_rho_slot = nullptr, g_kappa_slot = nullptr;
  const float* c_read = g_sd_slot != nullptr ? c_save : nullptr;           // c_save and c0: read for the syn_decay gradient alone
  const float* c0_read = g_sd_slot != nullptr ? c0 : nullptr;
  const float* v_read = g_beta_slot != nullptr ? v0 : nullptr;             // v0: for the beta gradient alone
  const bool vec = (N % kSgVec == 0) &&
                   lane::all_aligned16(h_save, c_read, a_save, c0_read, v_read, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0,
                                       g_sd_slot, g_beta_slot, g_vth_slot, g_rho_slot, g_kappa_slot) &&
                   param_vec(syn_decay, sd_period) && param_vec(beta, beta_period) && param_vec(v_th, vth_period) &&
                   (!adapt || (param_vec(rho, rho_period) && param_vec(kappa, kappa_period)));
  be_dispatch_bool(adapt, [&](auto A) {
    launch_backward<SynapticPerSlot<decltype(A)::value>>(
        vec, reset_mode == BE_LIF_RESET_HARD, surrogate, N, static_cast<hipStream_t>(stream), h_save, a_save, c_read, c0_read, v_read,
        g_s, g_vseq, g_clast, g_vlast, g_alast, lane::ParamArr{syn_decay, sd_period}, lane::ParamArr{beta, beta_period},
        lane::ParamArr{v_th, vth_period}, lane::ParamArr{rho, rho_period}, lane::ParamArr{kappa, kappa_period}, g_x, g_c0, g_v0, g_a0,
        g_sd_slot, g_beta_slot, g_vth_slot, g_rho_slot, g_kappa_slot, T, N, (int)(detach_reset != 0), p);
    return BE_OK;
  });
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
