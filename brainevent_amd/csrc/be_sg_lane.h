// be_sg_lane.h — what one lane of a differentiable-neuron kernel does (DESIGN.md §2.19 – §2.23), stated once: S consecutive f32
// slots moved as one S * 4-byte access, a parameter read with a period, the surrogate's derivative, and the neuron's step on
// scalars — forwards (forward_step) and backwards (backward_step, backward_carry) — for every model: the plain LIF, per-slot beta /
// v_th, the synaptic current (SYN) and the adaptive threshold (ADAPT).  be_neuron_sg.hip calls the step per slot j of a lane,
// be_neuron_sg_rec.hip per owned neuron k.  Everything is rounded operation by operation (no FMA contraction; the pragma is
// lexical, so every function here that holds arithmetic carries it), in the order and with the parentheses include/brainevent_amd.h
// states.  The checks the entry points share are here too.
#pragma once
#include "be_common.h"

namespace be_sg_lane {

template <int S> struct Pack;
template <> struct Pack<1> { using type = float; };
template <> struct Pack<4> { using type = float4; };

// S slots of one lane, in registers (every index is a compile-time constant once the loops over j are unrolled)
template <int S>
struct Vals {
  float f[S];
};

// one S * 4-byte load: p must be S * 4-byte aligned
template <int S>
__device__ __forceinline__ Vals<S> load(const float* __restrict__ p) {
  using P = typename Pack<S>::type;
  const P raw = *reinterpret_cast<const P*>(p);
  Vals<S> out;
  __builtin_memcpy(out.f, &raw, sizeof(P));
  return out;
}

// one S * 4-byte (vector) store
template <int S>
__device__ __forceinline__ void store(float* __restrict__ p, const Vals<S>& v) {
  using P = typename Pack<S>::type;
  P raw;
  __builtin_memcpy(&raw, v.f, sizeof(P));
  *reinterpret_cast<P*>(p) = raw;
}

template <int S>
__device__ __forceinline__ Vals<S> fill(float c) {
  Vals<S> out;
#pragma unroll
  for (int j = 0; j < S; ++j) out.f[j] = c;
  return out;
}

template <int S>
__device__ __forceinline__ Vals<S> zero() {
  return fill<S>(0.f);
}

// p NULL: zeros (a uniform branch)
template <int S>
__device__ __forceinline__ Vals<S> load_or_zero(const float* __restrict__ p, int64_t i) {
  return p != nullptr ? load<S>(p + i) : zero<S>();
}

// a parameter array and its period: slot i of a step reads p[i % period]
struct ParamArr {
  const float* p;
  int64_t period;
};

// the S parameter values of the slots i .. i + S - 1 (i % S == 0; period 1, or period % S == 0 with an aligned base)
template <int S>
__device__ __forceinline__ Vals<S> load_param(const ParamArr& a, int64_t i) {
  if (a.period == 1) return fill<S>(a.p[0]);
  return load<S>(a.p + i % a.period);
}

// the surrogate's constants: alpha, f32(pi / 2 * alpha), f32(alpha / 2), each rounded from the double once on the host
struct Surrogate {
  float alpha, atan_c, atan_half;
};

// every model's constants, each rounded from the double once on the host (a model reads the ones it has)
struct LifP {
  float syn_decay, beta, v_th, v_reset, rho, kappa;
  Surrogate sur;
};

// alpha is read backwards only: a forward pass gives any
inline LifP make_params(double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, double alpha) {
  return LifP{(float)syn_decay, (float)beta, (float)v_th, (float)v_reset, (float)rho, (float)kappa,
              Surrogate{(float)alpha, (float)(3.14159265358979323846 / 2 * alpha), (float)(alpha / 2)}};
}

// the surrogate's derivative at u = h - threshold (SG: BE_LIF_SG_*)
template <int SG>
__device__ __forceinline__ float derivative(float u, const Surrogate& p) {
#pragma clang fp contract(off)
  if (SG == BE_LIF_SG_FAST_SIGMOID) {
    const float d = 1.0f + p.alpha * fabsf(u);
    return 1.0f / (d * d);
  }
  if (SG == BE_LIF_SG_ATAN) {
    const float q = p.atan_c * u;
    return p.atan_half / (1.0f + q * q);
  }
  const float a = 1.0f - p.alpha * fabsf(u);     // triangle; a NaN compares false: 0, as fmaxf(0, NaN)
  return p.alpha * (a > 0.0f ? a : 0.0f);
}

// the membrane a step leaves behind, from its h and the threshold it was compared with.  The soft reset subtracts the BASE
// threshold v_th (the constant, or the slot's own), never the adaptive th.
template <bool HARD>
__device__ __forceinline__ float membrane_after(float h, float th, float v_th, float v_reset) {
#pragma clang fp contract(off)
  const bool s = h >= th;
  return HARD ? (s ? v_reset : h) : (s ? h - v_th : h);
}

struct Fired {
  float h, th;
  bool s;
};

// One step forwards on the input x: c (SYN), v and a (ADAPT) become the state after it.  Without SYN h = (beta * v) + x directly —
// not the synaptic step with syn_decay = 0, which would turn a -0 input into +0 and an inf / NaN c into NaN.
template <bool HARD, bool SYN, bool ADAPT>
__device__ __forceinline__ Fired forward_step(float x, float& c, float& v, float& a, float beta, float v_th, const LifP& p) {
#pragma clang fp contract(off)
  if (SYN) c = (p.syn_decay * c) + x;
  const float h = (beta * v) + (SYN ? c : x);
  const float th = ADAPT ? v_th + (p.kappa * a) : v_th;
  const bool s = h >= th;
  v = membrane_after<HARD>(h, th, v_th, p.v_reset);
  if (ADAPT) a = (p.rho * a) + (s ? 1.0f : 0.0f);
  return Fired{h, th, s};
}

struct Grad {
  float g_u, g_h;
  bool s;
};

// One step backwards from the saved h and the threshold th it was compared with (v_th: the base threshold, as above).  g_sp is
// what reaches the spike from outside the neuron (g_s, the recurrent term; +0 where none is given), g_vo what reaches the
// membrane after the step, ca the trace's carry (ADAPT).  g_u goes to h - th through the surrogate, g_h to h.
template <bool HARD, int SG, bool ADAPT>
__device__ __forceinline__ Grad backward_step(float h, float th, float v_th, float g_sp, float g_vo, float ca, int detach_reset,
                                              const LifP& p) {
#pragma clang fp contract(off)
  const bool s = h >= th;
  const float u = h - th;
  const float sg = derivative<SG>(u, p.sur);
  if (ADAPT) g_sp = g_sp + ca;
  if (!detach_reset) g_sp = HARD ? g_sp + g_vo * (p.v_reset - h) : g_sp - g_vo * v_th;
  const float g_u = g_sp * sg;
  const float g_h = g_u + (HARD ? (s ? 0.0f : g_vo) : g_vo);
  return Grad{g_u, g_h, s};
}

// The carries a step hands to the one before it: cc (SYN), cv, ca (ADAPT).  Returns the step's g_x.
template <bool SYN, bool ADAPT>
__device__ __forceinline__ float backward_carry(const Grad& g, float& cc, float& cv, float& ca, float beta, const LifP& p) {
#pragma clang fp contract(off)
  float g_x = g.g_h;
  if (SYN) {
    g_x = cc + g.g_h;
    cc = p.syn_decay * g_x;
  }
  cv = beta * g.g_h;
  if (ADAPT) ca = (p.rho * ca) - (p.kappa * g.g_u);
  return g_x;
}

// ---------------------------------------------------------------------------------------------- host side
inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

// NULL counts as aligned: an array that is not given is not accessed
template <typename... Ptr>
inline bool all_aligned16(Ptr... ptrs) {
  return (aligned16(ptrs) && ...);
}

// the checks the entry points share (BE_REQUIRE would name these functions, not the entry point); the periods are those of per-slot
// parameters, where the entry point has them
inline int check_common(const char* who, int64_t T, int64_t N, int reset_mode, int64_t beta_period = 1, int64_t vth_period = 1,
                        int64_t sd_period = 1, int64_t rho_period = 1, int64_t kappa_period = 1) {
  const int64_t periods[] = {beta_period, vth_period, sd_period, rho_period, kappa_period};
  bool small = false, split = false;
  for (const int64_t period : periods) small = small || period < 1;
  for (const int64_t period : periods) split = split || (!small && N % period != 0);
  const char* msg = (T < 0 || N < 0) ? ": T < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : small ? ": a period must be >= 1"
                    : split ? ": a period must divide N" : nullptr;
  if (msg == nullptr) return BE_OK;
  be_set_error(std::string(who) + msg);
  return BE_ERR_INVALID;
}

inline int check_surrogate(const char* who, int surrogate, double alpha) {
  const char* msg = (surrogate != BE_LIF_SG_FAST_SIGMOID && surrogate != BE_LIF_SG_ATAN && surrogate != BE_LIF_SG_TRIANGLE)
                        ? ": unknown surrogate"
                        : !(alpha > 0.) ? ": alpha must be positive" : nullptr;
  if (msg == nullptr) return BE_OK;
  be_set_error(std::string(who) + msg);
  return BE_ERR_INVALID;
}

}  // namespace be_sg_lane
