// be_sg_lane.h — what one lane of a differentiable-neuron kernel needs: S consecutive f32 slots moved as
// one S * 4-byte access, and the surrogate's derivative.  Everything is rounded operation by operation (no FMA contraction).
// be_neuron_sg_syn.hip includes it; be_neuron_sg.hip and be_neuron_sg_param.hip state the same helpers themselves (their text is
// held by tests) and could include this file instead.
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
__device__ __forceinline__ Vals<S> zero() {
  Vals<S> out;
#pragma unroll
  for (int j = 0; j < S; ++j) out.f[j] = 0.f;
  return out;
}

// p NULL: zeros (a uniform branch)
template <int S>
__device__ __forceinline__ Vals<S> load_or_zero(const float* __restrict__ p, int64_t i) {
  return p != nullptr ? load<S>(p + i) : zero<S>();
}

// the surrogate's constants: alpha, f32(pi / 2 * alpha), f32(alpha / 2), each rounded from the double once on the host
struct Surrogate {
  float alpha, atan_c, atan_half;
};

inline Surrogate make_surrogate(double alpha) {
  return Surrogate{(float)alpha, (float)(3.14159265358979323846 / 2 * alpha), (float)(alpha / 2)};
}

// the surrogate's derivative at u = h - threshold (SG: BE_LIF_SG_*), the operations and order of include/brainevent_amd.h
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

inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

}  // namespace be_sg_lane
