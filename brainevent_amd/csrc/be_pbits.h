// be_pbits.h — raw-bit access of the four weight dtypes (shared by be_plasticity.hip and be_grad.hip): the 16-bit types go
// through their bit patterns so every load / store can be non-temporal; `acc` is the accumulation type (f32, f64 for f64).
#pragma once
#include "be_common.h"

template <typename W> struct PB;
template <> struct PB<float> {
  using bits = uint32_t; using acc = float;
  __device__ static __forceinline__ acc get(bits b) { return __uint_as_float(b); }
  __device__ static __forceinline__ bits put(acc v) { return __float_as_uint(v); }
};
template <> struct PB<double> {
  using bits = uint64_t; using acc = double;
  __device__ static __forceinline__ acc get(bits b) { return __longlong_as_double((long long)b); }
  __device__ static __forceinline__ bits put(acc v) { return (bits)__double_as_longlong(v); }
};
template <> struct PB<__half> {
  using bits = uint16_t; using acc = float;
  __device__ static __forceinline__ acc get(bits b) { return __half2float(__ushort_as_half(b)); }
  __device__ static __forceinline__ bits put(acc v) { return __half_as_ushort(__float2half(v)); }
};
template <> struct PB<__hip_bfloat16> {
  using bits = uint16_t; using acc = float;
  __device__ static __forceinline__ acc get(bits b) { return __uint_as_float((uint32_t)b << 16); }
  __device__ static __forceinline__ bits put(acc v) {
    const __hip_bfloat16 h = __float2bfloat16(v);
    bits b;
    __builtin_memcpy(&b, &h, sizeof(b));
    return b;
  }
};
