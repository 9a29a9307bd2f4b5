// be_csr_shared.h — helpers shared by the CSR translation units (be_csr.hip: compaction, direct scatter, gather;
// be_csr_plan.hip: the scatter plan; be_csr_binned.hip: the binned route).  Device helpers are inline; the one host function
// with a single definition (be_resolve_active, be_csr.hip) is declared here.
#pragma once
#include "be_common.h"
#include <cmath>
#include <type_traits>

// ---------------------------------------------------------------- host-side launch helpers
static inline int grid_for(int64_t n, int block, int cap) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

constexpr int kMaxBatch = 65535;
constexpr int kFusedMinBatch = 4;      // batched gather: fuse over the batch from this many columns ...
constexpr int64_t kFusedMinWork = 768; // ... when (average row length x columns) reaches this (and rows average >= 16 entries)

static inline int64_t counts_bytes(int64_t nb) { return be_align_up(nb * 4, 256); }
static inline int64_t active_stride_of(int64_t m) { return be_align_up(m * 4, 256) / 4; }   // in uint32 elements

static inline bool check_rows(const void* indptr, int64_t row_len) { return indptr != nullptr || row_len >= 0; }

static inline int64_t width_of(int slice_shift, int slice_width) { return slice_width > 0 ? slice_width : (1ll << slice_shift); }
static inline int n_slices_of(int64_t k, int slice_shift, int slice_width = 0) {
  const int64_t w = width_of(slice_shift, slice_width);
  return (int)((k + w - 1) / w);
}

// Active-row list of a scatter call: the spikes compacted into the workspace, or (BE_SPIKE_IDS, n_batch = 1) the
// caller's own list — `spikes` is then a HOST pointer to a be_spike_ids_t holding two device pointers.
struct ActiveList {
  const uint32_t* ids;
  const uint32_t* count;
};
int be_resolve_active(const void* spikes, int sd, int64_t n, int64_t nb, uint32_t* ws_active, int64_t astride,
                      uint32_t* ws_count, hipStream_t st, bool zero_first, ActiveList* al);

// Plasticity's view of a spike vector (be_plasticity.hip; a spike is any NONZERO value, all four spike codes): the active ids
// as a device list in `workspace` (>= be_plast_active_bytes(n) bytes) and, with `rp`, the 64-bit exclusive offsets of their
// rows' entries (offs[n_active] = total) — what be_plasticity_rows walks, for the plan upkeep that follows it.
int64_t be_plast_active_bytes(int64_t n);
int be_plast_active_offsets(const void* spikes, int sd, int64_t n, const RowPtr* rp, void* workspace, hipStream_t st,
                            ActiveList* al, const int64_t** offs);

// ---------------------------------------------------------------- device helpers
// block-wide inclusive scan over 1024 threads (wave shuffles + one LDS hop): 2 barriers instead of 20
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t* wave_tot /* [16] in LDS */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w)
    if (w < wave) base += wave_tot[w];
  __syncthreads();
  return base + incl;
}

// ---------------------------------------------------------------- integer accumulation in LDS (plan and binned route)
template <bool HOMO> struct PlanAcc;
template <> struct PlanAcc<true> { using type = uint32_t; };
template <> struct PlanAcc<false> { using type = unsigned long long; };

// (the fixed-point encoding itself, fixed_from_f32, is in be_common.h: the JITC scatter kernels use it too)
template <bool HOMO>
__device__ __forceinline__ void plan_add4(typename PlanAcc<HOMO>::type* acc, uint2 iv, float4 wv, float scale) {
  const uint32_t i0 = iv.x & 0xffffu, i1 = iv.x >> 16, i2 = iv.y & 0xffffu, i3 = iv.y >> 16;
  if (HOMO) {
    atomicAdd(&acc[i0], 1u);
    atomicAdd(&acc[i1], 1u);
    atomicAdd(&acc[i2], 1u);
    atomicAdd(&acc[i3], 1u);
  } else {
    atomicAdd(&acc[i0], fixed_from_f32(wv.x, scale));
    atomicAdd(&acc[i1], fixed_from_f32(wv.y, scale));
    atomicAdd(&acc[i2], fixed_from_f32(wv.z, scale));
    atomicAdd(&acc[i3], fixed_from_f32(wv.w, scale));
  }
}

__device__ __forceinline__ void plan_count8(uint32_t* acc, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  atomicAdd(&acc[a & 0xffffu], 1u); atomicAdd(&acc[a >> 16], 1u);
  atomicAdd(&acc[b & 0xffffu], 1u); atomicAdd(&acc[b >> 16], 1u);
  atomicAdd(&acc[c & 0xffffu], 1u); atomicAdd(&acc[c >> 16], 1u);
  atomicAdd(&acc[d & 0xffffu], 1u); atomicAdd(&acc[d >> 16], 1u);
}

// ---------------------------------------------------------------- FP8 weights as exact integers (q8 plan and direct f8 route)
// Q(c) = decode(c) * 2^E of a finite OCP FP8 code, E = 9 (e4m3) / 16 (e5m2), as a 64-bit two's-complement integer, decoded
// with integer operations only: with MB mantissa bits the magnitude is m for a subnormal (exponent field 0) and
// (2^MB + m) << (e - 1) otherwise — both formats' bias puts the subnormal step at 2^-E.  |Q| <= 229 376 / 3 758 096 384.
// Non-finite codes are the caller's to keep out (include/brainevent_amd.h).
constexpr int kF8ExpE4M3 = 9, kF8ExpE5M2 = 16;
template <int FMT>
__device__ __forceinline__ unsigned long long f8_fixed(uint32_t c) {
  constexpr uint32_t MB = FMT == BE_F8_E4M3 ? 3u : 2u;
  const uint32_t mant = c & ((1u << MB) - 1u), e = (c & 0x7fu) >> MB;
  const uint32_t mag = e ? ((mant | (1u << MB)) << (e - 1u)) : mant;
  return (c & 0x80u) ? 0ull - (unsigned long long)mag : (unsigned long long)mag;
}

typedef unsigned be_v2u __attribute__((ext_vector_type(2)));
typedef unsigned be_v4u __attribute__((ext_vector_type(4)));
constexpr int kBufFlags = 0x00020000;   // raw buffer, 32-bit data format (guide T8)
