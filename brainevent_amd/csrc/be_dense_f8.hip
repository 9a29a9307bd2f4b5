// be_dense_f8.hip — event-driven dense products with OCP FP8 weights (e4m3 = float8_e4m3fn, e5m2) for gfx950.
//
//   transpose=1: W8[k, n], spikes_bm[nb, k] -> out[nb, n] = fl32((sum_{i : e(s[b, i])} decode(W8[i, :])) * scale)
//   transpose=0: W8[m, k], spikes_bm[nb, k] -> out[nb, m] = fl32((sum_{j : e(s[b, j])} decode(W8[:, j])) * scale)
// The weights are multiplied by 0 or 1 only and summed in f32, so the products are as exact as with wider weights, and the
// contraction is bound by the bytes of the weight rows that carry a spike (be_dense.hip): a byte per weight halves them
// against f16.  The output is always f32; `scale` is one f32 per matrix, applied once to the finished sum.
//
// Same structure as be_dense.hip (spikes -> per-row batch masks -> ordered row lists -> row parts -> fixed-order reduce), with
// this file's own small mask / list kernels:
//   k8_densemm_t     vector route of S @ W8 (fewer than 8 batch rows, or a matrix the 16-B loads cannot take): a lane owns 16
//                    columns (one 16-B load = 16 codes), v_cvt_pk_f32_{fp8,bf8}, 4 x 16 f32 accumulators
//   k8_densemm_mfma  S @ W8 from 8 batch rows on: the union-row K loop of k_densemm_mfma; the codes are staged in LDS as the
//                    bytes they are, read back through ds_read_b64_tr_b8 and multiplied by v_mfma_f32_32x32x16_{fp8_fp8,
//                    bf8_bf8} (the spike tile's 1.0 is 0x38 / 0x3C).  BE_F8_MFMA_BYTES=0 builds the other way to feed the MFMA:
//                    the codes widened to bf16 while they are stashed (every e4m3 / e5m2 value, subnormals included, is a
//                    NORMAL bf16 number), then ds_read_b64_tr_b16 + v_mfma_f32_32x32x16_bf16 — HBM bytes halve, LDS bytes do not.
//   k8_densemm_nt    W8 @ S.T: one wave streams a weight row with 16-B loads against the masks (every batch size)
// PRECONDITION: every code is finite (e4m3: (c & 0x7f) != 0x7f; e5m2: (c & 0x7c) != 0x7c).  Inside an MFMA 0 * inf = NaN, and
// this file has no repair path: the Python layer refuses non-finite codes once per tensor version, a C caller guarantees it.
#include "be_common.h"
#include <algorithm>

typedef unsigned be8_v4u __attribute__((ext_vector_type(4)));
typedef float be8_v2f __attribute__((ext_vector_type(2)));
typedef __bf16 be8_v8bf __attribute__((ext_vector_type(8)));
typedef short be8_v8s __attribute__((ext_vector_type(8)));
typedef short be8_v4s __attribute__((__vector_size__(4 * sizeof(short))));
typedef float be8_v16f __attribute__((ext_vector_type(16)));
typedef int be8_v2i __attribute__((ext_vector_type(2)));

namespace {

constexpr int k8Group = 4;        // batch rows per wave in the vector S @ W8 kernel
constexpr int k8MaxChunk = 32;    // batch rows per pass (one uint32 mask per row)
constexpr int k8MaxGroups = k8MaxChunk / k8Group;
constexpr int k8Tile = 2048;      // rows per workgroup of the list kernels (256 threads x 8)
constexpr int k8Vec = 16;         // codes per 16-B load

// ---- decode.  FMT 0 = e4m3 (v_cvt_*_fp8), 1 = e5m2 (v_cvt_*_bf8); gfx950 reads both as OCP.
template <int FMT, bool HI> __device__ __forceinline__ be8_v2f f8_pair(uint32_t w) {
  if constexpr (FMT == 0) return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  else return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
}
template <int FMT> __device__ __forceinline__ float f8_one(const uint8_t* p) {
  if constexpr (FMT == 0) return __builtin_amdgcn_cvt_f32_fp8((int)(uint32_t)p[0], 0);
  else return __builtin_amdgcn_cvt_f32_bf8((int)(uint32_t)p[0], 0);
}
template <int POL> __device__ __forceinline__ uint4 f8_load16(const void* p) {
  if (POL) { const be8_v4u t = __builtin_nontemporal_load(reinterpret_cast<const be8_v4u*>(p)); return make_uint4(t.x, t.y, t.z, t.w); }
  return *reinterpret_cast<const uint4*>(p);
}
template <int FMT> __device__ __forceinline__ void f8_decode16(const uint4& t, float (&v)[16]) {
  const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const be8_v2f lo = f8_pair<FMT, false>(w[i]), hi = f8_pair<FMT, true>(w[i]);
    v[4 * i] = lo.x; v[4 * i + 1] = lo.y; v[4 * i + 2] = hi.x; v[4 * i + 3] = hi.y;
  }
}
// VEC codes at p as f32: one 16-B load (VEC = 16) or one byte (VEC = 1, any alignment)
template <int FMT, int VEC, int POL> __device__ __forceinline__ void f8_row_load(const uint8_t* p, float (&v)[VEC]) {
  if constexpr (VEC == 16) { const uint4 t = f8_load16<POL>(p); f8_decode16<FMT>(t, v); }
  else v[0] = f8_one<FMT>(p);
}
// two codes -> two bf16 in one word (the high halves of their f32 values: exact, see the head of the file)
template <int FMT, bool HI> __device__ __forceinline__ uint32_t f8_pair_bf16(uint32_t w) {
  const be8_v2f f = f8_pair<FMT, HI>(w);
  return (__float_as_uint(f.x) >> 16) | (__float_as_uint(f.y) & 0xffff0000u);
}

// ------------------------------------------------------------------------------------------------
// spikes_bm rows b0 .. b0+nc -> mask[k], bit b set iff spike (b0+b, i) is active
// ------------------------------------------------------------------------------------------------
template <typename SP>
__global__ void __launch_bounds__(256) k8_masks(const typename SP::type* __restrict__ spikes, int64_t k, int nc,
                                                uint32_t* __restrict__ mask) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
    uint32_t mk = 0;
    for (int b0 = 0; b0 < nc; b0 += 8) {       // eight batch rows' loads in flight
      typename SP::type v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = spikes[(int64_t)(b0 + u < nc ? b0 + u : nc - 1) * k + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) mk |= ((b0 + u < nc && SP::active(v[u])) ? 1u : 0u) << (b0 + u);
    }
    mask[i] = mk;
  }
}
// BE_SPIKE_BITS rows (nc rows of ceil(k / 32) words): the same masks, read from the words as they are
__global__ void __launch_bounds__(256) k8_masks_bits(const uint32_t* __restrict__ words, int64_t k, int nc,
                                                     uint32_t* __restrict__ mask) {
  const int64_t n_words = (k + 31) / 32;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
    uint32_t mk = 0;
    for (int b0 = 0; b0 < nc; b0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = words[(int64_t)(b0 + u < nc ? b0 + u : nc - 1) * n_words + (i >> 5)];
#pragma unroll
      for (int u = 0; u < 8; ++u) mk |= (b0 + u < nc ? (v[u] >> (i & 31)) & 1u : 0u) << (b0 + u);
    }
    mask[i] = mk;
  }
}

// k8_masks and the per-tile counts of the rows with any bit set, in one launch: workgroup = one tile of k8Tile rows, a thread =
// 8 consecutive rows.  One-byte spikes are read 8 rows at a time (one 8-byte load per batch row and thread) where k and the
// operand's address allow it.
template <typename SP>
__global__ void __launch_bounds__(256) k8_masks_count(const typename SP::type* __restrict__ spikes, int64_t k, int nc,
                                                      uint32_t* __restrict__ mask, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t red[4];
  const int64_t base = (int64_t)blockIdx.x * k8Tile + (int64_t)threadIdx.x * 8;
  uint32_t mk[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  bool done = false;
  if constexpr (sizeof(typename SP::type) == 1) {
    if (base + 8 <= k && (k & 7) == 0 && (reinterpret_cast<uintptr_t>(spikes) & 7) == 0) {
      for (int b0 = 0; b0 < nc; b0 += 8) {
        uint2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = *reinterpret_cast<const uint2*>(spikes + (int64_t)(b0 + u < nc ? b0 + u : nc - 1) * k + base);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint32_t bit = b0 + u < nc ? 1u << (b0 + u) : 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            mk[i] |= ((v[u].x >> (8 * i)) & 0xffu) ? bit : 0u;
            mk[4 + i] |= ((v[u].y >> (8 * i)) & 0xffu) ? bit : 0u;
          }
        }
      }
      done = true;
    }
  }
  if (!done) {
    for (int i = 0; i < 8; ++i) {
      if (base + i >= k) break;
      for (int b0 = 0; b0 < nc; b0 += 8) {
        typename SP::type v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = spikes[(int64_t)(b0 + u < nc ? b0 + u : nc - 1) * k + base + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) mk[i] |= ((b0 + u < nc && SP::active(v[u])) ? 1u : 0u) << (b0 + u);
      }
    }
  }
  uint32_t c = 0;
  for (int i = 0; i < 8 && base + i < k; ++i) { mask[base + i] = mk[i]; c += mk[i] ? 1u : 0u; }
  c = wave_sum(c);
  if (lane_id() == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256) k8_masks_count_bits(const uint32_t* __restrict__ words, int64_t k, int nc,
                                                           uint32_t* __restrict__ mask, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t red[4];
  const int64_t n_words = (k + 31) / 32;
  const int64_t base = (int64_t)blockIdx.x * k8Tile + (int64_t)threadIdx.x * 8;      // 8 consecutive rows: one byte of a word
  uint32_t mk[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (base < k) {
    for (int b0 = 0; b0 < nc; b0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = words[(int64_t)(b0 + u < nc ? b0 + u : nc - 1) * n_words + (base >> 5)];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t byte = b0 + u < nc ? (v[u] >> (base & 31)) & 0xffu : 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) mk[i] |= ((byte >> i) & 1u) << (b0 + u);
      }
    }
  }
  uint32_t c = 0;
  for (int i = 0; i < 8 && base + i < k; ++i) { mask[base + i] = mk[i]; c += mk[i] ? 1u : 0u; }
  c = wave_sum(c);
  if (lane_id() == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ordered compaction of the rows whose sub-mask for batch group g (= blockIdx.y) is non-zero; WHOLE: one list of the rows
// with any bit set.  entry = row | submask << 28 (rows < 2^28).  Three passes: per-tile counts, scan, write.
template <bool WHOLE> __device__ __forceinline__ uint32_t f8_submask(uint32_t mk, int g) {
  return WHOLE ? (mk ? 1u : 0u) : (mk >> (k8Group * g)) & ((1u << k8Group) - 1u);
}
template <bool WHOLE>
__global__ void __launch_bounds__(256) k8_gl_count(const uint32_t* __restrict__ mask, int64_t k, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t red[4];
  const int g = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * k8Tile + (int64_t)threadIdx.x * 8;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (base + i < k && f8_submask<WHOLE>(mask[base + i], g)) ++c;
  c = wave_sum(c);
  if (lane_id() == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[(int64_t)g * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// one workgroup per list: exclusive scan of its tile counts; count[g] = total
__global__ void __launch_bounds__(1024) k8_gl_scan(uint32_t* __restrict__ tile_cnt, int64_t n_tiles, uint32_t* __restrict__ count) {
  __shared__ uint32_t part[1024];
  __shared__ uint32_t carry;
  uint32_t* tc = tile_cnt + (int64_t)blockIdx.x * n_tiles;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_tiles; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = (i < n_tiles) ? tc[i] : 0u;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      uint32_t t = 0;
      if ((int)threadIdx.x >= off) t = part[threadIdx.x - off];
      __syncthreads();
      part[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < n_tiles) tc[i] = carry + part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) count[blockIdx.x] = carry;
}
// SELF_SCAN (one list, at most 1024 tiles): tile_off holds the raw per-tile counts and every workgroup sums the tiles in front
// of it itself; the last one also writes the total to *count — no scan launch.
template <bool WHOLE, bool SELF_SCAN>
__global__ void __launch_bounds__(256) k8_gl_write(const uint32_t* __restrict__ mask, int64_t k, const uint32_t* __restrict__ tile_off,
                                                   uint32_t* __restrict__ lists, int64_t list_stride, uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t front_s[4];
  uint32_t front = 0;
  if (SELF_SCAN) {
    uint32_t f = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = q * 256 + (int)threadIdx.x;
      f += t < (int)blockIdx.x ? tile_off[t] : 0u;
    }
    f = wave_sum(f);
    if (lane_id() == 0) front_s[threadIdx.x >> 6] = f;
    __syncthreads();
    front = front_s[0] + front_s[1] + front_s[2] + front_s[3];
  }
  const int g = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * k8Tile + (int64_t)threadIdx.x * 8;
  uint32_t sm[8];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sm[i] = (base + i < k) ? f8_submask<WHOLE>(mask[base + i], g) : 0u;
    c += sm[i] ? 1u : 0u;
  }
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t wave_off = 0;
  for (int w = 0; w < wave; ++w) wave_off += wave_tot[w];
  uint32_t pos = (SELF_SCAN ? front : tile_off[(int64_t)g * gridDim.x + blockIdx.x]) + wave_off + incl - c;   // pos + c <= k: the list has k slots
  if (SELF_SCAN && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) count[0] = front + wave_off + incl;   // the total
  uint32_t* out = lists + (int64_t)g * list_stride;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (sm[i]) out[pos++] = (uint32_t)(base + i) | (sm[i] << 28);
}

// ------------------------------------------------------------------------------------------------
// S @ W8, vector route: wave task = (strip of 64 * VEC columns, group of 4 batch rows); blockIdx.y = row part
// ------------------------------------------------------------------------------------------------
template <int FMT, int VEC>
__global__ void __launch_bounds__(256) k8_densemm_t(const uint8_t* __restrict__ weights, int64_t n, const uint32_t* __restrict__ lists,
                                                    int64_t list_stride, const uint32_t* __restrict__ count, int n_groups, int nc,
                                                    float* __restrict__ partial, int64_t nb_total, int b0) {
  const int lane = lane_id();
  const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_strips = (n + 64 * VEC - 1) / (64 * VEC);
  if (task >= n_strips * n_groups) return;
  const int g = (int)(task % n_groups);
  const int64_t strip = task / n_groups;
  const int64_t col = strip * (64 * VEC) + (int64_t)lane * VEC;
  const bool in = col < n;            // VEC = 16 only when n % 16 == 0, so a lane is all-in or all-out
  const uint32_t cnt = count[g];
  const uint32_t* list = lists + (int64_t)g * list_stride;
  const uint32_t part = blockIdx.y, parts = gridDim.y;

  float acc[k8Group][VEC];
#pragma unroll
  for (int b = 0; b < k8Group; ++b)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[b][v] = 0.f;

  // rows of this part: a = part, part + parts, ...  (UNR row loads of 16 B in flight per lane)
  constexpr int UNR = 4;
  uint32_t a = part;
  for (; a + (uint32_t)(UNR - 1) * parts < cnt; a += (uint32_t)UNR * parts) {
    uint32_t e[UNR];
    uint4 t[UNR];
    float w1[UNR];
#pragma unroll
    for (int q = 0; q < UNR; ++q) e[q] = list[a + q * parts];
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      const uint8_t* p = weights + (int64_t)(e[q] & 0x0fffffffu) * n + col;
      if constexpr (VEC == 16) t[q] = in ? f8_load16<1>(p) : make_uint4(0, 0, 0, 0);
      else w1[q] = in ? f8_one<FMT>(p) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      float w[VEC];
      if constexpr (VEC == 16) f8_decode16<FMT>(t[q], w);
      else w[0] = w1[q];
      const uint32_t sm = e[q] >> 28;
#pragma unroll
      for (int b = 0; b < k8Group; ++b)
        if (sm & (1u << b)) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[b][v] += w[v];
        }
    }
  }
  for (; a < cnt; a += parts) {
    const uint32_t e = list[a];
    float w[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) w[v] = 0.f;
    if (in) f8_row_load<FMT, VEC, 1>(weights + (int64_t)(e & 0x0fffffffu) * n + col, w);
    const uint32_t sm = e >> 28;
#pragma unroll
    for (int b = 0; b < k8Group; ++b)
      if (sm & (1u << b)) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[b][v] += w[v];
      }
  }
  if (!in) return;
#pragma unroll
  for (int b = 0; b < k8Group; ++b) {
    const int bb = k8Group * g + b;
    if (bb >= nc) break;
    float* dst = partial + ((int64_t)part * nb_total + b0 + bb) * n + col;
    if constexpr (VEC == 16) {
#pragma unroll
      for (int v = 0; v < 16; v += 4) *reinterpret_cast<float4*>(dst + v) = make_float4(acc[b][v], acc[b][v + 1], acc[b][v + 2], acc[b][v + 3]);
    } else {
      dst[0] = acc[b][0];
    }
  }
}

// out[i] = fl32((sum over the parts, in their order) * scale): the epilogue of both S @ W8 routes
__global__ void __launch_bounds__(256) k8_reduce(const float* __restrict__ partial, int parts, int64_t part_stride, int64_t total,
                                                 float scale, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    float s = 0.f;
    for (int p0 = 0; p0 < parts; p0 += 8) {      // eight parts' loads in flight; the sum keeps the order of the parts
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(p0 + u < parts ? p0 + u : parts - 1) * part_stride + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p0 + u < parts ? v[u] : 0.f;
    }
    out[i] = s * scale;
  }
}

// ------------------------------------------------------------------------------------------------
// S @ W8 on MFMA (8 batch rows or more).  v_mfma_f32_32x32x16_{fp8_fp8,bf8_bf8}: M = 32 batch rows, N = 32 weight columns,
// K = 16 union rows per step.  Workgroup = 4 waves = 512 columns x one K range (a wave owns 128: four 32 x 32 accumulators); a
// thread loads 2 x 16 B = 2 x 16 codes per step (16 rows x 512 B = 256 threads x 32 B: the bytes a step of k_densemm_mfma moves
// at 256 f16 columns) and stores them into the LDS tile as they are; one ds_read_b64_tr_b8 per accumulator block hands every
// lane the 8 K values of its column (lane layout at tr8_off below); the A operand (the 0/1 spike tile) is rebuilt in registers
// from the 16 row masks of the step.  K is split over gridDim.y parts; the f32 partials are reduced in fixed order.
// C5 shape (32 x 65536 spikes at 1 %, 65536^2 weights), whole product, f16 0.40 ms.  Widened to bf16 (BE_F8_MFMA_BYTES=0): 256
// columns per workgroup 0.300 ms (ring depth 2 / 4 / 8 alike: 0.305 / 0.300 / 0.307; 1536 workgroups 0.28), 512 columns 0.255-0.259
// (1536 workgroups 0.27-0.29).  Bytes + fp8 MFMA, 512 columns: 0.241-0.245 ms (1152 / 1536 workgroups 0.255 /
// 0.27; 256 columns at 1536 workgroups 0.26-0.27), and 0.233-0.236 ms at ring depth 2.
// ------------------------------------------------------------------------------------------------
#ifndef BE_F8_MFMA_COLS
#define BE_F8_MFMA_COLS 512
#endif
constexpr int k8MfmaCols = BE_F8_MFMA_COLS;            // columns per workgroup (256 or 512): a tile row is 256 / 512 B of one weight row
#ifndef BE_F8_MFMA_BYTES
#define BE_F8_MFMA_BYTES 1                             // 1: stage the codes as bytes, ds_read_b64_tr_b8 + the fp8 / bf8 MFMA; 0: widen to bf16
#endif
constexpr bool k8Bytes = BE_F8_MFMA_BYTES != 0;
// LDS row stride, padded: bytes + 32 B (8 mod 64 banks: the 8 rows x 32 B a half-wave's transpose read touches fill the 64 banks
// once), bf16 + 64 B (16 mod 64 banks, be_dense.hip)
constexpr int k8MfmaRowBytes = k8Bytes ? k8MfmaCols + 32 : k8MfmaCols * 2 + 64;
constexpr int k8MfmaTileBytes = 16 * k8MfmaRowBytes;   // one K-step tile
constexpr int k8MfmaChunk = 64;                        // K-steps whose row ids / masks are staged in LDS at a time
#ifndef BE_F8_MFMA_D
#define BE_F8_MFMA_D 2                                 // K-steps of codes in flight per thread (register ring; even).  C5, bytes + fp8
#endif                                                 // MFMA at 512 columns: 2 / 4 steps 0.233-0.236 / 0.241-0.245 ms
#ifndef BE_F8_MFMA_WG_TARGET
#define BE_F8_MFMA_WG_TARGET 768                       // workgroups (column tiles x row parts): 3 per CU, as BE_MFMA_WG_TARGET
#endif

// orders LDS traffic only (__syncthreads() would also drain the global loads of the ring)
__device__ __forceinline__ void f8_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int FMT>
__global__ void __launch_bounds__(256) k8_densemm_mfma(const uint8_t* __restrict__ weights, int64_t n, const uint32_t* __restrict__ mask,
                                                       const uint32_t* __restrict__ ulist, const uint32_t* __restrict__ ucount,
                                                       float* __restrict__ partial) {
  constexpr int D = BE_F8_MFMA_D;
  static_assert(D % 2 == 0 && D >= 2, "the ring depth must be even");
  __shared__ __align__(16) unsigned char tile[2][k8MfmaTileBytes];
  // D extra all-zero steps behind every chunk: the ring runs past the chunk end without any branch
  __shared__ uint32_t rows_s[(k8MfmaChunk + D) * 16];
  __shared__ uint32_t masks_s[(k8MfmaChunk + D) * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t col0 = (int64_t)blockIdx.x * k8MfmaCols;
  const uint32_t n_union = ucount[0];
  const uint32_t steps_total = (n_union + 15u) >> 4;
  const uint32_t per_part = (steps_total + gridDim.y - 1) / gridDim.y;
  const uint32_t t_begin = blockIdx.y * per_part;
  const uint32_t t_end = t_begin + per_part < steps_total ? t_begin + per_part : steps_total;

  // staging role: thread loads the 16 codes `ch` of tile rows r0, r0 + RSTEP, ...
  constexpr int CPR = k8MfmaCols / 16;                 // 16-byte pieces per tile row
  constexpr int RSTEP = 256 / CPR;
  constexpr int NLD = 16 / RSTEP;                      // loads per thread and step (1 or 2)
  constexpr int NB = k8MfmaCols / 128;                 // 32-column accumulator blocks per wave
  const int ch = tid % CPR, r0 = tid / CPR;
  const bool col_ok = col0 + (int64_t)ch * 16 < n;     // n % 16 == 0: a piece is all-in or all-out
  const uint8_t* wcol = weights + (col_ok ? col0 + (int64_t)ch * 16 : 0);

  // MFMA role (the lane layout of k_densemm_mfma)
  const int grp = lane >> 4, gi = lane & 15, q = gi >> 2, pq = gi & 3;
  const int b_row = lane & 31, h = lane >> 5;
  const int tr_off = ((grp >> 1) * 8 + q) * k8MfmaRowBytes + (wave * (k8MfmaCols / 4) + (grp & 1) * 16 + 4 * pq) * 2;
  // ds_read_b64_tr_b8: lane 16g + 8p + c receives byte c of what the lanes 16g + 2j + p address, j = 0 .. 7.  Source
  // lane 2j + p of a group addresses tile row 8h + j, columns 16 (g & 1) + 8p ...: the group's 16 lanes then hold 16 consecutive
  // columns, each its 8 K values of rows 8h .. 8h + 7 in order — the B operand of the 32x32x16 fp8 MFMA.
  const int tr8_off = (8 * h + (gi >> 1)) * k8MfmaRowBytes + wave * (k8MfmaCols / 4) + (grp & 1) * 16 + 8 * (gi & 1);

  be8_v16f acc[NB] = {};
  uint4 rr[D][NLD];
  uint32_t rk[D];

  for (uint32_t c0 = t_begin; c0 < t_end; c0 += k8MfmaChunk) {
    const uint32_t c_end = c0 + k8MfmaChunk < t_end ? c0 + k8MfmaChunk : t_end;
    __syncthreads();                                   // previous chunk fully consumed
    for (int j = tid; j < (k8MfmaChunk + D) * 16; j += 256) {
      const uint32_t i = c0 * 16u + j;
      const bool v = i < n_union && (c0 + (j >> 4)) < c_end;
      const uint32_t rid = v ? (ulist[i] & 0x0fffffffu) : 0u;
      rows_s[j] = rid;
      masks_s[j] = v ? mask[rid] : 0u;                 // mask 0 => the row contributes nothing
    }
    __syncthreads();

    // fetch only issues the load (clamped address: row 0 / column 0 for padding, zeroed when the slot is stashed)
    auto fetch = [&](uint32_t t, uint4 (&r)[NLD], uint32_t& ok) {     // steps past c_end are zero steps
      const uint32_t s = (t - c0) < (uint32_t)(k8MfmaChunk + D - 1) ? (t - c0) : (uint32_t)(k8MfmaChunk + D - 1);
      ok = 0u;
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        r[u] = f8_load16<1>(wcol + (int64_t)rows_s[s * 16 + r0 + u * RSTEP] * n);
        ok |= (col_ok && masks_s[s * 16 + r0 + u * RSTEP] != 0u ? 1u : 0u) << u;
      }
    };
    auto stash = [&](int buf, const uint4 (&r)[NLD], uint32_t ok) {   // registers -> bf16 -> LDS
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const uint4 c = ((ok >> u) & 1u) ? r[u] : make_uint4(0, 0, 0, 0);         // code 0 is +0.0 in both formats
        if constexpr (k8Bytes) {
          *reinterpret_cast<uint4*>(&tile[buf][(r0 + u * RSTEP) * k8MfmaRowBytes + ch * 16]) = c;
          continue;
        }
        uint4* dst = reinterpret_cast<uint4*>(&tile[buf][(r0 + u * RSTEP) * k8MfmaRowBytes + ch * 32]);
        dst[0] = make_uint4(f8_pair_bf16<FMT, false>(c.x), f8_pair_bf16<FMT, true>(c.x), f8_pair_bf16<FMT, false>(c.y),
                            f8_pair_bf16<FMT, true>(c.y));
        dst[1] = make_uint4(f8_pair_bf16<FMT, false>(c.z), f8_pair_bf16<FMT, true>(c.z), f8_pair_bf16<FMT, false>(c.w),
                            f8_pair_bf16<FMT, true>(c.w));
      }
    };

    // prologue: step c0 -> LDS[0]; steps c0+1 .. c0+D -> ring slots 1 .. D-1, 0
    fetch(c0, rr[0], rk[0]);
    stash(0, rr[0], rk[0]);
#pragma unroll
    for (int s = 1; s <= D; ++s) fetch(c0 + s, rr[s % D], rk[s % D]);
    f8_lds_barrier();
    for (uint32_t t0 = c0; t0 < c_end; t0 += D) {
#pragma unroll
      for (int ii = 0; ii < D; ++ii) {
        const uint32_t t = t0 + ii;          // no branch: steps in [c_end, c_end + D) multiply zeros (rows_s / masks_s)
        const int buf = ii & 1;              // D is even and chunks start at ring position 0
        const uint32_t* mk = &masks_s[(t - c0) * 16 + 8 * h];
        if constexpr (k8Bytes) {
          // A operand: byte j of this lane = spike bit of batch row b_row at tile row 8h + j; 1.0 is 0x38 in e4m3, 0x3C in e5m2
          constexpr uint32_t one = FMT == 0 ? 0x38u : 0x3Cu;
          uint32_t a2[2] = {0u, 0u};
#pragma unroll
          for (int j = 0; j < 8; ++j) a2[j >> 2] |= (((mk[j] >> b_row) & 1u) * one) << (8 * (j & 3));
          const long a = (long)(((unsigned long long)a2[1] << 32) | a2[0]);
          const unsigned char* tb = &tile[buf][0] + tr8_off;
          typedef __attribute__((address_space(3))) be8_v2i* lds_v2i;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const be8_v2i bv = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i)(tb + 32 * j));
            const long b = (long)(((unsigned long long)(uint32_t)bv.y << 32) | (uint32_t)bv.x);
            if constexpr (FMT == 0) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc[j], 0, 0, 0);
            else acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(a, b, acc[j], 0, 0, 0);
          }
        }
        // A operand: element j of this lane = spike bit of batch row b_row at tile row 8h + j (bf16 1.0 = 0x3F80)
        be8_v8s a;
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (short)(((mk[j] >> b_row) & 1u) * 0x3F80u);
        const unsigned char* tb = &tile[buf][0] + tr_off;
        typedef __attribute__((address_space(3))) be8_v4s* lds_v4s;
#pragma unroll
        for (int j = 0; j < (k8Bytes ? 0 : NB); ++j) {
          const be8_v4s blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(tb + 64 * j));
          const be8_v4s bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(tb + 64 * j + 4 * k8MfmaRowBytes));
          const be8_v8s b = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(be8_v8bf, a), __builtin_bit_cast(be8_v8bf, b), acc[j], 0, 0, 0);
        }
        // next step's rows go to the other LDS buffer; their ring slot is refilled D steps ahead
        stash(buf ^ 1, rr[(ii + 1) % D], rk[(ii + 1) % D]);
        fetch(t + 1 + D, rr[(ii + 1) % D], rk[(ii + 1) % D]);
        f8_lds_barrier();
      }
    }
  }
  // C layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float* pbase = partial + (int64_t)blockIdx.y * 32 * n;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    const int64_t c = col0 + wave * (k8MfmaCols / 4) + (lane & 31);
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (c + 32 * j < n) pbase[(int64_t)row * n + c + 32 * j] = acc[j][r];
  }
}

// ------------------------------------------------------------------------------------------------
// W8 @ S.T: one wave per weight row, streamed with 16-B loads against the masks
// ------------------------------------------------------------------------------------------------
template <int FMT, int VEC, int NBT>
__global__ void __launch_bounds__(256) k8_densemm_nt(const uint8_t* __restrict__ weights, int64_t m, int64_t k,
                                                     const uint32_t* __restrict__ mask, int nc, float scale, float* __restrict__ out_bm,
                                                     int b0) {
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < m; r += n_waves) {
    const uint8_t* row = weights + r * k;
    float acc[NBT];
#pragma unroll
    for (int b = 0; b < NBT; ++b) acc[b] = 0.f;
    // U row pieces and their masks in flight per lane, then the tail piece by piece (VEC = 16 only when k % 16 == 0)
    constexpr int U = 2;
    int64_t j = (int64_t)lane * VEC;
    for (; j + (int64_t)(U - 1) * 64 * VEC < k; j += (int64_t)U * 64 * VEC) {
      float w[U][VEC];
      uint32_t mk[U][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) f8_row_load<FMT, VEC, 1>(row + j + (int64_t)u * 64 * VEC, w[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t* mp = mask + j + (int64_t)u * 64 * VEC;
        if constexpr (VEC == 16) {
#pragma unroll
          for (int v4 = 0; v4 < 4; ++v4) {
            const uint4 t = reinterpret_cast<const uint4*>(mp)[v4];
            mk[u][4 * v4] = t.x; mk[u][4 * v4 + 1] = t.y; mk[u][4 * v4 + 2] = t.z; mk[u][4 * v4 + 3] = t.w;
          }
        } else {
          mk[u][0] = mp[0];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (mk[u][v]) {
#pragma unroll
            for (int b = 0; b < NBT; ++b) acc_add_inplace(acc[b], ((mk[u][v] >> b) & 1u) ? w[u][v] : 0.f);
          }
        }
    }
    for (; j < k; j += 64 * VEC) {
      float w[VEC];
      f8_row_load<FMT, VEC, 1>(row + j, w);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const uint32_t mk = mask[j + v];
        if (mk) {
#pragma unroll
          for (int b = 0; b < NBT; ++b) acc_add_inplace(acc[b], ((mk >> b) & 1u) ? w[v] : 0.f);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
      float s = acc[b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0 && b < nc) out_bm[(int64_t)(b0 + b) * m + r] = s * scale;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
inline int f8_grid_cap(int64_t n, int block, int cap) {
  int64_t g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
inline int64_t f8_tiles_of(int64_t k) { return (k + k8Tile - 1) / k8Tile; }

struct F8Ws {
  uint32_t* mask;      // k
  uint32_t* lists;     // (k8MaxGroups + 1) * k   (group lists; the last one is the union list)
  uint32_t* tile_cnt;  // (k8MaxGroups + 1) * n_tiles
  uint32_t* count;     // 16
  float* partial;
};

inline int64_t f8_ws_bytes(int64_t rows_w, int64_t cols_w, int64_t nb, int transpose) {
  const int64_t k = transpose ? rows_w : cols_w;
  int64_t b = be_align_up(k * 4, 256);
  b += be_align_up((int64_t)(k8MaxGroups + 1) * k * 4, 256);
  b += be_align_up((int64_t)(k8MaxGroups + 1) * f8_tiles_of(k) * 4, 256);
  b += 256;
  if (transpose) {
    const int64_t rows_p = nb < 32 ? 32 : nb;                          // the MFMA route keeps 32 batch rows per part
    b += be_align_up((int64_t)16 * rows_p * cols_w * 4, 256);          // <= 16 parts x >= 32 rows: also 32 parts x <= 4 rows
  }
  return b;
}
inline F8Ws f8_carve(void* ws, int64_t k) {
  unsigned char* p = static_cast<unsigned char*>(ws);
  F8Ws d;
  d.mask = reinterpret_cast<uint32_t*>(p); p += be_align_up(k * 4, 256);
  d.lists = reinterpret_cast<uint32_t*>(p); p += be_align_up((int64_t)(k8MaxGroups + 1) * k * 4, 256);
  d.tile_cnt = reinterpret_cast<uint32_t*>(p); p += be_align_up((int64_t)(k8MaxGroups + 1) * f8_tiles_of(k) * 4, 256);
  d.count = reinterpret_cast<uint32_t*>(p); p += 256;
  d.partial = reinterpret_cast<float*>(p);
  return d;
}
inline size_t f8_spike_row_bytes(int sd, int64_t k) {
  return sd == BE_SPIKE_BITS ? (size_t)((k + 31) / 32) * 4 : (size_t)k * (sd == BE_SPIKE_FLOAT ? 4 : 1);
}

int f8_masks(const void* chunk, int sd, int64_t k, int nc, uint32_t* mask, hipStream_t st) {
  const dim3 grid(f8_grid_cap(k, 256, 2048));
  if (sd == BE_SPIKE_BITS) hipLaunchKernelGGL(k8_masks_bits, grid, dim3(256), 0, st, static_cast<const uint32_t*>(chunk), k, nc, mask);
  else if (sd == BE_SPIKE_FLOAT) hipLaunchKernelGGL(k8_masks<SpikeFloat>, grid, dim3(256), 0, st, static_cast<const float*>(chunk), k, nc, mask);
  else hipLaunchKernelGGL(k8_masks<SpikeBool>, grid, dim3(256), 0, st, static_cast<const uint8_t*>(chunk), k, nc, mask);
  BE_LAUNCH_CHECK();
  return BE_OK;
}
int f8_masks_count(const void* chunk, int sd, int64_t k, int nc, uint32_t* mask, uint32_t* tile_cnt, int64_t nt, hipStream_t st) {
  if (sd == BE_SPIKE_BITS)
    hipLaunchKernelGGL(k8_masks_count_bits, dim3((unsigned)nt), dim3(256), 0, st, static_cast<const uint32_t*>(chunk), k, nc, mask, tile_cnt);
  else if (sd == BE_SPIKE_FLOAT)
    hipLaunchKernelGGL(k8_masks_count<SpikeFloat>, dim3((unsigned)nt), dim3(256), 0, st, static_cast<const float*>(chunk), k, nc, mask, tile_cnt);
  else
    hipLaunchKernelGGL(k8_masks_count<SpikeBool>, dim3((unsigned)nt), dim3(256), 0, st, static_cast<const uint8_t*>(chunk), k, nc, mask, tile_cnt);
  BE_LAUNCH_CHECK();
  return BE_OK;
}
// masks of a chunk of batch rows, then its ordered lists: n_groups per-group lists (slots 0 ..), or the union list (last slot).
// One list (the union, or the only group's: with at most 4 batch rows its sub-mask is the whole mask): masks and tile counts in
// one launch, and up to 1024 tiles no scan launch — two launches where the general form takes four.
template <bool WHOLE>
int f8_lists(const void* chunk, int sd, int64_t k, int nc, int n_groups, const F8Ws& d, hipStream_t st) {
  const int64_t nt = f8_tiles_of(k);
  const int slot = WHOLE ? k8MaxGroups : 0, nl = WHOLE ? 1 : n_groups;
  uint32_t* tc = d.tile_cnt + (int64_t)slot * nt;
  uint32_t* list = d.lists + (int64_t)slot * k;
  if (nl == 1) {
    const int rc = f8_masks_count(chunk, sd, k, nc, d.mask, tc, nt, st);
    if (rc != BE_OK) return rc;
    if (nt <= 1024) {
      hipLaunchKernelGGL((k8_gl_write<WHOLE, true>), dim3((unsigned)nt, 1), dim3(256), 0, st, d.mask, k, tc, list, k, d.count + slot);
      BE_LAUNCH_CHECK();
      return BE_OK;
    }
  } else {
    const int rc = f8_masks(chunk, sd, k, nc, d.mask, st);
    if (rc != BE_OK) return rc;
    hipLaunchKernelGGL(k8_gl_count<WHOLE>, dim3((unsigned)nt, nl), dim3(256), 0, st, d.mask, k, tc);
    BE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k8_gl_scan, dim3(nl), dim3(1024), 0, st, tc, nt, d.count + slot);
  BE_LAUNCH_CHECK();
  hipLaunchKernelGGL((k8_gl_write<WHOLE, false>), dim3((unsigned)nt, nl), dim3(256), 0, st, d.mask, k, tc, list, k,
                     static_cast<uint32_t*>(nullptr));
  BE_LAUNCH_CHECK();
  return BE_OK;
}

inline int f8_parts_for(int64_t n, int vec, int n_groups) {
  const int64_t tasks = ((n + 64 * vec - 1) / (64 * vec)) * n_groups;
  const int64_t wgs = (tasks + 3) / 4;
  // as parts_for of be_dense.hip: a single batch group has few strips and wants many row parts in flight
  const int64_t target = n_groups == 1 ? 2048 : 1024, cap = n_groups == 1 ? 32 : 16;
  int64_t p = target / (wgs > 0 ? wgs : 1);
  if (p < 1) p = 1;
  if (p > cap) p = cap;
  return (int)p;
}
inline int f8_mfma_parts(int64_t n) {
  const int64_t tiles = (n + k8MfmaCols - 1) / k8MfmaCols;
  int64_t p = BE_F8_MFMA_WG_TARGET / (tiles > 0 ? tiles : 1);
  return (int)(p < 1 ? 1 : (p > 16 ? 16 : p));
}

template <int FMT, int VEC>
int f8_t_vec(const uint8_t* weights, float scale, const void* spikes_bm, int sd, float* out_bm, int64_t k, int64_t n, int64_t nb,
             void* ws, hipStream_t st) {
  F8Ws d = f8_carve(ws, k);
  // the same parts for every chunk so that one reduce pass serves the whole batch
  const int parts = f8_parts_for(n, VEC, (int)((std::min<int64_t>(nb, k8MaxChunk) + k8Group - 1) / k8Group));
  for (int64_t b0 = 0; b0 < nb; b0 += k8MaxChunk) {
    const int nc = (int)std::min<int64_t>(k8MaxChunk, nb - b0);
    const int n_groups = (nc + k8Group - 1) / k8Group;
    const void* chunk = static_cast<const unsigned char*>(spikes_bm) + (size_t)b0 * f8_spike_row_bytes(sd, k);
    const int rc = f8_lists<false>(chunk, sd, k, nc, n_groups, d, st);
    if (rc != BE_OK) return rc;
    const int64_t tasks = ((n + 64 * VEC - 1) / (64 * VEC)) * n_groups;
    hipLaunchKernelGGL((k8_densemm_t<FMT, VEC>), dim3((unsigned)((tasks + 3) / 4), parts), dim3(256), 0, st, weights, n, d.lists, k,
                       d.count, n_groups, nc, d.partial, nb, (int)b0);
    BE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k8_reduce, dim3(f8_grid_cap(nb * n, 256, 2048)), dim3(256), 0, st, d.partial, parts, nb * n, nb * n, scale, out_bm);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <int FMT>
int f8_t_mfma(const uint8_t* weights, float scale, const void* spikes_bm, int sd, float* out_bm, int64_t k, int64_t n, int64_t nb,
              void* ws, hipStream_t st) {
  F8Ws d = f8_carve(ws, k);
  const int parts = f8_mfma_parts(n);
  const int prof = be_prof_begin(st);
  for (int64_t b0 = 0; b0 < nb; b0 += k8MaxChunk) {
    const int nc = (int)std::min<int64_t>(k8MaxChunk, nb - b0);
    const void* chunk = static_cast<const unsigned char*>(spikes_bm) + (size_t)b0 * f8_spike_row_bytes(sd, k);
    const int rc = f8_lists<true>(chunk, sd, k, nc, 1, d, st);
    if (rc != BE_OK) return rc;
    hipLaunchKernelGGL(k8_densemm_mfma<FMT>, dim3((unsigned)((n + k8MfmaCols - 1) / k8MfmaCols), parts), dim3(256), 0, st, weights, n,
                       d.mask, d.lists + (int64_t)k8MaxGroups * k, d.count + k8MaxGroups, d.partial);
    BE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k8_reduce, dim3(f8_grid_cap((int64_t)nc * n, 256, 2048)), dim3(256), 0, st, d.partial, parts, (int64_t)32 * n,
                       (int64_t)nc * n, scale, out_bm + b0 * n);
    BE_LAUNCH_CHECK();
  }
  be_prof_end(prof, st);
  return BE_OK;
}

template <int FMT, int VEC>
int f8_nt_vec(const uint8_t* weights, float scale, const void* spikes_bm, int sd, float* out_bm, int64_t m, int64_t k, int64_t nb,
              void* ws, hipStream_t st) {
  F8Ws d = f8_carve(ws, k);
  for (int64_t b0 = 0; b0 < nb; b0 += k8MaxChunk) {
    const int nc = (int)std::min<int64_t>(k8MaxChunk, nb - b0);
    const void* chunk = static_cast<const unsigned char*>(spikes_bm) + (size_t)b0 * f8_spike_row_bytes(sd, k);
    const int rc = f8_masks(chunk, sd, k, nc, d.mask, st);
    if (rc != BE_OK) return rc;
    const dim3 grid(f8_grid_cap(m, 4, 2048));
    if (nc == 1) hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 1>), grid, dim3(256), 0, st, weights, m, k, d.mask, nc, scale, out_bm, (int)b0);
    else if (nc <= 8) hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 8>), grid, dim3(256), 0, st, weights, m, k, d.mask, nc, scale, out_bm, (int)b0);
    else hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 32>), grid, dim3(256), 0, st, weights, m, k, d.mask, nc, scale, out_bm, (int)b0);
    BE_LAUNCH_CHECK();
  }
  return BE_OK;
}

template <int FMT>
int f8_any(const void* weights, float scale, const void* spikes_bm, int sd, float* out_bm, int64_t rows_w, int64_t cols_w, int64_t nb,
           int transpose, void* ws, hipStream_t st) {
  const uint8_t* w = static_cast<const uint8_t*>(weights);
  const bool vec_ok = (cols_w % k8Vec == 0) && ((reinterpret_cast<uintptr_t>(weights) & 15) == 0);
  if (transpose) {
    if (vec_ok && nb >= 8) return f8_t_mfma<FMT>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);
    if (vec_ok) return f8_t_vec<FMT, 16>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);
    return f8_t_vec<FMT, 1>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);
  }
  if (vec_ok) return f8_nt_vec<FMT, 16>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);
  return f8_nt_vec<FMT, 1>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);
}

}  // namespace

extern "C" {

int64_t be_binary_densemm_f8_workspace_bytes(int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, int f8_format) {
  (void)f8_format;      // both formats are a byte per weight
  return f8_ws_bytes(rows_w, cols_w, n_batch, transpose);
}

int be_binary_densemm_f8(const void* weights, int f8_format, double scale, const void* spikes_bm, int spike_dtype, void* out_f32_bm,
                         int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, void* workspace, int64_t workspace_bytes,
                         be_stream_t stream) {
  BE_REQUIRE(rows_w >= 0 && cols_w >= 0 && n_batch >= 0, BE_ERR_INVALID, "bad shape");
  const int64_t k = transpose ? rows_w : cols_w;
  BE_REQUIRE(k < (1ll << 28), BE_ERR_RANGE, "contraction dimension must be < 2^28");
  const int64_t out_len = transpose ? cols_w : rows_w;
  if (out_len == 0 || n_batch == 0) return BE_OK;
  BE_REQUIRE(out_f32_bm != nullptr, BE_ERR_INVALID, "out is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (k == 0) {
    BE_HIP(be_fill_async(out_f32_bm, 0, (size_t)out_len * n_batch * sizeof(float), st));
    return BE_OK;
  }
  BE_REQUIRE(weights && spikes_bm, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(spike_dtype == BE_SPIKE_BOOL || spike_dtype == BE_SPIKE_FLOAT || spike_dtype == BE_SPIKE_BITS, BE_ERR_INVALID,
             "unknown spike dtype");
  BE_REQUIRE(workspace != nullptr && workspace_bytes >= f8_ws_bytes(rows_w, cols_w, n_batch, transpose), BE_ERR_WORKSPACE,
             "workspace too small");
  BE_REQUIRE(f8_format == BE_F8_E4M3 || f8_format == BE_F8_E5M2, BE_ERR_INVALID, "unknown FP8 format");
  const float sc = (float)scale;      // rounded to f32 once
  float* out = static_cast<float*>(out_f32_bm);
  if (f8_format == BE_F8_E4M3)
    return f8_any<0>(weights, sc, spikes_bm, spike_dtype, out, rows_w, cols_w, n_batch, transpose, workspace, st);
  return f8_any<1>(weights, sc, spikes_bm, spike_dtype, out, rows_w, cols_w, n_batch, transpose, workspace, st);
}

}  // extern "C"
