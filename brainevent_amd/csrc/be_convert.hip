// be_convert.hip — CSR -> CSC structure conversion on the device, in column blocks, without an entry-count limit
// (what makes the unfavourable direction `CSR @ spk` / `spk @ CSC` / `FixedNumPerPre @ spk` event-driven).
//
// Stands in for the reference's column-block route (read as text): brainevent/_csr/csr_to_csc.cu:62-114 (count with one
// atomic per stored entry; fill of one column block through per-column cursors — "row order inside each column is
// intentionally not stable", :26-27) and its host orchestration brainevent/_misc.py:1380-1513
// (`_csr_to_csc_index_gpu_column_block`: global count -> prefix sum -> per block: cursors, fill, append).
//
// Differences that matter on this machine:
//   * everything stays on the device (the reference copies every block back to the host and appends there), offsets are
//     64-bit throughout, so C2 / C4 (1e10 stored entries) convert in place: the count is one pass of the index stream
//     (40 GB at ~5 TB/s) bound by the chip's ~25 G/s random global atomics (0.4 s), a block's fill is the same pass with
//     atomics only for the entries of the block;
//   * the fill moves the weights along (2 / 4 / 8-byte elements) so that the mirror needs no `data[perm]` pass, and writes
//     `perm` only when asked (8 bytes per entry at 1e10 entries would be 80 GB);
//   * rows are walked by 1 ... 64 lanes each, chosen from the average row length (the reference: one thread per row).
#include "be_csr_shared.h"

namespace {

// ------------------------------------------------------------------------------------------------ count
// entry-parallel: four column ids per 16-byte load; ids outside [0, n_cols) are the caller's error and are skipped
__global__ void __launch_bounds__(256) k_t_count(const int32_t* __restrict__ indices, int64_t nnz, int64_t n_cols,
                                                 unsigned long long* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t head = ((16 - (reinterpret_cast<uintptr_t>(indices) & 15)) & 15) >> 2;   // entries before the first 16-B boundary
  const int64_t h = head < nnz ? head : nnz;
  const int64_t n4 = (nnz - h) >> 2;
  typedef int be_v4i __attribute__((ext_vector_type(4)));
  const be_v4i* v = reinterpret_cast<const be_v4i*>(indices + h);
  for (int64_t i = t; i < n4; i += stride) {
    const be_v4i c = __builtin_nontemporal_load(v + i);
    if ((uint32_t)c.x < (uint64_t)n_cols) atomicAdd(counts + c.x, 1ull);
    if ((uint32_t)c.y < (uint64_t)n_cols) atomicAdd(counts + c.y, 1ull);
    if ((uint32_t)c.z < (uint64_t)n_cols) atomicAdd(counts + c.z, 1ull);
    if ((uint32_t)c.w < (uint64_t)n_cols) atomicAdd(counts + c.w, 1ull);
  }
  for (int64_t i = t; i < h; i += stride) {
    const int32_t c = indices[i];
    if ((uint32_t)c < (uint64_t)n_cols) atomicAdd(counts + c, 1ull);
  }
  for (int64_t i = h + (n4 << 2) + t; i < nnz; i += stride) {
    const int32_t c = indices[i];
    if ((uint32_t)c < (uint64_t)n_cols) atomicAdd(counts + c, 1ull);
  }
}

// ------------------------------------------------------------------------------------------------ exclusive scan (int64)
// three launches: per-tile totals -> one workgroup scans the totals -> per-tile scan + offset.  A tile = 1024 threads x 8.
constexpr int kScanTile = 1024 * 8;

__global__ void __launch_bounds__(1024) k_scan64_totals(const unsigned long long* __restrict__ a, int64_t n,
                                                        unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long wsum[16];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 8;
  unsigned long long s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (base + i < n) s += a[base + i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int w = 0; w < 16; ++w) tot += wsum[w];
    totals[blockIdx.x] = tot;
  }
}

__global__ void __launch_bounds__(1024) k_scan64_of_totals(unsigned long long* __restrict__ totals, int64_t n_tiles,
                                                           unsigned long long* __restrict__ grand) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t b = 0; b < n_tiles; b += 1024) {
    const int64_t i = b + threadIdx.x;
    const unsigned long long v = i < n_tiles ? totals[i] : 0;
    unsigned long long incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long u = __shfl_up(incl, off, 64);
      if ((threadIdx.x & 63) >= off) incl += u;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned long long pre = carry_s;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += wsum[w];
    if (i < n_tiles) totals[i] = pre + incl - v;          // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = pre + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *grand = carry_s;
}

template <typename OUT>
__global__ void __launch_bounds__(1024) k_scan64_apply(const unsigned long long* __restrict__ a, int64_t n,
                                                       const unsigned long long* __restrict__ totals,
                                                       const unsigned long long* __restrict__ grand, OUT* __restrict__ out) {
  __shared__ unsigned long long wsum[16];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 8;
  unsigned long long v[8], s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = base + i < n ? a[base + i] : 0;
    s += v[i];
  }
  unsigned long long incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long u = __shfl_up(incl, off, 64);
    if ((threadIdx.x & 63) >= off) incl += u;
  }
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned long long pre = totals[blockIdx.x] + incl - s;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += wsum[w];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (base + i < n) out[base + i] = (OUT)pre;
    pre += v[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = (OUT)*grand;
}

// ------------------------------------------------------------------------------------------------ fill of one column block
__global__ void __launch_bounds__(256) k_t_cursor_init(const int64_t* __restrict__ t_ptr, int64_t col_lo, int64_t n_block_cols,
                                                       unsigned long long* __restrict__ cursor) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t base = t_ptr[col_lo];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_block_cols; i += stride)
    cursor[i] = (unsigned long long)(t_ptr[col_lo + i] - base);
}

// LPR lanes walk one stored row: consecutive lanes read consecutive entries, consecutive groups consecutive rows.  An entry
// whose column lies in [col_lo, col_hi) draws its slot from the column's cursor (one returning global atomic) and is written
// there: the row id, optionally the weight (moved, so the mirror needs no gather pass) and the source position (perm).
template <int LPR, typename PT, int WB>
__global__ void __launch_bounds__(256) k_t_fill(const int32_t* __restrict__ indices, RowPtr rp, int64_t m, int64_t col_lo,
                                                int64_t col_hi, unsigned long long* __restrict__ cursor,
                                                int32_t* __restrict__ rows_out, PT* __restrict__ perm_out,
                                                const unsigned char* __restrict__ w_in, unsigned char* __restrict__ w_out) {
  constexpr int kGroups = 256 / LPR;
  const int sub = threadIdx.x % LPR;
  const int64_t g0 = (int64_t)blockIdx.x * kGroups + threadIdx.x / LPR;
  const int64_t gstride = (int64_t)gridDim.x * kGroups;
  const uint64_t span = (uint64_t)(col_hi - col_lo);
  for (int64_t r = g0; r < m; r += gstride) {
    const int64_t b = rp.at(r), e = rp.at(r + 1);
    for (int64_t j = b + sub; j < e; j += LPR) {
      const int64_t c = (int64_t)indices[j] - col_lo;
      if ((uint64_t)c >= span) continue;
      const unsigned long long slot = atomicAdd(cursor + c, 1ull);
      rows_out[slot] = (int32_t)r;
      if (perm_out != nullptr) perm_out[slot] = (PT)j;
      if (WB == 1) w_out[slot] = w_in[j];
      if (WB == 2) reinterpret_cast<uint16_t*>(w_out)[slot] = reinterpret_cast<const uint16_t*>(w_in)[j];
      if (WB == 4) reinterpret_cast<uint32_t*>(w_out)[slot] = reinterpret_cast<const uint32_t*>(w_in)[j];
      if (WB == 8) reinterpret_cast<unsigned long long*>(w_out)[slot] = reinterpret_cast<const unsigned long long*>(w_in)[j];
    }
  }
}

// out[i] = src[perm[i]] (2 / 4 / 8-byte elements): a mirror that kept its permutation follows a weight update with one
// gather-copy (reference: slot j reads weights[perm[j]] on every step, brainevent/_csr/binary_indexed_csrmv_hybrid.cu:16-23)
template <typename PT, typename E>
__global__ void __launch_bounds__(256) k_gather_by_perm(const E* __restrict__ src, const PT* __restrict__ perm, int64_t n,
                                                        E* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[perm[i]];
}

template <int LPR, typename PT>
int launch_fill(int wbytes, const int32_t* indices, RowPtr rp, int64_t m, int64_t col_lo, int64_t col_hi,
                unsigned long long* cursor, int32_t* rows_out, PT* perm_out, const void* w_in, void* w_out, hipStream_t st) {
  const int grid = grid_for(m, 256 / LPR, 256 * 16);
  const unsigned char* wi = static_cast<const unsigned char*>(w_in);
  unsigned char* wo = static_cast<unsigned char*>(w_out);
#define BE_T_FILL(WB_)                                                                                                    \
  hipLaunchKernelGGL((k_t_fill<LPR, PT, WB_>), dim3(grid), dim3(256), 0, st, indices, rp, m, col_lo, col_hi, cursor, rows_out, \
                     perm_out, wi, wo)
  switch (wbytes) {
    case 0: BE_T_FILL(0); break;
    case 1: BE_T_FILL(1); break;      // (be_csr_to_csc_fill_block_u8 only: fill_block never passes a public 1 on)
    case 2: BE_T_FILL(2); break;
    case 4: BE_T_FILL(4); break;
    case 8: BE_T_FILL(8); break;
    default: be_set_error("be_csr_to_csc_fill_block: weight element size must be 0, 2, 4 or 8"); return BE_ERR_INVALID;
  }
#undef BE_T_FILL
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename PT>
int fill_by_row_length(int64_t avg_row, int wbytes, const int32_t* indices, RowPtr rp, int64_t m, int64_t col_lo, int64_t col_hi,
                       unsigned long long* cursor, int32_t* rows_out, PT* perm_out, const void* w_in, void* w_out,
                       hipStream_t st) {
  if (avg_row <= 2) return launch_fill<1, PT>(wbytes, indices, rp, m, col_lo, col_hi, cursor, rows_out, perm_out, w_in, w_out, st);
  if (avg_row <= 8) return launch_fill<4, PT>(wbytes, indices, rp, m, col_lo, col_hi, cursor, rows_out, perm_out, w_in, w_out, st);
  if (avg_row <= 48) return launch_fill<16, PT>(wbytes, indices, rp, m, col_lo, col_hi, cursor, rows_out, perm_out, w_in, w_out, st);
  return launch_fill<64, PT>(wbytes, indices, rp, m, col_lo, col_hi, cursor, rows_out, perm_out, w_in, w_out, st);
}

// The fill of one column block behind be_csr_to_csc_fill_block (`weight_bytes` 0, 2, 4 or 8) and be_csr_to_csc_fill_block_u8
// (`one_byte`: weight_bytes is 1).  `who` names the entry point in the error text.  A public weight_bytes of 1 is refused where
// every other unknown size is: by launch_fill's default case.
inline int fb_fail(const char* who, int code, const char* msg) {
  be_set_error(std::string(who) + ": " + msg);
  return code;
}
int fill_block(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m, int64_t nnz,
               int64_t col_lo, int64_t col_hi, const int64_t* csc_indptr, int64_t* cursor, int32_t* rows_out, void* perm_out,
               int perm_is_i64, const void* weights, int weight_bytes, void* weights_out, bool one_byte, be_stream_t stream,
               const char* who) {
  if (!(m >= 0 && m <= 0x7fffffffll && nnz >= 0)) return fb_fail(who, BE_ERR_INVALID, "bad shape");
  if (!(0 <= col_lo && col_lo <= col_hi && col_hi <= 0x7fffffffll)) return fb_fail(who, BE_ERR_INVALID, "bad column block");
  if (!check_rows(indptr, row_len)) return fb_fail(who, BE_ERR_INVALID, "indptr is NULL and row_len < 0");
  if (!(weight_bytes == 0 || (weights != nullptr && weights_out != nullptr)))
    return fb_fail(who, BE_ERR_INVALID, "weights / weights_out is NULL");
  if (col_hi == col_lo || m == 0 || nnz == 0) return BE_OK;
  if (!(indices && csc_indptr && cursor && rows_out)) return fb_fail(who, BE_ERR_INVALID, "null pointer");
  if (!(perm_out == nullptr || perm_is_i64 || nnz <= 0x7fffffffll))
    return fb_fail(who, BE_ERR_RANGE, "an int32 perm holds at most 2^31 - 1 entries");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nb = col_hi - col_lo;
  unsigned long long* cur = reinterpret_cast<unsigned long long*>(cursor);
  hipLaunchKernelGGL(k_t_cursor_init, dim3(grid_for(nb, 256, 2048)), dim3(256), 0, st, csc_indptr, col_lo, nb, cur);
  BE_LAUNCH_CHECK();
  RowPtr rp{indptr, indptr_is_i64, row_len};
  const int64_t avg = nnz / m;
  const int wsel = one_byte ? 1 : (weight_bytes == 1 ? -1 : weight_bytes);      // (-1: no case of launch_fill, as any unknown size)
  if (perm_out != nullptr && !perm_is_i64)
    return fill_by_row_length<int32_t>(avg, wsel, indices, rp, m, col_lo, col_hi, cur, rows_out,
                                       static_cast<int32_t*>(perm_out), weights, weights_out, st);
  return fill_by_row_length<int64_t>(avg, wsel, indices, rp, m, col_lo, col_hi, cur, rows_out,
                                     static_cast<int64_t*>(perm_out), weights, weights_out, st);
}

}  // namespace

extern "C" {

int64_t be_csr_to_csc_scratch_bytes(int64_t n_cols) {
  const int64_t tiles = (n_cols + kScanTile - 1) / kScanTile;
  return be_align_up((tiles + 2) * 8, 256);
}

int be_csr_to_csc_count(const int32_t* indices, int64_t nnz, int64_t n_cols, int64_t* counts, be_stream_t stream) {
  BE_REQUIRE(nnz >= 0 && n_cols >= 0 && n_cols <= 0x7fffffffll, BE_ERR_INVALID, "bad nnz / n_cols");
  BE_REQUIRE(n_cols == 0 || counts != nullptr, BE_ERR_INVALID, "counts is NULL");
  BE_REQUIRE(nnz == 0 || indices != nullptr, BE_ERR_INVALID, "indices is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_cols > 0) BE_HIP(be_fill_async(counts, 0, (size_t)n_cols * 8, st));
  if (nnz == 0 || n_cols == 0) return BE_OK;
  hipLaunchKernelGGL(k_t_count, dim3(grid_for((nnz + 3) / 4, 256, 256 * 16)), dim3(256), 0, st, indices, nnz, n_cols,
                     reinterpret_cast<unsigned long long*>(counts));
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_csr_to_csc_indptr(const int64_t* counts, int64_t n_cols, void* csc_indptr_out, int out_is_i64, int64_t* nnz_host,
                         void* scratch, int64_t scratch_bytes, be_stream_t stream) {
  BE_REQUIRE(n_cols >= 0 && n_cols <= 0x7fffffffll, BE_ERR_INVALID, "bad n_cols");
  BE_REQUIRE(csc_indptr_out != nullptr && (n_cols == 0 || counts != nullptr), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(scratch != nullptr && scratch_bytes >= be_csr_to_csc_scratch_bytes(n_cols), BE_ERR_WORKSPACE, "scratch too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t tiles = std::max<int64_t>(1, (n_cols + kScanTile - 1) / kScanTile);
  unsigned long long* totals = static_cast<unsigned long long*>(scratch);
  unsigned long long* grand = totals + tiles;
  const unsigned long long* a = reinterpret_cast<const unsigned long long*>(counts);
  hipLaunchKernelGGL(k_scan64_totals, dim3((unsigned)tiles), dim3(1024), 0, st, a, n_cols, totals);
  BE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_scan64_of_totals, dim3(1), dim3(1024), 0, st, totals, tiles, grand);
  BE_LAUNCH_CHECK();
  if (out_is_i64)
    hipLaunchKernelGGL(k_scan64_apply<int64_t>, dim3((unsigned)tiles), dim3(1024), 0, st, a, n_cols, totals, grand,
                       static_cast<int64_t*>(csc_indptr_out));
  else
    hipLaunchKernelGGL(k_scan64_apply<int32_t>, dim3((unsigned)tiles), dim3(1024), 0, st, a, n_cols, totals, grand,
                       static_cast<int32_t*>(csc_indptr_out));
  BE_LAUNCH_CHECK();
  if (nnz_host != nullptr) {
    unsigned long long g = 0;
    BE_HIP(hipMemcpyAsync(&g, grand, 8, hipMemcpyDeviceToHost, st));
    BE_HIP(hipStreamSynchronize(st));
    *nnz_host = (int64_t)g;
    BE_REQUIRE(out_is_i64 || g <= 0x7fffffffull, BE_ERR_RANGE, "entry count does not fit an int32 indptr");
  }
  return BE_OK;
}

int be_csr_to_csc_fill_block(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m,
                             int64_t nnz, int64_t col_lo, int64_t col_hi, const int64_t* csc_indptr, int64_t* cursor,
                             int32_t* rows_out, void* perm_out, int perm_is_i64, const void* weights, int weight_bytes,
                             void* weights_out, be_stream_t stream) {
  return fill_block(indices, indptr, indptr_is_i64, row_len, m, nnz, col_lo, col_hi, csc_indptr, cursor, rows_out, perm_out,
                    perm_is_i64, weights, weight_bytes, weights_out, false, stream, __func__);
}

int be_csr_to_csc_fill_block_u8(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m,
                                int64_t nnz, int64_t col_lo, int64_t col_hi, const int64_t* csc_indptr, int64_t* cursor,
                                int32_t* rows_out, void* perm_out, int perm_is_i64, const void* bytes, void* bytes_out,
                                be_stream_t stream) {
  BE_REQUIRE(bytes != nullptr && bytes_out != nullptr, BE_ERR_INVALID, "bytes / bytes_out is NULL");
  return fill_block(indices, indptr, indptr_is_i64, row_len, m, nnz, col_lo, col_hi, csc_indptr, cursor, rows_out, perm_out,
                    perm_is_i64, bytes, 1, bytes_out, true, stream, __func__);
}

int be_gather_by_perm(const void* src, int elem_bytes, const void* perm, int perm_is_i64, int64_t n, void* out,
                      be_stream_t stream) {
  BE_REQUIRE(n >= 0, BE_ERR_INVALID, "n < 0");
  if (n == 0) return BE_OK;
  BE_REQUIRE(src && perm && out, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for(n, 256, 256 * 16);
#define BE_GATHER(PT_, E_)                                                                                          \
  hipLaunchKernelGGL((k_gather_by_perm<PT_, E_>), dim3(grid), dim3(256), 0, st, static_cast<const E_*>(src),           \
                     static_cast<const PT_*>(perm), n, static_cast<E_*>(out))
  switch (elem_bytes) {
    case 2: if (perm_is_i64) BE_GATHER(int64_t, uint16_t); else BE_GATHER(int32_t, uint16_t); break;
    case 4: if (perm_is_i64) BE_GATHER(int64_t, uint32_t); else BE_GATHER(int32_t, uint32_t); break;
    case 8: if (perm_is_i64) BE_GATHER(int64_t, unsigned long long); else BE_GATHER(int32_t, unsigned long long); break;
    default: be_set_error("be_gather_by_perm: element size must be 2, 4 or 8"); return BE_ERR_INVALID;
  }
#undef BE_GATHER
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
