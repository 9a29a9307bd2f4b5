// be_arith.hip — container arithmetic on a stored pattern (brainevent_amd/_arith.py, brainevent_amd/_diag.py).
//
// 1. be_entries_dense_op: a dense operand sampled on the pattern, one value per stored entry e of row r(e), stored index c(e),
//      out[e] = op(w[e or 0], D[r(e) * s0 + c(e) * s1]),   op in {take, mul, div, rdiv}
//    — `csr * D`, `csr / D`, `D / csr` and the `take` every other callable is served through.  D is read in place through its
//    two int64 element strides (the host swaps them for the containers that store the transpose), in the weight dtype or as
//    uint8 (a mask).  One operation in f32 (f64 for f64) and one rounding; an entry whose row or stored index lies outside D
//    uses 0 and reads nothing through it.
//
// 2. diag_add (CSR / CSC): `A + diag(d)` with the missing diagonal entries inserted.  be_diag_scan finds, per row below
//    n_diag, the largest entry offset with c == r and the smallest with c > r (64-bit integer atomicMax / atomicMin on two words
//    per row: order-independent, so deterministic); the host turns them into a per-row plan (shift, insertion offset, offset of
//    the existing diagonal); be_diag_move relocates structure and / or values, new position = e + shift[r] + (inserted before
//    e); be_diag_fill writes the diagonal slots.  Every slot of the result is written by exactly one of move and fill, except
//    an existing diagonal, where fill overwrites move's copy in stream order.  No memset, no float atomics.
//
// Reference semantics (read as text): brainevent/_csr/main.py:1501-1593 (the dense operand of a binary operator),
// brainevent/_csr/diag_add.py:99-110, :196-238, :325-329.
//
// Work is balanced per entry, as k_sddmm / k_grad_rows do it: a tile is kTile consecutive entries with 64-bit offsets, the grid
// is capped and strides over the tiles beyond; a lane finds the row of its first entry by a binary search and walks forward (by
// a bounded search again as soon as the next row is empty).  In the sample and the move kernel a lane owns entry tile + lane,
// then every kThreads-th one (coalesced streams); in the scan kernel a lane owns kScanPer CONSECUTIVE entries, folds those of
// one row in registers and issues at most one pair of atomics per row run.  col / w loads and out stores are non-temporal
// (read-once streams).  No LDS, no scratch.
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

constexpr int kThreads = 256;    // threads per block
constexpr int kTile = 2048;      // entries per tile
constexpr int kGridCap = 4096;   // blocks; grid-strided over the tiles beyond
constexpr int kScanPer = kTile / kThreads;   // consecutive entries per lane of the scan kernel

enum { kOpTake = 0, kOpMul = 1, kOpDiv = 2, kOpRdiv = 3 };

// the last r in [lo, hi] with indptr[r] <= e (given indptr[lo] <= e); every probe lies in (lo, hi]
__device__ __forceinline__ int64_t row_in(const RowPtr& rp, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (rp.at(mid) <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The row walk shared by the three per-entry kernels: `r` / `row_end` describe the row of the previous entry of this lane;
// afterwards they describe the row of e (the LAST r with indptr[r] <= e; r stays below n_rows).  Returns whether r changed.
template <bool FIXED>
__device__ __forceinline__ bool row_of(const RowPtr& rp, int64_t n_rows, int64_t e, int64_t& r, int64_t& row_end) {
  if (e < row_end) return false;
  if (FIXED) {
    r = e / rp.fixed;
    row_end = (r + 1) * rp.fixed;
    return true;
  }
  if (r + 1 < n_rows) {
    ++r;
    row_end = rp.at(r + 1);
  }
  if (e >= row_end) {                 // an empty row (or more): search instead of walking
    r = row_in(rp, r, n_rows - 1, e);
    row_end = rp.at(r + 1);
  }
  return true;
}

template <bool FIXED>
__device__ __forceinline__ void row_first(const RowPtr& rp, int64_t n_rows, int64_t e, int64_t& r, int64_t& row_end) {
  if (FIXED) {
    r = e / rp.fixed;
    row_end = (r + 1) * rp.fixed;
  } else {
    r = row_in(rp, 0, n_rows - 1, e);
    row_end = rp.at(r + 1);
  }
}

// ------------------------------------------------------------------------------------------ the sampled dense operand
template <typename W, bool DU8, bool FIXED>
__global__ void __launch_bounds__(kThreads) k_entries_dense_op(typename PB<W>::bits* __restrict__ out,
                                                               const typename PB<W>::bits* __restrict__ w, int w_homo,
                                                               const int32_t* __restrict__ col, RowPtr rp, int64_t n_rows,
                                                               int64_t n_cols, int64_t nse, const void* __restrict__ dmat,
                                                               int64_t s0, int64_t s1, int op) {
  using ACC = typename PB<W>::acc;
  using B = typename PB<W>::bits;
  ACC w0 = 0;
  if (w_homo && op != kOpTake) w0 = PB<W>::get(w[0]);
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < nse; tile += (int64_t)gridDim.x * kTile) {
    int64_t e = tile + threadIdx.x;
    if (e >= nse) break;
    int64_t r, row_end;
    row_first<FIXED>(rp, n_rows, e, r, row_end);
    for (int u = 0; u < kTile / kThreads; ++u, e += kThreads) {
      if (e >= nse) break;
      row_of<FIXED>(rp, n_rows, e, r, row_end);
      const int64_t c = __builtin_nontemporal_load(col + e);
      ACC d = 0;
      // an index outside the operand gives 0 (nothing is read through it)
      if ((uint64_t)c < (uint64_t)n_cols && (uint64_t)r < (uint64_t)n_rows) {
        const int64_t at = r * s0 + c * s1;
        if (DU8) d = (ACC) static_cast<const uint8_t*>(dmat)[at];
        else d = PB<W>::get(static_cast<const B*>(dmat)[at]);
      }
      ACC v = d;
      if (op != kOpTake) {
        const ACC x = w_homo ? w0 : PB<W>::get(__builtin_nontemporal_load(w + e));
        v = op == kOpMul ? x * d : (op == kOpDiv ? x / d : d / x);
      }
      __builtin_nontemporal_store(PB<W>::put(v), out + e);
    }
  }
}

template <typename W>
int entries_dense_op_t(void* out, const void* w, int w_homo, const int32_t* col, RowPtr rp, int64_t n_rows, int64_t n_cols,
                       int64_t nse, const void* dmat, int d_is_u8, int64_t s0, int64_t s1, int op, hipStream_t st) {
  using B = typename PB<W>::bits;
  const int grid = grid_for(nse, kTile, kGridCap);
  const bool fixed = rp.p == nullptr;
  const int prof = be_prof_begin(st);
#define BE_ARITH_LAUNCH(DU8, FIXED)                                                                                        \
  hipLaunchKernelGGL((k_entries_dense_op<W, DU8, FIXED>), dim3(grid), dim3(kThreads), 0, st, static_cast<B*>(out),          \
                     static_cast<const B*>(w), w_homo, col, rp, n_rows, n_cols, nse, dmat, s0, s1, op)
  if (d_is_u8) {
    if (fixed) BE_ARITH_LAUNCH(true, true); else BE_ARITH_LAUNCH(true, false);
  } else {
    if (fixed) BE_ARITH_LAUNCH(false, true); else BE_ARITH_LAUNCH(false, false);
  }
#undef BE_ARITH_LAUNCH
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

// ------------------------------------------------------------------------------------------ diag_add: the row scan
// found [n_diag, 2] int64, set by the host to (-1, INT64_MAX): [r][0] <- max offset with c == r, [r][1] <- min offset with c > r
__device__ __forceinline__ void scan_flush(long long* __restrict__ found, int64_t r, int64_t n_diag, int64_t eq, int64_t gt) {
  if (r >= n_diag) return;
  if (eq >= 0) atomicMax(found + 2 * r, (long long)eq);
  if (gt != INT64_MAX) atomicMin(found + 2 * r + 1, (long long)gt);
}

__global__ void __launch_bounds__(kThreads) k_diag_scan(const int32_t* __restrict__ col, RowPtr rp, int64_t n_rows,
                                                        int64_t n_diag, int64_t nse, long long* __restrict__ found) {
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < nse; tile += (int64_t)gridDim.x * kTile) {
    int64_t e = tile + (int64_t)threadIdx.x * kScanPer;
    if (e >= nse) continue;                       // (the lanes behind it are past the end too; other tiles of this block are not)
    int64_t r, row_end;
    row_first<false>(rp, n_rows, e, r, row_end);
    int64_t eq = -1, gt = INT64_MAX;
    for (int u = 0; u < kScanPer; ++u, ++e) {
      if (e >= nse) break;
      const int64_t prev = r;
      if (row_of<false>(rp, n_rows, e, r, row_end)) {
        scan_flush(found, prev, n_diag, eq, gt);
        eq = -1;
        gt = INT64_MAX;
      }
      const int64_t c = __builtin_nontemporal_load(col + e);
      if (c == r) eq = e;                         // (ascending e: the last one stays)
      else if (c > r && gt == INT64_MAX) gt = e;  // (the first one stays)
    }
    scan_flush(found, r, n_diag, eq, gt);
  }
}

// ------------------------------------------------------------------------------------------ diag_add: move and fill
// dst(e) = e + shift[r] + (ins[r] >= 0 && ins[r] <= e).  Any of new_indices / nd / old_to_new may be NULL.
template <typename W>
__global__ void __launch_bounds__(kThreads) k_diag_move(const typename PB<W>::bits* __restrict__ w, int w_homo,
                                                        const int32_t* __restrict__ col, RowPtr rp, int64_t n_rows, int64_t nse,
                                                        const int64_t* __restrict__ shift, const int64_t* __restrict__ ins,
                                                        int64_t new_nse, int32_t* __restrict__ new_indices,
                                                        typename PB<W>::bits* __restrict__ nd, void* __restrict__ old_to_new,
                                                        int o2n_is64) {
  using B = typename PB<W>::bits;
  B w0 = 0;
  if (nd != nullptr && w_homo) w0 = w[0];
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < nse; tile += (int64_t)gridDim.x * kTile) {
    int64_t e = tile + threadIdx.x;
    if (e >= nse) break;
    int64_t r, row_end;
    row_first<false>(rp, n_rows, e, r, row_end);
    int64_t sh = shift[r], at = ins[r];
    for (int u = 0; u < kTile / kThreads; ++u, e += kThreads) {
      if (e >= nse) break;
      if (row_of<false>(rp, n_rows, e, r, row_end)) {
        sh = shift[r];
        at = ins[r];
      }
      const int64_t dst = e + sh + ((uint64_t)at <= (uint64_t)e ? 1 : 0);
      if ((uint64_t)dst >= (uint64_t)new_nse) continue;       // (a plan that does not belong to this structure writes nothing)
      if (new_indices != nullptr) __builtin_nontemporal_store(__builtin_nontemporal_load(col + e), new_indices + dst);
      if (nd != nullptr) __builtin_nontemporal_store(w_homo ? w0 : __builtin_nontemporal_load(w + e), nd + dst);
      if (old_to_new != nullptr) {
        if (o2n_is64) __builtin_nontemporal_store(dst, static_cast<int64_t*>(old_to_new) + e);
        else __builtin_nontemporal_store((int32_t)dst, static_cast<int32_t*>(old_to_new) + e);
      }
    }
  }
}

// one thread per diagonal element i: dest = (exist[i] >= 0 ? exist[i] : ins[i]) + shift[i]
template <typename W>
__global__ void __launch_bounds__(kThreads) k_diag_fill(const typename PB<W>::bits* __restrict__ w, int w_homo, int64_t nse,
                                                        int64_t n_diag, const int64_t* __restrict__ shift,
                                                        const int64_t* __restrict__ ins, const int64_t* __restrict__ exist,
                                                        const typename PB<W>::bits* __restrict__ d, int64_t new_nse,
                                                        int32_t* __restrict__ new_indices, typename PB<W>::bits* __restrict__ nd) {
  using ACC = typename PB<W>::acc;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_diag; i += (int64_t)gridDim.x * kThreads) {
    const int64_t src = exist[i];
    const int64_t dest = (src >= 0 ? src : ins[i]) + shift[i];
    if ((uint64_t)dest >= (uint64_t)new_nse) continue;
    if (src < 0 && new_indices != nullptr) new_indices[dest] = (int32_t)i;
    if (nd != nullptr) {
      ACC v = 0;
      if (src >= 0 && src < nse) v = PB<W>::get(w[w_homo ? 0 : src]);
      nd[dest] = PB<W>::put(v + PB<W>::get(d[i]));
    }
  }
}

template <typename W>
int diag_move_t(const void* w, int w_homo, const int32_t* col, RowPtr rp, int64_t n_rows, int64_t nse, const int64_t* shift,
                const int64_t* ins, int64_t new_nse, int32_t* new_indices, void* nd, void* old_to_new, int o2n_is64,
                hipStream_t st) {
  using B = typename PB<W>::bits;
  const int prof = be_prof_begin(st);
  hipLaunchKernelGGL((k_diag_move<W>), dim3(grid_for(nse, kTile, kGridCap)), dim3(kThreads), 0, st, static_cast<const B*>(w),
                     w_homo, col, rp, n_rows, nse, shift, ins, new_nse, new_indices, static_cast<B*>(nd), old_to_new, o2n_is64);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int diag_fill_t(const void* w, int w_homo, int64_t nse, int64_t n_diag, const int64_t* shift, const int64_t* ins,
                const int64_t* exist, const void* d, int64_t new_nse, int32_t* new_indices, void* nd, hipStream_t st) {
  using B = typename PB<W>::bits;
  const int prof = be_prof_begin(st);
  hipLaunchKernelGGL((k_diag_fill<W>), dim3(grid_for(n_diag, kThreads, kGridCap)), dim3(kThreads), 0, st,
                     static_cast<const B*>(w), w_homo, nse, n_diag, shift, ins, exist, static_cast<const B*>(d), new_nse,
                     new_indices, static_cast<B*>(nd));
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int be_entries_dense_op(void* out, const void* weights, int w_homo, int wdtype, const int32_t* indices, const void* indptr,
                        int indptr_is_i64, int64_t row_len, int64_t n_rows, int64_t n_cols, int64_t nse, const void* dense,
                        int dense_is_u8, int64_t stride_row, int64_t stride_col, int op, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && nse >= 0, BE_ERR_INVALID, "shape out of range");
  BE_REQUIRE(op >= kOpTake && op <= kOpRdiv, BE_ERR_INVALID, "unknown op (0 take, 1 mul, 2 div, 3 rdiv)");
  if (nse == 0) return BE_OK;
  BE_REQUIRE(out && indices && dense, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(weights || op == kOpTake, BE_ERR_INVALID, "null weights");
  BE_REQUIRE(n_rows > 0, BE_ERR_INVALID, "entries but no row");
  if (indptr == nullptr) {
    BE_REQUIRE(row_len > 0, BE_ERR_INVALID, "no row source: indptr or a fixed row length > 0");
    BE_REQUIRE((nse + row_len - 1) / row_len <= n_rows, BE_ERR_INVALID, "more entries than n_rows rows of row_len hold");
  }
  const RowPtr rp{indptr, indptr_is_i64, row_len};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return entries_dense_op_t<W>(out, weights, w_homo, indices, rp, n_rows, n_cols, nse, dense, dense_is_u8, stride_row, stride_col, op,
                                 st);
  });
}

int be_diag_scan(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n_rows, int64_t n_diag, int64_t nse,
                 void* found, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && nse >= 0 && n_diag >= 0 && n_diag <= n_rows, BE_ERR_INVALID, "shape out of range");
  if (nse == 0 || n_diag == 0) return BE_OK;
  BE_REQUIRE(indices && indptr && found, BE_ERR_INVALID, "null pointer");
  const RowPtr rp{indptr, indptr_is_i64, -1};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int prof = be_prof_begin(st);
  hipLaunchKernelGGL(k_diag_scan, dim3(grid_for(nse, kTile, kGridCap)), dim3(kThreads), 0, st, indices, rp, n_rows, n_diag, nse,
                     static_cast<long long*>(found));
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_diag_move(const void* weights, int w_homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                 int64_t n_rows, int64_t nse, const int64_t* shift, const int64_t* ins, int64_t new_nse, int32_t* new_indices,
                 void* new_data, void* old_to_new, int old_to_new_is_i64, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && nse >= 0 && new_nse >= nse, BE_ERR_INVALID, "shape out of range");
  if (nse == 0 || (!new_indices && !new_data && !old_to_new)) return BE_OK;
  BE_REQUIRE(indices && indptr && shift && ins, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(n_rows > 0, BE_ERR_INVALID, "entries but no row");
  BE_REQUIRE(weights || !new_data, BE_ERR_INVALID, "values to move but no weights");
  const RowPtr rp{indptr, indptr_is_i64, -1};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return be_dispatch_wdtype(new_data ? wdtype : BE_F32, [&](auto w) {
    using T = typename decltype(w)::type;
    using W = std::conditional_t<std::is_same_v<T, __hip_bfloat16>, __half, T>;      // (a move of 16-bit patterns)
    return diag_move_t<W>(weights, w_homo, indices, rp, n_rows, nse, shift, ins, new_nse, new_indices, new_data, old_to_new,
                          old_to_new_is_i64, st);
  });
}

int be_diag_fill(const void* weights, int w_homo, int wdtype, int64_t nse, int64_t n_diag, const int64_t* shift,
                 const int64_t* ins, const int64_t* exist, const void* diag, int64_t new_nse, int32_t* new_indices,
                 void* new_data, be_stream_t stream) {
  BE_REQUIRE(nse >= 0 && n_diag >= 0 && new_nse >= 0, BE_ERR_INVALID, "shape out of range");
  if (n_diag == 0 || (!new_indices && !new_data)) return BE_OK;
  BE_REQUIRE(shift && ins && exist, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(!new_data || (diag && (weights || nse == 0)), BE_ERR_INVALID, "values to write but no weights / diagonal");
  hipStream_t st = static_cast<hipStream_t>(stream);
  return be_dispatch_wdtype(new_data ? wdtype : BE_F32, [&](auto w) {
    using W = typename decltype(w)::type;
    return diag_fill_t<W>(weights, w_homo, nse, n_diag, shift, ins, exist, diag, new_nse, new_indices, new_data, st);
  });
}

}  // extern "C"
