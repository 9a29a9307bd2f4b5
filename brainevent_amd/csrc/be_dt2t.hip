// be_dt2t.hip — the per-synapse products ("dt2t"): one output per stored entry, the entry's value scaled by a per-neuron factor.
//
// Reference semantics (read as text): brainevent/_csr/dt2t.py:237-300 (csrmv_dt2t CPU loops), :690-760 (csrmm_dt2t),
// brainevent/_fcn/dt2t.py:173-175, :342-344.  For every batch row b and stored entry j of row r(j) with stored index c(j):
//   by row:     out[b, j] = w[b, j] * y[b, r(j)]
//   by column:  out[b, j] = w[b, j] * y[b, c(j)]
// the product formed in f32 (f64 for f64) and rounded once to the weight dtype.  homo: w is one shared value w[0].
//
// The operation is a stream — read w, write out, a few bytes of structure — so all three kernels are entry-centric: a tile
// is kTile = kThreads * kRuns * V consecutive entries (V = the entries of the dtype in kVecBytes), a thread owns kRuns runs
// of V entries, one 16-byte load of w and one 16-byte store of out each, both non-temporal.  Tiles are laid out from the
// 16-byte boundary at or below out's first element ("virtual" positions v = j + pad), so that the stores of full runs are
// aligned whatever view the caller passes; the runs that hang over either end of the array go entry by entry, and a w or
// indices stream whose phase differs from out's is read entry by entry too.  Each entry is read by the one thread that
// writes it, and before it writes: out == w is safe.
//
// By row with an indptr, the row of an entry is never searched from the whole array per thread: the block finds the rows of
// the first and the last entry of its tile (waves 0 and 1, a 64-way search each: the last r with indptr[r] <= j, which
// steps over runs of empty rows), a thread then places the first entry of each of its runs by a binary search inside that
// range and steps forward as its entries cross row ends — one row at a time, and by another bounded search as soon as
// the next row is empty.  Work per block therefore does not depend on how the entries are spread over the rows.
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

constexpr int kThreads = 256;   // threads per block
constexpr int kVecBytes = 16;   // bytes of w (and of out) per run
constexpr int kRuns = 2;        // runs per thread in one tile
constexpr int kGridCap = 2048;  // blocks over all batch rows (256 CUs x 8 resident blocks); grid-strided beyond

enum { kByCol = 0, kByRowFixed = 1, kByRowPtr = 2 };

// ------------------------------------------------------------------------------------------ 16-byte streams
template <typename B, int V>
__device__ __forceinline__ void load_run(const B* p, bool aligned, B (&v)[V]) {
  if (aligned) {
    const be_v4u q = __builtin_nontemporal_load(reinterpret_cast<const be_v4u*>(p));
    __builtin_memcpy(v, &q, kVecBytes);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = __builtin_nontemporal_load(p + e);
  }
}

template <typename B, int V>
__device__ __forceinline__ void store_run(B* p, const B (&v)[V]) {
  be_v4u q;
  __builtin_memcpy(&q, v, kVecBytes);
  __builtin_nontemporal_store(q, reinterpret_cast<be_v4u*>(p));
}

// the V indices beside one run: 8 bytes (f64), 16 (f32) or 2 x 16 (f16 / bf16)
template <int V>
__device__ __forceinline__ void load_idx(const int32_t* p, bool aligned, int32_t (&c)[V]) {
  if (aligned) {
    if constexpr (V == 2) {
      const be_v2u q = __builtin_nontemporal_load(reinterpret_cast<const be_v2u*>(p));
      __builtin_memcpy(c, &q, 8);
    } else {
#pragma unroll
      for (int h = 0; h < V / 4; ++h) {
        const be_v4u q = __builtin_nontemporal_load(reinterpret_cast<const be_v4u*>(p) + h);
        __builtin_memcpy(c + 4 * h, &q, 16);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) c[e] = __builtin_nontemporal_load(p + e);
  }
}

// ------------------------------------------------------------------------------------------ rows of entries
// the last r in [lo, hi] with indptr[r] <= j (given indptr[lo] <= j); every probe lies in (lo, hi]
__device__ __forceinline__ int64_t row_in(const RowPtr& rp, int64_t lo, int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (rp.at(mid) <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the same over [0, n_rows - 1] by a whole wave: 64 probes a round (1M rows: 4 rounds of one load instead of 20)
__device__ __forceinline__ int64_t wave_row_of(const RowPtr& rp, int64_t n_rows, int64_t j) {
  int64_t lo = 0, hi = n_rows - 1;
  const int64_t lane1 = lane_id() + 1;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t p = lo + lane1 * step;
    const bool le = p <= hi && rp.at(p) <= j;
    const int64_t c = __popcll(__ballot(le));      // the probes that hold form a prefix (indptr ascends)
    const int64_t top = lo + (c + 1) * step - 1;
    lo += c * step;
    hi = top < hi ? top : hi;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------ the kernel
// w and out may be the same array: neither is __restrict__.
template <typename W, int MODE, bool HOMO>
__global__ void __launch_bounds__(kThreads) k_dt2t(const typename PB<W>::bits* w, const typename PB<W>::bits* __restrict__ y,
                                                   const int32_t* __restrict__ idx, RowPtr rp, typename PB<W>::bits* out,
                                                   int64_t n_rows, int64_t n_y, int64_t nnz) {
  using B = typename PB<W>::bits;
  using ACC = typename PB<W>::acc;
  constexpr int V = kVecBytes / (int)sizeof(B);
  constexpr int64_t kTile = (int64_t)kThreads * kRuns * V;
  constexpr int kIdxAlign = V * 4 < kVecBytes ? V * 4 : kVecBytes;

  const int64_t b = blockIdx.y;
  const B* wb = HOMO ? w : w + b * nnz;
  B* ob = out + b * nnz;
  const B* yb = y + b * n_y;
  const int64_t pad = (int64_t)(reinterpret_cast<uintptr_t>(ob) % kVecBytes) / (int64_t)sizeof(B);
  const int64_t vend = pad + nnz;
  const bool w_al = HOMO || reinterpret_cast<uintptr_t>(wb) % kVecBytes == reinterpret_cast<uintptr_t>(ob) % kVecBytes;
  const bool i_al = MODE != kByCol || (reinterpret_cast<uintptr_t>(idx) + 64 - (uintptr_t)pad * 4) % kIdxAlign == 0;
  ACC w_homo = 0;
  if (HOMO) w_homo = PB<W>::get(w[0]);
  __shared__ int64_t s_rows[2];

  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < vend; tile += (int64_t)gridDim.x * kTile) {
    // the read-once streams first: they are in flight while the rows are searched
    B wv[kRuns][V];
    int32_t cv[kRuns][V];
#pragma unroll
    for (int u = 0; u < kRuns; ++u) {
      const int64_t v0 = tile + ((int64_t)u * kThreads + threadIdx.x) * V;
      const int64_t j = v0 - pad;
      if (v0 >= pad && v0 + V <= vend) {
        if (!HOMO) load_run<B, V>(wb + j, w_al, wv[u]);
        if (MODE == kByCol) load_idx<V>(idx + j, i_al, cv[u]);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int64_t jj = j + e;
          const bool on = jj >= 0 && jj < nnz;
          wv[u][e] = 0;
          cv[u][e] = 0;
          if (on && !HOMO) wv[u][e] = wb[jj];
          if (on && MODE == kByCol) cv[u][e] = idx[jj];
        }
      }
    }

    int64_t r_lo = 0, r_hi = 0;
    if (MODE == kByRowPtr) {
      // rows of the tile's first and last entry (0 <= j_first <= j_last < nnz: tile < vend and pad < V <= kTile)
      const int64_t j_first = tile > pad ? tile - pad : 0;
      const int64_t j_last = (tile + kTile < vend ? tile + kTile : vend) - pad - 1;
      const int wave = threadIdx.x >> 6;
      if (wave < 2) {
        const int64_t r = wave_row_of(rp, n_rows, wave ? j_last : j_first);
        if (lane_id() == 0) s_rows[wave] = r;
      }
      __syncthreads();
      r_lo = s_rows[0];
      r_hi = s_rows[1];
      __syncthreads();          // (the next trip writes s_rows again)
    }

#pragma unroll
    for (int u = 0; u < kRuns; ++u) {
      const int64_t v0 = tile + ((int64_t)u * kThreads + threadIdx.x) * V;
      const int64_t j = v0 - pad;
      if (v0 >= vend || v0 + V <= pad) continue;           // no entry of the array in this run
      const bool full = v0 >= pad && v0 + V <= vend;
      B ov[V];
      if (MODE == kByCol) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int64_t jj = j + e;
          ov[e] = 0;
          if (full || (jj >= 0 && jj < nnz))
            ov[e] = PB<W>::put((HOMO ? w_homo : PB<W>::get(wv[u][e])) * PB<W>::get(yb[cv[u][e]]));
        }
      } else {
        const int64_t j_run = j < 0 ? 0 : j;               // first entry of the run that exists
        int64_t r, row_end;
        if (MODE == kByRowFixed) {
          r = j_run / rp.fixed;                            // one division per run
          row_end = (r + 1) * rp.fixed;
        } else {
          r = row_in(rp, r_lo, r_hi, j_run);
          row_end = rp.at(r + 1);
        }
        ACC yr = PB<W>::get(yb[r]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int64_t jj = j + e;
          ov[e] = 0;
          if (!(full || (jj >= 0 && jj < nnz))) continue;
          if (MODE == kByRowFixed) {
            if (jj >= row_end) {
              do { ++r; row_end += rp.fixed; } while (jj >= row_end);
              yr = PB<W>::get(yb[r]);
            }
          } else if (jj >= row_end && r < r_hi) {           // (r never leaves the tile's rows, whatever indptr holds)
            ++r;
            row_end = rp.at(r + 1);
            if (jj >= row_end) {                           // an empty row: search instead of walking a run of them
              r = row_in(rp, r, r_hi, jj);
              row_end = rp.at(r + 1);
            }
            yr = PB<W>::get(yb[r]);
          }
          ov[e] = PB<W>::put((HOMO ? w_homo : PB<W>::get(wv[u][e])) * yr);
        }
      }
      if (full) {
        store_run<B, V>(ob + j, ov);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int64_t jj = j + e;
          if (jj >= 0 && jj < nnz) ob[jj] = ov[e];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host
template <typename W, int MODE, bool HOMO>
void launch_dt2t(const void* w, const void* y, const int32_t* idx, RowPtr rp, void* out, int64_t n_rows, int64_t n_y,
                 int64_t n_batch, int64_t nnz, hipStream_t st) {
  using B = typename PB<W>::bits;
  constexpr int V = kVecBytes / (int)sizeof(B);
  constexpr int64_t kTile = (int64_t)kThreads * kRuns * V;
  const int64_t cap = kGridCap / n_batch > 1 ? kGridCap / n_batch : 1;
  const int gx = grid_for(nnz + V - 1, (int)kTile, (int)cap);          // (+ V - 1: the largest pad)
  hipLaunchKernelGGL((k_dt2t<W, MODE, HOMO>), dim3(gx, (unsigned)n_batch), dim3(kThreads), 0, st, static_cast<const B*>(w),
                     static_cast<const B*>(y), idx, rp, static_cast<B*>(out), n_rows, n_y, nnz);
}

template <typename W>
int dt2t_t(int mode, int homo, const void* w, const void* y, const int32_t* idx, RowPtr rp, void* out, int64_t n_rows,
           int64_t n_y, int64_t n_batch, int64_t nnz, hipStream_t st) {
  const int prof = be_prof_begin(st);
#define BE_DT2T_MODE(M)                                                                              \
  if (homo) launch_dt2t<W, M, true>(w, y, idx, rp, out, n_rows, n_y, n_batch, nnz, st);              \
  else launch_dt2t<W, M, false>(w, y, idx, rp, out, n_rows, n_y, n_batch, nnz, st)
  if (mode == kByCol) { BE_DT2T_MODE(kByCol); }
  else if (mode == kByRowFixed) { BE_DT2T_MODE(kByRowFixed); }
  else { BE_DT2T_MODE(kByRowPtr); }
#undef BE_DT2T_MODE
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int be_dt2t(const void* w, int homo, int wdtype, const void* y, const int32_t* indices, const void* indptr, int indptr_is_i64,
            int64_t row_len, void* out, int64_t n_rows, int64_t n_cols, int64_t n_batch, int64_t nnz, int by_col,
            be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0 && n_batch >= 0 && n_batch <= kMaxBatch, BE_ERR_INVALID, "shape out of range");
  if (nnz == 0 || n_batch == 0) return BE_OK;
  BE_REQUIRE(w && y && out, BE_ERR_INVALID, "null pointer");
  int mode;
  if (by_col) {
    BE_REQUIRE(indices != nullptr, BE_ERR_INVALID, "by column needs the indices");
    BE_REQUIRE(n_cols > 0, BE_ERR_INVALID, "entries but no column");
    mode = kByCol;
  } else if (indptr == nullptr) {
    BE_REQUIRE(row_len > 0, BE_ERR_INVALID, "fixed row length <= 0 without indptr");
    BE_REQUIRE((nnz + row_len - 1) / row_len <= n_rows, BE_ERR_INVALID, "more entries than n_rows rows of row_len hold");
    mode = kByRowFixed;
  } else {
    BE_REQUIRE(n_rows > 0, BE_ERR_INVALID, "entries but no row");
    mode = kByRowPtr;
  }
  const RowPtr rp{by_col ? nullptr : indptr, indptr_is_i64, row_len};
  const int64_t n_y = by_col ? n_cols : n_rows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return be_dispatch_wdtype(wdtype, [&](auto tag) {
    using W = typename decltype(tag)::type;
    return dt2t_t<W>(mode, homo, w, y, indices, rp, out, n_rows, n_y, n_batch, nnz, st);
  });
}

}  // extern "C"
