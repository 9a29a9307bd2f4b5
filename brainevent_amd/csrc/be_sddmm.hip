// be_sddmm.hip — the sampled dense-dense product on a stored pattern: one value per stored entry,
//   out[e] = sum_{b < nb} P[r(e), b] * Q[c(e), b]
// with r(e) / c(e) the row / stored index of entry e, P [n_rows, nb] and Q [n_cols, nb] neuron-major (contiguous in b), all in
// the weight dtype.  It is the weight gradient of the float-operand products (brainevent_amd/_autograd.py: A @ X -> P = g,
// Q = X; A.T @ X -> P = X, Q = g) and the public sddmm_* / M.sddmm (brainevent_amd/_sddmm.py).
//
// Reference semantics (read as text): brainevent/_sddmm.py (sddmm_indices / sddmm_coo_indices), brainevent/_csr/float.py:825-860
// (the mm weight rule), :287-330 (mv: nb = 1).
//
// Work is balanced per entry, as k_grad_rows does it: a tile is kTile consecutive entries, a group of LPE lanes owns entry
// tile + group, then every (kThreads / LPE)-th one; it finds the row of its first entry by a search and walks forward (by a
// bounded search again as soon as the next row is empty).  The row comes from one of three sources: an indptr (int32 / int64),
// a fixed row length, or an explicit row_ids[e] array (COO).  Entry offsets are 64-bit.  Every entry is written exactly once
// by one lane: no memset, no atomics.
//
// Lanes per entry depend on nb and the dtype only (lanes_for): with V = kVecBytes / sizeof(element), 1 lane up to V elements,
// 2 up to 2 V, 4, 8, and kMaxLanes beyond 8 V.  Lane s of a group takes the elements [j0, j0 + V) for j0 = s V, (s + LPE) V, ...
// in ascending order into ONE accumulator (f32; f64 for f64) by explicit fused multiply-adds, then the group adds its
// accumulators by a fixed xor-shuffle tree, and lane 0 rounds once to the weight dtype.  Whether the V elements arrive as one
// 16-byte load (nb a multiple of V and both operands on a 16-byte boundary) or one by one does not change that order, and
// neither do the grid, the row lengths, the row source or the place of the entry in its tile: the result of an entry is a pure
// function of (its operands, nb, dtype).  P[r, :] is shared by a row and stays in cache; Q[c, :] is a gather of nb contiguous
// elements.  No LDS.
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

constexpr int kThreads = 256;    // threads per block
constexpr int kTile = 2048;      // entries per tile
constexpr int kGridCap = 4096;   // blocks; grid-strided over the tiles beyond
constexpr int kVecBytes = 16;    // bytes of P (and of Q) per lane and trip
constexpr int kMaxLanes = 16;    // lanes per entry at most

enum { kSrcPtr = 0, kSrcFixed = 1, kSrcCoo = 2 };

__device__ __forceinline__ float fma_acc(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_acc(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the last r in [lo, hi] with indptr[r] <= e (given indptr[lo] <= e); every probe lies in (lo, hi]
__device__ __forceinline__ int64_t row_in(const RowPtr& rp, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (rp.at(mid) <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename W, int SRC, int LPE, bool VEC>
__global__ void __launch_bounds__(kThreads) k_sddmm(typename PB<W>::bits* __restrict__ out, const int32_t* __restrict__ col,
                                                    RowPtr rp, const int32_t* __restrict__ row_ids, int64_t n_rows,
                                                    int64_t n_cols, int64_t nse, const typename PB<W>::bits* __restrict__ P,
                                                    const typename PB<W>::bits* __restrict__ Q, int nb) {
  using ACC = typename PB<W>::acc;
  using B = typename PB<W>::bits;
  constexpr int V = kVecBytes / (int)sizeof(B);
  constexpr int G = kThreads / LPE;           // entries in flight per block
  const int sub = threadIdx.x % LPE, grp = threadIdx.x / LPE;
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < nse; tile += (int64_t)gridDim.x * kTile) {
    int64_t e = tile + grp;
    if (e >= nse) break;
    int64_t r = 0, row_end = 0;
    if (SRC == kSrcFixed) {
      r = e / rp.fixed;
      row_end = (r + 1) * rp.fixed;
    } else if (SRC == kSrcPtr) {
      r = row_in(rp, 0, n_rows - 1, e);       // (empty rows are stepped over: the LAST r with indptr[r] <= e)
      row_end = rp.at(r + 1);
    }
    for (int u = 0; u < kTile / G; ++u, e += G) {
      if (e >= nse) break;
      if (SRC == kSrcCoo) {
        r = __builtin_nontemporal_load(row_ids + e);
      } else if (e >= row_end) {
        if (SRC == kSrcFixed) {
          r = e / rp.fixed;
          row_end = (r + 1) * rp.fixed;
        } else {
          if (r + 1 < n_rows) {
            ++r;
            row_end = rp.at(r + 1);
          }
          if (e >= row_end) {                 // an empty row (or more): search instead of walking; r stays below n_rows
            r = row_in(rp, r, n_rows - 1, e);
            row_end = rp.at(r + 1);
          }
        }
      }
      const int64_t c = __builtin_nontemporal_load(col + e);
      ACC acc = 0;
      // an index outside the operands gives 0 (nothing is read through it)
      if ((uint64_t)c < (uint64_t)n_cols && (uint64_t)r < (uint64_t)n_rows) {
        const B* __restrict__ p = P + r * nb;
        const B* __restrict__ q = Q + c * nb;
        for (int j0 = sub * V; j0 < nb; j0 += LPE * V) {
          if (VEC) {
            B pv[V], qv[V];
            const be_v4u pq = *reinterpret_cast<const be_v4u*>(p + j0);
            const be_v4u qq = *reinterpret_cast<const be_v4u*>(q + j0);
            __builtin_memcpy(pv, &pq, kVecBytes);
            __builtin_memcpy(qv, &qq, kVecBytes);
#pragma unroll
            for (int j = 0; j < V; ++j) acc = fma_acc(PB<W>::get(pv[j]), PB<W>::get(qv[j]), acc);
          } else {
            const int j1 = j0 + V < nb ? j0 + V : nb;
            for (int j = j0; j < j1; ++j) acc = fma_acc(PB<W>::get(p[j]), PB<W>::get(q[j]), acc);
          }
        }
      }
#pragma unroll
      for (int off = LPE >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      if (sub == 0) __builtin_nontemporal_store(PB<W>::put(acc), out + e);
    }
  }
}

// ------------------------------------------------------------------------------------------ host
// lanes per entry: a function of nb and the element size only
int lanes_for(int64_t nb, int elem_bytes) {
  const int64_t v = kVecBytes / elem_bytes;
  if (nb <= v) return 1;
  if (nb <= 2 * v) return 2;
  if (nb <= 4 * v) return 4;
  if (nb <= 8 * v) return 8;
  return kMaxLanes;
}

template <typename W, int SRC, int LPE>
void launch_sddmm(void* out, const int32_t* col, RowPtr rp, const int32_t* row_ids, int64_t n_rows, int64_t n_cols, int64_t nse,
                  const void* p, const void* q, int nb, bool vec, hipStream_t st) {
  using B = typename PB<W>::bits;
  const int grid = grid_for(nse, kTile, kGridCap);
  if (vec)
    hipLaunchKernelGGL((k_sddmm<W, SRC, LPE, true>), dim3(grid), dim3(kThreads), 0, st, static_cast<B*>(out), col, rp, row_ids,
                       n_rows, n_cols, nse, static_cast<const B*>(p), static_cast<const B*>(q), nb);
  else
    hipLaunchKernelGGL((k_sddmm<W, SRC, LPE, false>), dim3(grid), dim3(kThreads), 0, st, static_cast<B*>(out), col, rp, row_ids,
                       n_rows, n_cols, nse, static_cast<const B*>(p), static_cast<const B*>(q), nb);
}

template <typename W, int SRC>
void launch_lanes(void* out, const int32_t* col, RowPtr rp, const int32_t* row_ids, int64_t n_rows, int64_t n_cols, int64_t nse,
                  const void* p, const void* q, int nb, hipStream_t st) {
  constexpr int kElem = (int)sizeof(typename PB<W>::bits);
  const bool vec = nb % (kVecBytes / kElem) == 0 && reinterpret_cast<uintptr_t>(p) % kVecBytes == 0 &&
                   reinterpret_cast<uintptr_t>(q) % kVecBytes == 0;
  switch (lanes_for(nb, kElem)) {
    case 1:  launch_sddmm<W, SRC, 1>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, vec, st); break;
    case 2:  launch_sddmm<W, SRC, 2>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, vec, st); break;
    case 4:  launch_sddmm<W, SRC, 4>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, vec, st); break;
    case 8:  launch_sddmm<W, SRC, 8>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, vec, st); break;
    default: launch_sddmm<W, SRC, kMaxLanes>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, vec, st); break;
  }
}

template <typename W>
int sddmm_t(int src, void* out, const int32_t* col, RowPtr rp, const int32_t* row_ids, int64_t n_rows, int64_t n_cols,
            int64_t nse, const void* p, const void* q, int nb, hipStream_t st) {
  const int prof = be_prof_begin(st);
  if (src == kSrcCoo) launch_lanes<W, kSrcCoo>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, st);
  else if (src == kSrcFixed) launch_lanes<W, kSrcFixed>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, st);
  else launch_lanes<W, kSrcPtr>(out, col, rp, row_ids, n_rows, n_cols, nse, p, q, nb, st);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int be_sddmm_rows(void* out, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                  const int32_t* row_ids, int64_t n_rows, int64_t n_cols, int64_t nse, const void* p, const void* q,
                  int64_t n_batch, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && nse >= 0 && n_batch >= 0 && n_batch <= (1ll << 30), BE_ERR_INVALID,
             "shape out of range");
  if (nse == 0 || n_batch == 0 || n_rows == 0) return BE_OK;
  BE_REQUIRE(out && indices && p && q, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(n_cols > 0, BE_ERR_INVALID, "entries but no column");
  int src;
  if (row_ids != nullptr) {
    src = kSrcCoo;
  } else if (indptr != nullptr) {
    src = kSrcPtr;
  } else {
    BE_REQUIRE(row_len > 0, BE_ERR_INVALID, "no row source: indptr, row_ids or a fixed row length > 0");
    BE_REQUIRE((nse + row_len - 1) / row_len <= n_rows, BE_ERR_INVALID, "more entries than n_rows rows of row_len hold");
    src = kSrcFixed;
  }
  const RowPtr rp{src == kSrcPtr ? indptr : nullptr, indptr_is_i64, row_len};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = (int)n_batch;
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return sddmm_t<W>(src, out, indices, rp, row_ids, n_rows, n_cols, nse, p, q, nb, st);
  });
}

}  // extern "C"
