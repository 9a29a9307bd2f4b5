// be_slice.hip — reading rows out of a stored matrix: W[rows] as a dense block, its gradient, and the sparse sub-matrix.
//
// Reference semantics (read as text): brainevent/_csr/slice.py:97-115 (csr_slice_rows CPU loops), :353-360 (its gradient),
// brainevent/_misc.py:1199-1252 (build_sub_csr).  With rows[k] the k-th selected row of a CSR reading (indices, indptr) —
// indptr NULL + row_len for fixed-length rows:
//   forward:  out[k, c] = sum of data[j] over the entries j of row rows[k] with indices[j] == c, zero elsewhere
//   gradient: dw[j]     = sum of ct[k, indices[j]] over the k with rows[k] == row(j), zero for the rows not selected
//   copy:     the indices (and data) segments of the selected rows, one after the other, at the places new_indptr names
// A row index outside [0, n_rows) is a zero row forward and contributes nothing backward (the reference's kernel rule).
//
// Bit-reproducible, no float atomics.  Duplicate column ids inside a row are summed in ascending storage order j, in f32
// (f64 for f64), and rounded once — the reference sums f16 in f16; this is be_grad.hip's rule.  One shared weight: the
// entries of a column are COUNTED (LDS integer atomics) and out = count * w, one product — the reference adds w repeatedly.
//
// Forward: one workgroup owns (k, column tile); the tile is an accumulator and an int32 owner word per column in LDS, and the
// workgroup streams the whole row (so the cost grows as ceil(n_cols / tile) x row length).  Per-entry weights keep the
// ascending-j order in rounds: every unresolved entry of a pass does an LDS atomicMin of its position on its column's owner
// word; after a barrier the one winner per column adds its value with a plain read-modify-write, retires and resets the
// word; the losers repeat.  The rounds of a pass are the largest multiplicity in it; a block-wide vote ends the loop after
// the first round when nothing lost.  Every element of out is written by the kernel, zeros included: no memset.
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

constexpr int kThreads = 256;         // threads per block (all three kernels)
constexpr int kTileCols = 4096;       // columns per forward tile with an f32 accumulator (f32 / f16 / bf16): 32 KB of LDS
constexpr int kTileColsF64 = 2048;    // ... with an f64 accumulator: 24 KB
constexpr int kPer = 8;               // entries per thread in one pass over a row (forward, per-entry weights)
constexpr int kVecBytes = 16;         // widest store of out
constexpr int kGradSplit = 8;         // blocks that share one selected row in the gradient (per-entry weights)
constexpr int kCopyPer = 4;           // entries per thread in one tile of the copy
constexpr int kGridCap = 1 << 22;     // blocks in x (x threads: below 2^31); grid-strided beyond
constexpr int kNoOwner = 0x7fffffff;

template <typename W> struct Tile { static constexpr int cols = sizeof(typename PB<W>::acc) == 8 ? kTileColsF64 : kTileCols; };

// ------------------------------------------------------------------------------------------ forward
template <typename W, bool HOMO>
__global__ void __launch_bounds__(kThreads) k_slice_rows(const typename PB<W>::bits* __restrict__ data,
                                                         const int32_t* __restrict__ idx, RowPtr rp,
                                                         const int64_t* __restrict__ rows, typename PB<W>::bits* __restrict__ out,
                                                         int64_t n_rows, int64_t n_cols, int64_t nse, int64_t n_tiles,
                                                         int64_t n_jobs) {
  using B = typename PB<W>::bits;
  using ACC = typename PB<W>::acc;
  constexpr int T = Tile<W>::cols;
  constexpr int V = kVecBytes / (int)sizeof(B);
  __shared__ ACC s_acc[HOMO ? 1 : T];
  __shared__ int s_own[T];              // per-entry weights: the position that owns the column this round; shared: the count
  const int tid = threadIdx.x;
  ACC w_homo = 0;
  if (HOMO) w_homo = PB<W>::get(data[0]);

  for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const int64_t k = job / n_tiles;
    const int64_t c0 = (job - k * n_tiles) * T;
    const int width = (int)(n_cols - c0 < T ? n_cols - c0 : T);
    const int64_t r = rows[k];
    int64_t beg = 0, end = 0;
    if (r >= 0 && r < n_rows) {
      beg = rp.at(r);
      end = rp.at(r + 1);
      if (beg < 0) beg = 0;              // (whatever indptr holds, no entry outside [0, nse) is read)
      if (end > nse) end = nse;
    }
    for (int c = tid; c < width; c += kThreads) {
      if (!HOMO) s_acc[c] = 0;
      s_own[c] = HOMO ? 0 : kNoOwner;
    }
    __syncthreads();

    if (HOMO) {
      for (int64_t j = beg + tid; j < end; j += kThreads) {
        const int64_t c = (int64_t)__builtin_nontemporal_load(idx + j) - c0;
        if (c >= 0 && c < width) atomicAdd(&s_own[c], 1);
      }
    } else {
      for (int64_t base = beg; base < end; base += (int64_t)kThreads * kPer) {
        int col[kPer];
        ACC val[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
          const int64_t j = base + u * kThreads + tid;
          col[u] = -1;
          val[u] = 0;
          if (j < end) {
            const int64_t c = (int64_t)__builtin_nontemporal_load(idx + j) - c0;
            if (c >= 0 && c < width) {
              col[u] = (int)c;
              val[u] = PB<W>::get(__builtin_nontemporal_load(data + j));
            }
          }
        }
        for (;;) {
#pragma unroll
          for (int u = 0; u < kPer; ++u)
            if (col[u] >= 0) atomicMin(&s_own[col[u]], u * kThreads + tid);      // ascending in j
          __syncthreads();
          bool won[kPer];
          int lost = 0;
#pragma unroll
          for (int u = 0; u < kPer; ++u) {
            won[u] = col[u] >= 0 && s_own[col[u]] == u * kThreads + tid;
            lost |= (int)(col[u] >= 0 && !won[u]);
          }
          const int again = __syncthreads_or(lost);         // (every owner word is read before any is reset)
#pragma unroll
          for (int u = 0; u < kPer; ++u) {
            if (won[u]) {                                   // one owner per column: a plain read-modify-write
              s_acc[col[u]] += val[u];
              s_own[col[u]] = kNoOwner;
              col[u] = -1;
            }
          }
          __syncthreads();                                  // the resets, before the next round's or the next pass's atomicMin
          if (!again) break;
        }
      }
    }
    __syncthreads();

    // the tile, in out's dtype: entry by entry up to the first 16-byte boundary of the row, 16-byte stores, the rest
    B* orow = out + k * n_cols + c0;
    int head = (int)((kVecBytes - reinterpret_cast<uintptr_t>(orow) % kVecBytes) % kVecBytes) / (int)sizeof(B);
    if (head > width) head = width;
    const int n_vec = (width - head) / V;
    auto value = [&](int c) -> B {
      if (HOMO) {                                          // (a column without an entry is +0 whatever the sign of w)
        const int n = s_own[c];
        return n ? PB<W>::put((ACC)n * w_homo) : (B)0;
      }
      return PB<W>::put(s_acc[c]);
    };
    for (int i = tid; i < n_vec; i += kThreads) {
      B v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = value(head + i * V + e);
      be_v4u q;
      __builtin_memcpy(&q, v, kVecBytes);
      __builtin_nontemporal_store(q, reinterpret_cast<be_v4u*>(orow + head + i * V));
    }
    if (tid < head) orow[tid] = value(tid);
    for (int c = head + n_vec * V + tid; c < width; c += kThreads) orow[c] = value(c);
    __syncthreads();                                        // (the next job initialises the tile again)
  }
}

// ------------------------------------------------------------------------------------------ gradient
// urows [n_u]: the distinct selected rows; seg [n_u + 1]: where each one's k's lie in ks; ks: the k's, ascending per row.
template <typename W>
__device__ __forceinline__ typename PB<W>::acc ct_sum(const typename PB<W>::bits* __restrict__ ct, const int64_t* __restrict__ ks,
                                                       int64_t s0, int64_t s1, int64_t n_sel, int64_t n_cols, int64_t c) {
  typename PB<W>::acc s = 0;
  for (int64_t i = s0; i < s1; ++i) {
    const int64_t k = ks[i];
    if (k >= 0 && k < n_sel) s += PB<W>::get(ct[k * n_cols + c]);
  }
  return s;
}

template <typename W, bool HOMO>
__global__ void __launch_bounds__(kThreads) k_slice_rows_grad(const typename PB<W>::bits* __restrict__ ct,
                                                              const int32_t* __restrict__ idx, RowPtr rp,
                                                              const int64_t* __restrict__ urows, const int64_t* __restrict__ seg,
                                                              const int64_t* __restrict__ ks, int64_t n_u, int64_t n_sel,
                                                              typename PB<W>::bits* __restrict__ dw, int64_t n_rows,
                                                              int64_t n_cols, int64_t nse,
                                                              typename PB<W>::acc* __restrict__ partials) {
  using ACC = typename PB<W>::acc;
  __shared__ ACC wave_tot[kThreads / 64];
  for (int64_t u = blockIdx.x; u < n_u; u += gridDim.x) {
    const int64_t r = urows[u];
    int64_t beg = 0, end = 0;
    if (r >= 0 && r < n_rows) {
      beg = rp.at(r);
      end = rp.at(r + 1);
      if (beg < 0) beg = 0;
      if (end > nse) end = nse;
    }
    const int64_t s0 = seg[u] > 0 ? seg[u] : 0, s1 = seg[u + 1] < n_sel ? seg[u + 1] : n_sel;     // (ks holds n_sel entries)
    ACC total = 0;
    for (int64_t j = beg + (int64_t)blockIdx.y * kThreads + threadIdx.x; j < end; j += (int64_t)gridDim.y * kThreads) {
      const int64_t c = __builtin_nontemporal_load(idx + j);
      ACC v = 0;
      if (c >= 0 && c < n_cols) v = ct_sum<W>(ct, ks, s0, s1, n_sel, n_cols, c);
      if (HOMO) total += v;
      else dw[j] = PB<W>::put(v);
    }
    if (HOMO) {                         // (gridDim.y == 1) one partial per selected row, in a fixed tree order
      total = wave_sum(total);
      if (lane_id() == 0) wave_tot[threadIdx.x >> 6] = total;
      __syncthreads();
      if (threadIdx.x == 0) {
        ACC s = 0;
        for (int w = 0; w < kThreads / 64; ++w) s += wave_tot[w];
        partials[u] = s;
      }
      __syncthreads();
    }
  }
}

// one workgroup, fixed order
template <typename W>
__global__ void __launch_bounds__(kThreads) k_slice_rows_grad_finish(const typename PB<W>::acc* __restrict__ partials, int64_t n,
                                                                     typename PB<W>::bits* __restrict__ dw) {
  using ACC = typename PB<W>::acc;
  __shared__ ACC wave_tot[kThreads / 64];
  ACC s = 0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) s += partials[i];
  s = wave_sum(s);
  if (lane_id() == 0) wave_tot[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    ACC t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += wave_tot[w];
    dw[0] = PB<W>::put(t);
  }
}

// ------------------------------------------------------------------------------------------ copy
// the last k in [lo, hi] with ptr[k] <= e (given ptr[lo] <= e): steps over selected rows without entries
__device__ __forceinline__ int64_t seg_of(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Balanced per entry: a tile is kThreads * kCopyPer consecutive output entries whatever the rows' lengths; the block finds the
// selected rows of its first and last entry once, every entry then searches inside that range only (be_dt2t.hip's scheme).
template <typename D>
__global__ void __launch_bounds__(kThreads) k_slice_rows_copy(const int32_t* __restrict__ idx, const D* __restrict__ data, RowPtr rp,
                                                              const int64_t* __restrict__ rows, const int64_t* __restrict__ new_ptr,
                                                              int64_t n_sel, int64_t n_rows, int64_t nse, int64_t new_nse,
                                                              int32_t* __restrict__ out_idx, D* __restrict__ out_data) {
  constexpr int64_t kTile = (int64_t)kThreads * kCopyPer;
  __shared__ int64_t s_k[2];
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < new_nse; tile += (int64_t)gridDim.x * kTile) {
    const int64_t last = (tile + kTile < new_nse ? tile + kTile : new_nse) - 1;
    if (threadIdx.x < 2) s_k[threadIdx.x] = seg_of(new_ptr, 0, n_sel - 1, threadIdx.x ? last : tile);
    __syncthreads();
    const int64_t k_lo = s_k[0], k_hi = s_k[1];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kCopyPer; ++u) {
      const int64_t e = tile + (int64_t)u * kThreads + threadIdx.x;
      if (e > last) break;
      const int64_t k = seg_of(new_ptr, k_lo, k_hi, e);
      const int64_t r = rows[k];
      if (r < 0 || r >= n_rows) continue;
      const int64_t src = rp.at(r) + (e - new_ptr[k]);
      if (src < 0 || src >= nse) continue;
      __builtin_nontemporal_store(__builtin_nontemporal_load(idx + src), out_idx + e);
      if (data != nullptr) __builtin_nontemporal_store(__builtin_nontemporal_load(data + src), out_data + e);
    }
  }
}

// ------------------------------------------------------------------------------------------ host
template <typename W>
int slice_rows_t(const void* data, int homo, const int32_t* idx, RowPtr rp, const int64_t* rows, int64_t n_sel, void* out,
                 int64_t n_rows, int64_t n_cols, int64_t nse, hipStream_t st) {
  using B = typename PB<W>::bits;
  const int64_t n_tiles = (n_cols + Tile<W>::cols - 1) / Tile<W>::cols;
  const int64_t n_jobs = n_sel * n_tiles;
  const int gx = (int)(n_jobs < kGridCap ? n_jobs : kGridCap);
  const int prof = be_prof_begin(st);
  if (homo)
    hipLaunchKernelGGL((k_slice_rows<W, true>), dim3(gx), dim3(kThreads), 0, st, static_cast<const B*>(data), idx, rp, rows,
                       static_cast<B*>(out), n_rows, n_cols, nse, n_tiles, n_jobs);
  else
    hipLaunchKernelGGL((k_slice_rows<W, false>), dim3(gx), dim3(kThreads), 0, st, static_cast<const B*>(data), idx, rp, rows,
                       static_cast<B*>(out), n_rows, n_cols, nse, n_tiles, n_jobs);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int slice_rows_grad_t(const void* ct, const int32_t* idx, RowPtr rp, const int64_t* urows, const int64_t* seg, const int64_t* ks,
                      int64_t n_u, int64_t n_sel, void* dw, int homo, int64_t n_rows, int64_t n_cols, int64_t nse, void* ws,
                      hipStream_t st) {
  using B = typename PB<W>::bits;
  using ACC = typename PB<W>::acc;
  const int gx = (int)(n_u < kGridCap ? n_u : kGridCap);
  if (homo) {
    hipLaunchKernelGGL((k_slice_rows_grad<W, true>), dim3(gx), dim3(kThreads), 0, st, static_cast<const B*>(ct), idx, rp, urows, seg,
                       ks, n_u, n_sel, static_cast<B*>(dw), n_rows, n_cols, nse, static_cast<ACC*>(ws));
    BE_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_slice_rows_grad_finish<W>), dim3(1), dim3(kThreads), 0, st, static_cast<const ACC*>(ws), n_u,
                       static_cast<B*>(dw));
  } else {
    hipLaunchKernelGGL((k_slice_rows_grad<W, false>), dim3(gx, kGradSplit), dim3(kThreads), 0, st, static_cast<const B*>(ct), idx, rp,
                       urows, seg, ks, n_u, n_sel, static_cast<B*>(dw), n_rows, n_cols, nse, static_cast<ACC*>(nullptr));
  }
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename D>
int slice_rows_copy_t(const int32_t* idx, const void* data, RowPtr rp, const int64_t* rows, const int64_t* new_ptr, int64_t n_sel,
                      int64_t n_rows, int64_t nse, int64_t new_nse, int32_t* out_idx, void* out_data, hipStream_t st) {
  const int gx = grid_for(new_nse, kThreads * kCopyPer, 1 << 20);
  hipLaunchKernelGGL((k_slice_rows_copy<D>), dim3(gx), dim3(kThreads), 0, st, idx, static_cast<const D*>(data), rp, rows, new_ptr,
                     n_sel, n_rows, nse, new_nse, out_idx, static_cast<D*>(out_data));
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int wbytes(int wdtype) { return wdtype == BE_F32 ? 4 : wdtype == BE_F64 ? 8 : (wdtype == BE_F16 || wdtype == BE_BF16) ? 2 : 0; }

bool structure_ok(const void* indptr, int64_t row_len, int64_t n_rows, int64_t nse) {
  if (indptr != nullptr) return true;
  return row_len > 0 ? (nse + row_len - 1) / row_len <= n_rows && nse % row_len == 0 : nse == 0 && row_len == 0;
}

}  // namespace

extern "C" {

int be_slice_rows_tile_cols(int wdtype) {
  switch (wdtype) {
    case BE_F32: return Tile<float>::cols;
    case BE_F64: return Tile<double>::cols;
    case BE_F16: return Tile<__half>::cols;
    case BE_BF16: return Tile<__hip_bfloat16>::cols;
    default: return -1;
  }
}

int be_slice_rows(const void* data, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                  int64_t row_len, const int64_t* rows, int64_t n_sel, void* out, int64_t n_rows, int64_t n_cols, int64_t nse,
                  be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && nse >= 0 && n_sel >= 0, BE_ERR_INVALID, "shape out of range");
  BE_REQUIRE(wbytes(wdtype) != 0, BE_ERR_INVALID, "unknown weight dtype");
  if (n_sel == 0 || n_cols == 0) return BE_OK;
  BE_REQUIRE(rows && out, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(nse == 0 || (data && indices), BE_ERR_INVALID, "entries but no data / indices");
  BE_REQUIRE(!homo || data, BE_ERR_INVALID, "a shared weight needs its value");
  BE_REQUIRE(structure_ok(indptr, row_len, n_rows, nse), BE_ERR_INVALID, "fixed row length does not fit n_rows and nse");
  const RowPtr rp{indptr, indptr_is_i64, indptr ? -1 : row_len};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return slice_rows_t<W>(data, homo, indices, rp, rows, n_sel, out, n_rows, n_cols, nse, st);
  });
}

int64_t be_slice_rows_grad_workspace_bytes(int64_t n_sel, int wdtype) {
  return be_align_up((n_sel > 0 ? n_sel : 1) * (wdtype == BE_F64 ? 8 : 4), 256);
}

int be_slice_rows_grad(const void* ct, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                       const int64_t* urows, const int64_t* seg, const int64_t* ks, int64_t n_u, int64_t n_sel, void* dw, int homo,
                       int64_t n_rows, int64_t n_cols, int64_t nse, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && nse >= 0 && n_sel >= 0 && n_u >= 0 && n_u <= n_sel, BE_ERR_INVALID, "shape out of range");
  const int wb = wbytes(wdtype);
  BE_REQUIRE(wb != 0, BE_ERR_INVALID, "unknown weight dtype");
  BE_REQUIRE(dw != nullptr || (!homo && nse == 0), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(structure_ok(indptr, row_len, n_rows, nse), BE_ERR_INVALID, "fixed row length does not fit n_rows and nse");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the entries of the rows that were not selected (a shared weight: the empty sum).  be_fill_async: the house fill, a kernel
  // (hipMemsetAsync nodes replayed wrongly under graph capture on this ROCm, be_common.h)
  const int64_t fill = homo ? wb : nse * wb;
  if (fill > 0) BE_HIP(be_fill_async(dw, 0, (size_t)fill, st));
  if (n_u == 0 || nse == 0 || n_cols == 0) return BE_OK;
  BE_REQUIRE(ct && indices && urows && seg && ks, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(!homo || (workspace != nullptr && workspace_bytes >= be_slice_rows_grad_workspace_bytes(n_sel, wdtype)),
             BE_ERR_WORKSPACE, "workspace too small");
  const RowPtr rp{indptr, indptr_is_i64, indptr ? -1 : row_len};
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return slice_rows_grad_t<W>(ct, indices, rp, urows, seg, ks, n_u, n_sel, dw, homo, n_rows, n_cols, nse, workspace, st);
  });
}

int be_slice_rows_copy(const int32_t* indices, const void* data, int elem_bytes, const void* indptr, int indptr_is_i64,
                       int64_t row_len, const int64_t* rows, const int64_t* new_indptr, int64_t n_sel, int64_t n_rows, int64_t nse,
                       int64_t new_nse, int32_t* out_indices, void* out_data, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && nse >= 0 && n_sel >= 0 && new_nse >= 0, BE_ERR_INVALID, "shape out of range");
  if (new_nse == 0 || n_sel == 0) return BE_OK;
  BE_REQUIRE(indices && rows && new_indptr && out_indices, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE((data == nullptr) == (out_data == nullptr), BE_ERR_INVALID, "data and out_data go together");
  BE_REQUIRE(structure_ok(indptr, row_len, n_rows, nse), BE_ERR_INVALID, "fixed row length does not fit n_rows and nse");
  const RowPtr rp{indptr, indptr_is_i64, indptr ? -1 : row_len};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (data == nullptr || elem_bytes == 4)
    return slice_rows_copy_t<uint32_t>(indices, data, rp, rows, new_indptr, n_sel, n_rows, nse, new_nse, out_indices, out_data, st);
  if (elem_bytes == 2)
    return slice_rows_copy_t<uint16_t>(indices, data, rp, rows, new_indptr, n_sel, n_rows, nse, new_nse, out_indices, out_data, st);
  if (elem_bytes == 8)
    return slice_rows_copy_t<uint64_t>(indices, data, rp, rows, new_indptr, n_sel, n_rows, nse, new_nse, out_indices, out_data, st);
  be_set_error("be_slice_rows_copy: data elements of 2, 4 or 8 bytes");
  return BE_ERR_INVALID;
}

}  // extern "C"
