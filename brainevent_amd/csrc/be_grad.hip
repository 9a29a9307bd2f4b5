// be_grad.hip — weight gradients of the event-driven products (torch.autograd backward, brainevent_amd/_autograd.py).
//
// Reference semantics (read as text): brainevent/_csr/binary.py:656-715 (_csrmv_jvp_weights / transpose rule), :1303-1360
// (mm through the SDDMM helper of _sddmm.py), brainevent/_dense/binary.py:290-330, brainevent/_fcn/binary.py:317-.
// The forward products are exactly linear in the weights, so with a = active(spike) (the forward kernels' IS_ACTIVE rule)
// and g the incoming gradient of the output:
//   s @ A (row side = activity of row r, column side = g):   dw[j] = sum_b a[b, r(j)] * g[b, c(j)]
//   A @ s (row side = g, column side = activity):            dw[j] = sum_b g[b, r(j)] * a[b, c(j)]
//   homogeneous weight: the scalar sum over j of the same;   dense: dW[i, :] = sum_{b: a[b, i]} g[b, :] and its transpose.
// Every sum runs over the ACTIVE batch rows only, in ascending b, in f32 (f64 for f64 weights), and is rounded once to the
// weight dtype.  The activity arrives packed per neuron: ceil(B / 32) words, bit b % 32 of word b / 32 (k_grad_pack, from any
// of the product's spike encodings), so one kernel serves mv (B = 1) and mm and both directions.
//
// k_grad_rows walks ALL nse entries in tiles of kTile (a thread binary-searches the row of its first entry, then walks
// forward), so the work is balanced per entry whatever the row lengths.  Every entry is written exactly once by one lane —
// zeros for an inactive row without reading its indices — so no memset and no atomics.  The homogeneous variant reduces
// instead of storing: per-workgroup partials in the accumulation type, then one workgroup sums them in a fixed order
// (deterministic: no float atomics anywhere).
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

// ------------------------------------------------------------------------------------------ activity -> packed bit mask
// mask[i * nw + w] bit t = active(spikes[32 w + t, i]); spikes batch-major [nb, n] (bytes: != 0, f32: > 0, words:
// [nb, ceil(n/32)] bit-packed rows).  Lanes run over i so the spike reads coalesce.
template <int SD>
__global__ void __launch_bounds__(256) k_grad_pack(const void* __restrict__ spikes, int64_t n, int64_t nb, int64_t nw,
                                                   uint32_t* __restrict__ mask) {
  const int64_t total = n * nw;
  const int64_t row_words = (n + 31) >> 5;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w = t / n, i = t - w * n;
    const int64_t b0 = w * 32, b1 = b0 + 32 < nb ? b0 + 32 : nb;
    uint32_t word = 0;
    for (int64_t b = b0; b < b1; ++b) {
      bool on;
      if (SD == BE_SPIKE_BOOL) on = static_cast<const uint8_t*>(spikes)[b * n + i] != 0;
      else if (SD == BE_SPIKE_FLOAT) on = static_cast<const float*>(spikes)[b * n + i] > 0.f;
      else on = (static_cast<const uint32_t*>(spikes)[b * row_words + (i >> 5)] >> (i & 31)) & 1u;
      word |= (uint32_t)on << (b - b0);
    }
    mask[i * nw + w] = word;
  }
}

// compacted ids (one vector): mask[ids[a]] = 1 for a < *count (ids distinct: one writer per word; zeroed before)
__global__ void __launch_bounds__(256) k_grad_pack_ids(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ count,
                                                       uint32_t* __restrict__ mask) {
  const uint32_t n_active = *count;
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n_active; a += gridDim.x * blockDim.x) mask[ids[a]] = 1u;
}

// sum_{b in mask words} g[b * sb] in ascending b (g already offset to the neuron)
template <typename W>
__device__ __forceinline__ typename PB<W>::acc masked_sum(const uint32_t* __restrict__ m, int nw,
                                                         const typename PB<W>::bits* __restrict__ g, int64_t sb) {
  typename PB<W>::acc acc = 0;
  for (int w = 0; w < nw; ++w) {
    uint32_t bits = m[w];
    while (bits) {
      const int t = __builtin_ctz(bits);
      bits &= bits - 1;
      acc += PB<W>::get(g[(int64_t)(w * 32 + t) * sb]);
    }
  }
  return acc;
}

__device__ __forceinline__ bool any_word(const uint32_t* __restrict__ m, int nw) {
  uint32_t o = 0;
  for (int w = 0; w < nw; ++w) o |= m[w];
  return o != 0;
}

// ------------------------------------------------------------------------------------------ row-stored structures
constexpr int kRowThreads = 256, kRowPer = 8, kTile = kRowThreads * kRowPer;

// T (s @ A): mask indexed by the row, g by the column.  !T (A @ s): g by the row, mask by the column.
// g element of (batch b, neuron x) = g[x * g_sn + b * g_sb].
template <typename W, bool T, bool HOMO>
__global__ void __launch_bounds__(kRowThreads) k_grad_rows(typename PB<W>::bits* __restrict__ dw, const int32_t* __restrict__ col,
                                                           RowPtr rp, int64_t n_rows, int64_t nse,
                                                           const uint32_t* __restrict__ mask, int nw,
                                                           const typename PB<W>::bits* __restrict__ g, int64_t g_sn,
                                                           int64_t g_sb, typename PB<W>::acc* __restrict__ partials) {
  using ACC = typename PB<W>::acc;
  using B = typename PB<W>::bits;
  ACC total = 0;
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < nse; tile += (int64_t)gridDim.x * kTile) {
    int64_t e = tile + threadIdx.x;
    if (e >= nse) break;
    // the row holding entry e: the last r with indptr[r] <= e (empty rows are stepped over)
    int64_t r;
    if (rp.p == nullptr) {
      r = e / rp.fixed;
    } else {
      int64_t lo = 0, hi = n_rows - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (rp.at(mid) <= e) lo = mid; else hi = mid - 1;
      }
      r = lo;
    }
    int64_t row_end = rp.at(r + 1);
    bool row_on = T ? any_word(mask + r * nw, nw) : true;
#pragma unroll 2
    for (int u = 0; u < kRowPer; ++u, e += kRowThreads) {
      if (e >= nse) break;
      bool moved = false;
      while (e >= row_end) {
        ++r;
        row_end = rp.at(r + 1);
        moved = true;
      }
      if (T && moved) row_on = any_word(mask + r * nw, nw);
      ACC v = 0;
      if (T) {
        if (row_on) {
          const int64_t c = __builtin_nontemporal_load(col + e);
          v = masked_sum<W>(mask + r * nw, nw, g + c * g_sn, g_sb);
        }
      } else {
        const int64_t c = __builtin_nontemporal_load(col + e);
        v = masked_sum<W>(mask + c * nw, nw, g + r * g_sn, g_sb);
      }
      if (HOMO) total += v;
      else __builtin_nontemporal_store(PB<W>::put(v), dw + e);
    }
  }
  if (HOMO) {
    __shared__ ACC wave_tot[kRowThreads / 64];
    total = wave_sum(total);
    if (lane_id() == 0) wave_tot[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
      ACC s = 0;
      for (int w = 0; w < kRowThreads / 64; ++w) s += wave_tot[w];
      partials[blockIdx.x] = s;
    }
  }
}

// second pass of the homogeneous reduction: one workgroup, fixed order
template <typename W>
__global__ void __launch_bounds__(256) k_grad_finish(const typename PB<W>::acc* __restrict__ partials, int n,
                                                     typename PB<W>::bits* __restrict__ dw) {
  using ACC = typename PB<W>::acc;
  __shared__ ACC wave_tot[4];
  ACC s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
  s = wave_sum(s);
  if (lane_id() == 0) wave_tot[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) dw[0] = PB<W>::put(wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]);
}

// ------------------------------------------------------------------------------------------ dense
// T (events @ W, W [n_rows, n_cols]):  dW[i, j] = sum_{b in mask[i]} g(b, j)   — an inactive row is written as zeros
// !T (W @ events):                      dW[i, j] = sum_{b in mask[j]} g(b, i)
// One lane per element, ascending b; gridDim.y splits the columns.
template <typename W, bool T>
__global__ void __launch_bounds__(256) k_grad_dense(typename PB<W>::bits* __restrict__ dw, int64_t n_rows, int64_t n_cols,
                                                    const uint32_t* __restrict__ mask, int nw,
                                                    const typename PB<W>::bits* __restrict__ g, int64_t g_sn, int64_t g_sb,
                                                    int64_t cols_per_y) {
  using B = typename PB<W>::bits;
  const int64_t c0 = (int64_t)blockIdx.y * cols_per_y;
  const int64_t c1 = c0 + cols_per_y < n_cols ? c0 + cols_per_y : n_cols;
  for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
    B* row = dw + i * n_cols;
    if (T) {
      const uint32_t* mi = mask + i * nw;
      if (!any_word(mi, nw)) {
        for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) __builtin_nontemporal_store(PB<W>::put(0), row + j);
        continue;
      }
      for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x)
        __builtin_nontemporal_store(PB<W>::put(masked_sum<W>(mi, nw, g + j * g_sn, g_sb)), row + j);
    } else {
      for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x)
        __builtin_nontemporal_store(PB<W>::put(masked_sum<W>(mask + j * nw, nw, g + i * g_sn, g_sb)), row + j);
    }
  }
}

// ------------------------------------------------------------------------------------------ host helpers
int rows_grid(int64_t nse) { return grid_for(nse, kTile, 4096); }

int64_t grad_ws_bytes(int64_t nse) { return be_align_up((int64_t)rows_grid(nse) * 8, 256); }

template <typename W, bool T, bool HOMO>
void launch_rows(void* dw, const int32_t* col, RowPtr rp, int64_t n_rows, int64_t nse, const uint32_t* mask, int nw,
                 const void* g, int64_t g_sn, int64_t g_sb, void* ws, hipStream_t st) {
  using B = typename PB<W>::bits;
  using ACC = typename PB<W>::acc;
  const int grid = rows_grid(nse);
  hipLaunchKernelGGL((k_grad_rows<W, T, HOMO>), dim3(grid), dim3(kRowThreads), 0, st, static_cast<B*>(dw), col, rp, n_rows,
                     nse, mask, nw, static_cast<const B*>(g), g_sn, g_sb, static_cast<ACC*>(ws));
  if (HOMO) hipLaunchKernelGGL(k_grad_finish<W>, dim3(1), dim3(256), 0, st, static_cast<const ACC*>(ws), grid, static_cast<B*>(dw));
}

template <typename W>
int grad_rows_t(int t, int homo, void* dw, const int32_t* col, RowPtr rp, int64_t n_rows, int64_t nse, const uint32_t* mask,
                int nw, const void* g, int64_t g_sn, int64_t g_sb, void* ws, hipStream_t st) {
  const int prof = be_prof_begin(st);
  if (t) {
    if (homo) launch_rows<W, true, true>(dw, col, rp, n_rows, nse, mask, nw, g, g_sn, g_sb, ws, st);
    else launch_rows<W, true, false>(dw, col, rp, n_rows, nse, mask, nw, g, g_sn, g_sb, ws, st);
  } else {
    if (homo) launch_rows<W, false, true>(dw, col, rp, n_rows, nse, mask, nw, g, g_sn, g_sb, ws, st);
    else launch_rows<W, false, false>(dw, col, rp, n_rows, nse, mask, nw, g, g_sn, g_sb, ws, st);
  }
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int grad_dense_t(int t, void* dw, int64_t n_rows, int64_t n_cols, const uint32_t* mask, int nw, const void* g, int64_t g_sn,
                 int64_t g_sb, hipStream_t st) {
  using B = typename PB<W>::bits;
  const int64_t cols_per_y = 4096;
  const unsigned gy = (unsigned)((n_cols + cols_per_y - 1) / cols_per_y);
  const unsigned gx = (unsigned)grid_for(n_rows, 1, (int)(4096 / gy > 8 ? 4096 / gy : 8));
  const int prof = be_prof_begin(st);
  if (t)
    hipLaunchKernelGGL((k_grad_dense<W, true>), dim3(gx, gy), dim3(256), 0, st, static_cast<B*>(dw), n_rows, n_cols, mask, nw,
                       static_cast<const B*>(g), g_sn, g_sb, cols_per_y);
  else
    hipLaunchKernelGGL((k_grad_dense<W, false>), dim3(gx, gy), dim3(256), 0, st, static_cast<B*>(dw), n_rows, n_cols, mask, nw,
                       static_cast<const B*>(g), g_sn, g_sb, cols_per_y);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int64_t be_grad_mask_bytes(int64_t n, int64_t n_batch) {
  if (n < 0 || n_batch < 1) return (int64_t)BE_ERR_INVALID;
  return be_align_up(n * ((n_batch + 31) / 32) * 4, 256);
}

int be_grad_pack_activity(const void* spikes, int spike_dtype, int64_t n, int64_t n_batch, uint32_t* mask, be_stream_t stream) {
  BE_REQUIRE(n >= 0 && n <= 0xffffffffll && n_batch >= 1 && n_batch <= kMaxBatch, BE_ERR_INVALID, "n / n_batch out of range");
  BE_REQUIRE(spike_dtype != BE_SPIKE_IDS || n_batch == 1, BE_ERR_INVALID, "id lists are single vectors");
  if (n == 0) return BE_OK;
  BE_REQUIRE(spikes && mask, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nw = (n_batch + 31) / 32;
  const int grid = grid_for(n * nw, 256, 8192);
  switch (spike_dtype) {
    case BE_SPIKE_BOOL:
      hipLaunchKernelGGL(k_grad_pack<BE_SPIKE_BOOL>, dim3(grid), dim3(256), 0, st, spikes, n, n_batch, nw, mask);
      break;
    case BE_SPIKE_FLOAT:
      hipLaunchKernelGGL(k_grad_pack<BE_SPIKE_FLOAT>, dim3(grid), dim3(256), 0, st, spikes, n, n_batch, nw, mask);
      break;
    case BE_SPIKE_BITS:
      hipLaunchKernelGGL(k_grad_pack<BE_SPIKE_BITS>, dim3(grid), dim3(256), 0, st, spikes, n, n_batch, nw, mask);
      break;
    case BE_SPIKE_IDS: {
      const be_spike_ids_t* ids = static_cast<const be_spike_ids_t*>(spikes);
      BE_HIP(be_fill_async(mask, 0, (size_t)n * 4, st));
      hipLaunchKernelGGL(k_grad_pack_ids, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, ids->active_ids, ids->n_active, mask);
      break;
    }
    default: be_set_error("unknown spike dtype"); return BE_ERR_INVALID;
  }
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int64_t be_grad_rows_workspace_bytes(int64_t nse) { return nse < 0 ? (int64_t)BE_ERR_INVALID : grad_ws_bytes(nse); }

int be_grad_rows(int transpose, void* dw, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                 int64_t row_len, int64_t n_rows, int64_t nse, const uint32_t* mask, int64_t n_batch, const void* g,
                 int64_t g_sn, int64_t g_sb, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && nse >= 0 && n_batch >= 1 && n_batch <= kMaxBatch, BE_ERR_INVALID, "shape out of range");
  BE_REQUIRE(indptr != nullptr || row_len > 0 || nse == 0, BE_ERR_INVALID, "fixed row length <= 0 without indptr");
  BE_REQUIRE(!homo || (workspace != nullptr && workspace_bytes >= grad_ws_bytes(nse)), BE_ERR_WORKSPACE, "workspace too small");
  BE_REQUIRE(dw != nullptr || (!homo && nse == 0), BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nse == 0 || n_rows == 0) {
    if (homo) {    // an empty sum
      BE_HIP(be_fill_async(dw, 0, be_wbytes(wdtype), st));
    }
    return BE_OK;
  }
  BE_REQUIRE(indices && mask && g, BE_ERR_INVALID, "null pointer");
  const RowPtr rp{indptr, indptr_is_i64, row_len};
  const int nw = (int)((n_batch + 31) / 32);
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return grad_rows_t<W>(transpose, homo, dw, indices, rp, n_rows, nse, mask, nw, g, g_sn, g_sb, workspace, st);
  });
}

int64_t be_grad_dense_workspace_bytes(int64_t n_rows, int64_t n_cols) {
  return (n_rows < 0 || n_cols < 0) ? (int64_t)BE_ERR_INVALID : 0;
}

int be_grad_dense(int transpose, void* dw, int wdtype, int64_t n_rows, int64_t n_cols, const uint32_t* mask, int64_t n_batch,
                  const void* g, int64_t g_sn, int64_t g_sb, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_batch >= 1 && n_batch <= kMaxBatch, BE_ERR_INVALID, "shape out of range");
  if (n_rows == 0 || n_cols == 0) return BE_OK;
  BE_REQUIRE(dw && mask && g, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nw = (int)((n_batch + 31) / 32);
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return grad_dense_t<W>(transpose, dw, n_rows, n_cols, mask, nw, g, g_sn, g_sb, st);
  });
}

}  // extern "C"
