// be_plasticity.hip — spike-triggered additive weight updates (pair-based STDP) for CSR, CSC, fixed-number
// connectivity and dense matrices.
//
// Reference semantics (read as text): brainevent/_csr/plasticity_binary.py:45-173 (pre), :477-618 (post, through the
// CSC->CSR permutation), brainevent/_dense/plasticity_binary.py:42-140 / :360-458, brainevent/_fcn/plasticity_binary.py
// :181-300.  For every active row r and every stored entry e of r:  w[e] = w[e] + trace[col(e)]  (one rounding to the
// weight dtype: f16 / bf16 add in f32, f32 in f32, f64 in f64), then — when the caller asks for it — clip(w[e], lo, hi)
// = min(max(w, lo), hi) in the weight dtype (NaN stays NaN, lo > hi gives hi).  The reference clips the WHOLE array; the
// host layer either clamps the whole array after an unclipped call or, when it holds a certificate that every untouched
// entry already lies in [lo, hi], lets these kernels clip the touched entries only (same result).
//
// Work is balanced per ENTRY: the active rows are compacted, an exclusive scan of their lengths gives each active row its
// offset in the virtual concatenation of the active rows, and the update kernel walks that concatenation in tiles of
// kTile entries (a thread binary-searches the row of its first entry, then walks forward).  Each entry is read and written
// by exactly one lane: no atomics (a duplicated column is two entries, each updated once).  The index and weight streams
// are read once (non-temporal); the trace vector is gathered through the caches.
//
// Delayed synapses: be_plasticity_rows_aged is the same permuted walk over the transposed structure of a matrix
// stacked by delay, with the trace looked up by age in a ring of per-neuron values (the TraceAged policy of k_plast_rows).
#include "be_csr_shared.h"
#include "be_pbits.h"

namespace {

// clip bounds, already rounded to the weight dtype by the caller (exact in acc)
struct ClipArgs {
  int lo_on, hi_on;
  double lo, hi;
};

// w + t rounded once to W, then (CLIP) min(max(., lo), hi) in W
template <typename W, bool CLIP>
__device__ __forceinline__ typename PB<W>::bits plast_add(typename PB<W>::bits w, typename PB<W>::bits t, ClipArgs c) {
  using ACC = typename PB<W>::acc;
  typename PB<W>::bits r = PB<W>::put(PB<W>::get(w) + PB<W>::get(t));
  if (CLIP) {
    ACC a = PB<W>::get(r);
    if (c.lo_on && a < (ACC)c.lo) a = (ACC)c.lo;   // comparisons are false for NaN: NaN stays NaN
    if (c.hi_on && a > (ACC)c.hi) a = (ACC)c.hi;
    r = PB<W>::put(a);                               // exact: a is a W value
  }
  return r;
}

// ------------------------------------------------------------------------------------------ float spikes -> 0/1 bytes
// (the plasticity rule takes any NONZERO value as a spike, plasticity_binary.py:192-197; the product path's float code
// means > 0, so float events are turned into bytes first and compacted by the shared compaction)
__global__ void __launch_bounds__(256) k_plast_nonzero(const float* __restrict__ s, int64_t n, uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = s[i] != 0.f ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ offsets of the active rows
// One workgroup of 1024 threads: offs[a] = sum of the lengths of active rows 0 .. a-1, offs[n_active] = total.  A thread
// sums kPer consecutive rows, so one pass covers 16K active rows (1 % of 1M rows: one pass).
constexpr int kScanThreads = 1024, kScanPer = 16;

__global__ void __launch_bounds__(kScanThreads) k_plast_offsets(RowPtr rp, const uint32_t* __restrict__ active,
                                                                const uint32_t* __restrict__ n_active_p,
                                                                int64_t* __restrict__ offs) {
  __shared__ int64_t wave_tot[kScanThreads / 64];
  const uint32_t n_active = *n_active_p;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < (int64_t)n_active; base += (int64_t)kScanThreads * kScanPer) {
    const int64_t first = base + (int64_t)threadIdx.x * kScanPer;
    int64_t len[kScanPer];
    int64_t mine = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
      len[u] = 0;
      if (first + u < (int64_t)n_active) {
        const int64_t r = active[first + u];
        len[u] = rp.at(r + 1) - rp.at(r);
      }
      mine += len[u];
    }
    int64_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int64_t wave_off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      if (w < wave) wave_off += wave_tot[w];
      total += wave_tot[w];
    }
    __syncthreads();
    int64_t run = carry + wave_off + incl - mine;   // exclusive prefix of this thread's first row
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
      if (first + u < (int64_t)n_active) offs[first + u] = run;
      run += len[u];
    }
    carry += total;
  }
  if (threadIdx.x == 0) offs[n_active] = carry;
}

// ------------------------------------------------------------------------------------------ sparse update
// Row-driven (perm == nullptr): entry e of active row r is updated in place, w[e] += trace[col[e]].
// Permuted (perm != nullptr): the rows are those of the transposed structure; slot k of row r updates w[perm[k]] +=
// trace[col[k]] (random read-modify-write, one per slot, each weight owned by one slot).
constexpr int kRowThreads = 256, kRowPer = 8, kTile = kRowThreads * kRowPer;

// What an entry adds, given its secondary id j = col[e]: the trace lookup of k_plast_rows, a policy of two kinds.
// Plain: trace[j].
template <typename B>
struct TracePlain {
  const B* __restrict__ trace;
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ B at(int32_t j) const { return trace[j]; }
};

// Aged (delayed synapses): j is a row id d * n + i of a matrix stacked by delay (be_delay.hip) and the value is
// the one neuron i had d pushes ago in a ring of per-neuron values, values[depth][n] with age a in slot (head - 1 - a) mod depth.
// head is read once per workgroup (thread 0, broadcast through LDS).  d < depth is the caller's contract (be_plasticity_rows_aged
// checks ages <= depth), so one conditional add is the whole modulo.  The division is a 32-bit unsigned one: j < 2^31.
template <typename B>
struct TraceAged {
  const B* __restrict__ values;
  const int32_t* __restrict__ head;
  uint32_t n;
  int depth;
  int h;
  __device__ __forceinline__ void begin() {
    __shared__ int h_sh;
    if (threadIdx.x == 0) {
      const int v = *head;
      h_sh = ((unsigned)v < (unsigned)depth) ? v : 0;
    }
    __syncthreads();
    h = h_sh;
  }
  __device__ __forceinline__ B at(int32_t j) const {
    const uint32_t d = (uint32_t)j / n;
    const uint32_t i = (uint32_t)j - d * n;
    int slot = h - 1 - (int)(d < (uint32_t)depth ? d : (uint32_t)depth - 1u);   // (the clamp only keeps a broken id in bounds)
    if (slot < 0) slot += depth;
    return values[(int64_t)slot * n + i];
  }
};

template <typename W, typename PT, bool PERM, bool CLIP, typename TR>
__global__ void __launch_bounds__(kRowThreads) k_plast_rows(typename PB<W>::bits* __restrict__ w,
                                                            const int32_t* __restrict__ col, RowPtr rp,
                                                            const PT* __restrict__ perm, TR tr,
                                                            const uint32_t* __restrict__ active,
                                                            const uint32_t* __restrict__ n_active_p,
                                                            const int64_t* __restrict__ offs, ClipArgs c) {
  using B = typename PB<W>::bits;
  tr.begin();
  const int64_t n_active = *n_active_p;
  const int64_t total = offs[n_active];
  for (int64_t tile = (int64_t)blockIdx.x * kTile; tile < total; tile += (int64_t)gridDim.x * kTile) {
    int64_t p = tile + threadIdx.x;
    if (p >= total) break;
    // active row a holding virtual position p: the last a with offs[a] <= p
    int64_t lo = 0, hi = n_active - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (offs[mid] <= p) lo = mid; else hi = mid - 1;
    }
    int64_t a = lo;
    int64_t a_end = offs[a + 1];
    int64_t row_start = rp.at(active[a]) - offs[a];   // entry index = row_start + p
#pragma unroll 2
    for (int u = 0; u < kRowPer; ++u, p += kRowThreads) {
      if (p >= total) break;
      while (p >= a_end) {        // rows shorter than the stride (or empty) are stepped over
        ++a;
        a_end = offs[a + 1];
        row_start = rp.at(active[a]) - offs[a];
      }
      const int64_t e = row_start + p;
      const int32_t j = __builtin_nontemporal_load(col + e);
      const B t = tr.at(j);
      if (PERM) {
        const int64_t we = (int64_t)__builtin_nontemporal_load(perm + e);
        w[we] = plast_add<W, CLIP>(w[we], t, c);
      } else {
        const B old = __builtin_nontemporal_load(w + e);
        __builtin_nontemporal_store(plast_add<W, CLIP>(old, t, c), w + e);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ dense update
// pre: every active row i gets w[i, :] += trace[:] (contiguous); gridDim.y splits the columns
template <typename W, bool CLIP>
__global__ void __launch_bounds__(256) k_plast_dense_rows(typename PB<W>::bits* __restrict__ w, int64_t n_cols,
                                                          const typename PB<W>::bits* __restrict__ trace,
                                                          const uint32_t* __restrict__ active,
                                                          const uint32_t* __restrict__ n_active_p, int64_t cols_per_y,
                                                          ClipArgs c) {
  using B = typename PB<W>::bits;
  const uint32_t n_active = *n_active_p;
  const int64_t c0 = (int64_t)blockIdx.y * cols_per_y;
  const int64_t c1 = c0 + cols_per_y < n_cols ? c0 + cols_per_y : n_cols;
  for (uint32_t a = blockIdx.x; a < n_active; a += gridDim.x) {
    B* row = w + (int64_t)active[a] * n_cols;
    for (int64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
      const B old = __builtin_nontemporal_load(row + j);
      __builtin_nontemporal_store(plast_add<W, CLIP>(old, trace[j], c), row + j);
    }
  }
}

// post: every row i gets w[i, j] += trace[i] for each active column j
template <typename W, bool CLIP>
__global__ void __launch_bounds__(256) k_plast_dense_cols(typename PB<W>::bits* __restrict__ w, int64_t n_rows,
                                                          int64_t n_cols, const typename PB<W>::bits* __restrict__ trace,
                                                          const uint32_t* __restrict__ active,
                                                          const uint32_t* __restrict__ n_active_p, ClipArgs c) {
  using B = typename PB<W>::bits;
  const uint32_t n_active = *n_active_p;
  if (n_active == 0) return;
  for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
    B* row = w + i * n_cols;
    const B t = trace[i];
    for (uint32_t a = threadIdx.x; a < n_active; a += blockDim.x) {
      const uint32_t j = active[a];
      row[j] = plast_add<W, CLIP>(row[j], t, c);
    }
  }
}

// ------------------------------------------------------------------------------------------ host helpers
// workspace: count (256 B) | active ids | offsets (int64) | float-spike bytes
struct PlastWs {
  uint32_t* count;
  uint32_t* active;
  int64_t* offs;
  uint8_t* bytes;
};

int64_t plast_ws_bytes(int64_t n) {
  return counts_bytes(1) + active_stride_of(n) * 4 + be_align_up((n + 1) * 8, 256) + be_align_up(n, 256);
}

PlastWs plast_ws(void* ws, int64_t n) {
  unsigned char* b = static_cast<unsigned char*>(ws);
  PlastWs p;
  p.count = reinterpret_cast<uint32_t*>(b);
  b += counts_bytes(1);
  p.active = reinterpret_cast<uint32_t*>(b);
  b += active_stride_of(n) * 4;
  p.offs = reinterpret_cast<int64_t*>(b);
  b += be_align_up((n + 1) * 8, 256);
  p.bytes = b;
  return p;
}

// the active rows of `spikes` (any of the four spike codes) as a device list + device count
int plast_active(const void* spikes, int sd, int64_t n, const PlastWs& ws, hipStream_t st, ActiveList* al) {
  if (sd == BE_SPIKE_FLOAT) {
    if (n > 0) {
      hipLaunchKernelGGL(k_plast_nonzero, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, static_cast<const float*>(spikes),
                         n, ws.bytes);
      BE_LAUNCH_CHECK();
    }
    spikes = ws.bytes;
    sd = BE_SPIKE_BOOL;
  }
  BE_REQUIRE(sd == BE_SPIKE_BOOL || sd == BE_SPIKE_BITS || sd == BE_SPIKE_IDS, BE_ERR_INVALID, "unknown spike dtype");
  return be_resolve_active(spikes, sd, n, 1, ws.active, active_stride_of(n), ws.count, st, true, al);
}

template <typename W, typename PT, bool PERM, typename TR>
void launch_rows(void* weights, const int32_t* col, RowPtr rp, const void* perm, TR tr, const ActiveList& al,
                 const int64_t* offs, ClipArgs c, int grid, hipStream_t st) {
  using B = typename PB<W>::bits;
  if (c.lo_on || c.hi_on)
    hipLaunchKernelGGL((k_plast_rows<W, PT, PERM, true, TR>), dim3(grid), dim3(kRowThreads), 0, st, static_cast<B*>(weights), col,
                       rp, static_cast<const PT*>(perm), tr, al.ids, al.count, offs, c);
  else
    hipLaunchKernelGGL((k_plast_rows<W, PT, PERM, false, TR>), dim3(grid), dim3(kRowThreads), 0, st, static_cast<B*>(weights), col,
                       rp, static_cast<const PT*>(perm), tr, al.ids, al.count, offs, c);
}

// the trace operand as the host hands it in: make<W>() is the kernel's lookup policy; `permuted_only` leaves the row-driven
// instantiations of a policy that has no row-driven caller out of the library
struct PlainOperand {
  static constexpr bool permuted_only = false;
  const void* trace;
  template <typename W> TracePlain<typename PB<W>::bits> make() const {
    return {static_cast<const typename PB<W>::bits*>(trace)};
  }
};

struct AgedOperand {
  static constexpr bool permuted_only = true;
  const void* values;
  const int32_t* head;
  uint32_t n;
  int depth;
  template <typename W> TraceAged<typename PB<W>::bits> make() const {
    return {static_cast<const typename PB<W>::bits*>(values), head, n, depth, 0};
  }
};

template <typename W, typename OP>
int plast_rows_t(void* weights, const int32_t* col, RowPtr rp, const void* perm, int perm64, const OP& operand,
                 const ActiveList& al, const int64_t* offs, ClipArgs c, int64_t nnz_hint, hipStream_t st) {
  // enough tiles to fill the chip at the largest update, never more workgroups than tiles of the whole structure
  const int grid = grid_for(nnz_hint, kTile, 4096);
  const auto tr = operand.template make<W>();
  const int prof = be_prof_begin(st);
  if (perm == nullptr) {
    if constexpr (!OP::permuted_only) launch_rows<W, int32_t, false>(weights, col, rp, nullptr, tr, al, offs, c, grid, st);
  } else if (perm64) launch_rows<W, int64_t, true>(weights, col, rp, perm, tr, al, offs, c, grid, st);
  else launch_rows<W, int32_t, true>(weights, col, rp, perm, tr, al, offs, c, grid, st);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

// the shared body of be_plasticity_rows and be_plasticity_rows_aged: compaction of the spikes, offsets scan, update
template <typename OP>
int plast_rows_run(void* weights, int wdtype, const int32_t* indices, RowPtr rp, int64_t nnz, const void* perm, int perm64,
                   const void* spikes, int spike_dtype, int64_t n_rows, const OP& operand, ClipArgs c, void* workspace,
                   hipStream_t st) {
  const PlastWs ws = plast_ws(workspace, n_rows);
  ActiveList al;
  int rc = plast_active(spikes, spike_dtype, n_rows, ws, st, &al);
  if (rc != BE_OK) return rc;
  hipLaunchKernelGGL(k_plast_offsets, dim3(1), dim3(kScanThreads), 0, st, rp, al.ids, al.count, ws.offs);
  BE_LAUNCH_CHECK();
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return plast_rows_t<W>(weights, indices, rp, perm, perm64, operand, al, ws.offs, c, nnz, st);
  });
}

template <typename W>
int plast_dense_t(bool pre, void* weights, int64_t n_rows, int64_t n_cols, const void* trace, const ActiveList& al,
                  int64_t n_active_max, ClipArgs c, hipStream_t st) {
  using B = typename PB<W>::bits;
  const bool clip = c.lo_on || c.hi_on;
  const int prof = be_prof_begin(st);
  if (pre) {
    const int64_t cols_per_y = 4096;
    const unsigned gy = (unsigned)((n_cols + cols_per_y - 1) / cols_per_y);
    const unsigned gx = (unsigned)grid_for(n_active_max, 1, (int)(2048 / gy > 8 ? 2048 / gy : 8));   // ~2048 workgroups
    if (clip)
      hipLaunchKernelGGL((k_plast_dense_rows<W, true>), dim3(gx, gy), dim3(256), 0, st, static_cast<B*>(weights), n_cols,
                         static_cast<const B*>(trace), al.ids, al.count, cols_per_y, c);
    else
      hipLaunchKernelGGL((k_plast_dense_rows<W, false>), dim3(gx, gy), dim3(256), 0, st, static_cast<B*>(weights), n_cols,
                         static_cast<const B*>(trace), al.ids, al.count, cols_per_y, c);
  } else {
    const unsigned gx = (unsigned)grid_for(n_rows, 1, 8192);
    if (clip)
      hipLaunchKernelGGL((k_plast_dense_cols<W, true>), dim3(gx), dim3(256), 0, st, static_cast<B*>(weights), n_rows, n_cols,
                         static_cast<const B*>(trace), al.ids, al.count, c);
    else
      hipLaunchKernelGGL((k_plast_dense_cols<W, false>), dim3(gx), dim3(256), 0, st, static_cast<B*>(weights), n_rows, n_cols,
                         static_cast<const B*>(trace), al.ids, al.count, c);
  }
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

// the active list (and, with `rp`, the entry offsets) of a spike vector for the plan upkeep of be_csr_plan.hip (declared in
// be_csr_shared.h): the same workspace layout, compaction and offsets scan as be_plasticity_rows
int64_t be_plast_active_bytes(int64_t n) { return plast_ws_bytes(n); }

int be_plast_active_offsets(const void* spikes, int sd, int64_t n, const RowPtr* rp, void* workspace, hipStream_t st,
                            ActiveList* al, const int64_t** offs) {
  const PlastWs ws = plast_ws(workspace, n);
  int rc = plast_active(spikes, sd, n, ws, st, al);
  if (rc != BE_OK) return rc;
  if (rp != nullptr) {
    hipLaunchKernelGGL(k_plast_offsets, dim3(1), dim3(kScanThreads), 0, st, *rp, al->ids, al->count, ws.offs);
    BE_LAUNCH_CHECK();
    *offs = ws.offs;
  }
  return BE_OK;
}

extern "C" {

int64_t be_plasticity_workspace_bytes(int64_t n_rows) { return n_rows < 0 ? (int64_t)BE_ERR_INVALID : plast_ws_bytes(n_rows); }

int be_plasticity_rows(void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                       int64_t row_len, int64_t nnz, const void* perm, int perm_is_i64, const void* spikes, int spike_dtype,
                       int64_t n_rows, const void* trace, int clip_lo, double w_lo, int clip_hi, double w_hi,
                       void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_rows <= 0xffffffffll && nnz >= 0, BE_ERR_INVALID, "n_rows / nnz out of range");
  BE_REQUIRE(indptr != nullptr || row_len >= 0, BE_ERR_INVALID, "fixed row length < 0 without indptr");
  BE_REQUIRE(workspace_bytes >= plast_ws_bytes(n_rows) && workspace != nullptr, BE_ERR_WORKSPACE, "workspace too small");
  if (n_rows == 0 || nnz == 0) return BE_OK;
  BE_REQUIRE(weights && indices && trace && spikes, BE_ERR_INVALID, "null pointer");
  return plast_rows_run(weights, wdtype, indices, RowPtr{indptr, indptr_is_i64, row_len}, nnz, perm, perm_is_i64, spikes,
                        spike_dtype, n_rows, PlainOperand{trace}, ClipArgs{clip_lo, clip_hi, w_lo, w_hi}, workspace,
                        static_cast<hipStream_t>(stream));
}

int be_plasticity_rows_aged(void* weights, int wdtype, const int32_t* t_rows, const void* t_indptr, int indptr_is_i64,
                            int64_t nnz, const void* perm, int perm_is_i64, const void* spikes, int spike_dtype,
                            int64_t n_post, const void* values, const int32_t* head, int64_t n_pre, int ring_depth, int ages,
                            int clip_lo, double w_lo, int clip_hi, double w_hi, void* workspace, int64_t workspace_bytes,
                            be_stream_t stream) {
  BE_REQUIRE(n_post >= 0 && n_post <= 0xffffffffll && nnz >= 0, BE_ERR_INVALID, "n_post / nnz out of range");
  BE_REQUIRE(n_pre >= 1 && ages >= 1 && ages <= ring_depth && (int64_t)ring_depth * n_pre < (1ll << 31), BE_ERR_INVALID,
             "need n_pre >= 1, 1 <= ages <= ring_depth, ring_depth * n_pre < 2^31");
  BE_REQUIRE(workspace_bytes >= plast_ws_bytes(n_post) && workspace != nullptr, BE_ERR_WORKSPACE, "workspace too small");
  if (n_post == 0 || nnz == 0) return BE_OK;
  BE_REQUIRE(weights && t_rows && t_indptr && perm && values && head && spikes, BE_ERR_INVALID, "null pointer");
  return plast_rows_run(weights, wdtype, t_rows, RowPtr{t_indptr, indptr_is_i64, -1}, nnz, perm, perm_is_i64, spikes,
                        spike_dtype, n_post, AgedOperand{values, head, (uint32_t)n_pre, ring_depth},
                        ClipArgs{clip_lo, clip_hi, w_lo, w_hi}, workspace, static_cast<hipStream_t>(stream));
}

int be_plasticity_dense(int pre, void* weights, int wdtype, int64_t n_rows, int64_t n_cols, const void* spikes,
                        int spike_dtype, const void* trace, int clip_lo, double w_lo, int clip_hi, double w_hi,
                        void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows <= 0xffffffffll && n_cols <= 0xffffffffll, BE_ERR_INVALID,
             "shape out of range");
  const int64_t n_spk = pre ? n_rows : n_cols;
  BE_REQUIRE(workspace_bytes >= plast_ws_bytes(n_spk) && workspace != nullptr, BE_ERR_WORKSPACE, "workspace too small");
  if (n_rows == 0 || n_cols == 0) return BE_OK;
  BE_REQUIRE(weights && trace && spikes, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PlastWs ws = plast_ws(workspace, n_spk);
  ActiveList al;
  int rc = plast_active(spikes, spike_dtype, n_spk, ws, st, &al);
  if (rc != BE_OK) return rc;
  const ClipArgs c{clip_lo, clip_hi, w_lo, w_hi};
  return be_dispatch_wdtype(wdtype, [&](auto w) {
    using W = typename decltype(w)::type;
    return plast_dense_t<W>(pre != 0, weights, n_rows, n_cols, trace, al, n_spk, c, st);
  });
}

}  // extern "C"
