// be_csr_f8.hip — the exact direct route of `events @ Float8CSR` on gfx950 (semantics: include/brainevent_amd.h, "FP8 weights
// for the event-driven CSR products").  Every finite OCP FP8 code is an integer multiple of 2^-E (E = 9 for e4m3, 16 for e5m2), so a
// column's sum R_j is an exact 64-bit integer whatever the order of the adds: the spikes are compacted as in the other direct
// routes, a lane group walks each active row and adds Q(code) into an int64[k] workspace with global 64-bit INTEGER atomics, and
// one convert kernel applies out[j] = (float)((double)R_j * inv).  No layout, no limits on row length or slice count: this route
// serves what the sorted q8 plan (be_csr_plan.hip) refuses, and gives the same bits.
#include "be_csr_shared.h"

namespace {

// LPR lanes per active row (a row of r entries keeps min(r, LPR) lanes busy)
template <int FMT, int LPR>
__global__ void __launch_bounds__(256) k_csrmv_t_f8_direct(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices,
                                                           RowPtr rp, const uint32_t* __restrict__ active,
                                                           const uint32_t* __restrict__ n_active_p,
                                                           unsigned long long* __restrict__ acc, int64_t active_stride, int64_t k) {
  active += (int64_t)blockIdx.y * active_stride;
  acc += (int64_t)blockIdx.y * k;
  const uint32_t n_active = n_active_p[blockIdx.y];
  const uint32_t l = threadIdx.x % LPR;
  const uint32_t grp = (blockIdx.x * blockDim.x + threadIdx.x) / LPR;
  const uint32_t n_grp = (gridDim.x * blockDim.x) / LPR;
  for (uint32_t a = grp; a < n_active; a += n_grp) {
    const int64_t r = active[a];
    const int64_t b = rp.at(r), e = rp.at(r + 1);
    for (int64_t j = b + l; j < e; j += LPR) {
      const unsigned long long v = f8_fixed<FMT>(codes[j]);
      if (v != 0ull) atomicAdd(acc + indices[j], v);        // (both zeros add nothing)
    }
  }
}

// out[i] = (float)((double)(long long)R[i] * inv): one rounding of the exact product while |R| < 2^53
__global__ void __launch_bounds__(256) k_f8_convert(const unsigned long long* __restrict__ acc, float* __restrict__ out, int64_t n,
                                                    double inv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = (float)((double)(long long)acc[i] * inv);
}

constexpr int64_t kF8ShortRow = 16;     // average row length up to which 16 lanes walk a row (a wave per row above)

static inline int64_t f8_direct_ws_bytes(int64_t m, int64_t k, int64_t nb) {
  return counts_bytes(nb) + nb * active_stride_of(m) * 4 + be_align_up(nb * k * 8, 256);
}

}  // namespace

extern "C" {

int64_t be_binary_csrmm_t_f8_workspace_bytes(int64_t m, int64_t k, int64_t n_batch) {
  if (m < 0 || k < 0 || n_batch < 0) return (int64_t)BE_ERR_INVALID;
  return f8_direct_ws_bytes(m, k, n_batch);
}
int64_t be_binary_csrmv_t_f8_workspace_bytes(int64_t m, int64_t k) { return be_binary_csrmm_t_f8_workspace_bytes(m, k, 1); }

int be_binary_csrmm_t_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                         int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes_bm, int spike_dtype, void* out_bm,
                         int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(f8_format == BE_F8_E4M3 || f8_format == BE_F8_E5M2, BE_ERR_INVALID, "f8_format must be BE_F8_E4M3 or BE_F8_E5M2");
  BE_REQUIRE(m >= 0 && k >= 0 && m <= 0xffffffffll && k <= 0xffffffffll && nnz >= 0, BE_ERR_INVALID, "bad shape");
  BE_REQUIRE(n_batch >= 0 && n_batch <= kMaxBatch, BE_ERR_INVALID, "n_batch out of range");
  BE_REQUIRE(std::isfinite((float)scale), BE_ERR_INVALID, "scale must be a finite f32");
  BE_REQUIRE(spike_dtype >= BE_SPIKE_BOOL && spike_dtype <= BE_SPIKE_IDS, BE_ERR_INVALID, "unknown spike dtype");
  if (m == 0 || k == 0 || n_batch == 0) return BE_OK;
  BE_REQUIRE(spike_dtype != BE_SPIKE_IDS || n_batch == 1, BE_ERR_UNSUPPORTED, "BE_SPIKE_IDS takes a single event vector (n_batch = 1)");
  BE_REQUIRE(check_rows(indptr, row_len), BE_ERR_INVALID, "indptr is NULL and row_len < 0");
  BE_REQUIRE(spikes_bm && out_bm && (nnz == 0 || (codes && indices)), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(workspace != nullptr && workspace_bytes >= f8_direct_ws_bytes(m, k, n_batch), BE_ERR_WORKSPACE, "workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* wsb = static_cast<unsigned char*>(workspace);
  uint32_t* count = reinterpret_cast<uint32_t*>(wsb);
  uint32_t* active = reinterpret_cast<uint32_t*>(wsb + counts_bytes(n_batch));
  const int64_t astride = active_stride_of(m);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(wsb + counts_bytes(n_batch) + n_batch * astride * 4);
  BE_HIP(be_fill_async(acc, 0, (size_t)k * n_batch * 8, st));
  ActiveList al;
  const int rc = be_resolve_active(spikes_bm, spike_dtype, m, n_batch, active, astride, count, st, true, &al);
  if (rc != BE_OK) return rc;
  if (nnz > 0) {
    const RowPtr rp{indptr, indptr_is_i64, row_len};
    const int gx = n_batch >= 8 ? 512 : 2048;
    const bool short_rows = nnz / m <= kF8ShortRow;
    const int prof = be_prof_begin(st);
    const int rcl = be_dispatch_int<BE_F8_E4M3, BE_F8_E5M2>(f8_format, [&](auto f) {
      return be_dispatch_bool(short_rows, [&](auto s) {
        constexpr int LPR = decltype(s)::value ? 16 : 64;
        hipLaunchKernelGGL((k_csrmv_t_f8_direct<decltype(f)::value, LPR>), dim3(gx, (unsigned)n_batch), dim3(256), 0, st,
                           static_cast<const uint8_t*>(codes), indices, rp, al.ids, al.count, acc, astride, k);
        return (int)BE_OK;
      });
    });
    be_prof_end(prof, st);
    if (rcl != BE_OK) return rcl;
    BE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_f8_convert, dim3(grid_for(k * n_batch, 256, 2048)), dim3(256), 0, st, acc, static_cast<float*>(out_bm),
                     k * n_batch, ldexp((double)(float)scale, f8_format == BE_F8_E4M3 ? -kF8ExpE4M3 : -kF8ExpE5M2));
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_binary_csrmv_t_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                         int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes, int spike_dtype, void* out, int64_t m,
                         int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  return be_binary_csrmm_t_f8(codes, f8_format, scale, indices, indptr, indptr_is_i64, row_len, nnz, spikes, spike_dtype, out, m, k, 1,
                              workspace, workspace_bytes, stream);
}

}  // extern "C"
