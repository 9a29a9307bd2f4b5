// be_csr_f8_gather.hip — the streaming gather over FP8 stored rows on gfx950: out[b, i] = sum of the entries of stored row i whose
// input fired (semantics: include/brainevent_amd.h, "FP8 weights for the event-driven CSR products", gather direction).  It is the
// product `events @ W8.T` of a Float8CSR and `events @ Float8CSC`.  A row's sum R_i is an exact 64-bit integer of Q(code) =
// f8_fixed<FMT>, so the lanes of a row may split it any way: LPR lanes walk a row, each keeps an int64 partial sum, one cross-lane
// reduce per row, and the row's lane 0 stores f32(f64(R) * inv).  No atomics, no accumulator workspace, no convert launch: the
// workspace only holds the packed spike bitmaps (be_pack_spikes_batched; BE_SPIKE_BITS is read in place).
//
// The matrix streams are read once, 5 bytes per entry: 16 bytes of indices and 4 bytes of codes per lane and load (nt, as
// be_csr.hip's gather kernels load theirs).  A row may start at any byte of `codes`, so a row is walked in the QUADS of the code
// array — groups of four entries whose first code sits at a 4-byte-aligned address — starting at the quad that holds the row's
// first entry; entries of the quad outside [row start, row end) are masked.  A quad that does not lie wholly inside
// [0, nnz) — the first of a misaligned array, the last when the array's end is no quad boundary — is read entry by entry, and
// only the row's own entries: no load reaches past codes + nnz or indices + nnz.
#include "be_csr_shared.h"

namespace {

// The packed input bitmap goes to LDS when it is at most this large (k <= 1 228 800 columns) and is read from global memory
// (L2) above: one compile-time switch, IN_LDS.
constexpr int64_t kF8GatherLdsBitmapBytes = 150 * 1024;
// lanes per row by the average row length nnz / m; a wave per row above the last.  A pass of a row is 4 * LPR entries and a trip of
// the walk holds two, as in be_csr.hip's k_csrmv_nt_vec, whose thresholds these are: taken over by reasoning (the same entries per
// lane and trip), not searched for this kernel.  Measured here: against a first version with 4 / 16 / 64 lanes only (up to 16 / 128
// entries), rows of 200 went from 0.661 to 0.424 ms and rows of 30 from 0.373 to 0.300 ms (1M and 2M rows, 1 % firing) — lanes that
// a short row leaves idle still issue the whole trip; rows of 10, 100 and 1000 keep their instance and their time.
constexpr int64_t kF8GatherLpr2MaxRow = 8, kF8GatherLpr4MaxRow = 20, kF8GatherLpr8MaxRow = 45, kF8GatherLpr16MaxRow = 100,
                  kF8GatherLpr32MaxRow = 200;
// quads (passes of the row) a lane has in flight per trip of the walk.  Measured at 2, 4 and 8 (1M x 1M, 1 % firing; 4 / 16 / 64
// lanes on rows of 10 / 100 / 1000): 0.23 / 0.27 / 0.42, 0.22 / 0.29 / 0.44 and 1.42 / 1.46 / 1.99 ms — more in flight loses everywhere.
constexpr int kF8GatherQuads = 2;
constexpr int kF8GatherThreads = 1024;   // 16 waves share one LDS bitmap
constexpr int kF8GatherGridCap = 512;    // workgroups per batch row; rows beyond a grid trip are taken grid-stride

typedef unsigned be_f8g_v4u __attribute__((ext_vector_type(4)));
// four column ids of a quad: a quad is aligned for its CODE bytes, so its ids sit at any dword — the 16-byte load is declared with
// the 4-byte alignment it really has (global_load_dwordx4 needs no more)
typedef be_f8g_v4u be_f8g_v4u_a4 __attribute__((aligned(4)));

// the quad of entries [j, j + 4) of the row [b, e): columns, the four codes as one word, bit t of `valid` = entry j + t is the row's
__device__ __forceinline__ void f8_ld_quad(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices, int64_t j,
                                           int64_t b, int64_t e, int64_t nnz, be_f8g_v4u& c, uint32_t& w, uint32_t& valid) {
  c = be_f8g_v4u{0u, 0u, 0u, 0u};
  w = 0u;
  valid = 0u;
  if (j >= e) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) valid |= ((j + t >= b && j + t < e) ? 1u : 0u) << t;
  if (j >= 0 && j + 4 <= nnz) {        // wholly inside the arrays: codes + j is 4-byte aligned by the choice of the quads
    c = __builtin_nontemporal_load(reinterpret_cast<const be_f8g_v4u_a4*>(indices + j));
    w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(codes + j));
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if ((valid >> t) & 1u) {
        c[t] = (uint32_t)indices[j + t];
        w |= (uint32_t)codes[j + t] << (8 * t);
      }
  }
}

template <int FMT>
__device__ __forceinline__ unsigned long long f8_quad_sum(const uint32_t* __restrict__ bits, be_f8g_v4u c, uint32_t w, uint32_t valid) {
  uint32_t word[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t col = ((valid >> t) & 1u) ? c[t] : 0u;      // (what is not the row's may be anything: test column 0, then drop it)
    c[t] = col;
    word[t] = bits[col >> 5];
  }
  unsigned long long s = 0ull;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t on = (word[t] >> (c[t] & 31u)) & (valid >> t) & 1u;
    s += f8_fixed<FMT>((w >> (8 * t)) & 0xffu) & (0ull - (unsigned long long)on);
  }
  return s;
}

// LPR lanes per stored row; rows r0 + group, r0 advancing by the grid's groups (wave-uniform trip count: every lane reaches the
// reduce); batch row = blockIdx.y
template <int FMT, int LPR, bool IN_LDS>
__global__ void __launch_bounds__(kF8GatherThreads) k_csrmv_nt_f8(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices,
                                                                  RowPtr rp, int64_t nnz, const uint32_t* __restrict__ bits_g,
                                                                  int64_t n_words, float* __restrict__ out, int64_t m, double inv) {
  constexpr int PASS = 4 * LPR;          // entries of a row per pass; a trip of the walk holds two passes
  bits_g += (int64_t)blockIdx.y * n_words;
  out += (int64_t)blockIdx.y * m;
  extern __shared__ uint32_t bits_s[];
  if (IN_LDS) {
    for (int64_t i = threadIdx.x; i < n_words; i += kF8GatherThreads) bits_s[i] = bits_g[i];
    __syncthreads();
  }
  const uint32_t* __restrict__ bits = IN_LDS ? bits_s : bits_g;
  const int sub = threadIdx.x % LPR;
  const int64_t grp = ((int64_t)blockIdx.x * kF8GatherThreads + threadIdx.x) / LPR;
  const int64_t n_grp = (int64_t)gridDim.x * (kF8GatherThreads / LPR);
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(codes) & 3);
  for (int64_t r0 = 0; r0 < m; r0 += n_grp) {
    const int64_t r = r0 + grp;
    const bool live = r < m;
    int64_t b = 0, e = 0;
    if (live) {
      b = rp.at(r);
      e = rp.at(r + 1);
    }
    unsigned long long acc = 0ull;
    // the quad that holds entry b starts at b - ((b + mis) & 3): there codes + j is 4-byte aligned
    for (int64_t j = b - ((b + mis) & 3) + 4 * sub; j < e; j += kF8GatherQuads * PASS) {
      be_f8g_v4u c[kF8GatherQuads];
      uint32_t w[kF8GatherQuads], v[kF8GatherQuads];
#pragma unroll
      for (int u = 0; u < kF8GatherQuads; ++u) f8_ld_quad(codes, indices, j + u * PASS, b, e, nnz, c[u], w[u], v[u]);
#pragma unroll
      for (int u = 0; u < kF8GatherQuads; ++u) acc += f8_quad_sum<FMT>(bits, c[u], w[u], v[u]);
    }
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LPR);
    if (live && sub == 0) out[r] = (float)((double)(long long)acc * inv);
  }
}

static inline int64_t f8_gather_ws_bytes(int64_t k, int64_t nb) { return be_align_up(std::max<int64_t>(((k + 31) / 32) * nb * 4, 1), 256); }

static inline int f8_gather_lpr_of(int64_t avg) {
  if (avg <= kF8GatherLpr2MaxRow) return 2;
  if (avg <= kF8GatherLpr4MaxRow) return 4;
  if (avg <= kF8GatherLpr8MaxRow) return 8;
  if (avg <= kF8GatherLpr16MaxRow) return 16;
  return avg <= kF8GatherLpr32MaxRow ? 32 : 64;
}

template <int FMT, int LPR, bool IN_LDS>
int launch_f8_gather(const uint8_t* codes, const int32_t* indices, RowPtr rp, int64_t nnz, const uint32_t* bits, int64_t n_words,
                     float* out, int64_t m, int64_t nb, double inv, hipStream_t st) {
  auto kern = k_csrmv_nt_f8<FMT, LPR, IN_LDS>;
  const size_t lds = IN_LDS ? (size_t)n_words * 4 : 0;
  if (IN_LDS) BE_HIP(be_allow_lds(reinterpret_cast<const void*>(kern), (int)lds));
  const int grid = grid_for(m, kF8GatherThreads / LPR, kF8GatherGridCap);
  const int prof = be_prof_begin(st);
  hipLaunchKernelGGL(kern, dim3(grid, (unsigned)nb), dim3(kF8GatherThreads), lds, st, codes, indices, rp, nnz, bits, n_words, out, m, inv);
  be_prof_end(prof, st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int64_t be_binary_csrmm_nt_f8_workspace_bytes(int64_t m, int64_t k, int64_t n_batch) {
  if (m < 0 || k < 0 || n_batch < 0) return (int64_t)BE_ERR_INVALID;
  return f8_gather_ws_bytes(k, n_batch);
}
int64_t be_binary_csrmv_nt_f8_workspace_bytes(int64_t m, int64_t k) { return be_binary_csrmm_nt_f8_workspace_bytes(m, k, 1); }

int be_binary_csrmm_nt_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                          int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes_bm, int spike_dtype, void* out_bm,
                          int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(f8_format == BE_F8_E4M3 || f8_format == BE_F8_E5M2, BE_ERR_INVALID, "f8_format must be BE_F8_E4M3 or BE_F8_E5M2");
  BE_REQUIRE(m >= 0 && k >= 0 && m <= 0xffffffffll && k <= 0xffffffffll && nnz >= 0, BE_ERR_INVALID, "bad shape");
  BE_REQUIRE(n_batch >= 0 && n_batch <= kMaxBatch, BE_ERR_INVALID, "n_batch out of range");
  BE_REQUIRE(std::isfinite((float)scale), BE_ERR_INVALID, "scale must be a finite f32");
  BE_REQUIRE(spike_dtype >= BE_SPIKE_BOOL && spike_dtype <= BE_SPIKE_IDS, BE_ERR_INVALID, "unknown spike dtype");
  if (m == 0 || k == 0 || n_batch == 0) return BE_OK;
  BE_REQUIRE(spike_dtype != BE_SPIKE_IDS, BE_ERR_UNSUPPORTED, "BE_SPIKE_IDS is not taken by the gather direction (a bitmap is)");
  BE_REQUIRE(check_rows(indptr, row_len), BE_ERR_INVALID, "indptr is NULL and row_len < 0");
  BE_REQUIRE(indptr != nullptr || row_len == 0 || nnz / row_len >= m, BE_ERR_INVALID, "nnz is below m * row_len");
  BE_REQUIRE(spikes_bm && out_bm && (nnz == 0 || (codes && indices)), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(workspace != nullptr && workspace_bytes >= f8_gather_ws_bytes(k, n_batch), BE_ERR_WORKSPACE, "workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_words = (k + 31) / 32;
  const uint32_t* bits = static_cast<const uint32_t*>(spikes_bm);      // BE_SPIKE_BITS: read in place
  if (spike_dtype != BE_SPIKE_BITS) {
    const int rc = be_pack_spikes_batched(spikes_bm, spike_dtype, k, n_batch, static_cast<uint32_t*>(workspace), stream);
    if (rc != BE_OK) return rc;
    bits = static_cast<const uint32_t*>(workspace);
  }
  const RowPtr rp{indptr, indptr_is_i64, row_len};
  const double inv = ldexp((double)(float)scale, f8_format == BE_F8_E4M3 ? -kF8ExpE4M3 : -kF8ExpE5M2);
  const bool in_lds = n_words * 4 <= kF8GatherLdsBitmapBytes;
  return be_dispatch_int<BE_F8_E4M3, BE_F8_E5M2>(f8_format, [&](auto f) {
    return be_dispatch_int<2, 4, 8, 16, 32, 64>(f8_gather_lpr_of(nnz / m), [&](auto l) {
      return be_dispatch_bool(in_lds, [&](auto b) {
        return launch_f8_gather<decltype(f)::value, decltype(l)::value, decltype(b)::value>(
            static_cast<const uint8_t*>(codes), indices, rp, nnz, bits, n_words, static_cast<float*>(out_bm), m, n_batch, inv, st);
      });
    });
  });
}

int be_binary_csrmv_nt_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                          int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes, int spike_dtype, void* out, int64_t m,
                          int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  return be_binary_csrmm_nt_f8(codes, f8_format, scale, indices, indptr, indptr_is_i64, row_len, nnz, spikes, spike_dtype, out, m, k, 1,
                               workspace, workspace_bytes, stream);
}

}  // extern "C"
