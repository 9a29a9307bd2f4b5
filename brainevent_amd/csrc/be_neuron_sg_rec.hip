// be_neuron_sg_rec.hip — the differentiable recurrent spiking layer: §2.21's neuron (the step of be_sg_lane.h,
// as be_neuron_sg.hip runs it per slot) with a CSR recurrence INSIDE the time loop.  Step t's input is x[t] + s[t-1] @ W_rec, so
// the T steps of a sample are one dependent chain through all of its N neurons: one workgroup owns one sample for the whole
// launch and keeps its spikes on the chip.
//
// Forwards (k_lif_rec_forward), per step: the previous step's spikes — one bit per owned neuron, in registers — are compacted into
// an id list in LDS (ballot / popcount, as k_compact_spikes); the listed rows are walked kRecRowLanes lanes per row and scattered
// into 64-bit fixed-point sums in LDS with integer atomics (ds_add_u64: the fast kind, see the top of be_csr.hip; order
// independent, so the pass is a function of its inputs bit for bit); every thread then runs §2.21's step for its neurons on
// x[t] + r and clears the sums it read.  Backwards (k_lif_rec_backward), per step: g_x[t+1] of the sample stays in an f32 LDS
// array, g_rec is a row gather from it (kRecRowLanes lanes per row, each a strided f32 partial sum, then a butterfly: a fixed
// order), and §2.21's backward step follows.  A thread owns neurons tid, tid + kRecThreads, ... — at most kRecPerThread of them,
// their state in registers whose indices are compile-time constants (no scratch).  Everything is f32, every operation rounded on
// its own (no FMA contraction).  Global traffic is plain vector loads and stores; no global atomics.
#include "be_sg_lane.h"

namespace {

namespace lane = be_sg_lane;

constexpr int kRecThreads = 1024;
// one sample's neurons: forwards 8 B (sums) + 4 B (ids) per neuron in LDS — 96 KB of the CU's 160 KB at the limit
constexpr int kRecMaxN = 8192;
constexpr int kRecPerThread = kRecMaxN / kRecThreads;
constexpr int kRecRowLanes = 16;
constexpr int kRecWaves = kRecThreads / kWave;
constexpr int kRecRowGroups = kRecThreads / kRecRowLanes;
// entries of a row a lane loads before it uses the first: rows up to kRecUnroll * kRecRowLanes entries take one trip
constexpr int kRecUnroll = 4;
// the exponents be_fixed_point_exponent returns (2^(e - 32) must be a normal f32)
constexpr int kRecMinExp = -90, kRecMaxExp = 150;

struct RowSpan {
  int begin, end;
};

__device__ __forceinline__ RowSpan row_span(const int32_t* __restrict__ indptr, uint32_t row) {
  return RowSpan{indptr[row], indptr[row + 1]};
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N].  s0 / c0 / v0 / a0 NULL = 0;
// v_seq / h_save / th_save may be NULL.  Dynamic LDS: N 64-bit sums, then N ids.
template <bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kRecThreads)
k_lif_rec_forward(const float* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ indices,
                  const int32_t* __restrict__ indptr, const float* __restrict__ s0, const float* __restrict__ c0,
                  const float* __restrict__ v0, const float* __restrict__ a0, float* __restrict__ s_out, float* __restrict__ v_seq,
                  float* __restrict__ h_save, float* __restrict__ th_save, float* __restrict__ c_last, float* __restrict__ v_last,
                  float* __restrict__ a_last, int64_t T, int64_t B, int N, float scale, double inv, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_raw);
  uint32_t* ids = reinterpret_cast<uint32_t*>(acc + N);
  __shared__ uint32_t wave_tot[kRecWaves];
  const int tid = threadIdx.x, ln = tid & (kWave - 1), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  float c[kRecPerThread], v[kRecPerThread], a[kRecPerThread];
  uint32_t sbits = 0;                                    // bit k: neuron tid + k * kRecThreads spiked at the previous step
#pragma unroll
  for (int k = 0; k < kRecPerThread; ++k) {
    const int i = tid + k * kRecThreads;
    c[k] = v[k] = a[k] = 0.f;
    if (i < N) {
      if (c0 != nullptr) c[k] = c0[base + i];
      if (v0 != nullptr) v[k] = v0[base + i];
      if (ADAPT && a0 != nullptr) a[k] = a0[base + i];
      if (s0 != nullptr && s0[base + i] != 0.f) sbits |= 1u << k;
      acc[i] = 0ull;
    }
  }
  for (int64_t t = 0; t < T; ++t) {
    const int64_t at = t * step + base;
    float xv[kRecPerThread];                             // does not depend on the chain: in flight during the scatter
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      xv[k] = 0.f;
      if (i < N) xv[k] = x[at + i];
    }
    // the previous step's spikes -> ids[0 .. n_active) (unordered: the sums do not depend on the order)
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k)
      if (k * kRecThreads < N) tot += (uint32_t)__popcll(__ballot((sbits >> k) & 1u));
    if (ln == 0) wave_tot[wave] = tot;
    __syncthreads();
    uint32_t pos = 0, n_active = 0;
#pragma unroll
    for (int q = 0; q < kRecWaves; ++q) {
      const uint32_t n = wave_tot[q];
      if (q < wave) pos += n;
      n_active += n;
    }
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      if (k * kRecThreads < N) {
        const bool on = (sbits >> k) & 1u;
        const unsigned long long m = __ballot(on);
        if (on) ids[pos + (uint32_t)__popcll(m & ((1ull << ln) - 1ull))] = (uint32_t)(tid + k * kRecThreads);
        pos += (uint32_t)__popcll(m);
      }
    }
    __syncthreads();
    // the listed rows, kRecRowLanes lanes per row: R[col] += fixed(w)
    // (the next row's bounds and a lane's next kRecUnroll entries are loaded before anything waits for them: the walk is bound by
    // the latency of dependent loads, id -> indptr -> entry, not by bytes)
    uint32_t r = tid / kRecRowLanes;
    RowSpan cur = r < n_active ? row_span(indptr, ids[r]) : RowSpan{0, 0};
    while (r < n_active) {
      const uint32_t rn = r + kRecRowGroups;
      const RowSpan next = rn < n_active ? row_span(indptr, ids[rn]) : RowSpan{0, 0};
      for (int k = cur.begin + (tid % kRecRowLanes); k < cur.end; k += kRecUnroll * kRecRowLanes) {
        int col[kRecUnroll];
        float wk[kRecUnroll];
#pragma unroll
        for (int q = 0; q < kRecUnroll; ++q) {
          const bool in = k + q * kRecRowLanes < cur.end;
          col[q] = in ? indices[k + q * kRecRowLanes] : -1;
          wk[q] = in ? w[k + q * kRecRowLanes] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kRecUnroll; ++q)
          if (col[q] >= 0) atomicAdd(&acc[col[q]], fixed_from_f32(wk[q], scale));
      }
      r = rn;
      cur = next;
    }
    __syncthreads();
    sbits = 0;
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      if (i < N) {
        const unsigned long long R = acc[i];
        acc[i] = 0ull;                                   // read and cleared by its owner only: no barrier in between
        const float r = (float)((double)(long long)R * inv);
        const lane::Fired f = lane::forward_step<HARD, true, ADAPT>(xv[k] + r, c[k], v[k], a[k], p.beta, p.v_th, p);
        if (f.s) sbits |= 1u << k;
        s_out[at + i] = f.s ? 1.0f : 0.0f;
        if (v_seq != nullptr) v_seq[at + i] = v[k];
        if (h_save != nullptr) {
          h_save[at + i] = f.h;
          if (ADAPT) th_save[at + i] = f.th;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRecPerThread; ++k) {
    const int i = tid + k * kRecThreads;
    if (i < N) {
      c_last[base + i] = c[k];
      v_last[base + i] = v[k];
      if (ADAPT) a_last[base + i] = a[k];
    }
  }
}

// out[row] = sum over the entries k of row `row` of w[k] * G[col[k]], G in LDS: lane j of the row's kRecRowLanes takes the
// entries j, j + kRecRowLanes, ... in order, then a butterfly over the lanes (the same order on every call)
__device__ __forceinline__ void rec_gather(const float* __restrict__ w, const int32_t* __restrict__ indices,
                                           const int32_t* __restrict__ indptr, const float* G, int N, float* out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, sub = tid % kRecRowLanes;
  int row = tid / kRecRowLanes;
  RowSpan cur = row < N ? row_span(indptr, row) : RowSpan{0, 0};
  while (row < N) {
    const int rn = row + kRecRowGroups;
    const RowSpan next = rn < N ? row_span(indptr, rn) : RowSpan{0, 0};
    float sum = 0.f;
    for (int k = cur.begin + sub; k < cur.end; k += kRecUnroll * kRecRowLanes) {
      int col[kRecUnroll];
      float wk[kRecUnroll];
#pragma unroll
      for (int q = 0; q < kRecUnroll; ++q) {                 // in flight together; added below in the order of k
        const bool in = k + q * kRecRowLanes < cur.end;
        col[q] = in ? indices[k + q * kRecRowLanes] : -1;
        wk[q] = in ? w[k + q * kRecRowLanes] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < kRecUnroll; ++q) {
        const float term = wk[q] * G[col[q] >= 0 ? col[q] : 0];
        sum = col[q] >= 0 ? sum + term : sum;
      }
    }
#pragma unroll
    for (int off = kRecRowLanes / 2; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, kRecRowLanes);
    if (sub == 0) out[row] = sum;
    row = rn;
    cur = next;
  }
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; the others [B, N].  g_s / g_vseq / g_clast / g_vlast / g_alast
// NULL = 0; g_c0 / g_v0 / g_a0 / g_s0 may be NULL.  Dynamic LDS: g_x[t+1] of the sample, then g_rec (N floats each).
template <bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kRecThreads)
k_lif_rec_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ w,
                   const int32_t* __restrict__ indices, const int32_t* __restrict__ indptr, const float* __restrict__ g_s,
                   const float* __restrict__ g_vseq, const float* __restrict__ g_clast, const float* __restrict__ g_vlast,
                   const float* __restrict__ g_alast, float* __restrict__ g_x, float* __restrict__ g_c0, float* __restrict__ g_v0,
                   float* __restrict__ g_a0, float* __restrict__ g_s0, int64_t T, int64_t B, int N, int detach_reset, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* G = reinterpret_cast<float*>(smem_raw);
  float* grec = G + N;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  float cc[kRecPerThread], cv[kRecPerThread], ca[kRecPerThread];
#pragma unroll
  for (int k = 0; k < kRecPerThread; ++k) {
    const int i = tid + k * kRecThreads;
    cc[k] = cv[k] = ca[k] = 0.f;
    if (i < N) {
      if (g_clast != nullptr) cc[k] = g_clast[base + i];
      if (g_vlast != nullptr) cv[k] = g_vlast[base + i];
      if (ADAPT && g_alast != nullptr) ca[k] = g_alast[base + i];
    }
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t at = t * step + base;
    const bool rec = t < T - 1;
    float hv[kRecPerThread], tv[kRecPerThread], gsv[kRecPerThread], gvv[kRecPerThread];   // in flight during the gather
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = h_save[at + i];
        if (ADAPT) tv[k] = th_save[at + i];
        if (g_s != nullptr) gsv[k] = g_s[at + i];
        if (g_vseq != nullptr) gvv[k] = g_vseq[at + i];
      }
    }
    if (rec) {
      rec_gather(w, indices, indptr, G, N, grec);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], ADAPT ? tv[k] : p.v_th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        g_x[at + i] = g_c;
        G[i] = g_c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kRecPerThread; ++k) {
    const int i = tid + k * kRecThreads;
    if (i < N) {
      if (g_c0 != nullptr) g_c0[base + i] = cc[k];
      if (g_v0 != nullptr) g_v0[base + i] = cv[k];
      if (ADAPT && g_a0 != nullptr) g_a0[base + i] = ca[k];
    }
  }
  if (g_s0 != nullptr) rec_gather(w, indices, indptr, G, N, g_s0 + base);      // from g_x[0]
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int rec_check_common(const char* who, int64_t T, int64_t B, int64_t N, int reset_mode) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode" : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kRecMaxN || B > 0x7fffffffll) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons (limit: " + std::to_string(kRecMaxN) +
                 ", one sample's sums and spike ids in one workgroup's LDS), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

}  // namespace

extern "C" {

int be_lif_rec_sg_forward(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const float* s0,
                          const float* c0, const float* v0, const float* a0, float* s_out, float* v_seq, float* h_save,
                          float* th_save, float* c_last, float* v_last, float* a_last, int64_t T, int64_t B, int64_t N,
                          double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                          int adaptive, int scale_exp, be_stream_t stream) {
  if (const int rc = rec_check_common(__func__, T, B, N, reset_mode)) return rc;
  BE_REQUIRE(scale_exp >= kRecMinExp && scale_exp <= kRecMaxExp, BE_ERR_INVALID,
             "scale_exp outside the exponents be_fixed_point_exponent returns (-90 .. 150)");
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const float scale = ldexpf(1.0f, scale_exp - 32);   // see fixed_from_f32
  const double inv = ldexp(1.0, -scale_exp);
  const int lds = (int)be_align_up(N * 12, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      auto kern = k_lif_rec_forward<decltype(H)::value, decltype(A)::value>;
      allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
      if (allowed == hipSuccess)
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kRecThreads), lds, st, x, w, indices, indptr, s0, c0, v0, a0, s_out, v_seq,
                           h_save, th_save, c_last, v_last, a_last, T, B, (int)N, scale, inv, p);
      return BE_OK;
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_sg_backward(const float* h_save, const float* th_save, const float* w, const int32_t* indices, const int32_t* indptr,
                           const float* g_s, const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                           float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0, int64_t T, int64_t B, int64_t N,
                           double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                           int surrogate, double alpha, int adaptive, int detach_reset, be_stream_t stream) {
  if (const int rc = rec_check_common(__func__, T, B, N, reset_mode)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  const bool hard = reset_mode == BE_LIF_RESET_HARD;
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int lds = (int)be_align_up(N * 8, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int detach = detach_reset != 0;
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        auto kern = k_lif_rec_backward<decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
        allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
        if (allowed == hipSuccess)
          hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kRecThreads), lds, st, h_save, th_save, w, indices, indptr, g_s, g_vseq,
                             g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0, g_s0, T, B, (int)N, detach, p);
        return BE_OK;
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
