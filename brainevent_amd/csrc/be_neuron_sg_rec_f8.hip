// be_neuron_sg_rec_f8.hip — the fused recurrent spiking layer over a CSR recurrence kept in OCP FP8 CODES, e4m3 or
// e5m2, with one f32 scale: a Float8CSR's arrays as they are — one byte per stored entry in `codes`, its column in
// `indices`, the rows in an int32 `indptr`.  Step t's input is
//     xin[t][j] = x[t][j] + f32( f64(R[j]) * ldexp(f64(w_scale), -E) ),   R[j] = sum of Q(codes[k]) over the entries k of column j in the rows that spiked,
// Q(c) = decode(c) * 2^E (E = 9 / 16) an integer and R an exact 64-bit sum: Float8CSR's own product finish (be_csr_f8.hip), so the
// layer equals the per-step loop of `events @ W8` bit for bit and there is no exponent.  The split of work is be_neuron_sg_rec.hip's,
// restated (that file keeps its kernels to itself): one 1024-thread workgroup owns one sample for the whole launch, a thread's
// neurons tid + k * 1024 keep their state in registers, the previous step's spikes are compacted into an id list in LDS by ballot /
// popcount, the sums are ds_add_u64 on LDS words, the neuron is be_sg_lane.h's.  What is new is the ROW WALK, made for one byte per
// weight.
//
// Forwards (k_lif_rec_f8_forward).  The arrays are read as ALIGNED QUADS: quad q is the entries 4q .. 4q + 3, four codes in one
// 4-byte load and their four columns in one 16-byte load — two loads for four synapses where the f32 kernel issues eight.  A row
// [begin, end) covers the quads begin / 4 .. (end - 1) / 4; its kF8sRowLanes lanes take them round robin, kF8sUnroll quads of a lane
// in flight before the first is used and the next row's bounds before the current row's quads (the walk is bound by the latency of
// dependent loads, id -> indptr -> entry).  The entries of a quad outside [begin, end) — the neighbours' — are masked out of the code
// word: a code 0 is the integer 0 and adds nothing, and neither do the stored +0 / -0.  The decode is f8_fixed (be_csr_shared.h):
// integer ALU, no conversion, no table.  Integer sums: which lane adds which entry does not matter.  The container is not
// repacked.  VEC = false (codes not 4-byte aligned or indices not 16-byte aligned) reads the same quads an entry at a time, only
// the entries of the row; with VEC the one quad that reaches past nse is read that way too: nothing outside [0, nse) is ever read.
//
// Backwards (k_lif_rec_f8_backward).  g_rec[i] = fl32( (sum over row i of fl32(decode(codes[k])) * G[indices[k]]) * w_scale ), G = g_x[t+1]
// of the sample in LDS.  Here the order of the f32 sum is part of the contract — the row's length alone fixes it — so the quads
// are taken RELATIVE to the row's first entry: lane l of the row's kF8sRowLanes takes the entries begin + 4 * (l + m * kF8sRowLanes)
// .. + 3, m = 0, 1, ..., in ascending order, every product rounded on its own, one f32 partial sum per lane, then a butterfly over the
// lanes, then the scale, once per row.  A whole quad inside the row is still one 4-byte and one 16-byte load (at the entry's own
// alignment: 1 and 4 bytes), the row's last, partial quad is read an entry at a time: nothing outside the row is read, so this
// pass has one instance for every alignment and needs no nse.  The decode is v_cvt_pk_f32_fp8 / _bf8 (OCP on gfx950), exact.
//
// No global atomics, no spin waits, nothing between workgroups; every barrier sits in uniform control flow and every loop is bounded
// by T, N and the rows' lengths.  The caller guarantees finite codes, columns in [0, N) and a non-decreasing indptr within [0, nse].
#include "be_csr_shared.h"
#include "be_sg_lane.h"

typedef float f8s_v2f __attribute__((ext_vector_type(2)));

namespace {

namespace lane = be_sg_lane;

constexpr int kF8sThreads = 1024;
// one sample's neurons: forwards 8 B (sums) + 4 B (ids) per neuron in LDS — 96 KB of the CU's 160 KB at the limit
constexpr int kF8sMaxN = 8192;
constexpr int kF8sPerThread = kF8sMaxN / kF8sThreads;
constexpr int kF8sWaves = kF8sThreads / kWave;
// lanes per row: 8 lanes * 4 entries is one trip for a row of up to 32 entries and leaves 128 rows in flight per workgroup
constexpr int kF8sRowLanes = 8;
constexpr int kF8sRowGroups = kF8sThreads / kF8sRowLanes;
// quads a lane loads before it uses the first: rows up to 4 * kF8sUnroll * kF8sRowLanes = 64 entries take one trip (as the f32 kernel)
constexpr int kF8sUnroll = 2;

struct Span {
  uint32_t begin, end;
};

__device__ __forceinline__ Span f8s_span(const int32_t* __restrict__ indptr, uint32_t row) {
  return Span{(uint32_t)indptr[row], (uint32_t)indptr[row + 1]};
}

// four entries: their codes, the lowest byte first, and their columns
struct Quad {
  uint32_t codes;
  int col[4];
};
constexpr Quad kNoQuad{0u, {0, 0, 0, 0}};

// Quad q of the arrays with every entry outside [lo, hi) as code 0 (the quad overlaps [lo, hi) within [0, nse)).  VEC and the whole
// quad below nse: two loads, then the mask; else the entries inside [lo, hi) one by one.
template <bool VEC>
__device__ __forceinline__ Quad f8s_quad(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices, uint32_t q, uint32_t lo,
                                         uint32_t hi, uint32_t nse) {
  const uint32_t e0 = 4u * q;
  Quad out = kNoQuad;
  if (VEC && e0 + 4u <= nse) {
    const uint32_t word = reinterpret_cast<const uint32_t*>(codes)[q];
    const int4 c = reinterpret_cast<const int4*>(indices)[q];
    const uint32_t first = lo > e0 ? lo - e0 : 0u, last = hi < e0 + 4u ? hi - e0 : 4u;      // 0 <= first < last <= 4
    const uint32_t keep = (uint32_t)((1ull << (8u * last)) - 1ull) & ~((1u << (8u * first)) - 1u);
    out.codes = word & keep;
    out.col[0] = c.x, out.col[1] = c.y, out.col[2] = c.z, out.col[3] = c.w;
    return out;
  }
#pragma unroll
  for (uint32_t h = 0; h < 4u; ++h) {
    if (e0 + h >= lo && e0 + h < hi) {
      out.codes |= (uint32_t)codes[e0 + h] << (8u * h);
      out.col[h] = indices[e0 + h];
    }
  }
  return out;
}

// the id list's rows, kF8sRowLanes lanes per row: R[col] += Q(code) for every entry of every listed row
template <int FMT, bool VEC>
__device__ __forceinline__ void f8s_scatter(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices,
                                            const int32_t* __restrict__ indptr, uint32_t nse, const uint32_t* ids, uint32_t n_active,
                                            unsigned long long* acc) {
  const uint32_t tid = threadIdx.x, sub = tid % kF8sRowLanes;
  uint32_t r = tid / kF8sRowLanes;
  Span cur = r < n_active ? f8s_span(indptr, ids[r]) : Span{0u, 0u};
  while (r < n_active) {
    const uint32_t rn = r + kF8sRowGroups;
    const Span next = rn < n_active ? f8s_span(indptr, ids[rn]) : Span{0u, 0u};
    if (cur.begin < cur.end) {
      const uint32_t q1 = (cur.end + 3u) >> 2;             // one past the row's last quad
      for (uint32_t q = (cur.begin >> 2) + sub; q < q1; q += kF8sUnroll * kF8sRowLanes) {
        Quad qd[kF8sUnroll];
#pragma unroll
        for (int u = 0; u < kF8sUnroll; ++u) {               // in flight together
          const uint32_t qq = q + (uint32_t)u * kF8sRowLanes;
          qd[u] = kNoQuad;
          if (qq < q1) qd[u] = f8s_quad<VEC>(codes, indices, qq, cur.begin, cur.end, nse);
        }
#pragma unroll
        for (int u = 0; u < kF8sUnroll; ++u) {
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const unsigned long long v = f8_fixed<FMT>((qd[u].codes >> (8 * h)) & 0xffu);
            if (v != 0ull) atomicAdd(&acc[qd[u].col[h]], v);   // (a masked entry and both zeros add nothing)
          }
        }
      }
    }
    r = rn;
    cur = next;
  }
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N].  s0 / c0 / v0 / a0 NULL = 0; v_seq /
// h_save / th_save may be NULL.  Dynamic LDS: N 64-bit sums, then N ids.  inv = ldexp((double)w_scale, -E).
template <int FMT, bool HARD, bool ADAPT, bool VEC>
__global__ void __launch_bounds__(kF8sThreads)
k_lif_rec_f8_forward(const float* __restrict__ x, const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices,
                     const int32_t* __restrict__ indptr, uint32_t nse, const float* __restrict__ s0, const float* __restrict__ c0,
                     const float* __restrict__ v0, const float* __restrict__ a0, float* __restrict__ s_out, float* __restrict__ v_seq,
                     float* __restrict__ h_save, float* __restrict__ th_save, float* __restrict__ c_last, float* __restrict__ v_last,
                     float* __restrict__ a_last, int64_t T, int64_t B, int N, double inv, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_raw);
  uint32_t* ids = reinterpret_cast<uint32_t*>(acc + N);
  __shared__ uint32_t wave_tot[kF8sWaves];
  const int tid = threadIdx.x, ln = tid & (kWave - 1), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  float c[kF8sPerThread], v[kF8sPerThread], a[kF8sPerThread];
  uint32_t sbits = 0;                                    // bit k: neuron tid + k * kF8sThreads spiked at the previous step
#pragma unroll
  for (int k = 0; k < kF8sPerThread; ++k) {
    const int i = tid + k * kF8sThreads;
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
    float xv[kF8sPerThread];                             // does not depend on the chain: in flight during the scatter
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k) {
      const int i = tid + k * kF8sThreads;
      xv[k] = 0.f;
      if (i < N) xv[k] = x[at + i];
    }
    // the previous step's spikes -> ids[0 .. n_active) (unordered: the sums do not depend on the order)
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k)
      if (k * kF8sThreads < N) tot += (uint32_t)__popcll(__ballot((sbits >> k) & 1u));
    if (ln == 0) wave_tot[wave] = tot;
    __syncthreads();
    uint32_t pos = 0, n_active = 0;
#pragma unroll
    for (int q = 0; q < kF8sWaves; ++q) {
      const uint32_t n = wave_tot[q];
      if (q < wave) pos += n;
      n_active += n;
    }
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k) {
      if (k * kF8sThreads < N) {
        const bool on = (sbits >> k) & 1u;
        const unsigned long long m = __ballot(on);
        if (on) ids[pos + (uint32_t)__popcll(m & ((1ull << ln) - 1ull))] = (uint32_t)(tid + k * kF8sThreads);
        pos += (uint32_t)__popcll(m);
      }
    }
    __syncthreads();
    f8s_scatter<FMT, VEC>(codes, indices, indptr, nse, ids, n_active, acc);
    __syncthreads();
    sbits = 0;
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k) {
      const int i = tid + k * kF8sThreads;
      if (i < N) {
        const unsigned long long R = acc[i];
        acc[i] = 0ull;                                   // read and cleared by its owner only: no barrier in between
        const float r = (float)((double)(long long)R * inv);   // be_csr_f8.hip's k_f8_convert
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
  for (int k = 0; k < kF8sPerThread; ++k) {
    const int i = tid + k * kF8sThreads;
    if (i < N) {
      c_last[base + i] = c[k];
      v_last[base + i] = v[k];
      if (ADAPT) a_last[base + i] = a[k];
    }
  }
}

// two codes of a word -> two f32, exactly (HI: the upper pair)
template <int FMT, bool HI>
__device__ __forceinline__ f8s_v2f f8s_pair(uint32_t w) {
  if (FMT == BE_F8_E4M3) return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
}

// out[row] = (sum over the entries k of row `row` of decode(codes[k]) * G[indices[k]]) * w_scale, G in LDS: lane l of the row's
// kF8sRowLanes takes the quads l, l + kF8sRowLanes, ... COUNTED FROM THE ROW'S FIRST ENTRY, in order, then a butterfly over the
// lanes, then the scale (the same order on every call, fixed by the row's length).  Only the row's own entries are read.
template <int FMT>
__device__ __forceinline__ void f8s_gather(const uint8_t* __restrict__ codes, const int32_t* __restrict__ indices,
                                           const int32_t* __restrict__ indptr, const float* G, int N, float w_scale, float* out) {
#pragma clang fp contract(off)
  const uint32_t tid = threadIdx.x, sub = tid % kF8sRowLanes;
  int row = (int)(tid / kF8sRowLanes);
  Span cur = row < N ? f8s_span(indptr, (uint32_t)row) : Span{0u, 0u};
  while (row < N) {
    const int rn = row + kF8sRowGroups;
    const Span next = rn < N ? f8s_span(indptr, (uint32_t)rn) : Span{0u, 0u};
    float sum = 0.f;
    for (uint32_t k = cur.begin + 4u * sub; k < cur.end; k += 4u * kF8sUnroll * kF8sRowLanes) {
      Quad qd[kF8sUnroll];
#pragma unroll
      for (int u = 0; u < kF8sUnroll; ++u) {                 // in flight together; added below in the order of k
        const uint32_t kk = k + 4u * (uint32_t)u * kF8sRowLanes;
        qd[u] = kNoQuad;
        if (kk + 4u <= cur.end) {                            // a whole quad of the row: one load each, at the entry's alignment
          __builtin_memcpy(&qd[u].codes, codes + kk, 4);
          __builtin_memcpy(qd[u].col, indices + kk, 16);
        } else {
#pragma unroll
          for (uint32_t h = 0; h < 4u; ++h) {
            if (kk + h < cur.end) {
              qd[u].codes |= (uint32_t)codes[kk + h] << (8u * h);
              qd[u].col[h] = indices[kk + h];
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kF8sUnroll; ++u) {
        const uint32_t kk = k + 4u * (uint32_t)u * kF8sRowLanes;
        const f8s_v2f lo = f8s_pair<FMT, false>(qd[u].codes), hi = f8s_pair<FMT, true>(qd[u].codes);
        const float w[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
        for (uint32_t h = 0; h < 4u; ++h) {                  // (an absent entry: code 0 times G[0], not added)
          const float term = w[h] * G[qd[u].col[h]];
          sum = kk + h < cur.end ? sum + term : sum;
        }
      }
    }
#pragma unroll
    for (int off = kF8sRowLanes / 2; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, kF8sRowLanes);
    if (sub == 0) out[row] = sum * w_scale;
    row = rn;
    cur = next;
  }
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; the others [B, N].  g_s / g_vseq / g_clast / g_vlast / g_alast
// NULL = 0; g_c0 / g_v0 / g_a0 / g_s0 may be NULL.  Dynamic LDS: g_x[t+1] of the sample, then g_rec (N floats each).
template <int FMT, bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kF8sThreads)
k_lif_rec_f8_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const uint8_t* __restrict__ codes,
                      const int32_t* __restrict__ indices, const int32_t* __restrict__ indptr, const float* __restrict__ g_s,
                      const float* __restrict__ g_vseq, const float* __restrict__ g_clast, const float* __restrict__ g_vlast,
                      const float* __restrict__ g_alast, float* __restrict__ g_x, float* __restrict__ g_c0, float* __restrict__ g_v0,
                      float* __restrict__ g_a0, float* __restrict__ g_s0, int64_t T, int64_t B, int N, int detach_reset, float w_scale,
                      lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* G = reinterpret_cast<float*>(smem_raw);
  float* grec = G + N;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  float cc[kF8sPerThread], cv[kF8sPerThread], ca[kF8sPerThread];
#pragma unroll
  for (int k = 0; k < kF8sPerThread; ++k) {
    const int i = tid + k * kF8sThreads;
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
    float hv[kF8sPerThread], tv[kF8sPerThread], gsv[kF8sPerThread], gvv[kF8sPerThread];   // in flight during the gather
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k) {
      const int i = tid + k * kF8sThreads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = h_save[at + i];
        if (ADAPT) tv[k] = th_save[at + i];
        if (g_s != nullptr) gsv[k] = g_s[at + i];
        if (g_vseq != nullptr) gvv[k] = g_vseq[at + i];
      }
    }
    if (rec) {
      f8s_gather<FMT>(codes, indices, indptr, G, N, w_scale, grec);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kF8sPerThread; ++k) {
      const int i = tid + k * kF8sThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const float th = ADAPT ? tv[k] : p.v_th;         // the threshold h was compared with
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        g_x[at + i] = g_c;
        G[i] = g_c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kF8sPerThread; ++k) {
    const int i = tid + k * kF8sThreads;
    if (i < N) {
      if (g_c0 != nullptr) g_c0[base + i] = cc[k];
      if (g_v0 != nullptr) g_v0[base + i] = cv[k];
      if (ADAPT && g_a0 != nullptr) g_a0[base + i] = ca[k];
    }
  }
  if (g_s0 != nullptr) f8s_gather<FMT>(codes, indices, indptr, G, N, w_scale, g_s0 + base);      // from g_x[0]
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int f8s_check_common(const char* who, int64_t T, int64_t B, int64_t N, int reset_mode, int fmt_code, double w_scale, int64_t nse) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : (fmt_code != BE_F8_E4M3 && fmt_code != BE_F8_E5M2)                   ? ": fmt_code must be BE_F8_E4M3 or BE_F8_E5M2"
                    : !std::isfinite((float)w_scale)                                       ? ": w_scale must be a finite f32"
                    : (nse < 0 || nse > 0x7fffffffll)                                      ? ": nse must lie in 0 .. 2^31 - 1"
                                                                                           : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kF8sMaxN || B > 0x7fffffffll) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons (limit: " + std::to_string(kF8sMaxN) +
                 ", one sample's sums and spike ids in one workgroup's LDS), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

}  // namespace

extern "C" {

int be_lif_rec_f8_sg_forward(const float* x, const void* codes, int fmt_code, double w_scale, const int32_t* indices,
                             const int32_t* indptr, int64_t nse, const float* s0, const float* c0, const float* v0, const float* a0,
                             float* s_out, float* v_seq, float* h_save, float* th_save, float* c_last, float* v_last, float* a_last,
                             int64_t T, int64_t B, int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho,
                             double kappa, int reset_mode, int adaptive, be_stream_t stream) {
  if (const int rc = f8s_check_common(__func__, T, B, N, reset_mode, fmt_code, w_scale, nse)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(codes && indices && indptr, BE_ERR_INVALID, "null pointer (codes, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const bool vec = reinterpret_cast<uintptr_t>(codes) % 4 == 0 && reinterpret_cast<uintptr_t>(indices) % 16 == 0;
  const double inv = ldexp((double)(float)w_scale, fmt_code == BE_F8_E4M3 ? -kF8ExpE4M3 : -kF8ExpE5M2);
  const int lds = (int)be_align_up(N * 12, 16);
  const uint8_t* cp = static_cast<const uint8_t*>(codes);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_int<BE_F8_E4M3, BE_F8_E5M2>(fmt_code, [&](auto F) {
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        return be_dispatch_bool(vec, [&](auto V) {
          auto kern = k_lif_rec_f8_forward<decltype(F)::value, decltype(H)::value, decltype(A)::value, decltype(V)::value>;
          allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
          if (allowed == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kF8sThreads), lds, st, x, cp, indices, indptr, (uint32_t)nse, s0, c0, v0,
                               a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, B, (int)N, inv, p);
          return BE_OK;
        });
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_f8_sg_backward(const float* h_save, const float* th_save, const void* codes, int fmt_code, double w_scale,
                              const int32_t* indices, const int32_t* indptr, int64_t nse, const float* g_s, const float* g_vseq,
                              const float* g_clast, const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0,
                              float* g_a0, float* g_s0, int64_t T, int64_t B, int64_t N, double syn_decay, double beta, double v_th,
                              double v_reset, double rho, double kappa, int reset_mode, int surrogate, double alpha, int adaptive,
                              int detach_reset, be_stream_t stream) {
  if (const int rc = f8s_check_common(__func__, T, B, N, reset_mode, fmt_code, w_scale, nse)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(codes && indices && indptr, BE_ERR_INVALID, "null pointer (codes, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int lds = (int)be_align_up(N * 8, 16);
  const int detach = (int)(detach_reset != 0);
  const uint8_t* cp = static_cast<const uint8_t*>(codes);
  const float scale = (float)w_scale;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_int<BE_F8_E4M3, BE_F8_E5M2>(fmt_code, [&](auto F) {
    return be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
      return be_dispatch_bool(adapt, [&](auto A) {
        return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
          auto kern = k_lif_rec_f8_backward<decltype(F)::value, decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
          allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
          if (allowed == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kF8sThreads), lds, st, h_save, th_save, cp, indices, indptr, g_s, g_vseq,
                               g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0, g_s0, T, B, (int)N, detach, scale, p);
          return BE_OK;
        });
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
