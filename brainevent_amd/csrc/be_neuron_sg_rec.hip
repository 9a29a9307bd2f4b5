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
//
// PARAMS (be_lif_rec_sg_forward_params / _backward_params) is the same kernel pair with syn_decay, beta, v_th, rho and
// kappa read from DEVICE memory, one value for the layer (period 1) or one per neuron (period N), and with the per-(sample, neuron)
// accumulators of their gradients.  A 1024-thread workgroup leaves a lane 128 registers, and five values plus five accumulators
// for each of a thread's kRecPerThread neurons would be 80 of them: so a neuron's values are loaded where its step needs them
// ([N] arrays, at most 32 KB each: they stay in L2), and the accumulators live in the [B, N] output arrays themselves — an entry
// belongs to ONE thread, which at every step reads it (t = T-1: starts from +0 instead), adds the step's term and writes it back
// with plain 4-byte vector loads and stores, in program order: the additions are the ones a register accumulator would make, in
// the same order, so the bits are the same.  Without PARAMS none of this exists in the instantiation.
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

// PARAMS: the five parameter arrays, each with a period of 1 or N (the entry points check it)
struct RecParams {
  lane::ParamArr sd, beta, vth, rho, kappa;
};
constexpr RecParams kRecNoParams{{nullptr, 1}, {nullptr, 1}, {nullptr, 1}, {nullptr, 1}, {nullptr, 1}};

// PARAMS reaches every array it adds through a block-uniform base pointer plus a 32-bit byte offset, `off`, that a thread's arrays
// share (neuron i of the thread: off = 4 * i).  Addresses that do not change over the time loop — the five parameters, the five
// accumulators — would otherwise each be a 64-bit register pair per array and owned neuron, kept across the whole loop: 160
// registers where a lane has 128.  rec_fresh() makes the offset a new value at every step, so nothing derived from it is hoisted
// out of the loop; it emits no instruction.
__device__ __forceinline__ uint32_t rec_fresh(uint32_t off) {
  asm volatile("" : "+v"(off));
  return off;
}

__device__ __forceinline__ float rec_load(const float* base, uint32_t off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + off);
}

__device__ __forceinline__ void rec_store(float* base, uint32_t off, float value) {
  *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + off) = value;
}

// the neuron at `off`'s value of a parameter (no remainder is needed: the period is 1 or N)
__device__ __forceinline__ float rec_param(const lane::ParamArr& a, uint32_t off) {
  return rec_load(a.p, a.period == 1 ? 0u : off);
}

// Forward.  x, s_out, v_seq, h_save, th_save, c_save are [T, B, N]; s0, c0, v0, a0 and the *_last [B, N].  s0 / c0 / v0 / a0 NULL = 0;
// v_seq / h_save / th_save / c_save may be NULL.  Dynamic LDS: N 64-bit sums, then N ids.  With PARAMS q's arrays are read in the
// place of p's syn_decay, beta, v_th, rho and kappa, c_save (if given) takes the current after every step, and with ADAPT th_save
// takes the trace a the step STARTED from (the entry point's a_save), as in be_neuron_sg.hip; without PARAMS q and c_save are not
// touched.
template <bool HARD, bool ADAPT, bool PARAMS>
__global__ void __launch_bounds__(kRecThreads)
k_lif_rec_forward(const float* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ indices,
                  const int32_t* __restrict__ indptr, const float* __restrict__ s0, const float* __restrict__ c0,
                  const float* __restrict__ v0, const float* __restrict__ a0, RecParams q, float* __restrict__ s_out,
                  float* __restrict__ v_seq, float* __restrict__ h_save, float* __restrict__ th_save, float* __restrict__ c_save,
                  float* __restrict__ c_last, float* __restrict__ v_last, float* __restrict__ a_last, int64_t T, int64_t B, int N,
                  float scale, double inv, lane::LifP p) {
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
    const uint32_t off0 = PARAMS ? rec_fresh((uint32_t)tid * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      if (i < N) {
        const unsigned long long R = acc[i];
        acc[i] = 0ull;                                   // read and cleared by its owner only: no barrier in between
        const float r = (float)((double)(long long)R * inv);
        lane::LifP pi = p;                               // the step's constants: the kernel's, or the neuron's own
        if (PARAMS) {
          const uint32_t off = off0 + (uint32_t)k * (kRecThreads * 4u);
          pi.syn_decay = rec_param(q.sd, off), pi.beta = rec_param(q.beta, off), pi.v_th = rec_param(q.vth, off);
          if (ADAPT) pi.rho = rec_param(q.rho, off), pi.kappa = rec_param(q.kappa, off);
        }
        const float a_in = a[k];
        const lane::Fired f = lane::forward_step<HARD, true, ADAPT>(xv[k] + r, c[k], v[k], a[k], pi.beta, pi.v_th, pi);
        if (f.s) sbits |= 1u << k;
        s_out[at + i] = f.s ? 1.0f : 0.0f;
        if (v_seq != nullptr) v_seq[at + i] = v[k];
        if (h_save != nullptr) {
          h_save[at + i] = f.h;
          if (ADAPT) th_save[at + i] = PARAMS ? a_in : f.th;
        }
        if (PARAMS && c_save != nullptr) c_save[at + i] = c[k];
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
// With PARAMS q's arrays are the parameters, th_save holds the trace a_in every step started from (th = vth_i + (kappa_i * a_in) is
// formed as forwards) and each of the five slot arrays [B, N] that is given is the accumulator of its parameter's gradient, kept
// in memory by the entry's owner (see the top of the file):  a_sd += g_c * c_prev,  a_b += g_h * v_prev,  a_th -= g_u (+ the soft
// reset's direct term),  a_k -= g_u * a_in,  a_r += ca_in * a_in with the carry that ARRIVES at the step.  v_prev is recomputed
// from h_save[t-1] and its own threshold (v0 at t = 0, NULL = 0), c_prev is c_save[t-1] (c0 at t = 0, NULL = 0); c_save, c0 and
// v0 are read for g_sd_slot / g_beta_slot alone.  Without PARAMS none of these arguments is touched.
template <bool HARD, int SG, bool ADAPT, bool PARAMS>
__global__ void __launch_bounds__(kRecThreads)
k_lif_rec_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ c_save,
                   const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ w,
                   const int32_t* __restrict__ indices, const int32_t* __restrict__ indptr, const float* __restrict__ g_s,
                   const float* __restrict__ g_vseq, const float* __restrict__ g_clast, const float* __restrict__ g_vlast,
                   const float* __restrict__ g_alast, RecParams q, float* __restrict__ g_x, float* __restrict__ g_c0,
                   float* __restrict__ g_v0, float* __restrict__ g_a0, float* __restrict__ g_s0, float* __restrict__ g_sd_slot,
                   float* __restrict__ g_beta_slot, float* __restrict__ g_vth_slot, float* __restrict__ g_rho_slot,
                   float* __restrict__ g_kappa_slot, int64_t T, int64_t B, int N, int detach_reset, lane::LifP p) {
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
    const uint32_t off0 = PARAMS ? rec_fresh((uint32_t)tid * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < kRecPerThread; ++k) {
      const int i = tid + k * kRecThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        lane::LifP pi = p;                               // the step's constants: the kernel's, or the neuron's own
        float th = ADAPT ? tv[k] : p.v_th;               // the threshold h was compared with
        const uint32_t off = off0 + (uint32_t)k * (kRecThreads * 4u);
        if (PARAMS) {
          pi.syn_decay = rec_param(q.sd, off), pi.beta = rec_param(q.beta, off), pi.v_th = rec_param(q.vth, off);
          if (ADAPT) pi.rho = rec_param(q.rho, off), pi.kappa = rec_param(q.kappa, off);
          th = ADAPT ? pi.v_th + (pi.kappa * tv[k]) : pi.v_th;
        }
        const float ca_in = ca[k];
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, pi.v_th, g_sp, g_vo, ca[k], detach_reset, pi);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], pi.beta, pi);
        g_x[at + i] = g_c;
        G[i] = g_c;
        if (PARAMS) {
          // the accumulators, in memory: this thread alone reads and writes the entry at `off` of the sample's row, in program order
          const bool first = t == T - 1;
          if (g_sd_slot != nullptr) {
            float c_prev = 0.f;                          // the current the step started from
            if (t > 0) c_prev = rec_load(c_save + (at - step), off);
            else if (c0 != nullptr) c_prev = rec_load(c0 + base, off);
            const float sum = first ? 0.f : rec_load(g_sd_slot + base, off);
            rec_store(g_sd_slot + base, off, sum + (g_c * c_prev));
          }
          if (g_beta_slot != nullptr) {
            float v_prev = 0.f;                          // the membrane the step started from
            if (t > 0) {
              const float hp = rec_load(h_save + (at - step), off);
              const float tp = ADAPT ? pi.v_th + (pi.kappa * rec_load(th_save + (at - step), off)) : pi.v_th;
              v_prev = lane::membrane_after<HARD>(hp, tp, pi.v_th, p.v_reset);
            } else if (v0 != nullptr) {
              v_prev = rec_load(v0 + base, off);
            }
            const float sum = first ? 0.f : rec_load(g_beta_slot + base, off);
            rec_store(g_beta_slot + base, off, sum + (d.g_h * v_prev));
          }
          if (g_vth_slot != nullptr) {
            float direct = d.g_u;
            if (!HARD) direct = direct + (d.s ? g_vo : 0.0f);
            const float sum = first ? 0.f : rec_load(g_vth_slot + base, off);
            rec_store(g_vth_slot + base, off, sum - direct);
          }
          if (ADAPT && g_kappa_slot != nullptr) {
            const float sum = first ? 0.f : rec_load(g_kappa_slot + base, off);
            rec_store(g_kappa_slot + base, off, sum - (d.g_u * tv[k]));
          }
          if (ADAPT && g_rho_slot != nullptr) {
            const float sum = first ? 0.f : rec_load(g_rho_slot + base, off);
            rec_store(g_rho_slot + base, off, sum + (ca_in * tv[k]));
          }
        }
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

// a parameter's period: one value for the layer, or one per neuron
inline int rec_check_periods(const char* who, int64_t N, std::initializer_list<int64_t> periods) {
  for (const int64_t period : periods) {
    if (period == 1 || (period == N && N >= 1)) continue;
    be_set_error(std::string(who) + ": a period of " + std::to_string(period) + " (a parameter has period 1, one value for the layer, " +
                 "or period N = " + std::to_string(N) + ", one per neuron: the neurons are the same in every sample)");
    return BE_ERR_INVALID;
  }
  return BE_OK;
}

// the forward launch of both entry points (params: q holds the five arrays, th_save is a_save); the checks are the callers'
hipError_t rec_launch_forward(bool params, const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const float* s0,
                              const float* c0, const float* v0, const float* a0, const RecParams& q, float* s_out, float* v_seq,
                              float* h_save, float* th_save, float* c_save, float* c_last, float* v_last, float* a_last, int64_t T,
                              int64_t B, int64_t N, const lane::LifP& p, bool hard, bool adapt, int scale_exp, be_stream_t stream) {
  const float scale = ldexpf(1.0f, scale_exp - 32);   // see fixed_from_f32
  const double inv = ldexp(1.0, -scale_exp);
  const int lds = (int)be_align_up(N * 12, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      return be_dispatch_bool(params, [&](auto P) {
        auto kern = k_lif_rec_forward<decltype(H)::value, decltype(A)::value, decltype(P)::value>;
        allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
        if (allowed == hipSuccess)
          hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kRecThreads), lds, st, x, w, indices, indptr, s0, c0, v0, a0, q, s_out,
                             v_seq, h_save, th_save, c_save, c_last, v_last, a_last, T, B, (int)N, scale, inv, p);
        return BE_OK;
      });
    });
  });
  return allowed;
}

// the backward launch of both entry points
hipError_t rec_launch_backward(bool params, const float* h_save, const float* th_save, const float* c_save, const float* c0,
                               const float* v0, const float* w, const int32_t* indices, const int32_t* indptr, const float* g_s,
                               const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                               const RecParams& q, float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0, float* g_sd_slot,
                               float* g_beta_slot, float* g_vth_slot, float* g_rho_slot, float* g_kappa_slot, int64_t T, int64_t B,
                               int64_t N, const lane::LifP& p, bool hard, bool adapt, int surrogate, int detach, be_stream_t stream) {
  const int lds = (int)be_align_up(N * 8, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(hard, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        return be_dispatch_bool(params, [&](auto P) {
          auto kern = k_lif_rec_backward<decltype(H)::value, decltype(SG)::value, decltype(A)::value, decltype(P)::value>;
          allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
          if (allowed == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kRecThreads), lds, st, h_save, th_save, c_save, c0, v0, w, indices, indptr,
                               g_s, g_vseq, g_clast, g_vlast, g_alast, q, g_x, g_c0, g_v0, g_a0, g_s0, g_sd_slot, g_beta_slot,
                               g_vth_slot, g_rho_slot, g_kappa_slot, T, B, (int)N, detach, p);
          return BE_OK;
        });
      });
    });
  });
  return allowed;
}

constexpr const float* kNoIn = nullptr;
constexpr float* kNoOut = nullptr;

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
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const hipError_t allowed = rec_launch_forward(false, x, w, indices, indptr, s0, c0, v0, a0, kRecNoParams, s_out, v_seq, h_save, th_save, kNoOut, c_last,
                            v_last, a_last, T, B, N, p, reset_mode == BE_LIF_RESET_HARD, adapt, scale_exp, stream);
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
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const hipError_t allowed = rec_launch_backward(false, h_save, th_save, kNoIn, kNoIn, kNoIn, w, indices, indptr, g_s, g_vseq, g_clast, g_vlast, g_alast,
                             kRecNoParams, g_x, g_c0, g_v0, g_a0, g_s0, kNoOut, kNoOut, kNoOut, kNoOut, kNoOut, T, B, N, p,
                             reset_mode == BE_LIF_RESET_HARD, adapt, surrogate, (int)(detach_reset != 0), stream);
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_sg_forward_params(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const float* s0,
                                 const float* c0, const float* v0, const float* a0, const float* syn_decay, int64_t sd_period,
                                 const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period, const float* rho,
                                 int64_t rho_period, const float* kappa, int64_t kappa_period, float* s_out, float* v_seq,
                                 float* h_save, float* c_save, float* a_save, float* c_last, float* v_last, float* a_last, int64_t T,
                                 int64_t B, int64_t N, double v_reset, int reset_mode, int adaptive, int scale_exp,
                                 be_stream_t stream) {
  const bool adapt = adaptive != 0;
  if (!adapt) rho_period = 1, kappa_period = 1;                            // the adaptation's arguments are not looked at
  if (const int rc = rec_check_common(__func__, T, B, N, reset_mode)) return rc;
  if (const int rc = rec_check_periods(__func__, N, {sd_period, beta_period, vth_period, rho_period, kappa_period})) return rc;
  BE_REQUIRE(scale_exp >= kRecMinExp && scale_exp <= kRecMaxExp, BE_ERR_INVALID,
             "scale_exp outside the exponents be_fixed_point_exponent returns (-90 .. 150)");
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  BE_REQUIRE(syn_decay && beta && v_th, BE_ERR_INVALID, "null pointer (syn_decay, beta and v_th are required)");
  BE_REQUIRE(!adapt || (rho && kappa), BE_ERR_INVALID, "null pointer (adaptive: rho and kappa are required)");
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || a_save, BE_ERR_INVALID, "null pointer (adaptive: a_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., 1.);
  if (!adapt) a0 = nullptr, a_save = nullptr, a_last = nullptr, rho = nullptr, kappa = nullptr;   // neither read nor written
  const RecParams q{{syn_decay, sd_period}, {beta, beta_period}, {v_th, vth_period}, {rho, rho_period}, {kappa, kappa_period}};
  const hipError_t allowed = rec_launch_forward(true, x, w, indices, indptr, s0, c0, v0, a0, q, s_out, v_seq, h_save, a_save, c_save, c_last, v_last,
                            a_last, T, B, N, p, reset_mode == BE_LIF_RESET_HARD, adapt, scale_exp, stream);
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_sg_backward_params(const float* h_save, const float* c_save, const float* a_save, const float* c0, const float* v0,
                                  const float* w, const int32_t* indices, const int32_t* indptr, const float* g_s,
                                  const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                                  const float* syn_decay, int64_t sd_period, const float* beta, int64_t beta_period,
                                  const float* v_th, int64_t vth_period, const float* rho, int64_t rho_period, const float* kappa,
                                  int64_t kappa_period, float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0,
                                  float* g_sd_slot, float* g_beta_slot, float* g_vth_slot, float* g_rho_slot, float* g_kappa_slot,
                                  int64_t T, int64_t B, int64_t N, double v_reset, int reset_mode, int surrogate, double alpha,
                                  int adaptive, int detach_reset, be_stream_t stream) {
  const bool adapt = adaptive != 0;
  if (!adapt) rho_period = 1, kappa_period = 1;                            // the adaptation's arguments are not looked at
  if (const int rc = rec_check_common(__func__, T, B, N, reset_mode)) return rc;
  if (const int rc = rec_check_periods(__func__, N, {sd_period, beta_period, vth_period, rho_period, kappa_period})) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  BE_REQUIRE(syn_decay && beta && v_th, BE_ERR_INVALID, "null pointer (syn_decay, beta and v_th are required)");
  BE_REQUIRE(!adapt || (rho && kappa), BE_ERR_INVALID, "null pointer (adaptive: rho and kappa are required)");
  BE_REQUIRE(!adapt || a_save, BE_ERR_INVALID, "null pointer (adaptive: a_save is required)");
  BE_REQUIRE(!g_sd_slot || c_save, BE_ERR_INVALID, "null pointer (c_save is required where g_sd_slot is given)");
  const lane::LifP p = lane::make_params(0., 0., 0., v_reset, 0., 0., alpha);
  if (!adapt)                                                              // neither read nor written, whatever was passed
    a_save = nullptr, g_alast = nullptr, g_a0 = nullptr, rho = nullptr, kappa = nullptr, g_rho_slot = nullptr, g_kappa_slot = nullptr;
  const RecParams q{{syn_decay, sd_period}, {beta, beta_period}, {v_th, vth_period}, {rho, rho_period}, {kappa, kappa_period}};
  const hipError_t allowed = rec_launch_backward(true, h_save, a_save, c_save, c0, v0, w, indices, indptr, g_s, g_vseq, g_clast, g_vlast, g_alast, q, g_x,
                             g_c0, g_v0, g_a0, g_s0, g_sd_slot, g_beta_slot, g_vth_slot, g_rho_slot, g_kappa_slot, T, B, N, p,
                             reset_mode == BE_LIF_RESET_HARD, adapt, surrogate, (int)(detach_reset != 0), stream);
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
