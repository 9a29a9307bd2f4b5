// be_neuron_sg_rec_delay.hip — the recurrent spiking layer with SYNAPTIC DELAYS: §2.22's layer
// (be_neuron_sg_rec.hip) whose recurrent matrix is the stacked matrix of a delay split (be_delay.hip, §2.15): stacked row d * N + i
// holds the synapses of neuron i whose conduction delay is d steps.  Step t's input is
//     x[t] + sum over the delays d < depth of sp(t - 1 - d) @ W_d,      sp(tau) = the layer's own spikes, or s_hist before step 0,
// so a sample's last `depth` spike vectors stay on the chip: one workgroup owns one sample for the whole launch, as there.
//
// Forwards (k_lif_rec_delay_forward), per step: the history is a ring of bit-packed spike vectors in LDS, hist[depth][ceil(N / 64)]
// 64-bit words (the ballot of one wave over one of its neuron slots IS one word: neurons 64 q .. 64 q + 63).  A thread takes a
// contiguous chunk of the depth * ceil(N / 64) (age, word) pairs, ANDs each with row_mask[age] (the non-empty stacked rows) and
// counts bits; one block prefix sum (a wave scan, then the waves' totals) gives every thread the position of its first active
// stacked row in the step's list.  The active stacked rows regularly outnumber N (and the LDS left for the list), so the list is
// filled and walked in ROUNDS: round r holds the positions [r * cap, (r + 1) * cap) of that one prefix sum; a thread skips its
// chunk when it lies outside the window.  The walk is §2.22's with kDelRowLanes lanes per row — stacked rows are short: a row of
// 50 entries split over 16 delays leaves about 3 — into the same 64-bit fixed-point sums in LDS (integer atomics: order
// independent, so the pass is a function of its inputs bit for bit), and the step is be_sg_lane.h's, unchanged.  After the step
// the ballot of every neuron slot goes into the ring slot of the oldest age, which the step no longer needs.
//
// Backwards (k_lif_rec_delay_backward), per step t = T-1 .. 0: g_x[t + 1 .. t + depth] of the sample does not fit LDS in general
// (depth * N floats), so the gathers read the sample's own g_x rows back from global memory — stored by this workgroup at
// earlier iterations and ordered before the reads by the __syncthreads() that ends every iteration; g_x is therefore a required
// output and is not `__restrict__`.  THE ORDER OF THE f32 SUMS, fixed by the row lengths and T alone:
//     for neuron i, g_rec starts at +0; for d = 0, 1, ... ascending while t + 1 + d <= T - 1:
//         row sum of stacked row d * N + i: lane j of the row's kDelRowLanes lanes adds the rounded products w[k] * G[col k] of the
//         entries j, j + kDelRowLanes, ... in order, starting from +0; then the two partial sums are added (a butterfly, xor 1);
//         g_rec = g_rec + row sum          (an empty or masked row adds +0)
// and g_s_hist[a][b][i] is the same with d = a, a + 1, ... while d - a <= T - 1, reading g_x[d - a].  Then §2.21's backward step.
// Everything is f32, every operation rounded on its own (no FMA contraction).  Global traffic is plain vector loads and stores;
// no global atomics, no float atomics, nothing shared between workgroups.
#include "be_sg_lane.h"

namespace {

namespace lane = be_sg_lane;

constexpr int kDelThreads = 1024;
constexpr int kDelMaxN = 8192;
constexpr int kDelMaxDepth = 256;
constexpr int kDelPerThread = kDelMaxN / kDelThreads;
// lanes per stacked row, forwards and backwards: 2 lanes x kDelUnroll entries take a row of up to 8 entries in one trip (stacked
// rows are short; measured against 1, 4, 8 and 16 lanes: DESIGN.md §2.26)
constexpr int kDelRowLanes = 2;
constexpr int kDelUnroll = 4;
constexpr int kDelWaves = kDelThreads / kWave;
constexpr int kDelRowGroups = kDelThreads / kDelRowLanes;
// the dynamic LDS one workgroup may take (the CU's 160 KB less the static arrays and a margin), and the smallest id list a
// round may have.  THE LIMIT RULE: 8 * N + 8 * depth * ceil(N / 64) + 4 * kDelMinIds <= kDelLdsBytes  (sums, history, id list)
constexpr int kDelLdsBytes = 160 * 1024 - 1024;
constexpr int kDelMinIds = 4096;
// the exponents be_fixed_point_exponent returns (2^(e - 32) must be a normal f32)
constexpr int kDelMinExp = -90, kDelMaxExp = 150;

struct RowSpan {
  int begin, end;
};

__device__ __forceinline__ RowSpan row_span(const int32_t* __restrict__ indptr, uint32_t row) {
  return RowSpan{indptr[row], indptr[row + 1]};
}

inline int64_t del_fixed_lds(int64_t N, int64_t depth) { return 8 * N + 8 * depth * ((N + 63) / 64); }

// the (age d, word q) pair's active stacked rows: the ring slot of age d, gated by row_mask[d] (int32 [depth, ceil(N / 32)])
__device__ __forceinline__ unsigned long long del_pair_word(const unsigned long long* hist, const uint32_t* __restrict__ row_mask,
                                                            int W64, int W32, int depth, int head, int d, int q) {
  int slot = head - 1 - d;
  if (slot < 0) slot += depth;
  unsigned long long word = hist[slot * W64 + q];
  if (row_mask != nullptr && word != 0ull) {
    const uint32_t* m = row_mask + (int64_t)d * W32 + 2 * q;
    const unsigned long long lo = m[0], hi = 2 * q + 1 < W32 ? m[1] : 0u;
    word &= lo | (hi << 32);
  }
  return word;
}

// Forward.  x, s_out, v_seq, h_save, th_save are [T, B, N]; s_hist [hist_ages, B, N]; c0, v0, a0 and the *_last [B, N].  row_mask
// NULL keeps every stacked row; c0 / v0 / a0 NULL = 0; v_seq / h_save / th_save may be NULL.  Dynamic LDS: N 64-bit sums, the
// history ring depth * ceil(N / 64) 64-bit words, then ids_cap ids.
template <bool HARD, bool ADAPT>
__global__ void __launch_bounds__(kDelThreads)
k_lif_rec_delay_forward(const float* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ indices,
                        const int32_t* __restrict__ indptr, const uint32_t* __restrict__ row_mask, const float* __restrict__ s_hist,
                        const float* __restrict__ c0, const float* __restrict__ v0, const float* __restrict__ a0,
                        float* __restrict__ s_out, float* __restrict__ v_seq, float* __restrict__ h_save, float* __restrict__ th_save,
                        float* __restrict__ c_last, float* __restrict__ v_last, float* __restrict__ a_last, int64_t T, int64_t B, int N,
                        int depth, int hist_ages, uint32_t ids_cap, float scale, double inv, lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int W64 = (N + 63) / 64, W32 = (N + 31) / 32;
  const int pairs = depth * W64;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_raw);
  unsigned long long* hist = acc + N;
  uint32_t* ids = reinterpret_cast<uint32_t*>(hist + pairs);
  __shared__ uint32_t wave_tot[kDelWaves];
  const int tid = threadIdx.x, ln = tid & (kWave - 1), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * N;          // this sample's row of a [B, N] array
  const int64_t step = B * (int64_t)N;                   // one time step of a [T, B, N] array
  float c[kDelPerThread], v[kDelPerThread], a[kDelPerThread];
#pragma unroll
  for (int k = 0; k < kDelPerThread; ++k) {
    const int i = tid + k * kDelThreads;
    c[k] = v[k] = a[k] = 0.f;
    if (i < N) {
      if (c0 != nullptr) c[k] = c0[base + i];
      if (v0 != nullptr) v[k] = v0[base + i];
      if (ADAPT && a0 != nullptr) a[k] = a0[base + i];
      acc[i] = 0ull;
    }
  }
  // the ring: slot tau mod depth holds the spikes of step tau; step 0 writes slot 0, so age a of the history is slot depth - 1 - a
  for (int q = tid; q < pairs; q += kDelThreads) hist[q] = 0ull;
  __syncthreads();
  for (int age = 0; age < hist_ages; ++age) {
    const float* sh = s_hist + (int64_t)age * step + base;
#pragma unroll
    for (int k = 0; k < kDelPerThread; ++k) {
      if (k * kDelThreads < N) {
        const int i = tid + k * kDelThreads;
        const unsigned long long m = __ballot(i < N && sh[i] != 0.f);
        if (ln == 0 && i < N) hist[(depth - 1 - age) * W64 + k * kDelWaves + wave] = m;
      }
    }
  }
  __syncthreads();
  // this thread's chunk of the (age, word) pairs: [p0, p1), age-major
  const int per = (pairs + kDelThreads - 1) / kDelThreads;
  const int p0 = min(tid * per, pairs), p1 = min(p0 + per, pairs);
  const int d0 = p0 / W64, q0 = p0 - d0 * W64;
  int head = 0;                                          // the ring slot step t writes
  for (int64_t t = 0; t < T; ++t) {
    const int64_t at = t * step + base;
    float xv[kDelPerThread];                             // does not depend on the chain: in flight during the scatter
#pragma unroll
    for (int k = 0; k < kDelPerThread; ++k) {
      const int i = tid + k * kDelThreads;
      xv[k] = 0.f;
      if (i < N) xv[k] = x[at + i];
    }
    // the active stacked rows of this thread's pairs, and its place in the block's prefix sum
    uint32_t cnt = 0;
    for (int pr = p0, d = d0, q = q0; pr < p1; ++pr) {
      cnt += (uint32_t)__popcll(del_pair_word(hist, row_mask, W64, W32, depth, head, d, q));
      if (++q == W64) q = 0, ++d;
    }
    uint32_t inc = cnt;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t below = __shfl_up(inc, off, kWave);
      if (ln >= off) inc += below;
    }
    if (ln == kWave - 1) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t pos = inc - cnt, n_active = 0;
#pragma unroll
    for (int q = 0; q < kDelWaves; ++q) {
      const uint32_t n = wave_tot[q];
      if (q < wave) pos += n;
      n_active += n;
    }
    // rounds: the list positions [first, first + ids_cap) -> ids[] (unordered sums: the order inside the list does not matter)
    for (uint32_t first = 0;; first += ids_cap) {
      if (cnt != 0 && pos < first + ids_cap && pos + cnt > first) {
        uint32_t to = pos;
        for (int pr = p0, d = d0, q = q0; pr < p1; ++pr) {
          unsigned long long word = del_pair_word(hist, row_mask, W64, W32, depth, head, d, q);
          while (word != 0ull) {
            const int bit = __builtin_ctzll(word);
            word &= word - 1ull;
            if (to - first < ids_cap) ids[to - first] = (uint32_t)(d * N + q * 64 + bit);   // (to < first wraps past ids_cap)
            ++to;
          }
          if (++q == W64) q = 0, ++d;
        }
      }
      __syncthreads();
      // the listed stacked rows, kDelRowLanes lanes per row: R[col] += fixed(w)
      // (the next row's bounds and a lane's next kDelUnroll entries are loaded before anything waits for them: the walk is bound
      // by the latency of dependent loads, id -> indptr -> entry, not by bytes)
      const uint32_t n_round = min(ids_cap, n_active - first);
      uint32_t r = tid / kDelRowLanes;
      RowSpan cur = r < n_round ? row_span(indptr, ids[r]) : RowSpan{0, 0};
      while (r < n_round) {
        const uint32_t rn = r + kDelRowGroups;
        const RowSpan next = rn < n_round ? row_span(indptr, ids[rn]) : RowSpan{0, 0};
        for (int k = cur.begin + (tid % kDelRowLanes); k < cur.end; k += kDelUnroll * kDelRowLanes) {
          int col[kDelUnroll];
          float wk[kDelUnroll];
#pragma unroll
          for (int q = 0; q < kDelUnroll; ++q) {
            const bool in = k + q * kDelRowLanes < cur.end;
            col[q] = in ? indices[k + q * kDelRowLanes] : -1;
            wk[q] = in ? w[k + q * kDelRowLanes] : 0.f;
          }
#pragma unroll
          for (int q = 0; q < kDelUnroll; ++q)
            if (col[q] >= 0) atomicAdd(&acc[col[q]], fixed_from_f32(wk[q], scale));
        }
        r = rn;
        cur = next;
      }
      __syncthreads();
      if (first + ids_cap >= n_active) break;            // (block-uniform: n_active is)
    }
#pragma unroll
    for (int k = 0; k < kDelPerThread; ++k) {
      if (k * kDelThreads < N) {
        const int i = tid + k * kDelThreads;
        bool fired = false;
        if (i < N) {
          const unsigned long long R = acc[i];
          acc[i] = 0ull;                                 // read and cleared by its owner only: no barrier in between
          const float r = (float)((double)(long long)R * inv);
          const lane::Fired f = lane::forward_step<HARD, true, ADAPT>(xv[k] + r, c[k], v[k], a[k], p.beta, p.v_th, p);
          fired = f.s;
          s_out[at + i] = f.s ? 1.0f : 0.0f;
          if (v_seq != nullptr) v_seq[at + i] = v[k];
          if (h_save != nullptr) {
            h_save[at + i] = f.h;
            if (ADAPT) th_save[at + i] = f.th;
          }
        }
        // the wave's 64 neurons of this slot are one word of the ring (every reader of the slot's old content is past the barrier)
        const unsigned long long m = __ballot(fired);
        if (ln == 0 && k * kDelThreads + wave * kWave < N) hist[head * W64 + k * kDelWaves + wave] = m;
      }
    }
    head = head + 1 == depth ? 0 : head + 1;
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kDelPerThread; ++k) {
    const int i = tid + k * kDelThreads;
    if (i < N) {
      c_last[base + i] = c[k];
      v_last[base + i] = v[k];
      if (ADAPT) a_last[base + i] = a[k];
    }
  }
}

// the bounds of stacked row d * N + i, or an empty span where row_mask says the row is empty
__device__ __forceinline__ RowSpan del_row(const int32_t* __restrict__ indptr, const uint32_t* __restrict__ row_mask, int W32, int N,
                                           int d, int i) {
  if (row_mask != nullptr && ((row_mask[(int64_t)d * W32 + (i >> 5)] >> (i & 31)) & 1u) == 0u) return RowSpan{0, 0};
  return row_span(indptr, (uint32_t)(d * N + i));
}

// out[i] = sum over d = d_lo .. d_hi (ascending, from +0) of the row sum of stacked row d * N + i against gx[(t + 1 + d) * step + .]
// (gx: the sample's column of g_x; the order of the sums is the one the top of the file states).  d_lo = max(0, -1 - t),
// d_hi = min(depth - 1, T - 2 - t): the steps 0 .. T-1 that exist.  t = -1 - a gives g_s_hist[a].
__device__ __forceinline__ void del_gather(const float* __restrict__ w, const int32_t* __restrict__ indices,
                                           const int32_t* __restrict__ indptr, const uint32_t* __restrict__ row_mask, const float* gx,
                                           int64_t step, int64_t t, int64_t T, int N, int depth, float* out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, sub = tid % kDelRowLanes;
  const int W32 = (N + 31) / 32;
  const int d_lo = t >= 0 ? 0 : (int)(-1 - t);
  const int d_hi = (int)(T - 2 - t < (int64_t)depth - 1 ? T - 2 - t : (int64_t)depth - 1);
  for (int i = tid / kDelRowLanes; i < N; i += kDelRowGroups) {
    float total = 0.f;
    RowSpan cur = d_lo <= d_hi ? del_row(indptr, row_mask, W32, N, d_lo, i) : RowSpan{0, 0};
    for (int d = d_lo; d <= d_hi; ++d) {
      const RowSpan next = d < d_hi ? del_row(indptr, row_mask, W32, N, d + 1, i) : RowSpan{0, 0};
      const float* G = gx + (t + 1 + d) * step;
      float sum = 0.f;
      for (int k = cur.begin + sub; k < cur.end; k += kDelUnroll * kDelRowLanes) {
        int col[kDelUnroll];
        float wk[kDelUnroll];
#pragma unroll
        for (int q = 0; q < kDelUnroll; ++q) {               // in flight together; added below in the order of k
          const bool in = k + q * kDelRowLanes < cur.end;
          col[q] = in ? indices[k + q * kDelRowLanes] : -1;
          wk[q] = in ? w[k + q * kDelRowLanes] : 0.f;
        }
        float gv[kDelUnroll];
#pragma unroll
        for (int q = 0; q < kDelUnroll; ++q) gv[q] = G[col[q] >= 0 ? col[q] : 0];
#pragma unroll
        for (int q = 0; q < kDelUnroll; ++q) {
          const float term = wk[q] * gv[q];
          sum = col[q] >= 0 ? sum + term : sum;
        }
      }
#pragma unroll
      for (int off = kDelRowLanes / 2; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, kDelRowLanes);
      total = total + sum;
      cur = next;
    }
    if (sub == 0) out[i] = total;
  }
}

// Backward.  h_save, th_save, g_s, g_vseq, g_x are [T, B, N]; g_s_hist [hist_ages, B, N]; the others [B, N].  g_s / g_vseq / g_clast
// / g_vlast / g_alast NULL = 0; g_c0 / g_v0 / g_a0 / g_s_hist may be NULL.  g_x is written AND read back (the gathers of later
// iterations): no __restrict__.  Dynamic LDS: g_rec (N floats).
template <bool HARD, int SG, bool ADAPT>
__global__ void __launch_bounds__(kDelThreads)
k_lif_rec_delay_backward(const float* __restrict__ h_save, const float* __restrict__ th_save, const float* __restrict__ w,
                         const int32_t* __restrict__ indices, const int32_t* __restrict__ indptr,
                         const uint32_t* __restrict__ row_mask, const float* __restrict__ g_s, const float* __restrict__ g_vseq,
                         const float* __restrict__ g_clast, const float* __restrict__ g_vlast, const float* __restrict__ g_alast,
                         float* g_x, float* __restrict__ g_c0, float* __restrict__ g_v0, float* __restrict__ g_a0,
                         float* __restrict__ g_s_hist, int64_t T, int64_t B, int N, int depth, int hist_ages, int detach_reset,
                         lane::LifP p) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* grec = reinterpret_cast<float*>(smem_raw);
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * N;
  const int64_t step = B * (int64_t)N;
  float cc[kDelPerThread], cv[kDelPerThread], ca[kDelPerThread];
#pragma unroll
  for (int k = 0; k < kDelPerThread; ++k) {
    const int i = tid + k * kDelThreads;
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
    float hv[kDelPerThread], tv[kDelPerThread], gsv[kDelPerThread], gvv[kDelPerThread];   // in flight during the gather
#pragma unroll
    for (int k = 0; k < kDelPerThread; ++k) {
      const int i = tid + k * kDelThreads;
      hv[k] = tv[k] = gsv[k] = gvv[k] = 0.f;
      if (i < N) {
        hv[k] = h_save[at + i];
        if (ADAPT) tv[k] = th_save[at + i];
        if (g_s != nullptr) gsv[k] = g_s[at + i];
        if (g_vseq != nullptr) gvv[k] = g_vseq[at + i];
      }
    }
    if (rec) {
      del_gather(w, indices, indptr, row_mask, g_x + base, step, t, T, N, depth, grec);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kDelPerThread; ++k) {
      const int i = tid + k * kDelThreads;
      if (i < N) {
        float g_vo = cv[k];
        if (g_vseq != nullptr) g_vo = g_vo + gvv[k];
        float g_sp = gsv[k];                             // 0 when g_s is NULL
        if (rec) g_sp = g_sp + grec[i];
        const float th = ADAPT ? tv[k] : p.v_th;         // the threshold h was compared with
        const lane::Grad d = lane::backward_step<HARD, SG, ADAPT>(hv[k], th, p.v_th, g_sp, g_vo, ca[k], detach_reset, p);
        const float g_c = lane::backward_carry<true, ADAPT>(d, cc[k], cv[k], ca[k], p.beta, p);
        g_x[at + i] = g_c;
      }
    }
    __syncthreads();                                     // g_x[t] is stored before any thread gathers from it; grec is free again
  }
#pragma unroll
  for (int k = 0; k < kDelPerThread; ++k) {
    const int i = tid + k * kDelThreads;
    if (i < N) {
      if (g_c0 != nullptr) g_c0[base + i] = cc[k];
      if (g_v0 != nullptr) g_v0[base + i] = cv[k];
      if (ADAPT && g_a0 != nullptr) g_a0[base + i] = ca[k];
    }
  }
  if (g_s_hist != nullptr)
    for (int age = 0; age < hist_ages; ++age)
      del_gather(w, indices, indptr, row_mask, g_x + base, step, -1 - (int64_t)age, T, N, depth, g_s_hist + (int64_t)age * step + base);
}

// the checks both entry points share (BE_REQUIRE would name this function, not the entry point)
inline int del_check_common(const char* who, int64_t T, int64_t B, int64_t N, int depth, int hist_ages, int reset_mode) {
  const char* msg = (T < 0 || B < 0 || N < 0) ? ": T < 0, B < 0 or N < 0"
                    : (reset_mode != BE_LIF_RESET_HARD && reset_mode != BE_LIF_RESET_SOFT) ? ": unknown reset_mode"
                    : (depth < 1 || depth > kDelMaxDepth) ? ": depth outside 1 .. 256"
                    : (hist_ages < 0 || hist_ages > depth) ? ": hist_ages outside 0 .. depth" : nullptr;
  if (msg != nullptr) {
    be_set_error(std::string(who) + msg);
    return BE_ERR_INVALID;
  }
  if (N > kDelMaxN || B > 0x7fffffffll || del_fixed_lds(N, depth) + 4 * kDelMinIds > kDelLdsBytes) {
    be_set_error(std::string(who) + ": N = " + std::to_string(N) + " neurons at depth " + std::to_string(depth) + " (limits: N <= " +
                 std::to_string(kDelMaxN) + " and 8 * N + 8 * depth * ceil(N / 64) + " + std::to_string(4 * kDelMinIds) + " <= " +
                 std::to_string(kDelLdsBytes) + ": one sample's sums, spike history and a list of active rows in one workgroup's " +
                 "LDS), B = " + std::to_string(B) + " (limit: 2^31 - 1)");
    return BE_ERR_RANGE;
  }
  return BE_OK;
}

// [T, B, N] spikes (and [hist_ages, B, N] before step 0) -> the activity of the stacked rows over the T * B batch rows (t, b):
// mask[(d * N + i) * nw + word] bit p % 32, p = t * B + b, = sp(t - 1 - d)[b][i] != 0.  Lanes run over i: the reads coalesce.
__global__ void __launch_bounds__(256) k_pack_aged(const float* __restrict__ s, const float* __restrict__ s_hist, int64_t N, int64_t B,
                                                   int64_t T, int depth, int hist_ages, int64_t nw, uint32_t* __restrict__ mask) {
  const int64_t total = (int64_t)depth * nw * N, nb = T * B;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e % N, dw = e / N, word = dw % nw, d = dw / nw;
    const int64_t p0 = word * 32, p1 = p0 + 32 < nb ? p0 + 32 : nb;
    uint32_t bits = 0;
    int64_t t = p0 / B, b = p0 - t * B;
    for (int64_t pp = p0; pp < p1; ++pp) {
      const int64_t tau = t - 1 - d;
      bool on = false;
      if (tau >= 0) on = s[(tau * B + b) * N + i] != 0.f;
      else if (-1 - tau < hist_ages) on = s_hist[((-1 - tau) * B + b) * N + i] != 0.f;
      bits |= (uint32_t)on << (pp - p0);
      if (++b == B) b = 0, ++t;
    }
    mask[(d * N + i) * nw + word] = bits;
  }
}

}  // namespace

extern "C" {

int be_lif_rec_delay_sg_forward(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const uint32_t* row_mask,
                                int depth, const float* s_hist, int hist_ages, const float* c0, const float* v0, const float* a0,
                                float* s_out, float* v_seq, float* h_save, float* th_save, float* c_last, float* v_last, float* a_last,
                                int64_t T, int64_t B, int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho,
                                double kappa, int reset_mode, int adaptive, int scale_exp, be_stream_t stream) {
  if (const int rc = del_check_common(__func__, T, B, N, depth, hist_ages, reset_mode)) return rc;
  BE_REQUIRE(scale_exp >= kDelMinExp && scale_exp <= kDelMaxExp, BE_ERR_INVALID,
             "scale_exp outside the exponents be_fixed_point_exponent returns (-90 .. 150)");
  BE_REQUIRE(hist_ages == 0 || s_hist, BE_ERR_INVALID, "null pointer (s_hist is required where hist_ages > 0)");
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(x && s_out && c_last && v_last, BE_ERR_INVALID, "null pointer (x, s_out, c_last and v_last are required)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || a_last, BE_ERR_INVALID, "null pointer (adaptive: a_last is required)");
  BE_REQUIRE(!adapt || !h_save || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required where h_save is given)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, 1.);
  if (!adapt) a0 = nullptr, th_save = nullptr, a_last = nullptr;          // neither read nor written, whatever was passed
  const float scale = ldexpf(1.0f, scale_exp - 32);   // see fixed_from_f32
  const double inv = ldexp(1.0, -scale_exp);
  // the id list: what the sums and the history leave, no more than the stacked rows there are
  const int64_t fixed = del_fixed_lds(N, depth);
  const int64_t room = (kDelLdsBytes - fixed) / 4, rows = (int64_t)depth * N;
  const uint32_t ids_cap = (uint32_t)(room < rows ? room : rows);
  const int lds = (int)be_align_up(fixed + 4 * (int64_t)ids_cap, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      auto kern = k_lif_rec_delay_forward<decltype(H)::value, decltype(A)::value>;
      allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
      if (allowed == hipSuccess)
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kDelThreads), lds, st, x, w, indices, indptr, row_mask, s_hist, c0, v0, a0,
                           s_out, v_seq, h_save, th_save, c_last, v_last, a_last, T, B, (int)N, depth, hist_ages, ids_cap, scale, inv, p);
      return BE_OK;
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_lif_rec_delay_sg_backward(const float* h_save, const float* th_save, const float* w, const int32_t* indices,
                                 const int32_t* indptr, const uint32_t* row_mask, int depth, const float* g_s, const float* g_vseq,
                                 const float* g_clast, const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0,
                                 float* g_a0, float* g_s_hist, int hist_ages, int64_t T, int64_t B, int64_t N, double syn_decay,
                                 double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode, int surrogate,
                                 double alpha, int adaptive, int detach_reset, be_stream_t stream) {
  if (const int rc = del_check_common(__func__, T, B, N, depth, hist_ages, reset_mode)) return rc;
  if (const int rc = lane::check_surrogate(__func__, surrogate, alpha)) return rc;
  if (T == 0 || B == 0 || N == 0) return BE_OK;
  BE_REQUIRE(h_save && g_x, BE_ERR_INVALID, "null pointer (h_save and g_x are required: the gathers read g_x back)");
  BE_REQUIRE(w && indices && indptr, BE_ERR_INVALID, "null pointer (w, indices and indptr are required)");
  const bool adapt = adaptive != 0;
  BE_REQUIRE(!adapt || th_save, BE_ERR_INVALID, "null pointer (adaptive: th_save is required)");
  const lane::LifP p = lane::make_params(syn_decay, beta, v_th, v_reset, rho, kappa, alpha);
  if (!adapt) th_save = nullptr, g_alast = nullptr, g_a0 = nullptr;       // neither read nor written, whatever was passed
  const int lds = (int)be_align_up(N * 4, 16);
  const int detach = (int)(detach_reset != 0);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t allowed = hipSuccess;
  be_dispatch_bool(reset_mode == BE_LIF_RESET_HARD, [&](auto H) {
    return be_dispatch_bool(adapt, [&](auto A) {
      return be_dispatch_int<BE_LIF_SG_FAST_SIGMOID, BE_LIF_SG_ATAN, BE_LIF_SG_TRIANGLE>(surrogate, [&](auto SG) {
        auto kern = k_lif_rec_delay_backward<decltype(H)::value, decltype(SG)::value, decltype(A)::value>;
        allowed = be_allow_lds(reinterpret_cast<const void*>(kern), lds);
        if (allowed == hipSuccess)
          hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kDelThreads), lds, st, h_save, th_save, w, indices, indptr, row_mask, g_s,
                             g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0, g_s_hist, T, B, (int)N, depth, hist_ages, detach,
                             p);
        return BE_OK;
      });
    });
  });
  BE_HIP(allowed);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int be_grad_pack_activity_aged(const float* s, const float* s_hist, int64_t N, int64_t B, int64_t T, int depth, int hist_ages,
                               uint32_t* mask, be_stream_t stream) {
  BE_REQUIRE(N >= 0 && N <= 0x7fffffffll && B >= 1 && T >= 1 && T * B <= 65535, BE_ERR_INVALID,
             "N / B / T out of range (T * B batch rows, at most 65535)");
  BE_REQUIRE(depth >= 1 && depth <= kDelMaxDepth && hist_ages >= 0 && hist_ages <= depth, BE_ERR_INVALID,
             "depth outside 1 .. 256 or hist_ages outside 0 .. depth");
  BE_REQUIRE(hist_ages == 0 || s_hist, BE_ERR_INVALID, "null pointer (s_hist is required where hist_ages > 0)");
  if (N == 0) return BE_OK;
  BE_REQUIRE(s && mask, BE_ERR_INVALID, "null pointer");
  const int64_t nw = (T * B + 31) / 32, words = (int64_t)depth * N * nw;
  const int64_t blocks = (words + 255) / 256;
  hipLaunchKernelGGL(k_pack_aged, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, static_cast<hipStream_t>(stream), s,
                     s_hist, N, B, T, depth, hist_ages, nw, mask);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
