// be_delay.hip — synaptic delays on the presynaptic side: the device-side split of a matrix's stored rows by
// delay, the bit-packed spike-history ring, and the compaction of the ring into the active-row list of the *stacked* matrix; and
// the push of the value-history ring that the plasticity of delayed synapses reads by age (be_plasticity.hip);
// and the batched ring: B histories under one head, and their age-ordered unroll into the bit-packed batch
// operand [B, depth * n] of the stacked matrix (a BE_SPIKE_BITS batch of the scatter entry points).
//
// Stored row d * m + i of the stacked matrix holds the entries of row i whose delay is d; a delayed step is then one ordinary
// scatter over the stacked rows {d * m + i : neuron i fired d steps ago} — a BE_SPIKE_IDS operand of the scatter entry points
// (be_csr*.hip), none of whose kernels this file touches.
//
// No float atomics here; the integer ones are the error word of the count pass, one reservation per workgroup in the
// compaction (as k_compact_bits, be_csr.hip) and one arrival ticket per workgroup in the push.
#include "be_pbits.h"

namespace {

constexpr int kMaxDepth = 256;
// split: a wave walks one stored row in order, 64 entries at a time; a workgroup is 4 such waves
constexpr int kSplitThreads = 256;
constexpr int kSplitTile = kSplitThreads;          // entries a workgroup takes per step of its waves
constexpr int kSplitGridCap = 4096;
constexpr int kMaskGridCap = 64;                   // row-mask kernel: 256 rows per workgroup and plane, as many rows per pass
// ring: one workgroup packs (push) or scans (compaction) kRingTileBits bits of one slot
constexpr int kRingThreads = 256, kRingPer = 32;
constexpr int kRingTileBits = kRingThreads * kRingPer;
static_assert(kRingTileBits == kRingThreads * 32, "the compaction gives every thread one 32-bit word of the push tile");
// batched ring: the batch row is the grid's second dimension, in the push and in the unroll (no stride over it), so the batch
// count is bounded by that dimension's limit — the n_batch bound of every batched entry point of the library
constexpr int kRingMaxBatch = 65535;
// unroll: one thread assembles one output word; a workgroup takes kUnrollThreads consecutive words of one batch row
constexpr int kUnrollThreads = 256;

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_wave_barrier(); }

// =================================================================================================
// delay split
// =================================================================================================
// COUNT: counts[1 + d * m + r] = entries of row r with delay d (counts[0] = 0: the inclusive scan of `counts` is indptr_s);
//        the smallest position holding a delay outside [0, depth) goes to *err.  Such an entry is skipped, here and in FILL.
// FILL : perm[indptr_s[d * m + r] + (rank of entry j among the earlier entries of row r with delay d)] = j, and the same slot
//        of indices_s takes indices[j].
// Both walk the row in order.  hist[d] (LDS, one table per wave) counts the entries of delay d in the chunks already passed.
// Inside a chunk the lanes with equal delay find each other by ballots over the bits of the delay (match-any), and the rank is
// the population count below the lane: stable, no global atomic places anything.  The LDS table is touched by its own wave
// only; LDS operations of one wave execute in order, wave_fence() keeps the compiler from reordering them.
template <bool FILL, typename PT>
__global__ void __launch_bounds__(kSplitThreads) k_delay_split(RowPtr rp, const int32_t* __restrict__ delays,
                                                               const int32_t* __restrict__ indices, int64_t m, int depth,
                                                               int nbits, PT* __restrict__ counts,
                                                               const PT* __restrict__ indptr_s, PT* __restrict__ perm,
                                                               int32_t* __restrict__ indices_s, unsigned long long* err) {
  __shared__ uint32_t hist_all[kSplitThreads / 64][kMaxDepth];
  volatile uint32_t* hist = hist_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * kSplitThreads + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kSplitThreads) >> 6;
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) counts[0] = PT(0);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t r = wave; r < m; r += n_waves) {
    for (int d = lane; d < depth; d += 64) hist[d] = 0u;
    wave_fence();
    const int64_t b = rp.at(r), e = rp.at(r + 1);
    for (int64_t j0 = b; j0 < e; j0 += 64) {
      const int64_t j = j0 + lane;
      const int d = (j < e) ? delays[j] : -1;
      const bool valid = (j < e) && (unsigned)d < (unsigned)depth;
      if (!FILL && (j < e) && !valid) atomicMin(err, (unsigned long long)j);
      unsigned long long same = __ballot(valid);
      for (int bit = 0; bit < nbits; ++bit) {
        const bool s = valid && ((d >> bit) & 1);
        const unsigned long long bal = __ballot(s);
        same &= s ? bal : ~bal;
      }
      const uint32_t rank = (uint32_t)__popcll(same & below);
      uint32_t base = 0;
      if (valid) base = hist[d];
      wave_fence();
      if (valid && rank == 0) hist[d] = base + (uint32_t)__popcll(same);
      wave_fence();
      if (FILL && valid) {
        const int64_t pos = (int64_t)indptr_s[(int64_t)d * m + r] + base + rank;
        perm[pos] = (PT)j;
        if (indices_s != nullptr) indices_s[pos] = indices[j];
      }
    }
    if (!FILL) {
      wave_fence();
      for (int d = lane; d < depth; d += 64) counts[1 + (int64_t)d * m + r] = (PT)hist[d];
    }
    wave_fence();
  }
}

// row_mask[d][i / 32] bit i % 32 = stacked row d * m + i is non-empty
template <typename PT>
__global__ void __launch_bounds__(256) k_delay_row_mask(const PT* __restrict__ indptr_s, int64_t m, int64_t n_words,
                                                        uint32_t* __restrict__ row_mask) {
  const int64_t d = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t m_round = (m + 63) & ~(int64_t)63;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m_round; i += stride) {
    const bool full = (i < m) && indptr_s[d * m + i + 1] > indptr_s[d * m + i];
    const unsigned long long mask = __ballot(full);
    const int lane = lane_id();
    if (lane == 0) row_mask[d * n_words + (i >> 5)] = (uint32_t)mask;
    if (lane == 32 && i < m) row_mask[d * n_words + (i >> 5)] = (uint32_t)(mask >> 32);
  }
}

// =================================================================================================
// spike-history ring: bits[depth][ceil(n/32)], head[1]
// =================================================================================================
__device__ __forceinline__ int ring_head(const int32_t* head, int depth) {
  const int h = *head;
  return ((unsigned)h < (unsigned)depth) ? h : 0;
}

struct SpikeWords { using type = uint32_t; };

// Packs the spikes into slot `head`, then advances head.  Every workgroup reads head (thread 0, broadcast through LDS) before
// it takes its arrival ticket, and the holder of the last ticket is the one that writes head and re-arms the ticket word: no
// workgroup reads head after it was written in this launch; later launches are ordered behind this one by the stream.
// The grid is (bit tiles, batch rows): workgroup (x, b) packs tile x of spikes[b] into row b of the slot, bits[head][b][.]; the
// rule holds over the whole grid, the last of gridDim.x * gridDim.y tickets advances head.  One vector is gridDim.y == 1.
template <typename SP>
__global__ void __launch_bounds__(kRingThreads) k_ring_push(const typename SP::type* __restrict__ spikes, int64_t n, int depth,
                                                            uint32_t* __restrict__ bits, int32_t* head, uint32_t* arrivals) {
  __shared__ int h_sh;
  if (threadIdx.x == 0) h_sh = ring_head(head, depth);
  __syncthreads();
  const int h = h_sh;
  const int64_t n_words = (n + 31) >> 5;
  const int64_t b = blockIdx.y;
  uint32_t* __restrict__ row = bits + ((int64_t)h * gridDim.y + b) * n_words;
  spikes += b * (std::is_same<SP, SpikeWords>::value ? n_words : n);
  const int64_t tile = (int64_t)blockIdx.x * kRingTileBits;
  if constexpr (std::is_same<SP, SpikeWords>::value) {
    const int64_t w = (tile >> 5) + threadIdx.x;
    if (w < n_words) {
      uint32_t v = spikes[w];
      const int64_t left = n - w * 32;
      if (left < 32) v &= (1u << left) - 1u;
      row[w] = v;
    }
  } else {
    const int lane = lane_id();
#pragma unroll 8
    for (int u = 0; u < kRingPer; ++u) {
      const int64_t i = tile + (int64_t)u * kRingThreads + threadIdx.x;
      const bool a = (i < n) && SP::active(spikes[i]);
      const unsigned long long mask = __ballot(a);
      if (lane == 0 && i < n) row[i >> 5] = (uint32_t)mask;
      if (lane == 32 && i < n) row[i >> 5] = (uint32_t)(mask >> 32);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = atomicAdd(arrivals, 1u);
    if (t == gridDim.x * gridDim.y - 1) {
      *arrivals = 0u;
      *head = (h + 1 == depth) ? 0 : h + 1;
    }
  }
}

// ages [0, gridDim.y) of the ring -> unordered list of a * n + i for every set bit i of the slot of age a, gated word for word by
// row_mask[a] (NULL: keep all).  The reservation is k_compact_bits' (be_csr.hip): one integer atomic per workgroup.
__global__ void __launch_bounds__(kRingThreads) k_ring_compact(const uint32_t* __restrict__ bits, const int32_t* __restrict__ head,
                                                               int64_t n, int64_t n_words, int depth,
                                                               const uint32_t* __restrict__ row_mask,
                                                               uint32_t* __restrict__ active, uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_tot[kRingThreads / 64];
  __shared__ uint32_t block_base;
  const int a = blockIdx.y;
  const int slot = (ring_head(head, depth) + depth - 1 - a) % depth;
  const int64_t w = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  uint32_t bw = 0;
  if (w < n_words) {
    bw = bits[(int64_t)slot * n_words + w];
    if (row_mask != nullptr) bw &= row_mask[(int64_t)a * n_words + w];
    const int64_t left = n - w * 32;
    if (left < 32) bw &= (1u << left) - 1u;
  }
  const uint32_t cnt = __popc(bw);
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t wave_off = 0, total = 0;
#pragma unroll
  for (int v = 0; v < kRingThreads / 64; ++v) {
    if (v < wave) wave_off += wave_tot[v];
    total += wave_tot[v];
  }
  if (threadIdx.x == 0) block_base = total ? atomicAdd(count, total) : 0u;
  __syncthreads();
  uint32_t pos = block_base + wave_off + incl - cnt;
  const uint32_t id0 = (uint32_t)((int64_t)a * n + w * 32);
  while (bw) {
    const int b = __ffs(bw) - 1;
    bw &= bw - 1;
    active[pos++] = id0 + (uint32_t)b;
  }
}

// The batched ring by age: out[b][.] is the bit string of ages * n bits whose bit p = a * n + i is bit i of the slot of age a of
// sample b — slot (head - 1 - a) mod depth, bits[slot][b][.] — ANDed with bit i of row_mask[a] (NULL: keep all); the bits from
// ages * n to the end of the row's last word are 0.  n is in general no multiple of 32, so age a starts at bit offset a * n of
// the row: a funnel shift, not a copy.  One thread assembles one output word, from pieces: a piece is the run of bits that
// comes from ONE source word of ONE age — it ends where the output word, the age (at bit n) or the source word (at a multiple
// of 32) ends.  For n >= 32 an output word spans at most two ages and at most two source words of each (at most four pieces,
// three unless an age boundary falls inside it); for n < 32 every age is one piece and the word draws on up to 32 ages (n = 1:
// exactly 32).  Every shift count is at most 31: `sh` is a bit position inside a source word, `filled` the number of bits
// already placed, which is below 32 while the loop runs, and a piece of all 32 bits (n % 32 == 0, word-aligned ages) is taken
// whole, without a mask.  The position arithmetic is one 32-bit unsigned divide per word (p < 2^31 + 32).  Lanes of a wave read
// consecutive source words (each word is read by at most two neighbouring lanes) and write consecutive output words; every
// output word is written once, by one lane: no atomics, nothing to zero beforehand.  head is read once per workgroup.
__global__ void __launch_bounds__(kUnrollThreads) k_ring_unroll(const uint32_t* __restrict__ bits, const int32_t* __restrict__ head,
                                                                 uint32_t n, int64_t n_words, int depth, uint32_t total,
                                                                 int64_t out_words, const uint32_t* __restrict__ row_mask,
                                                                 uint32_t* __restrict__ out) {
  __shared__ int h_sh;
  if (threadIdx.x == 0) h_sh = ring_head(head, depth);
  __syncthreads();
  const int64_t w = (int64_t)blockIdx.x * kUnrollThreads + threadIdx.x;
  if (w >= out_words) return;
  const int64_t b = blockIdx.y, n_batch = gridDim.y;
  uint32_t p = (uint32_t)w << 5;
  const uint32_t end = (total - p < 32u) ? total : p + 32u;
  uint32_t a = p / n, i = p - a * n;
  int slot = h_sh - 1 - (int)a;                       // a < ages <= depth, 0 <= head < depth: one conditional add is the modulo
  if (slot < 0) slot += depth;
  uint32_t word = 0, filled = 0;
  while (p < end) {
    const uint32_t sh = i & 31u;
    uint32_t take = end - p;
    if (n - i < take) take = n - i;
    if (32u - sh < take) take = 32u - sh;
    uint32_t src = bits[((int64_t)slot * n_batch + b) * n_words + (i >> 5)];
    if (row_mask != nullptr) src &= row_mask[(int64_t)a * n_words + (i >> 5)];
    uint32_t v = src >> sh;
    if (take < 32u) v &= (1u << take) - 1u;
    word |= v << filled;
    filled += take;
    p += take;
    i += take;
    if (i == n) {
      i = 0;
      ++a;
      slot = (slot == 0) ? depth - 1 : slot - 1;
    }
  }
  out[b * out_words + w] = word;
}

// =================================================================================================
// value-history ring: values[depth][n] in one of the four float dtypes, head[1]
// =================================================================================================
// one workgroup converts and copies kValueTile elements of the pushed vector; a lane moves 16 bytes of the ring's dtype at a time
constexpr int kValueThreads = 256, kValuePer = 16;
constexpr int kValueTile = kValueThreads * kValuePer;

template <typename T, int E>
struct alignas(sizeof(T) * E < 16 ? sizeof(T) * E : 16) ValuePack {
  T v[E];
};

// S -> D as torch's .to(): through the accumulation type of the narrower side (f64 -> f16 / bf16 rounds through f32); the same
// dtype is a copy of the bits
template <typename S, typename D>
__device__ __forceinline__ typename PB<D>::bits value_convert(typename PB<S>::bits b) {
  if constexpr (std::is_same<S, D>::value) return b;
  else return PB<D>::put((typename PB<D>::acc)PB<S>::get(b));
}

// Writes x[n], converted to the ring's dtype, into slot `head`, then advances head: k_ring_push's protocol (every workgroup
// reads head before it takes its ticket; the last ticket writes head and re-arms the ticket word).  A lane takes E = 16 bytes'
// worth of ring elements per step; where the slot and x are 16-byte aligned — the slot's address depends on head, so this is
// decided here — full groups of E move as one vector load (or 16-byte pieces of it) and one 16-byte store, the rest one by one.
template <typename S, typename D>
__global__ void __launch_bounds__(kValueThreads) k_value_ring_push(const typename PB<S>::bits* __restrict__ x, int64_t n, int depth,
                                                                   typename PB<D>::bits* __restrict__ values, int32_t* head,
                                                                   uint32_t* arrivals) {
  using SB = typename PB<S>::bits;
  using DB = typename PB<D>::bits;
  constexpr int E = 16 / (int)sizeof(DB);
  static_assert(kValuePer % E == 0, "a lane's share of the tile is a whole number of 16-byte groups");
  __shared__ int h_sh;
  if (threadIdx.x == 0) h_sh = ring_head(head, depth);
  __syncthreads();
  const int h = h_sh;
  DB* __restrict__ row = values + (int64_t)h * n;
  const int64_t tile = (int64_t)blockIdx.x * kValueTile;
  const int64_t tile_end = tile + kValueTile < n ? tile + kValueTile : n;
  const bool aligned = ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  for (int64_t i = tile + (int64_t)threadIdx.x * E; i < tile_end; i += (int64_t)kValueThreads * E) {
    if (aligned && i + E <= tile_end) {
      const ValuePack<SB, E> in = *reinterpret_cast<const ValuePack<SB, E>*>(x + i);
      ValuePack<DB, E> out;
#pragma unroll
      for (int u = 0; u < E; ++u) out.v[u] = value_convert<S, D>(in.v[u]);
      *reinterpret_cast<ValuePack<DB, E>*>(row + i) = out;
    } else {
      for (int u = 0; u < E && i + u < tile_end; ++u) row[i + u] = value_convert<S, D>(x[i + u]);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = atomicAdd(arrivals, 1u);
    if (t == gridDim.x - 1) {
      *arrivals = 0u;
      *head = (h + 1 == depth) ? 0 : h + 1;
    }
  }
}

template <typename S, typename D>
void launch_value_push(const void* x, int64_t n, int depth, void* values, int32_t* head, uint32_t* arrivals, hipStream_t st) {
  hipLaunchKernelGGL((k_value_ring_push<S, D>), dim3((unsigned)((n + kValueTile - 1) / kValueTile)), dim3(kValueThreads), 0, st,
                     static_cast<const typename PB<S>::bits*>(x), n, depth, static_cast<typename PB<D>::bits*>(values), head,
                     arrivals);
}

int ceil_log2(int depth) {
  int nbits = 0;
  while ((1 << nbits) < depth) ++nbits;
  return nbits;
}

unsigned mask_grid(int64_t m) {
  const int64_t g = (m + 255) / 256;
  return (unsigned)(g > kMaskGridCap ? kMaskGridCap : g);
}

int split_grid(int64_t m) {
  int64_t g = (m + kSplitThreads / 64 - 1) / (kSplitThreads / 64);
  if (g < 1) g = 1;
  return (int)(g > kSplitGridCap ? kSplitGridCap : g);
}

}  // namespace

extern "C" int64_t be_delay_split_workspace_bytes(int64_t m, int depth) {
  (void)m;
  (void)depth;
  return 256;      // the error word
}

extern "C" int be_delay_split_count(const void* indptr, int indptr_is64, int64_t row_len, const int32_t* delays, int64_t m,
                                    int depth, void* counts, int out_is64, void* workspace, int64_t workspace_bytes,
                                    be_stream_t stream) {
  BE_REQUIRE(m >= 0 && depth >= 1 && depth <= kMaxDepth, BE_ERR_INVALID, "need m >= 0 and 1 <= depth <= 256");
  BE_REQUIRE(indptr != nullptr || row_len >= 0, BE_ERR_INVALID, "indptr is NULL and row_len < 0");
  BE_REQUIRE(counts != nullptr && workspace != nullptr && workspace_bytes >= be_delay_split_workspace_bytes(m, depth),
             BE_ERR_INVALID, "null pointer or workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  BE_HIP(be_fill_async(workspace, 0xff, 8, st));      // "no offending position": the largest 64-bit value
  const RowPtr rp{indptr, indptr_is64, row_len};
  BE_REQUIRE(delays != nullptr || m == 0 || (indptr == nullptr && row_len == 0), BE_ERR_INVALID, "delays is NULL");
  unsigned long long* err = static_cast<unsigned long long*>(workspace);
  if (out_is64)
    hipLaunchKernelGGL((k_delay_split<false, int64_t>), dim3(split_grid(m)), dim3(kSplitThreads), 0, st, rp, delays, nullptr, m,
                       depth, ceil_log2(depth), static_cast<int64_t*>(counts), nullptr, nullptr, nullptr, err);
  else
    hipLaunchKernelGGL((k_delay_split<false, int32_t>), dim3(split_grid(m)), dim3(kSplitThreads), 0, st, rp, delays, nullptr, m,
                       depth, ceil_log2(depth), static_cast<int32_t*>(counts), nullptr, nullptr, nullptr, err);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

extern "C" int be_delay_split_fill(const void* indptr, int indptr_is64, int64_t row_len, const int32_t* delays,
                                   const int32_t* indices, int64_t m, int depth, const void* indptr_s, int out_is64, void* perm,
                                   int32_t* indices_s, uint32_t* row_mask, be_stream_t stream) {
  BE_REQUIRE(m >= 0 && depth >= 1 && depth <= kMaxDepth, BE_ERR_INVALID, "need m >= 0 and 1 <= depth <= 256");
  BE_REQUIRE(indptr != nullptr || row_len >= 0, BE_ERR_INVALID, "indptr is NULL and row_len < 0");
  BE_REQUIRE(indptr_s != nullptr && perm != nullptr, BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(indices_s == nullptr || indices != nullptr, BE_ERR_INVALID, "indices_s without indices");
  if (m == 0) return BE_OK;
  BE_REQUIRE(delays != nullptr || (indptr == nullptr && row_len == 0), BE_ERR_INVALID, "delays is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RowPtr rp{indptr, indptr_is64, row_len};
  const int64_t n_words = (m + 31) / 32;
  if (out_is64) {
    if (row_mask != nullptr)
      hipLaunchKernelGGL((k_delay_row_mask<int64_t>), dim3(mask_grid(m), depth),
                         dim3(256), 0, st, static_cast<const int64_t*>(indptr_s), m, n_words, row_mask);
    hipLaunchKernelGGL((k_delay_split<true, int64_t>), dim3(split_grid(m)), dim3(kSplitThreads), 0, st, rp, delays, indices, m,
                       depth, ceil_log2(depth), nullptr, static_cast<const int64_t*>(indptr_s), static_cast<int64_t*>(perm),
                       indices_s, nullptr);
  } else {
    if (row_mask != nullptr)
      hipLaunchKernelGGL((k_delay_row_mask<int32_t>), dim3(mask_grid(m), depth),
                         dim3(256), 0, st, static_cast<const int32_t*>(indptr_s), m, n_words, row_mask);
    hipLaunchKernelGGL((k_delay_split<true, int32_t>), dim3(split_grid(m)), dim3(kSplitThreads), 0, st, rp, delays, indices, m,
                       depth, ceil_log2(depth), nullptr, static_cast<const int32_t*>(indptr_s), static_cast<int32_t*>(perm),
                       indices_s, nullptr);
  }
  BE_LAUNCH_CHECK();
  return BE_OK;
}

namespace {

int ring_push_launch(const void* spikes, int spike_dtype, int64_t n, int depth, int64_t n_batch, uint32_t* bits, int32_t* head,
                     uint32_t* arrivals, be_stream_t stream) {
  BE_REQUIRE(n >= 1 && depth >= 1 && (int64_t)depth * n < (1ll << 31), BE_ERR_INVALID, "need n >= 1, depth >= 1, depth * n < 2^31");
  BE_REQUIRE(n_batch >= 1 && n_batch <= kRingMaxBatch, BE_ERR_INVALID, "need 1 <= n_batch <= 65535");
  BE_REQUIRE(spikes && bits && head && arrivals, BE_ERR_INVALID, "null pointer");
  const int64_t tiles = (n + kRingTileBits - 1) / kRingTileBits;
  BE_REQUIRE(tiles * n_batch < (1ll << 32), BE_ERR_INVALID, "more workgroups than the 32-bit ticket word counts");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)n_batch), block(kRingThreads);
  if (spike_dtype == BE_SPIKE_BOOL)
    hipLaunchKernelGGL(k_ring_push<SpikeBool>, grid, block, 0, st, static_cast<const uint8_t*>(spikes), n, depth, bits, head, arrivals);
  else if (spike_dtype == BE_SPIKE_FLOAT)
    hipLaunchKernelGGL(k_ring_push<SpikeFloat>, grid, block, 0, st, static_cast<const float*>(spikes), n, depth, bits, head, arrivals);
  else if (spike_dtype == BE_SPIKE_BITS)
    hipLaunchKernelGGL(k_ring_push<SpikeWords>, grid, block, 0, st, static_cast<const uint32_t*>(spikes), n, depth, bits, head, arrivals);
  else
    BE_REQUIRE(false, BE_ERR_UNSUPPORTED, "spike dtype must be BE_SPIKE_BOOL, BE_SPIKE_FLOAT or BE_SPIKE_BITS");
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" int be_spike_ring_push(const void* spikes, int spike_dtype, int64_t n, int depth, uint32_t* bits, int32_t* head,
                                  uint32_t* arrivals, be_stream_t stream) {
  return ring_push_launch(spikes, spike_dtype, n, depth, 1, bits, head, arrivals, stream);
}

extern "C" int be_spike_ring_push_batch(const void* spikes, int spike_dtype, int64_t n, int depth, int64_t n_batch, uint32_t* bits,
                                        int32_t* head, uint32_t* arrivals, be_stream_t stream) {
  return ring_push_launch(spikes, spike_dtype, n, depth, n_batch, bits, head, arrivals, stream);
}

extern "C" int be_spike_ring_unroll(const uint32_t* bits, const int32_t* head, int64_t n, int depth, int64_t n_batch, int ages,
                                    const uint32_t* row_mask, uint32_t* out, be_stream_t stream) {
  BE_REQUIRE(n >= 1 && depth >= 1 && ages >= 1 && ages <= depth && (int64_t)ages * n < (1ll << 31), BE_ERR_INVALID,
             "need n >= 1, 1 <= ages <= depth, ages * n < 2^31");
  BE_REQUIRE(n_batch >= 1 && n_batch <= kRingMaxBatch, BE_ERR_INVALID, "need 1 <= n_batch <= 65535");
  BE_REQUIRE(bits && head && out, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)ages * n, out_words = (total + 31) / 32;
  hipLaunchKernelGGL(k_ring_unroll, dim3((unsigned)((out_words + kUnrollThreads - 1) / kUnrollThreads), (unsigned)n_batch),
                     dim3(kUnrollThreads), 0, st, bits, head, (uint32_t)n, (n + 31) / 32, depth, (uint32_t)total, out_words, row_mask,
                     out);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

extern "C" int be_value_ring_push(const void* x, int x_dtype, int64_t n, int depth, void* values, int wdtype, int32_t* head,
                                  uint32_t* arrivals, be_stream_t stream) {
  BE_REQUIRE(n >= 1 && depth >= 1 && (int64_t)depth * n < (1ll << 31), BE_ERR_INVALID, "need n >= 1, depth >= 1, depth * n < 2^31");
  BE_REQUIRE(x && values && head && arrivals, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = be_dispatch_wdtype(x_dtype, [&](auto s) {
    return be_dispatch_wdtype(wdtype, [&](auto d) {
      launch_value_push<typename decltype(s)::type, typename decltype(d)::type>(x, n, depth, values, head, arrivals, st);
      return (int)BE_OK;
    });
  });
  if (rc != BE_OK) return rc;
  BE_LAUNCH_CHECK();
  return BE_OK;
}

extern "C" int be_spike_ring_compact(const uint32_t* bits, const int32_t* head, int64_t n, int depth, int ages,
                                     const uint32_t* row_mask, uint32_t* active_ids, uint32_t* count, be_stream_t stream) {
  BE_REQUIRE(n >= 1 && depth >= 1 && ages >= 1 && ages <= depth && ages <= 65535 && (int64_t)depth * n < (1ll << 31),
             BE_ERR_INVALID, "need n >= 1, 1 <= ages <= min(depth, 65535), depth * n < 2^31");
  BE_REQUIRE(bits && head && active_ids && count, BE_ERR_INVALID, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // count starts from zero on every call, under graph replay too: the house fill, a kernel node on the stream (be_common.h)
  BE_HIP(be_fill_async(count, 0, 4, st));
  const int64_t n_words = (n + 31) / 32;
  hipLaunchKernelGGL(k_ring_compact, dim3((unsigned)((n_words + kRingThreads - 1) / kRingThreads), (unsigned)ages),
                     dim3(kRingThreads), 0, st, bits, head, n, n_words, depth, row_mask, active_ids, count);
  BE_LAUNCH_CHECK();
  return BE_OK;
}
