// be_neuron_sg_reduce.hip — the sum that ends the backward pass of learnable, per-neuron beta / v_th: the lane
// kernel of be_neuron_sg.hip writes one f32 accumulator per slot (g_beta_slot, g_vth_slot [N]); be_lif_sg_reduce_slots sums the
// N / P slots of each of the P parameter elements in f64, in an order the shape alone fixes, and rounds to f32 once.  No float
// atomics anywhere: two calls give identical bits.  The only file of the differentiable neuron that uses LDS.
#include "be_common.h"
#include <algorithm>

namespace {

// the reduce: blocks of kSgpRedThreads; period 1 runs at most kSgpRedGridCap blocks over tiles of kSgpRedTile slots, then one
// block over their partials; a longer period runs kSgpRedCols columns by kSgpRedThreads / kSgpRedCols row lanes a block
constexpr int kSgpRedThreads = 256;
constexpr int kSgpRedTile = 4096;
constexpr int kSgpRedGridCap = 256;
constexpr int kSgpRedCols = 64;
static_assert(kSgpRedGridCap <= kSgpRedThreads && kSgpRedThreads % kSgpRedCols == 0, "the reduce's second stage is one block");

// the block's sum of one f64 per thread, in a fixed tree; valid in thread 0
__device__ __forceinline__ double sgp_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int half = kSgpRedThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) lds[threadIdx.x] += lds[threadIdx.x + half];
    __syncthreads();
  }
  return lds[0];
}

// period 1, first stage: block b sums the tiles b, b + gridDim.x, ... (a thread: its strided slots of each tile, in order)
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_tiles(const float* __restrict__ slot, int64_t N,
                                                                         double* __restrict__ partial) {
  __shared__ double lds[kSgpRedThreads];
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * kSgpRedTile; base < N; base += (int64_t)gridDim.x * kSgpRedTile) {
    const int64_t end = std::min<int64_t>(base + kSgpRedTile, N);
    for (int64_t i = base + threadIdx.x; i < end; i += kSgpRedThreads) acc += (double)slot[i];
  }
  const double sum = sgp_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// period 1, second stage: one block over the at most kSgpRedGridCap (<= kSgpRedThreads) partials; rounds to f32 once
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_final(const double* __restrict__ partial, int count,
                                                                         float* __restrict__ out) {
  __shared__ double lds[kSgpRedThreads];
  const double sum = sgp_block_sum((int)threadIdx.x < count ? partial[threadIdx.x] : 0.0, lds);
  if (threadIdx.x == 0) out[0] = (float)sum;
}

// period P > 1: a block owns kSgpRedCols consecutive elements p; row lane q sums the rows q, q + kRows, ... of its column in
// order, then the kRows partials of a column are added in order of q and rounded to f32 once
__global__ void __launch_bounds__(kSgpRedThreads) k_lif_sgp_reduce_columns(const float* __restrict__ slot, int64_t R, int64_t P,
                                                                           float* __restrict__ out) {
  constexpr int kRows = kSgpRedThreads / kSgpRedCols;
  __shared__ double lds[kRows][kSgpRedCols];
  const int col = threadIdx.x % kSgpRedCols, q = threadIdx.x / kSgpRedCols;
  const int64_t p = (int64_t)blockIdx.x * kSgpRedCols + col;
  double acc = 0.0;
  if (p < P)
    for (int64_t r = q; r < R; r += kRows) acc += (double)slot[r * P + p];
  lds[q][col] = acc;
  __syncthreads();
  if (q == 0 && p < P) {
    double sum = lds[0][col];
#pragma unroll
    for (int k = 1; k < kRows; ++k) sum += lds[k][col];
    out[p] = (float)sum;
  }
}

inline int sgp_reduce_blocks(int64_t N) {
  return (int)std::min<int64_t>((N + kSgpRedTile - 1) / kSgpRedTile, kSgpRedGridCap);
}

}  // namespace

extern "C" {

int64_t be_lif_sg_reduce_slots_workspace_bytes(int64_t N, int64_t P) {
  if (N <= 0 || P != 1) return 0;
  return (int64_t)sgp_reduce_blocks(N) * (int64_t)sizeof(double);
}

int be_lif_sg_reduce_slots(const float* slot, int64_t N, int64_t P, float* out, void* workspace, int64_t workspace_bytes,
                           be_stream_t stream) {
  BE_REQUIRE(N >= 0, BE_ERR_INVALID, "N < 0");
  BE_REQUIRE(P >= 1, BE_ERR_INVALID, "the period must be >= 1");
  BE_REQUIRE(N % P == 0, BE_ERR_INVALID, "the period must divide N");
  if (N == 0) return BE_OK;
  BE_REQUIRE(slot && out, BE_ERR_INVALID, "null pointer (slot and out are required)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (P == 1) {
    const int blocks = sgp_reduce_blocks(N);
    BE_REQUIRE(workspace != nullptr && workspace_bytes >= be_lif_sg_reduce_slots_workspace_bytes(N, P), BE_ERR_INVALID,
               "workspace too small (be_lif_sg_reduce_slots_workspace_bytes)");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, BE_ERR_INVALID, "workspace must be 8-byte aligned");
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_lif_sgp_reduce_tiles, dim3(blocks), dim3(kSgpRedThreads), 0, st, slot, N, partial);
    hipLaunchKernelGGL(k_lif_sgp_reduce_final, dim3(1), dim3(kSgpRedThreads), 0, st, partial, blocks, out);
  } else {
    const int64_t blocks = (P + kSgpRedCols - 1) / kSgpRedCols;
    BE_REQUIRE(blocks <= 0x7fffffff, BE_ERR_INVALID, "the period is too long for one grid");
    hipLaunchKernelGGL(k_lif_sgp_reduce_columns, dim3((unsigned)blocks), dim3(kSgpRedThreads), 0, st, slot, N / P, P, out);
  }
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
