// be_jitc_grad.hip — the parameter gradients of the JIT-connectivity products for gfx950.
//   reference: brainevent/_jit_normal/binary.py:442-505, brainevent/_jit_normal/float.py:843-910 (and the scalar / uniform twins):
//              the gradient of a parameter is a full float product with the parameters replaced by (1, 0) / (0, 1), then a dot
//              product — one walk of the matrix per parameter (per 8 columns of a matrix operand with the float twins here).
// Edge (r, j) of the generator carries w = w0 + t(r, j) * w1, so both parameter gradients of a call are sums over the same edges:
//   S0 = sum_edges sum_b P[r, b] Q[j, b]        S1 = sum_edges t(r, j) sum_b P[r, b] Q[j, b]
// (P indexed by generator row, Q by walk position; be_jitc_shared.h: the walk and the hashes).  One walk gives both, at any batch
// width: every load is widened to f64, products and sums are f64, t is formed in f32 as edge_weight forms it.  No float atomics:
// a thread adds its edges in walk order, a wave reduces by a fixed shuffle tree, a block adds its waves in order into its slot of
// the workspace, and a second launch of one workgroup adds the slots in a fixed order — two calls give the same 16 bytes.
#include "be_jitc_shared.h"

namespace {

constexpr int kParamGradThreads = 256;      // a block walks kParamGradThreads / stride generator rows of one chunk at a time
constexpr int kParamGradGridCap = 2048;     // workgroups per launch (8 per CU); the (row block, chunk) tasks beyond are taken grid-stride

// (s0, s1) of the block in thread 0: wave shuffle tree (xor: the same tree in every lane), then the waves in ascending order
__device__ __forceinline__ void block_sum2(double& s0, double& s1) {
  __shared__ double sh[2][kParamGradThreads / kWave];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, kWave);
    s1 += __shfl_xor(s1, off, kWave);
  }
  if (lane_id() == 0) {
    sh[0][threadIdx.x / kWave] = s0;
    sh[1][threadIdx.x / kWave] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s0 = sh[0][0];
    s1 = sh[1][0];
    for (int w = 1; w < kParamGradThreads / kWave; ++w) {
      s0 += sh[0][w];
      s1 += sh[1][w];
    }
  }
}

// A task (row block, chunk) is walked as in k_jit_f_gather: `stride` lanes per generator row, lane l visiting the chunk-local
// columns l + stride * q; each lane does the nb-long dot of its edges.  A generator row whose P row is all zero is not walked
// (the float scatter's `if (!any) continue`): the backward of an event-driven scatter stays proportional to the active rows.
// VEC: nb == 1, the row's P value lives in a register.
template <int MODE, typename W, bool VEC>
__global__ void __launch_bounds__(kParamGradThreads) k_jit_param_grad(JitP p, const W* __restrict__ P, const W* __restrict__ Q,
                                                                      int64_t n_rows, int64_t nb, int64_t row_blocks,
                                                                      double* __restrict__ partial) {
  const int S = p.stride;
  const uint32_t l = threadIdx.x % S;
  const int64_t tpb = kParamGradThreads / S;
  const int64_t tasks = row_blocks * p.n_chunks;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t t = blockIdx.x; t < tasks; t += gridDim.x) {      // (block-uniform: whole waves reach the shuffles below)
    const int64_t rb = t / p.n_chunks;
    const int chunk = (int)(t - rb * p.n_chunks);
    const int64_t row = rb * tpb + threadIdx.x / S;
    double p0 = 0.0;
    int any = 0;
    if (row < n_rows) {
      if (VEC) {
        p0 = (double)WTraits<W>::load(P, row);
        any = p0 != 0.0;
      } else {
        for (int64_t b = l; b < nb; b += S) any |= (double)WTraits<W>::load(P, row * nb + b) != 0.0;
      }
    }
    if (!VEC) {
      for (int off = S / 2; off > 0; off >>= 1) any |= __shfl_xor(any, off, kWave);
    }
    if (any) {
      const JitSpan span = jit_chunk_span(p, chunk);
      const int64_t cs = span.cs;
      const uint32_t qmax = jit_positions<uint32_t>(span.width, l, S);      // l + S q < width
      const uint32_t grow = (uint32_t)row;
      const W* prow = P + row * nb;
      JitWalk walk(p, grow, (uint32_t)chunk, l);
      while (walk.q < qmax) {
        const int64_t col = cs + l + (int64_t)S * walk.q;
        double d;
        if (VEC) {
          d = p0 * (double)WTraits<W>::load(Q, col);
        } else {
          const W* qrow = Q + col * nb;
          d = 0.0;
          for (int64_t b = 0; b < nb; ++b) d += (double)WTraits<W>::load(prow, b) * (double)WTraits<W>::load(qrow, b);
        }
        s0 += d;
        if (MODE == MODE_UNIFORM) s1 += (double)lr_uniform01(p.seed, grow, (uint32_t)col) * d;
        if (MODE == MODE_NORMAL) s1 += (double)lr_normal01(p.seed, grow, (uint32_t)col) * d;
        walk.next(p);
      }
    }
  }
  block_sum2(s0, s1);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = s0;
    partial[2 * (int64_t)blockIdx.x + 1] = s1;
  }
}

// one workgroup: thread i adds the slots i, i + kParamGradThreads, ... in ascending order, then the block sum (n_slots == 0: two zeros,
// nothing is read)
__global__ void __launch_bounds__(kParamGradThreads) k_jit_param_grad_reduce(const double* __restrict__ partial, int n_slots,
                                                                             double* __restrict__ sums) {
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < n_slots; i += kParamGradThreads) {
    s0 += partial[2 * i];
    s1 += partial[2 * i + 1];
  }
  block_sum2(s0, s1);
  if (threadIdx.x == 0) {
    sums[0] = s0;
    sums[1] = s1;
  }
}

struct ParamGradGeom { int64_t n_chunks, row_blocks; int grid; };
// a function of (shape1, n_rows, walk_len, stride) alone: the summation order, hence the result's bits, depends on nothing else
inline ParamGradGeom param_grad_geom(int64_t shape1, int64_t n_rows, int64_t walk_len, int stride) {
  ParamGradGeom g;
  const int64_t chunk = std::max<int64_t>(1, (shape1 + 3) / 4);
  const int64_t tpb = kParamGradThreads / (stride == 4 ? 4 : 32);
  g.n_chunks = (std::max<int64_t>(0, walk_len) + chunk - 1) / chunk;
  g.row_blocks = (std::max<int64_t>(0, n_rows) + tpb - 1) / tpb;
  const int64_t tasks = g.row_blocks * g.n_chunks;
  g.grid = (int)std::max<int64_t>(1, std::min<int64_t>(tasks, kParamGradGridCap));
  return g;
}

template <int MODE, typename W>
int run_param_grad(const JitP& p, const ParamGradGeom& g, const void* P, const void* Q, int64_t n_rows, int64_t nb, double* partial,
                   hipStream_t st) {
  const W* Pw = static_cast<const W*>(P);
  const W* Qw = static_cast<const W*>(Q);
  if (nb == 1)
    hipLaunchKernelGGL((k_jit_param_grad<MODE, W, true>), dim3(g.grid), dim3(kParamGradThreads), 0, st, p, Pw, Qw, n_rows, nb,
                       g.row_blocks, partial);
  else
    hipLaunchKernelGGL((k_jit_param_grad<MODE, W, false>), dim3(g.grid), dim3(kParamGradThreads), 0, st, p, Pw, Qw, n_rows, nb,
                       g.row_blocks, partial);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // namespace

extern "C" {

int64_t be_jit_param_grad_workspace_bytes(int64_t shape1, int64_t n_rows, int64_t walk_len, int stride) {
  return be_align_up((int64_t)param_grad_geom(shape1, n_rows, walk_len, stride).grid * 16, 256);
}

int be_jit_param_grad(int mode, int wdtype, int64_t clen, uint32_t seed, const void* P, const void* Q, int64_t shape1,
                      int64_t n_rows, int64_t walk_len, int64_t nb, int stride, double* sums, void* workspace,
                      int64_t workspace_bytes, be_stream_t stream) {
  BE_REQUIRE(mode >= 0 && mode <= 2, BE_ERR_INVALID, "mode must be 0 (scalar), 1 (uniform) or 2 (normal)");
  BE_REQUIRE(wdtype == BE_F32 || wdtype == BE_F64 || wdtype == BE_F16 || wdtype == BE_BF16, BE_ERR_INVALID, "unknown weight dtype");
  BE_REQUIRE(n_rows >= 0 && walk_len >= 0 && shape1 >= 0 && nb >= 0, BE_ERR_INVALID, "bad shape");
  BE_REQUIRE(stride == 32 || stride == 4, BE_ERR_INVALID, "stride must be 32 (the mv matrix) or 4 (the mm matrix)");
  BE_REQUIRE(n_rows < (1ll << 32) && walk_len < (1ll << 32), BE_ERR_RANGE, "dimensions must fit uint32 for the RNG keys");
  BE_REQUIRE(sums != nullptr, BE_ERR_INVALID, "sums is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (clen <= 0 || n_rows == 0 || walk_len == 0 || nb == 0) {      // nothing is drawn or nothing multiplies: two zeros, nothing read
    hipLaunchKernelGGL(k_jit_param_grad_reduce, dim3(1), dim3(kParamGradThreads), 0, st, (const double*)nullptr, 0, sums);
    BE_LAUNCH_CHECK();
    return BE_OK;
  }
  BE_REQUIRE(P != nullptr && Q != nullptr, BE_ERR_INVALID, "operand is NULL");
  const ParamGradGeom g = param_grad_geom(shape1, n_rows, walk_len, stride);
  BE_REQUIRE(g.n_chunks <= INT32_MAX, BE_ERR_RANGE, "the walk takes more than 2^31 - 1 chunks (a quarter of shape[1] each)");
  BE_REQUIRE(workspace != nullptr && workspace_bytes >= be_jit_param_grad_workspace_bytes(shape1, n_rows, walk_len, stride),
             BE_ERR_WORKSPACE, "workspace too small");
  const JitP p = make_params(shape1, walk_len, seed, clen, stride, 0.0, 0.0);      // (the chunks are a loop here, not a grid dimension)
  double* partial = static_cast<double*>(workspace);
  const int rc = jit_dispatch_mode(mode, [&](auto md) {
    return be_dispatch_wdtype(wdtype, [&](auto w) {
      using W = typename decltype(w)::type;
      return run_param_grad<decltype(md)::value, W>(p, g, P, Q, n_rows, nb, partial, st);
    });
  });
  if (rc != BE_OK) return rc;
  hipLaunchKernelGGL(k_jit_param_grad_reduce, dim3(1), dim3(kParamGradThreads), 0, st, (const double*)partial, g.grid, sums);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

}  // extern "C"
