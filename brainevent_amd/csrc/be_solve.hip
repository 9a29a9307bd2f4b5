// be_solve.hip — A x = b on CSR arrays for gfx950: right-preconditioned BiCGSTAB with the Jacobi preconditioner.
//   reference surface: brainevent/_csr/main.py:1778-1814 (CSR.solve -> cuSOLVER sparse QR); the method here is ITERATIVE.
//
//   r = b - A x0, rh = r;  per iteration (y = D^-1 p, z = D^-1 s; s overwrites r):
//     k_solve_p     rho = rh.r, beta = (rho / rho_old)(alpha / omega), p = r + beta (p - omega v), y = D^-1 p
//     k_solve_spmv  v = A y, partial sums of rh.v                                              (MODE 0)
//     k_solve_s     alpha = rho / rh.v, s = r - alpha v, z = D^-1 s, partial sums of s.s
//     k_solve_spmv  t = A z, partial sums of t.s and t.t                                        (MODE 1)
//     k_solve_x     omega = t.s / t.t, x += alpha y + omega z, r = s - omega t, partial sums of rh.r and r.r
//   five launches, no host synchronisation; order between the phases comes from the launch boundaries alone.  The scalars live
//   in SolveState; a consumer derives what it needs from its producer's partial sums — every workgroup sums the same partials in
//   the same order (sum_partials) and reaches the same value — and workgroup 0 stores it for the kernels of LATER launches.  No
//   kernel reads a field that a workgroup of the same launch writes, `status` excepted, and `status` is stored only on an exit
//   at which no workgroup of that launch owes any work (k_solve_p's converged exit, the breakdown exits): a workgroup that sees
//   it set returns, which is what it would have derived itself.  The half-step exit of k_solve_x is NOT such an exit — every
//   workgroup still owes x += alpha y — so its lead stores `half`, which k_solve_x never reads; every other kernel treats
//   `half` as converged (stopped()), and the next k_solve_p or k_solve_check copies it into `status`.
//   Sums: every dot product accumulates in f64, is reduced per workgroup by a fixed tree into partials[blockIdx], over a grid that
//   depends on (n, nnz) alone.  No float atomics: two calls on the same inputs give the same bytes.
//   Matrix passes are row gathers in aligned groups of four entries by 4, 16 or 64 lanes per row (the scheme of k_fcsrmv_nt,
//   be_float.hip); the matrix streams are loaded non-temporally.
#include "be_csr_shared.h"
#include <algorithm>

namespace {

constexpr int kSolveThreads = 256;
constexpr int kSolveVecGridCap = 1024;      // vector kernels: workgroups of 256 threads x 4 elements, grid-stride
constexpr int kSolveSpmvGridCap = 2048;     // matrix passes: workgroups of 256 / LPR x rows_in_flight(LPR) rows, grid-stride
constexpr int kSolvePartials = 2048;        // slots per partial-sum array (>= both caps)

enum { kRunning = 0, kConverged = 1, kBreakdown = 2 };

struct SolveState {          // mirrored by brainevent_amd/_solve.py (_STATE)
  double rho, rho_old, alpha, omega, rr;
  int32_t status, iters, first, offdiag, n_rr, half, pad[2];
};
static_assert(sizeof(SolveState) == 72, "SolveState layout");

enum { P_RR0 = 0, P_RR1, P_RV, P_SS, P_TS, P_TT, kPartialArrays };     // rh.r, r.r, rh.v, s.s, t.s, t.t

struct SolveWs {
  SolveState* st;
  double* part;
  char* vec;
  int64_t stride;          // bytes per vector
  template <typename W> W* v(int i) const { return reinterpret_cast<W*>(vec + (int64_t)i * stride); }
};
enum { V_R = 0, V_RH, V_P, V_V, V_T, V_Y, V_Z, V_DINV, kVectors };      // seven work vectors and D^-1

int64_t vec_stride(int64_t n, int wdtype) { return be_align_up(std::max<int64_t>(n, 1) * (int64_t)be_wbytes(wdtype), 256); }
int64_t part_bytes() { return (int64_t)kPartialArrays * kSolvePartials * 8; }

SolveWs carve(void* workspace, int64_t n, int wdtype) {
  char* base = static_cast<char*>(workspace);
  return SolveWs{reinterpret_cast<SolveState*>(base), reinterpret_cast<double*>(base + 256), base + 256 + part_bytes(),
                 vec_stride(n, wdtype)};
}

int vec_grid(int64_t n) { return grid_for((n + 3) / 4, kSolveThreads, kSolveVecGridCap); }
int lanes_per_row(int64_t n, int64_t nnz) {
  const int64_t avg = nnz / std::max<int64_t>(n, 1);
  return avg <= 24 ? 4 : (avg <= 160 ? 16 : 64);
}
// rows a lane group takes per step: short rows are latency-bound, their first groups are loaded together
constexpr int rows_in_flight(int lpr) { return lpr == 4 ? 4 : (lpr == 16 ? 2 : 1); }
int spmv_grid(int64_t n, int lpr) { return grid_for(n, (kSolveThreads / lpr) * rows_in_flight(lpr), kSolveSpmvGridCap); }

// ---------------------------------------------------------------- fixed-order reductions
// block sum by a fixed tree: xor shuffles inside a wave, the four wave sums in wave order.  Every thread returns the total.
__device__ __forceinline__ double block_sum(double v, double* red /* [4] in LDS */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                                   // (red may still be read from the previous use)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the sum of partials[0 .. count): thread t takes t, t + 256, ... in ascending order, then block_sum.  The same instructions in
// every workgroup of every launch: the same bits.
__device__ __forceinline__ double sum_partials(const double* __restrict__ p, int count, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < count; i += kSolveThreads) a += p[i];
  return block_sum(a, red);
}

__device__ __forceinline__ bool is_finite(double x) { return fabs(x) <= 1.79769313486231570e308; }      // (false for a NaN)
__device__ __forceinline__ bool finite_nonzero(double x) { return x != 0.0 && is_finite(x); }

// the status word as ONE value per workgroup (a workgroup of this launch may store it meanwhile)
__device__ __forceinline__ int block_status(const SolveState* st, int* slot) {
  if (threadIdx.x == 0) *slot = st->status;
  __syncthreads();
  return *slot;
}
// the same with `half` counted as converged: for every kernel but k_solve_x, whose lead stores `half` while its other
// workgroups still have their part of x to update
__device__ __forceinline__ int stopped(const SolveState* st, int* slot) {
  if (threadIdx.x == 0) *slot = st->half ? (int)kConverged : st->status;
  __syncthreads();
  return *slot;
}

// ---------------------------------------------------------------- four consecutive elements of a vector
template <typename W> struct Q4;
template <> struct Q4<float> {
  typedef float v4 __attribute__((ext_vector_type(4)));
  __device__ static __forceinline__ void load(const float* p, int64_t i, float (&o)[4]) {
    const v4 v = *reinterpret_cast<const v4*>(p + i);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  __device__ static __forceinline__ void load_nt(const float* p, int64_t i, float (&o)[4]) {
    const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p + i));
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  __device__ static __forceinline__ void store(float* p, int64_t i, const float (&o)[4]) {
    *reinterpret_cast<v4*>(p + i) = v4{o[0], o[1], o[2], o[3]};
  }
};
template <> struct Q4<double> {
  typedef double v2 __attribute__((ext_vector_type(2)));
  __device__ static __forceinline__ void load(const double* p, int64_t i, double (&o)[4]) {
    const v2 a = *reinterpret_cast<const v2*>(p + i), b = *reinterpret_cast<const v2*>(p + i + 2);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
  }
  __device__ static __forceinline__ void load_nt(const double* p, int64_t i, double (&o)[4]) {
    const v2 a = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p + i));
    const v2 b = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p + i + 2));
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
  }
  __device__ static __forceinline__ void store(double* p, int64_t i, const double (&o)[4]) {
    *reinterpret_cast<v2*>(p + i) = v2{o[0], o[1]};
    *reinterpret_cast<v2*>(p + i + 2) = v2{o[2], o[3]};
  }
};

// elements [i, i + 4) of a 16-byte aligned vector of n elements (i a multiple of 4); past n: zeros / nothing
template <typename W>
__device__ __forceinline__ void ld4(const W* p, int64_t i, int64_t n, W (&o)[4]) {
  if (i + 4 <= n) { Q4<W>::load(p, i, o); return; }
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = i + q < n ? p[i + q] : W(0);
}
template <typename W>
__device__ __forceinline__ void st4(W* p, int64_t i, int64_t n, const W (&o)[4]) {
  if (i + 4 <= n) { Q4<W>::store(p, i, o); return; }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (i + q < n) p[i + q] = o[q];
}

// ---------------------------------------------------------------- setup: D^-1, D, "is there an off-diagonal entry"
// D_ii = the sum of the stored (i, i) entries in storage order; 1 where that sum is zero or the diagonal is absent.
template <typename W>
__global__ void __launch_bounds__(kSolveThreads) k_solve_setup(const W* __restrict__ w, const int32_t* __restrict__ idx, RowPtr rp,
                                                               int64_t n, W* __restrict__ dinv, W* __restrict__ d, SolveState* st) {
  bool off = false;
  for (int64_t row = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x; row < n; row += (int64_t)gridDim.x * kSolveThreads) {
    const int64_t b = rp.at(row), e = rp.at(row + 1);
    W acc = W(0);
    for (int64_t j = b; j < e; ++j) {
      const W x = w[j];
      if ((int64_t)idx[j] == row) acc += x; else off |= x != W(0);
    }
    if (acc == W(0)) acc = W(1);
    d[row] = acc;
    dinv[row] = W(1) / acc;
  }
  if (off) st->offdiag = 1;             // (every writer stores the same value)
}

// a matrix without off-diagonal entries: x = b / D, one rounding per element
template <typename W>
__global__ void __launch_bounds__(kSolveThreads) k_solve_diagonal(const W* __restrict__ b, const W* __restrict__ d, W* __restrict__ x,
                                                                  int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSolveThreads)
    x[i] = b[i] / d[i];
}

// ---------------------------------------------------------------- matrix pass
// One aligned group of four entries [4g, 4g + 4) cut to the row [b, e) (load_group of be_float.hip, non-temporal).
template <typename W>
__device__ __forceinline__ uint32_t solve_group(const W* __restrict__ weights, const int32_t* __restrict__ indices, int64_t g,
                                                int64_t b, int64_t e, int64_t nnz, int32_t (&col)[4], W (&w)[4]) {
  typedef int i4 __attribute__((ext_vector_type(4)));
  const int64_t j0 = g << 2;
  uint32_t ok = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) ok |= (j0 + q >= b && j0 + q < e ? 1u : 0u) << q;
  if (j0 + 4 <= nnz) {
    const i4 c = __builtin_nontemporal_load(reinterpret_cast<const i4*>(indices + j0));
    col[0] = c.x; col[1] = c.y; col[2] = c.z; col[3] = c.w;
    Q4<W>::load_nt(weights, j0, w);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = j0 + q < nnz;
      col[q] = in ? indices[j0 + q] : 0;
      w[q] = in ? weights[j0 + q] : W(0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) col[q] = (ok >> q) & 1u ? col[q] : 0;       // a masked entry reads operand element 0 and adds nothing
  return ok;
}

// MODE 0: out = A in,      partials P_RV = rh.out                       (v = A y)
// MODE 1: out = A in,      partials P_TS = out.s, P_TT = out.out         (t = A z; s lives in r); skipped when s.s <= thr2
// MODE 2: out = b - A in (in == NULL: out = b), rh = out, partials P_RR0 = P_RR1 = out.out      (the true residual)
template <typename W, int LPR, int MODE, bool P64>
__global__ void __launch_bounds__(kSolveThreads) k_solve_spmv(const W* __restrict__ weights, const int32_t* __restrict__ indices,
                                                              const void* __restrict__ indptr, const W* __restrict__ in,
                                                              W* __restrict__ out, const W* __restrict__ aux /* rh | s | b */,
                                                              W* __restrict__ rh, int64_t n, SolveState* st,
                                                              double* __restrict__ part, int n_ss, double thr2) {
  using PT = typename std::conditional<P64, int64_t, int32_t>::type;
  typedef int i4 __attribute__((ext_vector_type(4)));
  const PT* __restrict__ ptr = static_cast<const PT*>(indptr);
  __shared__ double red[4];
  __shared__ int s_status;
  if (MODE != 2 && stopped(st, &s_status) != kRunning) return;
  if (MODE == 1 && sum_partials(part + P_SS * kSolvePartials, n_ss, red) <= thr2) return;     // converged at the half step
  constexpr int R = rows_in_flight(LPR), RPB = kSolveThreads / LPR;
  const int sub = threadIdx.x % LPR;
  const int64_t nnz = (int64_t)ptr[n];
  const bool walk = nnz > 0 && (MODE != 2 || in != nullptr);
  const int64_t g_full = (nnz >> 2) - 1;          // the last group that lies inside the arrays with all four entries
  const bool fast = walk && g_full >= 0;
  double d0 = 0.0, d1 = 0.0;
  for (int64_t r0 = (int64_t)blockIdx.x * (RPB * R); r0 < n; r0 += (int64_t)gridDim.x * (RPB * R)) {     // (whole waves stay in the loop: shuffles)
    int64_t row[R], b[R], e[R], next[R];
    W acc[R];
    // no load below sits under a per-lane condition: the compiler then issues the R rows' reads together instead of one
    // dependent round trip after the other (a row past the end reads the last row's pointers and is masked)
#pragma unroll
    for (int u = 0; u < R; ++u) {
      row[u] = r0 + u * RPB + threadIdx.x / LPR;
      const int64_t rc = min(row[u], n - 1);
      const int64_t pb = (int64_t)ptr[rc], pe = (int64_t)ptr[rc + 1];
      const bool live = row[u] < n && walk;
      b[u] = live ? pb : 0;
      e[u] = live ? pe : 0;
      next[u] = (b[u] >> 2) + sub;
      acc[u] = W(0);
    }
    if (fast) {
      // the first group of each of the R rows, as one aligned 16-byte load per array and lane.  A lane whose group lies past
      // the last full group of the arrays reads that one instead and masks it; the loop below takes its own group.
      int32_t c[R][4];
      W w[R][4], x[R][4];
      uint32_t ok[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int64_t g = next[u], gl = min(g, g_full), j0 = gl << 2;
        const i4 cv = __builtin_nontemporal_load(reinterpret_cast<const i4*>(indices + j0));
        Q4<W>::load_nt(weights, j0, w[u]);
        uint32_t m = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) m |= (j0 + q >= b[u] && j0 + q < e[u] ? 1u : 0u) << q;
        ok[u] = g == gl ? m : 0u;
        c[u][0] = ok[u] & 1u ? cv.x : 0; c[u][1] = ok[u] & 2u ? cv.y : 0; c[u][2] = ok[u] & 4u ? cv.z : 0; c[u][3] = ok[u] & 8u ? cv.w : 0;
        next[u] = g == gl ? g + LPR : g;
      }
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) x[u][q] = in[c[u][q]];
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[u] += (ok[u] >> q) & 1u ? w[u][q] * x[u][q] : W(0);
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int64_t g_end = (e[u] + 3) >> 2;
      for (int64_t g = next[u]; g < g_end; g += 2 * LPR) {                                    // the rest of a long row: two groups in flight
        int32_t c0[4], c1[4];
        W w_0[4], w_1[4], x0[4], x1[4];
        const bool second = g + LPR < g_end;
        const uint32_t ok0 = solve_group<W>(weights, indices, g, b[u], e[u], nnz, c0, w_0);
        const uint32_t ok1 = second ? solve_group<W>(weights, indices, g + LPR, b[u], e[u], nnz, c1, w_1) : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) x0[q] = in[c0[q]];
#pragma unroll
        for (int q = 0; q < 4; ++q) x1[q] = second ? in[c1[q]] : W(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if ((ok0 >> q) & 1u) acc[u] += w_0[q] * x0[q];
          if ((ok1 >> q) & 1u) acc[u] += w_1[q] * x1[q];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      W a = acc[u];
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
      if (sub == 0 && row[u] < n) {
        const W x_ = aux[row[u]];
        const W o = MODE == 2 ? x_ - a : a;
        out[row[u]] = o;
        if (MODE == 2) rh[row[u]] = o;
        d0 += (double)o * (double)(MODE == 2 ? o : x_);
        if (MODE == 1) d1 += (double)o * (double)o;
      }
    }
  }
  const double s0 = block_sum(d0, red);
  const double s1 = MODE == 1 ? block_sum(d1, red) : s0;
  if (threadIdx.x == 0) {
    if (MODE == 0) part[P_RV * kSolvePartials + blockIdx.x] = s0;
    if (MODE == 1) { part[P_TS * kSolvePartials + blockIdx.x] = s0; part[P_TT * kSolvePartials + blockIdx.x] = s1; }
    if (MODE == 2) { part[P_RR0 * kSolvePartials + blockIdx.x] = s0; part[P_RR1 * kSolvePartials + blockIdx.x] = s0; }
  }
}

// ---------------------------------------------------------------- vector phases
// p = r + beta (p - omega v) (the first iteration after a residual: p = r), y = D^-1 p
template <typename W>
__global__ void __launch_bounds__(kSolveThreads) k_solve_p(SolveState* st, const double* __restrict__ part, double thr2,
                                                           const W* __restrict__ r, const W* __restrict__ v, W* __restrict__ p,
                                                           W* __restrict__ y, const W* __restrict__ dinv, int64_t n) {
  __shared__ double red[4];
  __shared__ int s_status;
  if (stopped(st, &s_status) != kRunning) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && st->half) st->status = kConverged;      // (rr: k_solve_x stored it)
    return;
  }
  const int n_rr = st->n_rr;
  const double rho = sum_partials(part + P_RR0 * kSolvePartials, n_rr, red);
  const double rr = sum_partials(part + P_RR1 * kSolvePartials, n_rr, red);
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (rr <= thr2) {
    if (lead) { st->rr = rr; st->status = kConverged; }
    return;
  }
  const int first = st->first;
  const double omega = st->omega;
  const double beta = first ? 0.0 : (rho / st->rho_old) * (st->alpha / omega);
  if (!finite_nonzero(rho) || !is_finite(beta)) {
    if (lead) { st->rr = rr; st->status = kBreakdown; }
    return;
  }
  const W be = (W)beta, om = (W)omega;
  const int64_t n4 = (n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x; g < n4; g += (int64_t)gridDim.x * kSolveThreads) {
    const int64_t i = g << 2;
    W rv[4], pv[4], vv[4], dv[4], yv[4];
    ld4<W>(r, i, n, rv);
    ld4<W>(dinv, i, n, dv);
    if (first) {
#pragma unroll
      for (int q = 0; q < 4; ++q) pv[q] = rv[q];
    } else {
      ld4<W>(p, i, n, pv);
      ld4<W>(v, i, n, vv);
#pragma unroll
      for (int q = 0; q < 4; ++q) pv[q] = rv[q] + be * (pv[q] - om * vv[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) yv[q] = pv[q] * dv[q];
    st4<W>(p, i, n, pv);
    st4<W>(y, i, n, yv);
  }
  if (lead) st->rho = rho;
}

// alpha = rho / rh.v, s = r - alpha v (in place), z = D^-1 s, partials of s.s
template <typename W>
__global__ void __launch_bounds__(kSolveThreads) k_solve_s(SolveState* st, double* __restrict__ part, int n_rv, W* __restrict__ r,
                                                           const W* __restrict__ v, W* __restrict__ z, const W* __restrict__ dinv,
                                                           int64_t n) {
  __shared__ double red[4];
  __shared__ int s_status;
  if (stopped(st, &s_status) != kRunning) return;
  const double rv_dot = sum_partials(part + P_RV * kSolvePartials, n_rv, red);
  const double alpha = st->rho / rv_dot;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (!finite_nonzero(rv_dot) || !finite_nonzero(alpha)) {
    if (lead) st->status = kBreakdown;
    return;
  }
  const W al = (W)alpha;
  const int64_t n4 = (n + 3) >> 2;
  double ss = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x; g < n4; g += (int64_t)gridDim.x * kSolveThreads) {
    const int64_t i = g << 2;
    W rv[4], vv[4], dv[4], zv[4];
    ld4<W>(r, i, n, rv);
    ld4<W>(v, i, n, vv);
    ld4<W>(dinv, i, n, dv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rv[q] = rv[q] - al * vv[q];
      zv[q] = rv[q] * dv[q];
      ss += (double)rv[q] * (double)rv[q];
    }
    st4<W>(r, i, n, rv);
    st4<W>(z, i, n, zv);
  }
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) part[P_SS * kSolvePartials + blockIdx.x] = ss;
  if (lead) st->alpha = alpha;
}

// s.s <= thr2: x += alpha y in EVERY workgroup, and the lead stores `half` — not `status`, which the workgroups of this launch
// that start later gate on and would return on with their part of x not updated.  Else omega = t.s / t.t, x += alpha y + omega z, r = s - omega t, partials of rh.r, r.r
template <typename W>
__global__ void __launch_bounds__(kSolveThreads) k_solve_x(SolveState* st, double* __restrict__ part, int n_ss, int n_t, double thr2,
                                                           W* __restrict__ x, W* __restrict__ r, const W* __restrict__ rh,
                                                           const W* __restrict__ t, const W* __restrict__ y, const W* __restrict__ z,
                                                           int64_t n) {
  __shared__ double red[4];
  __shared__ int s_status;
  if (block_status(st, &s_status) != kRunning) return;
  const double ss = sum_partials(part + P_SS * kSolvePartials, n_ss, red);
  const bool half = ss <= thr2;
  double omega = 0.0;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (!half) {
    const double ts = sum_partials(part + P_TS * kSolvePartials, n_t, red);
    const double tt = sum_partials(part + P_TT * kSolvePartials, n_t, red);
    omega = ts / tt;
    if (!finite_nonzero(tt) || !finite_nonzero(omega)) {
      if (lead) st->status = kBreakdown;
      return;
    }
  }
  const W al = (W)st->alpha, om = (W)omega;
  const int64_t n4 = (n + 3) >> 2;
  double d0 = 0.0, d1 = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * kSolveThreads + threadIdx.x; g < n4; g += (int64_t)gridDim.x * kSolveThreads) {
    const int64_t i = g << 2;
    W xv[4], yv[4];
    ld4<W>(x, i, n, xv);
    ld4<W>(y, i, n, yv);
    if (half) {
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[q] = xv[q] + al * yv[q];
    } else {
      W zv[4], sv[4], tv[4], hv[4];
      ld4<W>(z, i, n, zv);
      ld4<W>(r, i, n, sv);
      ld4<W>(t, i, n, tv);
      ld4<W>(rh, i, n, hv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xv[q] = xv[q] + (al * yv[q] + om * zv[q]);
        sv[q] = sv[q] - om * tv[q];
        d0 += (double)hv[q] * (double)sv[q];
        d1 += (double)sv[q] * (double)sv[q];
      }
      st4<W>(r, i, n, sv);
    }
    st4<W>(x, i, n, xv);
  }
  if (half) {
    if (lead) { st->rr = ss; st->iters += 1; st->half = 1; }
    return;
  }
  d0 = block_sum(d0, red);
  d1 = block_sum(d1, red);
  if (threadIdx.x == 0) {
    part[P_RR0 * kSolvePartials + blockIdx.x] = d0;
    part[P_RR1 * kSolvePartials + blockIdx.x] = d1;
  }
  if (lead) { st->omega = omega; st->rho_old = st->rho; st->first = 0; st->n_rr = (int)gridDim.x; st->iters += 1; }
}

// one workgroup.  reset = 1 (after a residual pass over n_rr workgroups): rr = the sum, the state restarts from r, rh = r.
// reset = 0 (end of a chunk): rr and the status word, so that the host reads them without another launch.
__global__ void __launch_bounds__(kSolveThreads) k_solve_check(SolveState* st, double* __restrict__ part, int reset, int n_rr,
                                                               double thr2) {
  __shared__ double red[4];
  if (!reset) {
    if (st->half) {                              // converged at the half step; rr is k_solve_x's
      if (threadIdx.x == 0) st->status = kConverged;
      return;
    }
    if (st->status != kRunning) return;          // (one workgroup, nobody stores meanwhile)
    n_rr = st->n_rr;
  }
  const double rr = sum_partials(part + P_RR1 * kSolvePartials, n_rr, red);
  if (threadIdx.x != 0) return;
  st->rr = rr;
  if (reset) {
    part[P_RR0 * kSolvePartials] = rr;
    part[P_RR1 * kSolvePartials] = rr;
    st->n_rr = 1;
    st->first = 1;
    st->half = 0;
    st->status = kRunning;
  } else if (rr <= thr2) {
    st->status = kConverged;
  } else if (rr != rr) {
    st->status = kBreakdown;
  }
}

// ---------------------------------------------------------------- host side
template <typename W, int MODE>
void launch_spmv(int lpr, int grid, hipStream_t s, const W* w, const int32_t* idx, RowPtr rp, const W* in, W* out, const W* aux, W* rh,
                 int64_t n, SolveState* st, double* part, int n_ss, double thr2) {
#define BE_SOLVE_SPMV(LPR_, P64_) hipLaunchKernelGGL((k_solve_spmv<W, LPR_, MODE, P64_>), dim3(grid), dim3(kSolveThreads), 0, s, w, idx, rp.p, in, out, aux, rh, n, st, part, n_ss, thr2)
#define BE_SOLVE_SPMV_P(LPR_) do { if (rp.is64) BE_SOLVE_SPMV(LPR_, true); else BE_SOLVE_SPMV(LPR_, false); } while (0)
  if (lpr == 4) BE_SOLVE_SPMV_P(4); else if (lpr == 16) BE_SOLVE_SPMV_P(16); else BE_SOLVE_SPMV_P(64);
#undef BE_SOLVE_SPMV_P
#undef BE_SOLVE_SPMV
}

template <typename W>
int run_setup(const void* weights, const int32_t* indices, RowPtr rp, int64_t n, const SolveWs& ws, hipStream_t s) {
  BE_HIP(be_fill_async(ws.st, 0, 256, s));
  hipLaunchKernelGGL((k_solve_setup<W>), dim3(grid_for(n, kSolveThreads, 2048)), dim3(kSolveThreads), 0, s,
                     static_cast<const W*>(weights), indices, rp, n, ws.v<W>(V_DINV), ws.v<W>(V_T), ws.st);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int run_residual(const void* weights, const int32_t* indices, RowPtr rp, int64_t n, int64_t nnz, const void* b, const void* x,
                 const SolveWs& ws, hipStream_t s) {
  const int lpr = lanes_per_row(n, nnz), gm = spmv_grid(n, lpr);
  launch_spmv<W, 2>(lpr, gm, s, static_cast<const W*>(weights), indices, rp, static_cast<const W*>(x), ws.v<W>(V_R),
                    static_cast<const W*>(b), ws.v<W>(V_RH), n, ws.st, ws.part, 0, 0.0);
  BE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_solve_check, dim3(1), dim3(kSolveThreads), 0, s, ws.st, ws.part, 1, gm, 0.0);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int run_diagonal(const void* b, void* x, int64_t n, const SolveWs& ws, hipStream_t s) {
  hipLaunchKernelGGL((k_solve_diagonal<W>), dim3(grid_for(n, kSolveThreads, 2048)), dim3(kSolveThreads), 0, s,
                     static_cast<const W*>(b), ws.v<W>(V_T), static_cast<W*>(x), n);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

template <typename W>
int run_iterate(const void* weights, const int32_t* indices, RowPtr rp, int64_t n, int64_t nnz, void* x, int n_iter, double thr2,
                const SolveWs& ws, hipStream_t s) {
  const W* w = static_cast<const W*>(weights);
  const int lpr = lanes_per_row(n, nnz), gm = spmv_grid(n, lpr), gv = vec_grid(n);
  W *r = ws.v<W>(V_R), *rh = ws.v<W>(V_RH), *p = ws.v<W>(V_P), *v = ws.v<W>(V_V), *t = ws.v<W>(V_T), *y = ws.v<W>(V_Y),
    *z = ws.v<W>(V_Z), *dinv = ws.v<W>(V_DINV);
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL((k_solve_p<W>), dim3(gv), dim3(kSolveThreads), 0, s, ws.st, ws.part, thr2, r, v, p, y, dinv, n);
    launch_spmv<W, 0>(lpr, gm, s, w, indices, rp, y, v, rh, nullptr, n, ws.st, ws.part, 0, thr2);
    hipLaunchKernelGGL((k_solve_s<W>), dim3(gv), dim3(kSolveThreads), 0, s, ws.st, ws.part, gm, r, v, z, dinv, n);
    launch_spmv<W, 1>(lpr, gm, s, w, indices, rp, z, t, r, nullptr, n, ws.st, ws.part, gv, thr2);
    hipLaunchKernelGGL((k_solve_x<W>), dim3(gv), dim3(kSolveThreads), 0, s, ws.st, ws.part, gv, gm, thr2, static_cast<W*>(x), r, rh, t,
                       y, z, n);
    BE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_solve_check, dim3(1), dim3(kSolveThreads), 0, s, ws.st, ws.part, 0, 0, thr2);
  BE_LAUNCH_CHECK();
  return BE_OK;
}

int check_common(int wdtype, int64_t n, int64_t nnz, const void* workspace, int64_t workspace_bytes) {
  BE_REQUIRE(wdtype == BE_F32 || wdtype == BE_F64, BE_ERR_INVALID, "the solver takes f32 or f64 data");
  BE_REQUIRE(n >= 1 && n < (1ll << 31) && nnz >= 0, BE_ERR_INVALID, "bad shape");
  BE_REQUIRE(workspace != nullptr && workspace_bytes >= be_solve_workspace_bytes(n, wdtype), BE_ERR_WORKSPACE, "workspace too small");
  BE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, BE_ERR_INVALID, "workspace must be 16-byte aligned");
  return BE_OK;
}

}  // namespace

extern "C" {

int64_t be_solve_workspace_bytes(int64_t n, int wdtype) {
  return 256 + part_bytes() + (int64_t)kVectors * vec_stride(n, wdtype);
}

int be_solve_setup(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                   int64_t nnz, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  const int rc = check_common(wdtype, n, nnz, workspace, workspace_bytes);
  if (rc != BE_OK) return rc;
  BE_REQUIRE(indptr != nullptr && (nnz == 0 || (weights && indices)), BE_ERR_INVALID, "null pointer");
  const SolveWs ws = carve(workspace, n, wdtype);
  const RowPtr rp{indptr, indptr_is_i64, -1};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return wdtype == BE_F32 ? run_setup<float>(weights, indices, rp, n, ws, s) : run_setup<double>(weights, indices, rp, n, ws, s);
}

int be_solve_residual(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                      int64_t nnz, const void* b, const void* x, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  const int rc = check_common(wdtype, n, nnz, workspace, workspace_bytes);
  if (rc != BE_OK) return rc;
  BE_REQUIRE(indptr != nullptr && b != nullptr && (nnz == 0 || (weights && indices)), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(reinterpret_cast<uintptr_t>(weights) % 16 == 0 && reinterpret_cast<uintptr_t>(indices) % 16 == 0, BE_ERR_INVALID,
             "data and indices must be 16-byte aligned");
  const SolveWs ws = carve(workspace, n, wdtype);
  const RowPtr rp{indptr, indptr_is_i64, -1};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return wdtype == BE_F32 ? run_residual<float>(weights, indices, rp, n, nnz, b, x, ws, s)
                          : run_residual<double>(weights, indices, rp, n, nnz, b, x, ws, s);
}

int be_solve_diagonal(int wdtype, int64_t n, const void* b, void* x, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  const int rc = check_common(wdtype, n, 0, workspace, workspace_bytes);
  if (rc != BE_OK) return rc;
  BE_REQUIRE(b != nullptr && x != nullptr, BE_ERR_INVALID, "null pointer");
  const SolveWs ws = carve(workspace, n, wdtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return wdtype == BE_F32 ? run_diagonal<float>(b, x, n, ws, s) : run_diagonal<double>(b, x, n, ws, s);
}

int be_solve_iterate(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                     int64_t nnz, void* x, int n_iter, double thr2, void* workspace, int64_t workspace_bytes, be_stream_t stream) {
  const int rc = check_common(wdtype, n, nnz, workspace, workspace_bytes);
  if (rc != BE_OK) return rc;
  BE_REQUIRE(indptr != nullptr && x != nullptr && (nnz == 0 || (weights && indices)), BE_ERR_INVALID, "null pointer");
  BE_REQUIRE(n_iter >= 1 && n_iter <= 64, BE_ERR_INVALID, "n_iter must be in [1, 64]");
  BE_REQUIRE(reinterpret_cast<uintptr_t>(weights) % 16 == 0 && reinterpret_cast<uintptr_t>(indices) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(x) % 16 == 0, BE_ERR_INVALID, "data, indices and x must be 16-byte aligned");
  const SolveWs ws = carve(workspace, n, wdtype);
  const RowPtr rp{indptr, indptr_is_i64, -1};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return wdtype == BE_F32 ? run_iterate<float>(weights, indices, rp, n, nnz, x, n_iter, thr2, ws, s)
                          : run_iterate<double>(weights, indices, rp, n, nnz, x, n_iter, thr2, ws, s);
}

}  // extern "C"
