// kernels_lu.hip -- K4/K5: batched dense complex LU with partial pivoting on gfx950 (solve fused in).
// Replaces batch_tensorsolve.btensorsolve -> linalg.solve (LAPACK zgesv) at reference _biem.py:797.
// Layout: every system is the augmented row-major matrix [M | F] with n_pad rows, n_cols = n_pad + nrhs columns and
// leading dimension lda (complex128 elements).  Right-looking blocked LU, panel width NB:
//   panel_load   M[j:, j:j+NB] -> P (column-major workspace, so the pivot search and the rank-1 updates are coalesced)
//   panel_factor unblocked LU with partial pivoting on P (one workgroup per system)
//   panel_store  P -> M (L21 stays in P: it is the A operand of the trailing zgemm in exactly the [k][i] order
//                the f64 MFMA A-fragment wants, so it is staged to LDS without a transpose)
//   swap         row interchanges on the columns outside the panel (coalesced: rows are contiguous)
//   trsm         U12 = L11^{-1} M[j:j+NB, j+NB:]   (includes the right-hand-side columns: forward elimination rides along)
//   gemm         M[j+NB:, j+NB:] -= L21 * U12      3M zgemm on v_mfma_f64_4x4x4_4b_f64 (k_gemm3m_pipe; K = 64 / 128 / 192 / 256)
// then a blocked back substitution with U (kernels_trisolve.hip).  All kernels are batched over systems (blockIdx.z / .y).
// The same launcher runs the older COLUMN form A = L D L^T of the symmetric factorisation (symmetric = true: k_diag_nopiv, k_panel_l21,
// k_u_from_l, k_rhs_panel; production runs the row form, kernels_sym.hip).  The update kernel is kernels_gemm3m.hip's.
#include "dense.hpp"

namespace biem {

int lu_npad(int N) { return ((N + NB - 1) / NB) * NB; }

// (the layout: DenseWork, dense.hpp)
size_t lu_workspace_bytes(int nb, int n_pad, int nrhs) { return dense_work(nb, n_pad, nrhs).total; }

int check_factor_args(const char* who, int nb, int n_pad, int nrhs, long long lda, size_t work_bytes) {
  if (n_pad % NB) { set_error("%s: n_pad=%d is not a multiple of %d (use biem_lu_npad)", who, n_pad, NB); return BIEM_ERR_ARG; }
  if (nrhs < 0 || lda < n_pad + nrhs) { set_error("%s: lda < n_pad + nrhs", who); return BIEM_ERR_ARG; }
  if (nb > 65535 || nrhs > 65535) { set_error("%s: at most 65535 systems / right-hand sides per call (got %d / %d)", who, nb, nrhs); return BIEM_ERR_ARG; }
  if (work_bytes < lu_workspace_bytes(nb, n_pad, nrhs)) { set_error("%s: workspace too small", who); return BIEM_ERR_ARG; }
  return BIEM_OK;
}

void ldlt_thresholds(double& nopiv_rel, double& growth_max) {
  const char *e = getenv("BIEM_LDLT_PIVOT_REL"), *g = getenv("BIEM_LDLT_GROWTH_MAX");
  nopiv_rel = e && atof(e) > 0.0 ? atof(e) : NOPIV_REL;
  growth_max = g && atof(g) > 0.0 ? atof(g) : GROWTH_MAX;
}

// max |A| over the lower triangle and the diagonal 64 x 64 blocks: 8 rows per workgroup, coalesced along the row
__global__ void __launch_bounds__(256) k_absmax_lower(const cplx* __restrict__ A, long long lda, long long sys_stride, int n_pad,
                                                       unsigned long long* __restrict__ growth) {
  const int s = blockIdx.y;
  const cplx* As = A + (size_t)s * sys_stride;
  double m = 0.0;
  for (int r = 0; r < 8; ++r) {
    const int i = blockIdx.x * 8 + r;
    if (i >= n_pad) break;
    const int cend = (i / NB + 1) * NB;
    for (int c = threadIdx.x; c < cend; c += 256) m = nan_max(m, cabs1(As[(size_t)i * lda + c]));
  }
  block_max_publish(m, growth + 2 * (size_t)s);
}

// ---------------------------------------------------------------------------------------------
// panel load / store (transposing copies through LDS)
// ---------------------------------------------------------------------------------------------
constexpr int TR = 32;   // rows per transpose tile
__global__ void __launch_bounds__(256) k_panel_load(const cplx* __restrict__ A, long long lda, long long sys_stride,
                                                     cplx* __restrict__ Pw, long long ldp, long long p_stride, int n_pad, int j) {
  __shared__ cplx tile[TR][NB + 1];
  const int s = blockIdx.y, i0 = j + blockIdx.x * TR;
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Ps = Pw + (size_t)s * p_stride;
  for (int idx = threadIdx.x; idx < TR * NB; idx += 256) {
    int r = idx / NB, c = idx % NB, gi = i0 + r;
    if (gi < n_pad) tile[r][c] = As[(size_t)gi * lda + j + c];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < TR * NB; idx += 256) {
    int c = idx / TR, r = idx % TR, gi = i0 + r;
    if (gi < n_pad) Ps[(size_t)c * ldp + gi] = tile[r][c];
  }
}

__global__ void __launch_bounds__(256) k_panel_store(cplx* __restrict__ A, long long lda, long long sys_stride,
                                                      const cplx* __restrict__ Pw, long long ldp, long long p_stride, int n_pad, int j) {
  __shared__ cplx tile[TR][NB + 1];
  const int s = blockIdx.y, i0 = j + blockIdx.x * TR;
  cplx* As = A + (size_t)s * sys_stride;
  const cplx* Ps = Pw + (size_t)s * p_stride;
  for (int idx = threadIdx.x; idx < TR * NB; idx += 256) {
    int c = idx / TR, r = idx % TR, gi = i0 + r;
    if (gi < n_pad) tile[r][c] = Ps[(size_t)c * ldp + gi];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < TR * NB; idx += 256) {
    int r = idx / NB, c = idx % NB, gi = i0 + r;
    if (gi < n_pad) As[(size_t)gi * lda + j + c] = tile[r][c];
  }
}

// ---------------------------------------------------------------------------------------------
// panel factorisation: LU with partial pivoting of the column-major panel, blocked in strips of PW columns.
//   k_panel_strip  (one 1024-thread workgroup per system): unblocked right-looking elimination confined to the strip's PW
//                  columns (pivot = max |re| + |im|, LAPACK izamax's cabs1, ties -> smallest row; the interchange is
//                  applied to all NB panel columns; the pass that writes column c+1 also searches it), then
//                  U_strip,right = L_strip^{-1} P[strip rows, right columns]
//   k_panel_update (all CUs): the rank-PW update of the rows below the strip on the right columns
// History (profiles/): unblocked sweep 2.15 ms per 6400 x 64 panel (NB^2/2 column passes through L2); strips inside one
// workgroup 0.89 ms, then f64-VALU bound: the rank-8 updates are 92 MFLOP on ONE CU, and 32 systems keep only 32 of 256
// CUs busy - hence the update runs as its own launch over the whole chip.
// ---------------------------------------------------------------------------------------------
constexpr int PW = 8;

constexpr int STRIP_CACHE_ROWS = 1024;   // rows of the strip kept in LDS (one per thread): 1024 x 8 x 16 B = 128 KiB

__global__ void __launch_bounds__(1024) k_panel_strip(cplx* __restrict__ Pw, long long ldp, long long p_stride, int n_pad, int j, int c0,
                                                       int second, int* __restrict__ ipiv, int* __restrict__ info) {
  // Thread t owns the fixed rows rs + t + 1024 k of the strip (rs = j + c0).  Its first row (k = 0) lives in LDS for the whole
  // strip - the strip is read and written once per column pass otherwise, and with every CU running one system's strip the
  // kernel is bound by that traffic (6.5 TB/s at 256 systems); the upper rows are the ones every pass touches longest.
  extern __shared__ cplx tile[];   // [PW][STRIP_CACHE_ROWS]: tile[q * 1024 + (row - rs)]
  __shared__ double sval[2][16];   // per-wave pivot candidates, double-buffered over columns
  __shared__ int sidx[2][16];
  __shared__ cplx sU[PW];          // current pivot row restricted to the strip
  __shared__ cplx sL[PW][PW];      // unit-lower strip triangle
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  cplx* Ps = Pw + (size_t)s * p_stride;
  const int rs = j + c0;
  cplx* Pc = Ps + (size_t)c0 * ldp;
  const unsigned ldp32 = (unsigned)ldp;
  const int my0 = rs + tid;                      // the cached row of this thread
  const bool have0 = my0 < n_pad;
  auto sget = [&](int q, int row) -> cplx { return row - rs < STRIP_CACHE_ROWS ? tile[q * STRIP_CACHE_ROWS + (row - rs)] : Pc[(unsigned)q * ldp32 + (unsigned)row]; };
  auto sput = [&](int q, int row, cplx v) {
    if (row - rs < STRIP_CACHE_ROWS) tile[q * STRIP_CACHE_ROWS + (row - rs)] = v; else Pc[(unsigned)q * ldp32 + (unsigned)row] = v;
  };

  auto publish = [&](double best, int bi, int buf) {
    for (int o = 32; o > 0; o >>= 1) {
      double ob = __shfl_down(best, o, 64);
      int oi = __shfl_down(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { sval[buf][wave] = best; sidx[buf][wave] = bi; }
  };
  auto decide = [&](int buf, int r0) -> int {   // every thread reduces the 16 candidates redundantly (no extra barrier)
    double b = sval[buf][0]; int ix = sidx[buf][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) { double v = sval[buf][w]; int i2 = sidx[buf][w]; if (v > b || (v == b && i2 < ix)) { b = v; ix = i2; } }
    return ix == 0x7fffffff ? r0 : ix;          // all-NaN column: keep the diagonal
  };

  {  // stage the cached rows and search the strip's first column
    double best = -1.0; int bi = 0x7fffffff;
    if (have0) {
#pragma unroll
      for (int q = 0; q < PW; ++q) tile[q * STRIP_CACHE_ROWS + tid] = Pc[(unsigned)q * ldp32 + (unsigned)my0];
      const cplx v = tile[tid];
      const double a = fabs(v.x) + fabs(v.y);
      if (a > best) { best = a; bi = my0; }
    }
    for (int i = my0 + STRIP_CACHE_ROWS; i < n_pad; i += 1024) {
      const cplx v = Pc[(unsigned)i];
      const double a = fabs(v.x) + fabs(v.y);
      if (a > best) { best = a; bi = i; }
    }
    publish(best, bi, 0);
  }
  __syncthreads();
  int buf = 0;
  // the column loop is unrolled (cq = c - c0 is a compile-time index into the per-row register copy of the strip):
  // per row all PW columns are LOADED FIRST (independent requests in flight), then eliminated, then stored - the earlier
  // load/fma/store-per-element form was one dependent L2 round trip per element (no __restrict__ is possible here)
#pragma unroll
  for (int cq = 0; cq < PW; ++cq) {
    const int c = c0 + cq;
    const int r0 = j + c;
    const int p = decide(buf, r0);
    if (tid == 0) ipiv[(size_t)s * n_pad + r0] = p;
    if (tid < NB) {
      const bool mine = tid >= c0 && tid < c0 + PW;     // a strip column: rows may live in LDS
      cplx a = mine ? sget(tid - c0, r0) : Ps[(size_t)tid * ldp + r0];
      if (p != r0) {
        cplx b = mine ? sget(tid - c0, p) : Ps[(size_t)tid * ldp + p];
        if (mine) { sput(tid - c0, p, a); sput(tid - c0, r0, b); }
        else { Ps[(size_t)tid * ldp + p] = a; Ps[(size_t)tid * ldp + r0] = b; }
        a = b;
      }
      if (mine) sU[tid - c0] = a;   // row r0 after the interchange, strip columns
    }
    __syncthreads();
    const cplx piv = sU[cq];
    const bool singular = piv.x == 0.0 && piv.y == 0.0;
    if (singular && tid == 0 && info[s] == 0) info[s] = r0 + 1;
    const cplx rinv = singular ? make_double2(0.0, 0.0) : crecip(piv);
    cplx u[PW];
#pragma unroll
    for (int q = 0; q < PW; ++q) u[q] = sU[q];
    double best = -1.0; int bi = 0x7fffffff;
    if (have0 && my0 > r0) {                              // the cached row: LDS
      cplx v[PW];
#pragma unroll
      for (int q = cq; q < PW; ++q) v[q] = tile[q * STRIP_CACHE_ROWS + tid];
      if (!singular) {
        const cplx l = cmul(v[cq], rinv);
        v[cq] = l;
#pragma unroll
        for (int q = cq + 1; q < PW; ++q) v[q] = cfnma(l, u[q], v[q]);
      }
#pragma unroll
      for (int q = cq; q < PW; ++q) tile[q * STRIP_CACHE_ROWS + tid] = v[q];
      if (cq + 1 < PW) { double a = fabs(v[cq + 1 < PW ? cq + 1 : cq].x) + fabs(v[cq + 1 < PW ? cq + 1 : cq].y); if (a > best) { best = a; bi = my0; } }
    }
    for (int i = my0 + STRIP_CACHE_ROWS; i < n_pad; i += 1024) {     // the other rows: global memory (always below r0)
      cplx v[PW];
#pragma unroll
      for (int q = cq; q < PW; ++q) v[q] = Pc[(unsigned)q * ldp32 + (unsigned)i];
      if (!singular) {
        const cplx l = cmul(v[cq], rinv);
        v[cq] = l;
#pragma unroll
        for (int q = cq + 1; q < PW; ++q) v[q] = cfnma(l, u[q], v[q]);
      }
#pragma unroll
      for (int q = cq; q < PW; ++q) Pc[(unsigned)q * ldp32 + (unsigned)i] = v[q];
      if (cq + 1 < PW) { double a = fabs(v[cq + 1 < PW ? cq + 1 : cq].x) + fabs(v[cq + 1 < PW ? cq + 1 : cq].y); if (a > best) { best = a; bi = i; } }
    }
    if (cq + 1 < PW) { publish(best, bi, buf ^ 1); buf ^= 1; }
    __syncthreads();
  }
  // cached rows back to the panel
  if (have0) {
#pragma unroll
    for (int q = 0; q < PW; ++q) Pc[(unsigned)q * ldp32 + (unsigned)my0] = tile[q * STRIP_CACHE_ROWS + tid];
  }
  __syncthreads();
  const int nright = NB - (c0 + PW);
  if (nright <= 0) return;
  __shared__ cplx sL10[PW][PW];       // second strip of a pair: its rows x the first strip's columns
  if (tid < PW * PW) {
    int q = tid / PW, q2 = tid % PW;   // L[q][q2], q2 < q
    sL[q][q2] = (q2 < q) ? Ps[(size_t)(c0 + q2) * ldp + rs + q] : make_double2(0.0, 0.0);
    if (second) sL10[q][q2] = Ps[(size_t)(c0 - PW + q2) * ldp + rs + q];
  }
  __syncthreads();
  if (tid < nright) {
    cplx* colr = Ps + (size_t)(c0 + PW + tid) * ldp + rs;
    cplx x[PW];
#pragma unroll
    for (int q = 0; q < PW; ++q) x[q] = colr[q];
    if (second) {
      // the right columns have not received the first strip's update yet (it is applied together with this strip's as one
      // rank-16 update): bring this strip's rows up to date here, x -= L10 U0, U0 = the first strip's rows of this column
      cplx u0[PW];
#pragma unroll
      for (int q2 = 0; q2 < PW; ++q2) u0[q2] = colr[q2 - PW];
#pragma unroll
      for (int q = 0; q < PW; ++q)
#pragma unroll
        for (int q2 = 0; q2 < PW; ++q2) x[q] = cfnma(sL10[q][q2], u0[q2], x[q]);
    }
#pragma unroll
    for (int q = 1; q < PW; ++q)
#pragma unroll
      for (int q2 = 0; q2 < q; ++q2) x[q] = cfnma(sL[q][q2], x[q2], x[q]);
#pragma unroll
    for (int q = 0; q < PW; ++q) colr[q] = x[q];
  }
}

// rows below the strip, right columns:  P[cc][i] -= sum_q L[i][q] U[q][cc];  one thread per row, all CUs
template <int PWU>
__global__ void __launch_bounds__(256) k_panel_update(cplx* __restrict__ Pw, long long ldp, long long p_stride, int n_pad, int j, int c0,
                                                       int ncols) {
  // rank-PWU update of `ncols` (a multiple of 8) columns right of the PWU factored columns c0 .. c0+PWU-1, rows below them
  __shared__ cplx sUr[PWU][NB];
  const int s = blockIdx.y, tid = threadIdx.x;
  cplx* Ps = Pw + (size_t)s * p_stride;
  const int rs = j + c0;
  for (int e = tid; e < ncols * PWU; e += 256) {
    int t = e / PWU, q = e % PWU;
    sUr[q][t] = Ps[(size_t)(c0 + PWU + t) * ldp + rs + q];
  }
  __syncthreads();
  const int i = rs + PWU + blockIdx.x * 256 + tid;
  if (i >= n_pad) return;
  cplx l[PWU];
#pragma unroll
  for (int q = 0; q < PWU; ++q) l[q] = Ps[(size_t)(c0 + q) * ldp + i];
  // 8 independent loads, 8 PWU complex FMAs, 8 stores per group
  for (int t0 = 0; t0 < ncols; t0 += 8) {
    cplx v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = Ps[(size_t)(c0 + PWU + t0 + t) * ldp + i];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int q = 0; q < PWU; ++q) v[t] = cfnma(l[q], sUr[q][t0 + t], v[t]);
#pragma unroll
    for (int t = 0; t < 8; ++t) Ps[(size_t)(c0 + PWU + t0 + t) * ldp + i] = v[t];
  }
}

// ---------------------------------------------------------------------------------------------
// row interchanges outside the panel: thread per column, all NB swaps in order.
// columns: left part [0, j) when `left`, right part [j+NB, n_cols).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_swap(cplx* __restrict__ A, long long lda, long long sys_stride, int n_pad, int n_cols,
                                               int j, const int* __restrict__ ipiv, int left) {
  __shared__ int sp[NB];
  const int s = blockIdx.y;
  if (threadIdx.x < NB) sp[threadIdx.x] = ipiv[(size_t)s * n_pad + j + threadIdx.x];
  __syncthreads();
  int t = blockIdx.x * 256 + threadIdx.x;
  int col;
  if (left) { col = t < j ? t : t + NB; } else { col = t + j + NB; }
  if (col >= n_cols) return;
  cplx* As = A + (size_t)s * sys_stride + col;
  for (int c = 0; c < NB; ++c) {
    int p = sp[c];
    if (p != j + c) {
      cplx a = As[(size_t)(j + c) * lda], b = As[(size_t)p * lda];
      As[(size_t)(j + c) * lda] = b;
      As[(size_t)p * lda] = a;
    }
  }
}

// W = I - L11^{-1} for the unit-lower 64 x 64 diagonal block of a panel, stored [k][i] (the MFMA A-operand order), so that
//   U12 = L11^{-1} A12 = A12 - W A12
// runs on the streaming zgemm (C -= A*B with B = C's own rows; a tile reads all of its 64 x 128 block before it stores).
// One 64-thread workgroup per system; thread c owns column c of the inverse (forward substitution in LDS).
__global__ void __launch_bounds__(64) k_inv_l11(const cplx* __restrict__ Pj, long long ldp, long long p_stride, int j,
                                                 cplx* __restrict__ Winv) {
  extern __shared__ cplx sm[];
  cplx* sLT = sm;               // sLT[k][r] = L[r][k]
  cplx* sW = sm + NB * NB;      // sW[r][c]
  const int s = blockIdx.x, c = threadIdx.x;
  const cplx* Ps = Pj + (size_t)s * p_stride;
  for (int k = 0; k < NB; ++k) {
    sLT[k * NB + c] = Ps[(size_t)k * ldp + j + c];
    sW[k * NB + c] = (k == c) ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0);
  }
  __syncthreads();
  for (int r = 1; r < NB; ++r) {
    cplx acc = make_double2(0.0, 0.0);
    for (int k = 0; k < r; ++k) acc = cfma(sLT[k * NB + r], sW[k * NB + c], acc);
    if (r > c) sW[r * NB + c] = make_double2(-acc.x, -acc.y);
  }
  __syncthreads();
  cplx* Wo = Winv + (size_t)s * NB * NB;
  for (int k = 0; k < NB; ++k) {
    cplx v = sW[c * NB + k];                                   // inverse[i = c][k]
    Wo[k * NB + c] = (c > k) ? make_double2(-v.x, -v.y) : make_double2(0.0, 0.0);
  }
}

// apply the row interchanges of the second panel of a block to the stored multipliers of the first (P columns 0..NB-1)
__global__ void __launch_bounds__(64) k_swap_p(cplx* __restrict__ Pw, long long ldp, long long p_stride, int n_pad, int j, int ncols,
                                                const int* __restrict__ ipiv) {
  // the interchanges of the panel at column j on the multipliers of the EARLIER panels of the same K = 256 group
  // (workspace columns 0 .. ncols-1): their trailing update is still to come and needs the rows in their final order
  const int s = blockIdx.x;
  for (int c = threadIdx.x; c < ncols; c += 64) {
    cplx* col = Pw + (size_t)s * p_stride + (size_t)c * ldp;
    for (int q = 0; q < NB; ++q) {
      int p = ipiv[(size_t)s * n_pad + j + q];
      if (p != j + q) { cplx a = col[j + q]; col[j + q] = col[p]; col[p] = a; }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// symmetric path, few right-hand sides: the forward elimination of the right-hand-side columns as matrix-vector work
// (a 64 x 64 MFMA tile per 64 rows is almost empty for one column, and the triangular solve needs no inverse).
// ---------------------------------------------------------------------------------------------
// the 64 rows of the panel at column j (workspace columns pc ..): y = L11^{-1} (f - L[rows, 0:kd] y_prev), kd = pc = the columns
// of the group's earlier panels (rows jg .. jg+kd).  One 64-thread workgroup per (system, right-hand side).
__global__ void __launch_bounds__(64) k_rhs_panel(cplx* __restrict__ A, long long lda, long long sys_stride, const cplx* __restrict__ Pw,
                                                   long long ldp, long long p_stride, int n_pad, int j, int jg, int pc) {
  __shared__ cplx sy[4 * NB];
  __shared__ cplx sx;
  const int s = blockIdx.x, q = blockIdx.y, r = threadIdx.x;
  cplx* F = A + (size_t)s * sys_stride + n_pad + q;
  const cplx* Pr = Pw + (size_t)s * p_stride + j + r;            // row j + r of the workspace, column k at Pr[k * ldp]
  for (int k = r; k < pc; k += NB) sy[k] = F[(size_t)(jg + k) * lda];
  __syncthreads();
  cplx y = F[(size_t)(j + r) * lda];
  for (int k = 0; k < pc; ++k) y = cfnma(Pr[(size_t)k * ldp], sy[k], y);
  for (int c = 0; c < NB - 1; ++c) {
    if (r == c) sx = y;
    __syncthreads();
    if (r > c) y = cfnma(Pr[(size_t)(pc + c) * ldp], sx, y);
    __syncthreads();
  }
  F[(size_t)(j + r) * lda] = y;
}

// ---------------------------------------------------------------------------------------------
// panel factorisation without interchanges (symmetric path): the 64 x 64 diagonal block is factored by one workgroup per
// system (k_diag_nopiv, which also forms X = U11^{-1}); the rows below are L21 = A21 X, one thread per row over all CUs
// (k_panel_l21): 160 column passes per panel through HBM instead of the strips' 576, no per-column barriers.
// The acceptance test of the pivoted-path strips carries over unchanged: |pivot| >= rel * max |column below, updated| is
// |l_ic| <= 1 / rel for every multiplier; a violation marks the system (info = -(row + 1) of the panel's first row).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_diag_nopiv(cplx* __restrict__ Pj, long long ldp, long long p_stride, int n_pad, int j,
                                                     cplx* __restrict__ Xinv, int* __restrict__ ipiv, int* __restrict__ info, double rel,
                                                     unsigned long long* __restrict__ growth) {
  // 256 threads: row r = tid & 63, part = tid >> 6 (one wave each).  Elimination: the four parts share the trailing columns of a
  // step (c2 = c+1+part, +4, ...).  Inverse: X = U11^{-1} by anti-diagonals d = c - k (entries of one d are independent), the
  // sum over m of an entry split over the four parts and reduced through LDS.
  __shared__ cplx a[NB][NB + 1];     // a[c][r]: column c, row r (as in the workspace)
  __shared__ cplx x[NB][NB + 1];     // x[k][c] = (U11^{-1})[k][c]
  __shared__ cplx red[4][NB];
  __shared__ int bad;
  const int s = blockIdx.x, tid = threadIdx.x, r = tid & 63, part = tid >> 6;
  cplx* Ps = Pj + (size_t)s * p_stride + j;
  if (tid == 0) bad = 0;
  for (int c = part; c < NB; c += 4) { a[c][r] = Ps[(size_t)c * ldp + r]; x[c][r] = make_double2(0.0, 0.0); }
  if (part == 0) ipiv[(size_t)s * n_pad + j + r] = j + r;
  __syncthreads();
  for (int c = 0; c < NB; ++c) {
    const cplx piv = a[c][c];
    const double pa = fabs(piv.x) + fabs(piv.y);
    cplx l = make_double2(0.0, 0.0);
    if (r > c) {
      const cplx v = a[c][r];
      if (part == 0 && !(pa >= rel * (fabs(v.x) + fabs(v.y)))) bad = 1;
      l = cmul(v, crecip(piv));
      for (int c2 = c + 1 + part; c2 < NB; c2 += 4) a[c2][r] = cfnma(l, a[c2][c], a[c2][r]);
    } else if (r == c && part == 0 && !(pa > 0.0)) bad = 1;
    __syncthreads();                       // every part has read a[c][r]; the trailing columns are updated
    if (r > c && part == 0) a[c][r] = l;   // column c is not read again inside this loop
  }
  __syncthreads();
  // X: thread (k = r, part) works on the entry (k, k + d) of anti-diagonal d
  for (int d = 0; d < NB; ++d) {
    const int k = r, c = r + d;
    cplx acc = make_double2(0.0, 0.0);
    if (c < NB)
      for (int m = k + 1 + part; m <= c; m += 4) acc = cfma(a[m][k], x[m][c], acc);     // U[k][m] x[m][c]
    red[part][r] = acc;
    __syncthreads();
    if (part == 0 && c < NB) {
      cplx sum = red[0][r];
      sum.x += red[1][r].x + red[2][r].x + red[3][r].x; sum.y += red[1][r].y + red[2][r].y + red[3][r].y;
      cplx rhs = (d == 0) ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0);
      rhs.x -= sum.x; rhs.y -= sum.y;
      x[k][c] = cmul(rhs, crecip(a[k][k]));
    }
    __syncthreads();
  }
  double um = 0.0;                                   // U11 = the entries on and above the diagonal (row r <= column c)
  for (int c = part; c < NB; c += 4) { Ps[(size_t)c * ldp + r] = a[c][r]; if (r <= c) um = nan_max(um, cabs1(a[c][r])); }
  block_max_publish(um, growth + 2 * (size_t)s + 1);
  cplx* Xo = Xinv + (size_t)s * NB * NB;
  for (int k = part; k < NB; k += 4) Xo[k * NB + r] = x[k][r];
  if (tid == 0 && bad && info[s] == 0) info[s] = -(j + 1);
}

__global__ void __launch_bounds__(256) k_panel_l21(cplx* __restrict__ Pj, long long ldp, long long p_stride, int n_pad, int j,
                                                    const cplx* __restrict__ Xinv, int* __restrict__ info, double rel) {
  extern __shared__ cplx sX[];       // [k][c], 64 x 64
  const int s = blockIdx.y, tid = threadIdx.x;
  const cplx* Xs = Xinv + (size_t)s * NB * NB;
  for (int e = tid; e < NB * NB; e += 256) sX[e] = Xs[e];
  __syncthreads();
  const int i = j + NB + blockIdx.x * 256 + tid;
  if (i >= n_pad) return;
  cplx* Pr = Pj + (size_t)s * p_stride + i;
  double lmax = 0.0;
  // columns 32..63 first (they need a_0..a_63 and overwrite a_32..a_63), then 0..31 (a_0..a_31 only)
#pragma unroll 1
  for (int half = 1; half >= 0; --half) {
    const int cb = half * 32;
    cplx acc[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) acc[q] = make_double2(0.0, 0.0);
    if (half) {
#pragma unroll 4
      for (int k = 0; k < 32; ++k) {            // full 32 columns
        const cplx ak = Pr[(size_t)k * ldp];
#pragma unroll
        for (int q = 0; q < 32; ++q) acc[q] = cfma(ak, sX[k * NB + cb + q], acc[q]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {            // triangular part: X[k][c] = 0 for c < k
      const cplx ak = Pr[(size_t)(cb + kk) * ldp];
#pragma unroll
      for (int q = 0; q < 32; ++q)
        if (q >= kk) acc[q] = cfma(ak, sX[(cb + kk) * NB + cb + q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 32; ++q) {
      Pr[(size_t)(cb + q) * ldp] = acc[q];
      const double v = fabs(acc[q].x) + fabs(acc[q].y);
      if (!(v <= lmax)) lmax = v;                 // NaN-safe: a non-finite multiplier makes lmax NaN and marks the system
    }
  }
  if (!(lmax * rel <= 1.0) && info[s] == 0) info[s] = -(j + 1);
}

// U rows of a factored panel from its multipliers, symmetric path: U[j+i][c] = d_i L[c][i] for the columns c right of the panel
// (A = L D L^T, so U = D L^T needs no triangular solve and no pending updates).  P is column-major: both sides are contiguous in c.
// One workgroup: 256 columns x 16 of the panel's 64 rows; it also publishes max |U| of its entries (growth check).
__global__ void __launch_bounds__(256) k_u_from_l(cplx* __restrict__ A, long long lda, long long sys_stride, const cplx* __restrict__ Pj,
                                                   long long ldp, long long p_stride, int n_pad, int j, unsigned long long* __restrict__ growth) {
  const int s = blockIdx.z;
  const int c = j + NB + blockIdx.x * 256 + threadIdx.x;
  double um = 0.0;
  if (c < n_pad) {
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int i = blockIdx.y * 16 + q;
      const cplx* Pi = Pj + (size_t)s * p_stride + (size_t)i * ldp;
      const cplx u = cmul(Pi[j + i], Pi[c]);
      A[(size_t)s * sys_stride + (size_t)(j + i) * lda + c] = u;
      um = nan_max(um, cabs1(u));
    }
  }
  block_max_publish(um, growth + 2 * (size_t)s + 1);
}

int launch_lu_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_ipiv,
                           int* d_info, void* d_work, size_t work_bytes, hipStream_t st, bool keep_multipliers, bool symmetric,
                           bool amax_ready) {
  if (nb <= 0 || n_pad <= 0) return BIEM_OK;
  if (const int rc = check_factor_args("biem_lu", nb, n_pad, nrhs, lda, work_bytes)) return rc;
  cplx* A = (cplx*)d_A;
  const DenseWork W = dense_work(nb, n_pad, nrhs);
  cplx* Pw = W.panels_at(d_work);
  const long long ldp = ldp_of(n_pad), p_stride = (long long)PANEL_COLS * ldp;
  const int n_cols = n_pad + nrhs;
  launch_zero_int(st, d_info, nb);
  const size_t strip_lds = (size_t)PW * STRIP_CACHE_ROWS * sizeof(cplx);
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_panel_strip, hipFuncAttributeMaxDynamicSharedMemorySize, (int)strip_lds));
  // (per call, not once per process: the attribute belongs to the current device)
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_inv_l11, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * NB * NB * sizeof(cplx))));
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_panel_l21, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(NB * NB * sizeof(cplx))));

  // status of the update launches (the lambdas below cannot return it themselves): the first failure is kept and returned
  int gemm_rc = BIEM_OK;
  auto gemm = [&](auto&&... a) { const int r = launch_gemm_stream(a...); if (r != BIEM_OK && gemm_rc == BIEM_OK) gemm_rc = r; };
  cplx* Winv = W.block_at(d_work);              // 64 x 64 per system: I - L11^{-1} (LU) / U11^{-1} (symmetric path)
  int* const tri_map = W.tri_map_at(d_work);    // tile map of the triangular updates
  unsigned long long* growth = W.growth_at(d_work);                 // [nb][2]: max |A|, max |U| (symmetric path)
  double nopiv, growth_max; ldlt_thresholds(nopiv, growth_max);   // pivot acceptance, accepted max |U| / max |A| (symmetric path)
  // factor the 64-column panel at column j, multipliers into P columns [pc, pc + NB)
  auto panel = [&](int j, int pc, bool in_workspace = false) {
    cplx* Pj = Pw + (size_t)pc * ldp;
    const int rows = n_pad - j;
    ProfScope ps(PK_PANEL, st, 4.0 * (double)nb * rows * NB * NB);
    if (!in_workspace)     // (panels b, c, d of a group arrive in the workspace straight from the update that produced them)
      hipLaunchKernelGGL(k_panel_load, dim3((rows + TR - 1) / TR, nb), dim3(256), 0, st, A, lda, sys_stride, Pj, ldp, p_stride, n_pad, j);
    if (symmetric) {
      // no interchanges: diagonal block in one workgroup per system, then L21 = A21 U11^{-1} over all CUs
      hipLaunchKernelGGL(k_diag_nopiv, dim3(nb), dim3(256), 0, st, Pj, ldp, p_stride, n_pad, j, Winv, d_ipiv, d_info, nopiv, growth);
      if (rows > NB)
        hipLaunchKernelGGL(k_panel_l21, dim3((rows - NB + 255) / 256, nb), dim3(256), NB * NB * sizeof(cplx), st, Pj, ldp, p_stride, n_pad, j,
                           Winv, d_info, nopiv);
    } else
    // strips in pairs: after the first strip only the second strip's 8 columns are updated (rank 8); the columns right of
    // the pair get both strips' updates as ONE rank-16 pass (336 instead of 504 column passes per panel through HBM)
    for (int c0 = 0; c0 < NB; c0 += 2 * PW) {
      hipLaunchKernelGGL(k_panel_strip, dim3(nb), dim3(1024), strip_lds, st, Pj, ldp, p_stride, n_pad, j, c0, 0, d_ipiv, d_info);
      int below = n_pad - (j + c0 + PW);
      if (below > 0)
        hipLaunchKernelGGL(k_panel_update<PW>, dim3((below + 255) / 256, nb), dim3(256), 0, st, Pj, ldp, p_stride, n_pad, j, c0, PW);
      hipLaunchKernelGGL(k_panel_strip, dim3(nb), dim3(1024), strip_lds, st, Pj, ldp, p_stride, n_pad, j, c0 + PW, 1, d_ipiv, d_info);
      below = n_pad - (j + c0 + 2 * PW);
      const int ncols = NB - (c0 + 2 * PW);
      if (ncols > 0 && below > 0)
        hipLaunchKernelGGL(k_panel_update<2 * PW>, dim3((below + 255) / 256, nb), dim3(256), 0, st, Pj, ldp, p_stride, n_pad, j, c0, ncols);
    }
    // back to the row-major matrix: everything (factors for the caller) or only the 64 rows of the diagonal block - U11 is
    // all the rest of the solve reads from these columns (the trailing updates take L21 from the panel workspace)
    const int srows = keep_multipliers ? rows : (rows < NB ? rows : NB);
    hipLaunchKernelGGL(k_panel_store, dim3((srows + TR - 1) / TR, nb), dim3(256), 0, st, A, lda, sys_stride, Pj, ldp, p_stride,
                       keep_multipliers ? n_pad : j + srows, j);
    if (pc > 0 && !symmetric) hipLaunchKernelGGL(k_swap_p, dim3(nb), dim3(64), 0, st, Pw, ldp, p_stride, n_pad, j, pc, d_ipiv);
  };
  // the panel's row interchanges on the columns right of it
  auto swap_right = [&](int j) {
    const int rcols = n_cols - (j + NB);
    if (rcols <= 0) return;
    ProfScope ps(PK_SWAP, st, 64.0 * (double)nb * NB * rcols);
    hipLaunchKernelGGL(k_swap, dim3((rcols + 255) / 256, nb), dim3(256), 0, st, A, lda, sys_stride, n_pad, n_cols, j, d_ipiv, 0);
  };
  // U row block: M[j:j+NB, j+NB:] <- L11^{-1} M[j:j+NB, j+NB:]
  auto trsm = [&](int j, int pc, int col_begin = -1) {
    if (col_begin < 0) col_begin = j + NB;
    const int rcols = n_cols - col_begin;
    if (rcols <= 0) return;
    const double work = 4.0 * (double)nb * NB * NB * rcols;
    {
      ProfScope ps(PK_TRSM, st, 0.0);
      hipLaunchKernelGGL(k_inv_l11, dim3(nb), dim3(64), 2 * NB * NB * sizeof(cplx), st, Pw + (size_t)pc * ldp, ldp, p_stride, j, Winv);
    }
    // A operand W[k][i], i = row - j: hand the kernel the base shifted by -j rows (only rows j .. j+63 are addressed)
    gemm(st, nb, A, lda, sys_stride, Winv - j, NB, (long long)NB * NB, j, j + NB, col_begin, n_cols, j, NB, PK_TRSM, work);
  };
  // symmetric path: the panel's U rows over the matrix columns by transposition, over the right-hand sides by the solve
  const bool rhs_gemv = nrhs > 0 && nrhs <= 8;   // few right-hand sides: matrix-vector kernels instead of nearly empty MFMA tiles
  auto u_rows_sym = [&](int j, int jg, int pc) {
    const int rcols = n_pad - (j + NB);
    if (rcols > 0) {
      ProfScope ps(PK_TRSM, st, 0.0);
      hipLaunchKernelGGL(k_u_from_l, dim3((rcols + 255) / 256, NB / 16, nb), dim3(256), 0, st, A, lda, sys_stride, Pw + (size_t)pc * ldp, ldp, p_stride, n_pad, j, growth);
    }
    if (rhs_gemv) {
      ProfScope ps(PK_TRSM, st, 0.0);
      hipLaunchKernelGGL(k_rhs_panel, dim3(nb, nrhs), dim3(64), 0, st, A, lda, sys_stride, Pw, ldp, p_stride, n_pad, j, jg, pc);
    } else if (nrhs > 0) {
      if (pc > 0) gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, j, j + NB, n_pad, n_cols, jg, pc, PK_OTHER);
      trsm(j, pc, n_pad);
    }
  };

  if (symmetric) {
    // growth check, part 1: max |A| over what will be read (amax_ready: the caller's fill has already stored it), max |U| = 0
    if (!amax_ready) {
      launch_zero_int(st, (int*)growth, 4 * nb);
      ProfScope ps(PK_SWAP, st, 0.0);
      hipLaunchKernelGGL(k_absmax_lower, dim3((n_pad + 7) / 8, nb), dim3(256), 0, st, A, lda, sys_stride, n_pad, growth);
    }
    // the tile map of the triangular updates (full bands of the largest trailing matrix), behind the panels and W
    launch_tri_map(st, tri_map, n_pad);
    // A = L D L^T without interchanges (the caller guarantees a complex-symmetric matrix; a rejected diagonal is reported in
    // info).  Same four-panel groups and the same kernels; what changes: no interchanges; a panel's U rows are its transposed,
    // D-scaled multipliers; only the right-hand-side columns of those rows take pending updates and the triangular solve; the
    // K = 256 update runs over the lower triangle of tiles (and the right-hand sides): half the flops of the LU.
    for (int J = 0; J < n_pad; J += 4 * NB) {
      panel(J, 0); u_rows_sym(J, J, 0);
      for (int q = 1; q < 4; ++q) {
        const int jq = J + q * NB;
        if (jq >= n_pad) break;
        // the panel's columns: all pending updates of the group (K = 64 q) for all rows below, delivered into the workspace
        gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, jq, n_pad, jq, jq + NB, J, q * NB, PK_OTHER, -1.0,
                           Pw + (size_t)(q * NB) * ldp, ldp, p_stride, 0);
        panel(jq, q * NB, true);
        // right-hand sides of the panel's 64 rows: pending updates, then the solve; matrix columns: transposition
        u_rows_sym(jq, J, q * NB);
      }
      if (J + 4 * NB >= n_pad) break;
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 4 * NB, n_pad, J + 4 * NB, n_pad, J, 4 * NB, PK_GEMM, -1.0,
                         nullptr, 0, 0, 0, tri_map);
      if (rhs_gemv) launch_rhs_update(st, nb, nrhs, A, lda, sys_stride, Pw, ldp, p_stride, n_pad, J + 4 * NB, J, 4 * NB);
      else if (nrhs > 0)
        gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 4 * NB, n_pad, n_pad, n_cols, J, 4 * NB, PK_OTHER);
    }
  } else {
    // three-level schedule.  Group = four 64-column panels a, b | c, d (workspace columns 0, 64 | 128, 192):
    //   block E = (a, b): a: factor, interchanges, U row block; its K = 64 update goes only to the 64 columns panel b consists
    //      of; b: factor, interchanges (also on a's stored multipliers); only now - with the rows in their final order - a's
    //      update of the 64 rows of b's U block, then b's U row block.
    //   E's K = 128 update is applied only where block O needs it: O's 128 columns before O is factored (T1, all rows), and the
    //      64 U rows of c and of d right of O after the respective panel's interchanges (T2c; for d fused with c's own update
    //      of those rows into one K = 192 pass).
    //   block O = (c, d): the same as E, its interchanges also applied to E's multipliers in the workspace.
    //   ONE K = 256 update of everything below and right of the group with [L_a L_b L_c L_d] x [U_a; U_b; U_c; U_d]: the
    //   trailing matrix is read and written once per 256 columns instead of once per 128 (77 vs 65 TFLOP/s for the update
    //   itself: no C slices, C additions or tile stores in the second half of a tile's K loop).
    for (int J = 0; J < n_pad; J += 4 * NB) {
      panel(J, 0); swap_right(J); trsm(J, 0);
      if (J + NB >= n_pad) break;                        // odd tail: nothing below the panel, forward elimination done
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + NB, n_pad, J + NB, J + 2 * NB, J, NB, PK_OTHER, -1.0,
                         Pw + (size_t)NB * ldp, ldp, p_stride, 0);
      panel(J + NB, NB, true); swap_right(J + NB);
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + NB, J + 2 * NB, J + 2 * NB, n_cols, J, NB, PK_OTHER);
      trsm(J + NB, NB);
      if (J + 2 * NB >= n_pad) break;
      // T1: E's update of panel c's columns, ALL rows below E (the rows c's pivot search ranges over must be in one state);
      // the result goes straight into the workspace.  d's columns wait: they take E's and c's updates in one K = 192 pass.
      const int c_end = J + 3 * NB < n_pad ? J + 3 * NB : n_pad;
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 2 * NB, n_pad, J + 2 * NB, c_end, J, 2 * NB, PK_OTHER, -1.0,
                         Pw + (size_t)(2 * NB) * ldp, ldp, p_stride, 0);
      panel(J + 2 * NB, 2 * NB, true); swap_right(J + 2 * NB);
      // T2c: E's update of c's 64 U rows right of c - only now, after c's interchanges: rows that an interchange can exchange
      // must carry the same updates, and the rows below still wait for the K = 256 update
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 2 * NB, c_end, c_end, n_cols, J, 2 * NB, PK_OTHER);
      trsm(J + 2 * NB, 2 * NB);
      if (J + 3 * NB >= n_pad) break;
      // d's columns: E's and c's updates in one K = 192 pass, delivered into the workspace
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 3 * NB, n_pad, J + 3 * NB, J + 4 * NB, J, 3 * NB, PK_OTHER, -1.0,
                         Pw + (size_t)(3 * NB) * ldp, ldp, p_stride, 0);
      panel(J + 3 * NB, 3 * NB, true); swap_right(J + 3 * NB);
      // T2d and c's update of d's U rows in one K = 192 pass: [L_a L_b L_c] x [U_a; U_b; U_c]
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 3 * NB, J + 4 * NB, J + 4 * NB, n_cols, J, 3 * NB, PK_OTHER);
      trsm(J + 3 * NB, 3 * NB);
      gemm(st, nb, A, lda, sys_stride, Pw, ldp, p_stride, J + 4 * NB, n_pad, J + 4 * NB, n_cols, J, 4 * NB);
    }
  }
  if (symmetric) launch_growth_check(st, nb, n_pad, growth, d_info, growth_max);
  BIEM_LAUNCHCHK();
  if (gemm_rc != BIEM_OK) return gemm_rc;
  if (nrhs > 0) {
    ProfScope ps(PK_BACK, st, 4.0 * (double)nb * n_pad * (double)n_pad * nrhs);
    back_substitute_cols(st, nb, n_pad, nrhs, A, lda, sys_stride, A + n_pad, lda, sys_stride);
    BIEM_LAUNCHCHK();
  }
  return BIEM_OK;
}

}  // namespace biem
