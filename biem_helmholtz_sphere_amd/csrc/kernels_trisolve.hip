// kernels_trisolve.hip -- the triangular solves of the dense solver on gfx950: the column-form back substitution every fused path and
// both stored-factor solves run (back_substitute_cols), the solves with stored factors (launch_lu_solve, launch_sym_solve), k_rhs_update
// (the right-hand sides' share of a K = 256 update as matrix-vector work), the growth bookkeeping (described in dense.hpp) and k_zero_int.
#include "dense.hpp"

namespace biem {

unsigned long long* lu_growth_slots(void* d_work, int nb, int n_pad) { return dense_work(nb, n_pad, 0).growth_at(d_work); }
__global__ void k_growth_preset(int nb, unsigned long long* __restrict__ growth, double amax) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  growth[2 * s] = (unsigned long long)__double_as_longlong(amax);
  growth[2 * s + 1] = 0ULL;
}
int lu_growth_init(void* d_work, int nb, int n_pad, double amax, hipStream_t st) {
  if (nb <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_growth_preset, dim3((nb + 63) / 64), dim3(64), 0, st, nb, lu_growth_slots(d_work, nb, n_pad), amax);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}
__global__ void k_growth_check(int nb, int n_pad, const unsigned long long* __restrict__ growth, int* __restrict__ info, double limit) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  const double amax = __longlong_as_double((long long)growth[2 * s]), umax = __longlong_as_double((long long)growth[2 * s + 1]);
  if (!(umax <= limit * amax) && info[s] == 0) info[s] = -(n_pad + 1);
}
void launch_growth_check(hipStream_t st, int nb, int n_pad, const unsigned long long* growth, int* d_info, double limit) {
  hipLaunchKernelGGL(k_growth_check, dim3((nb + 63) / 64), dim3(64), 0, st, nb, n_pad, growth, d_info, limit);
}

__global__ void k_zero_int(int* p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}
void launch_zero_int(hipStream_t st, int* p, int n) { hipLaunchKernelGGL(k_zero_int, dim3((n + 63) / 64), dim3(64), 0, st, p, n); }

// ---------------------------------------------------------------------------------------------
// back substitution with U (row-major), block size BS
// ---------------------------------------------------------------------------------------------
// The right-hand sides are addressed as F[s * f_stride + row * ldf + q]: the augmented columns of the matrix itself
// (F = A + n_pad, ldf = lda, f_stride = sys_stride) in the fused solve, a separate array in biem_lu_solve.
// diagonal block: x = U[jr:jr+BS, jr:jr+BS]^{-1} y, one 64-thread workgroup per (system, rhs)
__global__ void __launch_bounds__(64) k_back_diag(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ F,
                                                   long long ldf, long long f_stride, int jr) {
  // the 64 x 64 block goes through LDS once (coalesced rows): read from global memory element by element inside the 64 dependent
  // steps it cost 24 us per block; one wave, so the steps need no barrier - x_c travels by a lane broadcast
  __shared__ cplx sU[BS][BS + 1];
  const int s = blockIdx.x, q = blockIdx.y, r = threadIdx.x;
  const cplx* Ub = A + (size_t)s * sys_stride + (size_t)jr * lda + jr;
  for (int rr = 0; rr < BS; ++rr) sU[rr][r] = Ub[(size_t)rr * lda + r];
  cplx* Fq = F + (size_t)s * f_stride + q;
  cplx y = Fq[(size_t)(jr + r) * ldf];
  __syncthreads();
  const cplx inv = crecip(sU[r][r]);           // every lane its own diagonal entry, once
  for (int c = BS - 1; c >= 0; --c) {
    const cplx t = cmul(y, inv);               // lane c holds x_c
    const cplx xc = make_double2(lane_bcast(t.x, c), lane_bcast(t.y, c));
    if (r == c) y = xc;
    if (r < c) y = cfnma(sU[r][c], xc, y);
  }
  Fq[(size_t)(jr + r) * ldf] = y;
}

// forward counterpart (stored factors, biem_lu_solve): the 64 interchanges of the panel at column j on the right-hand side, then
// y = L11^{-1} f with the unit-lower diagonal block; one 64-thread workgroup per (system, rhs)
__global__ void __launch_bounds__(64) k_fwd_diag(const cplx* __restrict__ A, long long lda, long long sys_stride, const int* __restrict__ ipiv,
                                                  int n_pad, cplx* __restrict__ F, long long ldf, long long f_stride, int j) {
  __shared__ cplx sx;
  const int s = blockIdx.x, q = blockIdx.y, r = threadIdx.x;
  cplx* Fq = F + (size_t)s * f_stride + q;
  if (r == 0) {
    for (int c = 0; c < NB; ++c) {
      const int p = ipiv[(size_t)s * n_pad + j + c];
      if (p != j + c) { const cplx a = Fq[(size_t)(j + c) * ldf], b = Fq[(size_t)p * ldf]; Fq[(size_t)(j + c) * ldf] = b; Fq[(size_t)p * ldf] = a; }
    }
  }
  __syncthreads();
  const cplx* Lrow = A + (size_t)s * sys_stride + (size_t)(j + r) * lda + j;
  cplx y = Fq[(size_t)(j + r) * ldf];
  for (int c = 0; c < NB - 1; ++c) {
    if (r == c) sx = y;
    __syncthreads();
    if (r > c) y = cfnma(Lrow[c], sx, y);
    __syncthreads();
  }
  Fq[(size_t)(j + r) * ldf] = y;
}

// rows [row_begin, row_end): y[i] -= M[i, jr:jr+64] . x[jr:jr+64]; one wave per row (back substitution: the rows above the
// solved block with M = U; forward substitution with stored factors: the rows below the panel with M = L)
// With `info` given (row form of the symmetric path) the pass also checks the entries it reads, u_ic of the strips right of the diagonal
// blocks: |u_ic|^2 <= inv_rel2 |u_ii|^2 (every multiplier l_ci = u_ic / u_ii within 1 / rel; NaN-safe) else info = -(first row of the
// 64-row panel + 1), and max |u_ii u_ic| into the growth slot.
__global__ void __launch_bounds__(256) k_back_update(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ F,
                                                      long long ldf, long long f_stride, int nrhs, int jr, int row_begin, int row_end,
                                                      int* __restrict__ info = nullptr, unsigned long long* __restrict__ growth = nullptr,
                                                      double inv_rel2 = 0.0) {
  // The 64 solution values are strided by ldf in memory (one cache line each): they are gathered ONCE per workgroup into LDS
  // instead of once per row
  __shared__ cplx sx[BS];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Fs = F + (size_t)s * f_stride;
  // this wave's rows of the block column: loaded once, used by the checks and by every right-hand side
  cplx u[BACK_ROWS / 4];
  const int i0 = row_begin + blockIdx.x * BACK_ROWS + wave * (BACK_ROWS / 4);
#pragma unroll
  for (int k = 0; k < BACK_ROWS / 4; ++k) u[k] = (i0 + k < row_end) ? As[(size_t)(i0 + k) * lda + jr + lane] : make_double2(0.0, 0.0);
  if (info != nullptr) {
    double um2 = 0.0;
    bool badm = false;
#pragma unroll
    for (int k = 0; k < BACK_ROWS / 4; ++k) {
      if (i0 + k >= row_end) break;
      const cplx d = As[(size_t)(i0 + k) * lda + i0 + k];
      const double m2 = u[k].x * u[k].x + u[k].y * u[k].y, d2 = d.x * d.x + d.y * d.y;
      if (!(m2 <= inv_rel2 * d2)) badm = true;
      um2 = nan_max(um2, m2 * d2);
    }
    block_max_publish(sqrt(um2), growth + 2 * (size_t)s + 1);
    if (badm && info[s] == 0) info[s] = -((i0 / NB) * NB + 1);
  }
  for (int q = 0; q < nrhs; ++q) {
    if (q > 0) __syncthreads();
    if (threadIdx.x < BS) sx[threadIdx.x] = Fs[(size_t)(jr + threadIdx.x) * ldf + q];
    __syncthreads();
    const cplx x = sx[lane];
#pragma unroll
    for (int k = 0; k < BACK_ROWS / 4; ++k) {
      const int i = i0 + k;
      if (i >= row_end) break;
      const cplx v = cmul(u[k], x);
      double vr = v.x, vi = v.y;
      for (int o = 32; o > 0; o >>= 1) { vr += __shfl_down(vr, o, 64); vi += __shfl_down(vi, o, 64); }
      if (lane == 0) {
        cplx* y = Fs + (size_t)i * ldf + q;
        cplx t = *y;
        t.x -= vr; t.y -= vi;
        *y = t;
      }
    }
  }
}

void back_substitute_cols(hipStream_t st, int nb, int n_pad, int nrhs, const cplx* A, long long lda, long long sys_stride, cplx* F,
                          long long ldf, long long f_stride, int* d_info, unsigned long long* growth, double inv_rel2) {
  for (int jr = n_pad - BS; jr >= 0; jr -= BS) {
    hipLaunchKernelGGL(k_back_diag, dim3(nb, nrhs), dim3(64), 0, st, A, lda, sys_stride, F, ldf, f_stride, jr);
    if (jr > 0) hipLaunchKernelGGL(k_back_update, dim3((jr + BACK_ROWS - 1) / BACK_ROWS, nb), dim3(256), 0, st, A, lda, sys_stride, F, ldf, f_stride,
                                   nrhs, jr, 0, jr, d_info, growth, inv_rel2);
  }
}

// rows below a group: f[i] -= L[i, 0:kd] y[jg : jg+kd]; a workgroup takes 64 rows, its four waves a quarter of the kd terms each
// (one thread per row over all kd terms left one system's update on n / 256 workgroups with 256 dependent loads per thread:
// 22 us per launch at N = 4064); the kd values of y in LDS
__global__ void __launch_bounds__(256) k_rhs_update(cplx* __restrict__ A, long long lda, long long sys_stride, const cplx* __restrict__ Pw,
                                                     long long ldp, long long p_stride, int n_pad, int row_begin, int jg, int kd) {
  __shared__ cplx sy[4 * NB];
  __shared__ cplx part[3][64];
  const int s = blockIdx.y, q = blockIdx.z;
  cplx* F = A + (size_t)s * sys_stride + n_pad + q;
  for (int k = threadIdx.x; k < kd; k += 256) sy[k] = F[(size_t)(jg + k) * lda];
  __syncthreads();
  const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
  const int i = row_begin + blockIdx.x * RHS_UPD_ROWS + lane, ic = i < n_pad ? i : n_pad - 1;
  const cplx* Pr = Pw + (size_t)s * p_stride + ic;
  const int k0 = (kd >> 2) * kq, k1 = kq == 3 ? kd : k0 + (kd >> 2);       // kd is a multiple of 4 here (64 .. 256)
  cplx a0 = make_double2(0.0, 0.0), a1 = a0, a2 = a0, a3 = a0;
  int k = k0;
  for (; k + 3 < k1; k += 4) {
    a0 = cfma(Pr[(size_t)k * ldp], sy[k], a0);
    a1 = cfma(Pr[(size_t)(k + 1) * ldp], sy[k + 1], a1);
    a2 = cfma(Pr[(size_t)(k + 2) * ldp], sy[k + 2], a2);
    a3 = cfma(Pr[(size_t)(k + 3) * ldp], sy[k + 3], a3);
  }
  for (; k < k1; ++k) a0 = cfma(Pr[(size_t)k * ldp], sy[k], a0);
  const cplx sum = make_double2((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y));
  if (kq > 0) part[kq - 1][lane] = sum;
  __syncthreads();
  if (kq == 0 && i < n_pad) {
    cplx f = F[(size_t)i * lda];
    f.x -= (sum.x + part[0][lane].x) + (part[1][lane].x + part[2][lane].x);
    f.y -= (sum.y + part[0][lane].y) + (part[1][lane].y + part[2][lane].y);
    F[(size_t)i * lda] = f;
  }
}
void launch_rhs_update(hipStream_t st, int nb, int nrhs, cplx* A, long long lda, long long sys_stride, const cplx* Pw, long long ldp,
                       long long p_stride, int n_pad, int row_begin, int jg, int kd) {
  ProfScope ps(PK_OTHER, st, 0.0);
  hipLaunchKernelGGL(k_rhs_update, dim3((n_pad - row_begin + RHS_UPD_ROWS - 1) / RHS_UPD_ROWS, nb, nrhs), dim3(256), 0, st, A, lda, sys_stride, Pw, ldp,
                     p_stride, n_pad, row_begin, jg, kd);
}

// ---------------------------------------------------------------------------------------------
// Solve with a stored U^T U factor (biem_sym_solve, biem_solve_factored): U^T y = f, then U x = y.  The fused path gets the forward
// elimination for free inside its trailing updates; a factor kept for later right-hand sides needs it on its own.  Per 64-row
// block j, top down:
//   k_fwd_utu_diag    y_j = U[j,j]^{-T} f_j (lower triangular): the block in LDS once per workgroup, one wave per right-hand side
//   k_fwd_utu_update  f[r] -= sum_{c in block j} U[c, r] y_c for every r right of the block: a 64-row strip of U, contiguous along r
//                     in the row-major factor.  TR columns per workgroup; each U element is loaded once, into registers, and used for
//                     every right-hand side (register tiles of FWD_NQ, the 64 rows c split over 256 / TR thread groups and summed in
//                     LDS in a fixed order, so two solves of the same data agree bit for bit).
// Launch form: TR = 64 when the step has enough 64-column tiles over all systems to fill the chip, else TR = 16 (four times the
// workgroups per system: one system alone spreads its strip over ~n_pad / 16 workgroups).  Back substitution: the column form of
// the fused path (k_back_diag + k_back_update, without the checks the factorisation already took).  4 n_pad / 64 launches in all.
// Each U element takes 8 nrhs flops per 16 bytes read: the update is bound by memory bandwidth below ~20 right-hand sides (78.6
// FP64 TFLOP/s over 8 TB/s) and by the VALU above.
// ---------------------------------------------------------------------------------------------
constexpr int FWD_RG = 4;          // right-hand sides per workgroup of the diagonal step (one per wave)
constexpr int FWD_NQ = 8;          // right-hand sides per register tile of the strip update
constexpr long long FWD_WIDE_MIN = 1024;   // workgroups of the TR = 64 form from which it is used (4 per CU)

__global__ void __launch_bounds__(256) k_fwd_utu_diag(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ F,
                                                       long long ldf, long long f_stride, int nrhs, int j) {
  __shared__ cplx sU[NB][NB + 1];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const cplx* Ub = A + (size_t)s * sys_stride + (size_t)j * lda + j;
  for (int e = threadIdx.x; e < NB * NB; e += 256) { const int r = e >> 6, c = e & 63; if (c >= r) sU[r][c] = Ub[(size_t)r * lda + c]; }
  __syncthreads();
  const int q = blockIdx.y * FWD_RG + wave;
  if (q >= nrhs) return;
  cplx* Fq = F + (size_t)s * f_stride + (size_t)j * ldf + q;
  cplx y = Fq[(size_t)lane * ldf];
  const cplx inv = crecip(sU[lane][lane]);
  // (U^T)[r][c] = u_cr: x_c = y_c / u_cc, then every row r > c takes u_cr x_c off (one wave: x_c travels by a lane broadcast)
  for (int c = 0; c < NB; ++c) {
    const cplx t = cmul(y, inv);
    const cplx xc = make_double2(lane_bcast(t.x, c), lane_bcast(t.y, c));
    if (lane == c) y = xc;
    if (lane > c) y = cfnma(sU[c][lane], xc, y);
  }
  Fq[(size_t)lane * ldf] = y;
}

template <int TR>
__global__ void __launch_bounds__(256) k_fwd_utu_update(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ F,
                                                         long long ldf, long long f_stride, int nrhs, int j, int n_pad) {
  constexpr int KG = 256 / TR;       // thread groups over the 64 rows c of the strip
  constexpr int KR = NB / KG;        // rows c per group
  __shared__ cplx sy[NB][FWD_NQ];
  __shared__ cplx sred[KG][FWD_NQ][TR + 1];
  const int s = blockIdx.y, t = threadIdx.x, col = t % TR, kg = t / TR;
  const int r0 = j + NB + blockIdx.x * TR;
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Fs = F + (size_t)s * f_stride;
  cplx u[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) u[k] = r0 + col < n_pad ? As[(size_t)(j + kg * KR + k) * lda + r0 + col] : make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < nrhs; q0 += FWD_NQ) {
    const int nq = nrhs - q0 < FWD_NQ ? nrhs - q0 : FWD_NQ;
    if (q0 > 0) __syncthreads();                  // the previous tile's sums have been read
    for (int e = t; e < NB * FWD_NQ; e += 256) {
      const int c = e / FWD_NQ, q = e % FWD_NQ;
      sy[c][q] = q < nq ? Fs[(size_t)(j + c) * ldf + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    cplx acc[FWD_NQ];
#pragma unroll
    for (int q = 0; q < FWD_NQ; ++q) acc[q] = make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < KR; ++k)
#pragma unroll
      for (int q = 0; q < FWD_NQ; ++q) acc[q] = cfma(u[k], sy[kg * KR + k][q], acc[q]);
#pragma unroll
    for (int q = 0; q < FWD_NQ; ++q) sred[kg][q][col] = acc[q];
    __syncthreads();
    // consecutive threads take consecutive right-hand sides of one row: the stores run along the row of F
    for (int o = t; o < TR * FWD_NQ; o += 256) {
      const int q = o % FWD_NQ, cc = o / FWD_NQ, r = r0 + cc;
      if (q >= nq || r >= n_pad) continue;
      cplx sum = sred[0][q][cc];
#pragma unroll
      for (int g = 1; g < KG; ++g) sum = cadd(sum, sred[g][q][cc]);
      cplx* y = Fs + (size_t)r * ldf + q0 + q;
      *y = csub(*y, sum);
    }
  }
}

int launch_sym_solve(int nb, int n_pad, int nrhs, const double* d_U, long long lda, long long sys_stride, double* d_B, long long ldb,
                     long long b_stride, hipStream_t st) {
  if (n_pad <= 0 || n_pad % NB) { set_error("biem_sym_solve: n_pad=%d is not a positive multiple of %d (use biem_lu_npad)", n_pad, NB); return BIEM_ERR_ARG; }
  if (lda < n_pad || ldb < nrhs) { set_error("biem_sym_solve: lda < n_pad or ldb < nrhs"); return BIEM_ERR_ARG; }
  if (nb < 0 || nrhs < 0 || nb > 65535 || nrhs > 65535) {
    set_error("biem_sym_solve: 0 .. 65535 systems / right-hand sides per call (got %d / %d)", nb, nrhs);
    return BIEM_ERR_ARG;
  }
  if (nb == 0 || nrhs == 0) return BIEM_OK;
  const cplx* A = (const cplx*)d_U;
  cplx* F = (cplx*)d_B;
  {
    ProfScope ps(PK_TRSM, st, 4.0 * (double)nb * n_pad * (double)n_pad * nrhs);
    for (int j = 0; j < n_pad; j += NB) {
      hipLaunchKernelGGL(k_fwd_utu_diag, dim3(nb, (nrhs + FWD_RG - 1) / FWD_RG), dim3(256), 0, st, A, lda, sys_stride, F, ldb, b_stride, nrhs, j);
      const int rem = n_pad - (j + NB);
      if (rem <= 0) continue;
      if ((long long)nb * ((rem + 63) / 64) >= FWD_WIDE_MIN)
        hipLaunchKernelGGL(k_fwd_utu_update<64>, dim3((rem + 63) / 64, nb), dim3(256), 0, st, A, lda, sys_stride, F, ldb, b_stride, nrhs, j, n_pad);
      else
        hipLaunchKernelGGL(k_fwd_utu_update<16>, dim3((rem + 15) / 16, nb), dim3(256), 0, st, A, lda, sys_stride, F, ldb, b_stride, nrhs, j, n_pad);
    }
  }
  {
    ProfScope ps(PK_BACK, st, 4.0 * (double)nb * n_pad * (double)n_pad * nrhs);
    back_substitute_cols(st, nb, n_pad, nrhs, A, lda, sys_stride, F, ldb, b_stride);
  }
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// Solve with the stored factors of launch_lu_factor_solve(keep_multipliers = true): the multipliers of a panel are stored in the
// row order its own 64 interchanges left (later panels' interchanges are not applied to them), so the forward substitution
// interleaves interchanges and eliminations panel by panel; L D L^T factors are the case ipiv = identity, U = D L^T.
int launch_lu_solve(int nb, int n_pad, int nrhs, const double* d_LU, long long lda, long long sys_stride, const int* d_ipiv, double* d_B,
                    long long ldb, long long b_stride, hipStream_t st) {
  if (nb <= 0 || n_pad <= 0 || nrhs <= 0) return BIEM_OK;
  if (n_pad % NB) { set_error("biem_lu_solve: n_pad=%d is not a multiple of %d (use biem_lu_npad)", n_pad, NB); return BIEM_ERR_ARG; }
  if (lda < n_pad || ldb < nrhs) { set_error("biem_lu_solve: lda < n_pad or ldb < nrhs"); return BIEM_ERR_ARG; }
  if (nb > 65535 || nrhs > 65535) { set_error("biem_lu_solve: at most 65535 systems / right-hand sides per call (got %d / %d)", nb, nrhs); return BIEM_ERR_ARG; }
  const cplx* A = (const cplx*)d_LU;
  cplx* F = (cplx*)d_B;
  for (int j = 0; j < n_pad; j += NB) {
    hipLaunchKernelGGL(k_fwd_diag, dim3(nb, nrhs), dim3(64), 0, st, A, lda, sys_stride, d_ipiv, n_pad, F, ldb, b_stride, j);
    const int below = n_pad - (j + NB);
    if (below > 0)
      hipLaunchKernelGGL(k_back_update, dim3((below + BACK_ROWS - 1) / BACK_ROWS, nb), dim3(256), 0, st, A, lda, sys_stride, F, ldb, b_stride,
                         nrhs, j, j + NB, n_pad);
  }
  back_substitute_cols(st, nb, n_pad, nrhs, A, lda, sys_stride, F, ldb, b_stride);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
