// kernels_sym.hip -- symmetric path in ROW form (what biem_solve_ldlt runs):  A = U^T U  with U = D^{1/2} L^T upper triangular, the complex-symmetric
// analogue of the Cholesky factorisation (no conjugation, principal complex square roots of the pivots; same pivots, same
// multipliers l_ci = u_ic / u_ii and same acceptance test as the L D L^T form it replaces).  Why this form: with A = U^T U the
// trailing update  A22 -= U12^T U12  takes BOTH zgemm operands from the same 64-row strip of the row-major matrix
// (A-operand[k][i] = U12[k][row i], B-operand[k][c] = U12[k][col c]), which is also exactly what the back substitution reads.
// So the factorisation works in place on the upper triangle: no column-major panel workspace, no transposing panel load / store,
// no transposed GEMM epilogue, no separate "U rows from L" pass - a panel is two passes over its strip instead of about six.
//   k_diag_utu_reg (one workgroup per system, defined with the small-system kernel below; k_diag_utu_blk: four pivots per barrier): the 64 x 64 diagonal block: pivots d,
//               U11 = D^{-1/2} (D L11^T), V = -U11^{-T} (and W = I + V where the back substitution keeps it), multiplier test inside the block
//   strip:      U12 = U11^{-T} A12 = -V^T A12 in place on the streaming zgemm's product form (k_gemm3m_strip, K = 64, B operand = the
//               strip's own rows, V = -U11^{-T}: C is neither loaded nor added).  More than 8 right-hand sides are columns of the
//               strip: forward elimination rides along; up to 8 live in the compact copy Y[s][q][row] - the diagonal-block kernel
//               solves its 64 entries, the strip's epilogue subtracts every tile's term from the 64 entries under it.  A one-thread-
//               per-column VALU form with the triangle of U11^{-T} from the scalar cache or LDS was 5x slower (292 vs 53 ms per 256 systems)
//   checks:     multiplier test |u_ic| <= 100 |u_ii| and growth max |u_ii u_ic| of the strip entries are taken where the entries
//               are read anyway: in the back substitution
//   back:       row form (large batches): ONE launch per group of up to 8 right-hand sides, the system's workgroup walks the block rows
//               bottom up (k_back_sweep; BIEM_BACK_ROW=blocks: one launch per block row, k_back_row); few systems: the column form
//               (k_back_update, kernels_trisolve.hip) or the stored inverses (k_back_step)
//   in-group:   the next panel's 64 rows take the group's pending updates (K = 64 q) for all columns right of them
//   stacked:    under the left-looking bulk update the in-group pass and the strip of the panels b, c, d are ONE pure product over
//               K = 64 (q + 1) (k_sym_slab, k_gemm3m_stack<KD>; the diagonal tile alone takes the pending update first)
//   K = 256:    one update of the UPPER triangle of tiles below the group (TileGrid.tri = 2), more than 8 right-hand sides as tile columns
// Only the upper triangle and the diagonal 64 x 64 tiles of A are read.  Growth check as in the L D L^T form, with moduli:
// max |d_i l_ci| = max |u_ii u_ic| against max |a_ij| over the part read.
// Large batches take the bulk update left-looking: launch_gemm_left before a group instead of the K = 256 update after it (sym_update_left).
// The update kernels are kernels_gemm3m.hip's; the column-form back substitution is kernels_trisolve.hip's.
#include "dense.hpp"

namespace biem {

__global__ void __launch_bounds__(256) k_absmax_upper(const cplx* __restrict__ A, long long lda, long long sys_stride, int n_pad,
                                                       unsigned long long* __restrict__ growth) {
  const int s = blockIdx.y;
  const cplx* As = A + (size_t)s * sys_stride;
  double m = 0.0;
  for (int r = 0; r < 8; ++r) {
    const int i = blockIdx.x * 8 + r;
    if (i >= n_pad) break;
    for (int c = (i / NB) * NB + threadIdx.x; c < n_pad; c += 256) { const cplx v = As[(size_t)i * lda + c]; m = nan_max(m, sqrt(v.x * v.x + v.y * v.y)); }
  }
  block_max_publish(m, growth + 2 * (size_t)s);
}

// Back substitution of the row form as one launch per 64-row block (bottom up; BIEM_BACK_ROW=blocks - production runs the one-launch
// k_back_sweep below, whose iterations are this kernel), one 1024-thread workgroup per system:
//   y_R -= U[R, C] x_C over all solved columns C right of the block - the 16 waves stream 4 rows each across the strip, 64 columns
//   per step, partial sums per lane and ONE reduction per row at the end - then the 64 x 64 triangular solve U[R,R] x_R = y_R in
//   the same launch (diagonal block in LDS, one wave).  Reads U exactly once in long contiguous runs (the column-block form
//   k_back_update re-launches per 64 columns with 16-KiB workgroups: 31 vs 84 GB / 5 TB/s = 17 ms per 256 systems at cfg 3).
// The pass also takes the checks of the strip entries (see k_back_update).  NQ right-hand sides per pass.
template <int NQ>
__global__ void __launch_bounds__(1024) k_back_row(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ Y,
                                                    int nrhs, int n_pad, int q0, int nq, int ib, int do_checks,
                                                    int* __restrict__ info, unsigned long long* __restrict__ growth, double inv_rel2) {
  // Y[s][q][row]: the right-hand sides / solutions in a compact copy (in the augmented matrix they sit one row stride apart:
  // gathering 64 of them per step from there cost more than the four 1-KiB row loads they are multiplied with)
  __shared__ cplx sU[NB][NB + 1];
  __shared__ cplx sy[NB][NQ];
  __shared__ double sm_max2[16];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Ys = Y + (size_t)s * nrhs * n_pad;
  const int rb = ib * NB;
  for (int e = tid; e < NB * NB; e += 1024) { const int r = e >> 6, c = e & 63; sU[r][c] = As[(size_t)(rb + r) * lda + rb + c]; }
  cplx acc[4][NQ];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[k][q] = make_double2(0.0, 0.0);
  double d2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { const cplx d = As[(size_t)(rb + 4 * wave + k) * lda + rb + 4 * wave + k]; d2[k] = d.x * d.x + d.y * d.y; }
  double um2 = 0.0;
  bool badm = false;
  const cplx* Ur = As + (size_t)(rb + 4 * wave) * lda + lane;
#pragma unroll 2
  for (int c0 = rb + NB; c0 < n_pad; c0 += NB) {
    cplx x[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) x[q] = q < nq ? Ys[(size_t)(q0 + q) * n_pad + c0 + lane] : make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const cplx u = Ur[(size_t)k * lda + c0];
      if (do_checks) {
        const double m2 = u.x * u.x + u.y * u.y;
        if (!(m2 <= inv_rel2 * d2[k])) badm = true;
        um2 = nan_max(um2, m2 * d2[k]);
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[k][q] = cfma(u, x[q], acc[k][q]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double vr = acc[k][q].x, vi = acc[k][q].y;
      for (int o = 32; o > 0; o >>= 1) { vr += __shfl_down(vr, o, 64); vi += __shfl_down(vi, o, 64); }
      if (lane == 0) {
        cplx y = q < nq ? Ys[(size_t)(q0 + q) * n_pad + rb + 4 * wave + k] : make_double2(0.0, 0.0);
        y.x -= vr; y.y -= vi;
        sy[4 * wave + k][q] = y;
      }
    }
  if (do_checks) {
    double m = sqrt(um2);
    for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_down(m, o, 64));
    if (lane == 0) sm_max2[wave] = m;
    if (badm && info[s] == 0) info[s] = -(rb + 1);
  }
  __syncthreads();
  if (do_checks && tid == 0) {
    double m = sm_max2[0];
    for (int w = 1; w < 16; ++w) m = nan_max(m, sm_max2[w]);
    unsigned long long* dst = growth + 2 * (size_t)s + 1;
    if (!(m <= __longlong_as_double((long long)*(volatile unsigned long long*)dst))) atomicMax(dst, (unsigned long long)__double_as_longlong(m));
  }
  if (wave == 0) {            // the triangular solve of the block: lane = row, wave-synchronous
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q >= nq) break;
      cplx y = sy[lane][q];
      for (int c = NB - 1; c >= 0; --c) {
        if (lane == c) y = cmul(y, crecip(sU[c][c]));
        const double xr = lane_bcast(y.x, c), xi = lane_bcast(y.y, c);
        if (lane < c) y = cfnma(sU[lane][c], make_double2(xr, xi), y);
      }
      Ys[(size_t)(q0 + q) * n_pad + rb + lane] = y;
    }
  }
}

// The same back substitution as ONE launch per group of right-hand sides: the system's workgroup walks its block rows bottom up itself,
// every iteration the arithmetic of one k_back_row launch in the same order (same lane-to-row/column mapping, per-lane sums over c0
// ascending, same shuffle reduction, same wave-0 solve), so X, info and the growth slot come out bit for bit as from the per-block
// launches (BIEM_BACK_ROW=blocks).  What the per-block launches wait for and this kernel does not: the launch boundary, and the loads
// that do not depend on x - while wave 0 solves block ib, block ib - 1's diagonal block (four registers per lane, then the second sU
// buffer; |d|^2 is read from there) and, with up to two accumulators per row, the c0 = rb + 64 entries of its strip are already in
// flight.  x stays in Y (global): the
// barrier behind the solve orders its stores before the next block row's loads (one workgroup, one CU, one L1).  The multiplier verdict
// and the growth maximum are kept per thread and published once at the end: the bottom-most offending block row is the smallest code,
// the maximum is order-free.  Every workgroup touches its own system only, every loop is bounded by n_pad.
// NQ = 8 walks the strip twice with four accumulators per row (128 VGPRs per lane is all a 1024-thread workgroup has; k_back_row<8>
// spills 440 of them): each sum keeps its order.
// one 64-column step of a wave's four rows; sd: the wave's first diagonal entry in the LDS copy of the block (wide instantiations read
// |d|^2 from there instead of keeping it in registers)
template <int NA>
__device__ __forceinline__ void sweep_step(const cplx (&u)[4], const cplx (&x)[NA], cplx (&acc)[4][NA], const double (&d2)[4], const cplx* sd,
                                           bool chk, double inv_rel2, bool& badm, double& um2) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (chk) {
      double dd = d2[k];
      if (NA > 2) { const cplx d = sd[k * (NB + 2)]; dd = d.x * d.x + d.y * d.y; }
      const double m2 = u[k].x * u[k].x + u[k].y * u[k].y;
      if (!(m2 <= inv_rel2 * dd)) badm = true;
      um2 = nan_max(um2, m2 * dd);
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[k][q] = cfma(u[k], x[q], acc[k][q]);
  }
}
constexpr int SWEEP_SU = NB * (NB + 1);                 // one padded diagonal block, in complex
static size_t sweep_lds(int nq) { return (size_t)(2 * SWEEP_SU + NB * nq + 16) * sizeof(cplx); }
template <int NQ>
__global__ void __launch_bounds__(1024) k_back_sweep(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ Y,
                                                      int nrhs, int n_pad, int q0, int nq, int do_checks,
                                                      int* __restrict__ info, unsigned long long* __restrict__ growth, double inv_rel2) {
  constexpr int NA = NQ > 4 ? 4 : NQ, NPASS = NQ / NA;   // accumulators per row and passes over the strip
  constexpr bool PRE = NA <= 2;                          // the strip's first entries ride in registers across the solve
  constexpr bool YPRE = NA <= 2;
  extern __shared__ cplx sw[];
  cplx* const sy = sw + 2 * SWEEP_SU;                    // [NB][NQ]
  double* const sm_max2 = (double*)(sy + NB * NQ);       // [16]
  int* const s_code = (int*)(sm_max2 + 16);
  // (the wave index as a scalar: the row addresses of the strip and of the block loads stay in SGPRs)
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Ys = Y + (size_t)s * nrhs * n_pad;
  double d2[4];
  cplx upre[4];
  {
    const int rb = n_pad - NB;
    for (int e = tid; e < NB * NB; e += 1024) { const int r = e >> 6, c = e & 63; sw[r * (NB + 1) + c] = As[(size_t)(rb + r) * lda + rb + c]; }
    if (tid == 0) *s_code = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const cplx d = sw[(4 * wave + k) * (NB + 2)];
      d2[k] = d.x * d.x + d.y * d.y;
      upre[k] = make_double2(0.0, 0.0);
    }
  }
  double um2 = 0.0;
  int code = 0;
  int cur = 0;
  for (int ib = n_pad / NB - 1; ib >= 0; --ib) {
    const int rb = ib * NB;
    const cplx* sU = sw + cur * SWEEP_SU;
    const cplx* sd = sU + 4 * wave * (NB + 2);
    const cplx* Ur = As + (size_t)(rb + 4 * wave) * lda + lane;
    bool badm = false;
#pragma unroll
    for (int h = 0; h < NPASS; ++h) {
      const int qh = h * NA;
      cplx acc[4][NA];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[k][q] = make_double2(0.0, 0.0);
      const bool chk = do_checks && h == 0;
      int c0 = rb + NB;
      if (PRE && h == 0 && c0 < n_pad) {         // the entries that came in while the block below was solved
        cplx x[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) x[q] = q < nq ? Ys[(size_t)(q0 + q) * n_pad + c0 + lane] : make_double2(0.0, 0.0);
        sweep_step<NA>(upre, x, acc, d2, sd, chk, inv_rel2, badm, um2);
        c0 += NB;
      }
#pragma unroll NA <= 2 ? 2 : 1
      for (; c0 < n_pad; c0 += NB) {
        cplx x[NA], u[4];
#pragma unroll
        for (int q = 0; q < NA; ++q) x[q] = qh + q < nq ? Ys[(size_t)(q0 + qh + q) * n_pad + c0 + lane] : make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = Ur[(size_t)k * lda + c0];
        sweep_step<NA>(u, x, acc, d2, sd, chk, inv_rel2, badm, um2);
      }
      // (narrow instantiations fetch the rows' y in one go, every lane the same address, instead of one dependent load per row)
      cplx yv[YPRE ? 4 : 1][YPRE ? NA : 1];
      if (YPRE) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int q = 0; q < NA; ++q) yv[k][q] = q < nq ? Ys[(size_t)(q0 + q) * n_pad + rb + 4 * wave + k] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < NA; ++q) {
          double vr = acc[k][q].x, vi = acc[k][q].y;
          for (int o = 32; o > 0; o >>= 1) { vr += __shfl_down(vr, o, 64); vi += __shfl_down(vi, o, 64); }
          if (lane == 0) {
            cplx y;
            if (YPRE) y = yv[k][q];
            else y = qh + q < nq ? Ys[(size_t)(q0 + qh + q) * n_pad + rb + 4 * wave + k] : make_double2(0.0, 0.0);
            y.x -= vr; y.y -= vi;
            sy[(4 * wave + k) * NQ + qh + q] = y;
          }
        }
    }
    if (badm && code == 0) code = -(rb + 1);
    __syncthreads();            // sy and this block's sU are complete
    // the next block row's loads that do not wait for x: issued now, in flight while wave 0 solves
    // (the top block row loads its own block once more instead of branching: unconditional loads stay in registers)
    const int rbn = ib > 0 ? rb - NB : rb, cpre = ib > 0 ? rb : 0;
    const cplx* Tn = As + (size_t)(rbn + wave) * lda + rbn + lane;       // (entry tid + 1024 x of the block: row wave + 16 x, column lane)
    const cplx t0 = Tn[0], t1 = Tn[(size_t)16 * lda], t2 = Tn[(size_t)32 * lda], t3 = Tn[(size_t)48 * lda];
    if (PRE) {
#pragma unroll
      for (int k = 0; k < 4; ++k) upre[k] = As[(size_t)(rbn + 4 * wave + k) * lda + cpre + lane];
    }
    if (wave == 0) {            // the triangular solve of the block: lane = row, wave-synchronous
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q >= nq) break;
        cplx y = sy[lane * NQ + q];
#pragma unroll NA <= 2 ? 8 : 2
        for (int c = NB - 1; c >= 0; --c) {
          if (lane == c) y = cmul(y, crecip(sU[c * (NB + 1) + c]));
          const double xr = lane_bcast(y.x, c), xi = lane_bcast(y.y, c);
          if (lane < c) y = cfnma(sU[lane * (NB + 1) + c], make_double2(xr, xi), y);
        }
        Ys[(size_t)(q0 + q) * n_pad + rb + lane] = y;
      }
    }
    cur ^= 1;
    cplx* sN = sw + cur * SWEEP_SU;
    cplx* Sn = sN + wave * (NB + 1) + lane;
    Sn[0] = t0; Sn[16 * (NB + 1)] = t1; Sn[32 * (NB + 1)] = t2; Sn[48 * (NB + 1)] = t3;
    __syncthreads();            // x of this block is stored, sy is free again, the next diagonal block is in LDS
    if (NA <= 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const cplx d = sN[(4 * wave + k) * (NB + 2)]; d2[k] = d.x * d.x + d.y * d.y; }
    }
  }
  if (!do_checks) return;
  if (code != 0) atomicMin(s_code, code);
  double m = sqrt(um2);
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_down(m, o, 64));
  if (lane == 0) sm_max2[wave] = m;
  __syncthreads();
  if (tid == 0) {
    m = sm_max2[0];
    for (int w = 1; w < 16; ++w) m = nan_max(m, sm_max2[w]);
    unsigned long long* dst = growth + 2 * (size_t)s + 1;
    if (!(m <= __longlong_as_double((long long)*(volatile unsigned long long*)dst))) atomicMax(dst, (unsigned long long)__double_as_longlong(m));
    if (*s_code != 0 && info[s] == 0) info[s] = *s_code;
  }
}

// Zeroes `width` complex columns from A on, in `rows` rows of lda complex (the right-hand-side columns of every row of every system of
// a chunk, whose systems lie one behind the other): one 16-byte store per thread, consecutive threads on consecutive entries of a row segment
__global__ void __launch_bounds__(256) k_clear_cols(cplx* __restrict__ A, long long lda, int width, long long rows) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long r = t / width;
  if (r >= rows) return;
  A[r * lda + (t - r * width)] = make_double2(0.0, 0.0);
}
void launch_clear_cols(hipStream_t st, double* d_A, long long lda, int width, long long rows) {
  if (width <= 0 || rows <= 0) return;
  const long long n = rows * width;
  hipLaunchKernelGGL(k_clear_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (cplx*)d_A, lda, width, rows);
}

// right-hand-side columns of the augmented matrix <-> compact Y[s][q][row]
__global__ void __launch_bounds__(256) k_rhs_compact(cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ Y, int nrhs,
                                                      int n_pad, int to_matrix) {
  const int s = blockIdx.z, q = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_pad) return;
  cplx* f = A + (size_t)s * sys_stride + (size_t)r * lda + n_pad + q;
  cplx* y = Y + ((size_t)s * nrhs + q) * n_pad + r;
  if (to_matrix) *f = *y; else *y = *f;
}

// One block step of the back substitution with the STORED inverses of the diagonal blocks (few systems per call: the chain of
// 2 n / 64 dependent launches is what one system per call waits for).  The factorisation keeps W_b = I - U_bb^{-T} of every panel
// (stored [k][i] = delta_ki - (U_bb^{-1})[k][i]), so  x_b = U_bb^{-1} y_b = y_b - sum_{i >= k} W_b[k][i] y_i  is a 64 x 64 product that
// every workgroup of the update forms for itself - no 64-step triangular solve (k_back_diag: 12 us) and one launch per block instead
// of two.  y_b must not be overwritten while other workgroups read it: the solution goes to X[(s nrhs + q) n_pad + row] and is copied
// back at the end (k_rhs_compact).  The update of the rows above (and the checks of the entries it reads) is k_back_update's.
__global__ void __launch_bounds__(256) k_back_step(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ F,
                                                    long long ldf, long long f_stride, const cplx* __restrict__ Wall, long long w_stride,
                                                    cplx* __restrict__ X, int n_pad, int nrhs, int jr, int* __restrict__ info,
                                                    unsigned long long* __restrict__ growth, double inv_rel2) {
  __shared__ cplx sx[BS], syb[BS];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const cplx* As = A + (size_t)s * sys_stride;
  cplx* Fs = F + (size_t)s * f_stride;
  const cplx* Wb = Wall + (size_t)s * w_stride + (size_t)(jr / NB) * NB * NB;
  cplx u[BACK_ROWS / 4];
  const int i0 = blockIdx.x * BACK_ROWS + wave * (BACK_ROWS / 4);
#pragma unroll
  for (int k = 0; k < BACK_ROWS / 4; ++k) u[k] = (i0 + k < jr) ? As[(size_t)(i0 + k) * lda + jr + lane] : make_double2(0.0, 0.0);
  // this wave's 16 rows of W_b (lanes along i): loaded once, used by every right-hand side
  cplx wr[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) { const int k = wave * 16 + kk; wr[kk] = lane >= k ? Wb[k * NB + lane] : make_double2(0.0, 0.0); }
  // (all loads of the prologue are issued together: the right-hand side's block, the diagonal entries of the checks)
  cplx ynext = threadIdx.x < BS ? Fs[(size_t)(jr + threadIdx.x) * ldf] : make_double2(0.0, 0.0);
  cplx dg[BACK_ROWS / 4];
#pragma unroll
  for (int k = 0; k < BACK_ROWS / 4; ++k) dg[k] = (i0 + k < jr) ? As[(size_t)(i0 + k) * lda + i0 + k] : make_double2(1.0, 0.0);
  for (int q = 0; q < nrhs; ++q) {
    __syncthreads();
    if (threadIdx.x < BS) syb[threadIdx.x] = ynext;
    if (q + 1 < nrhs && threadIdx.x < BS) ynext = Fs[(size_t)(jr + threadIdx.x) * ldf + q + 1];
    __syncthreads();
    const cplx yl = syb[lane];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const cplx v = cmul(wr[kk], yl);
      double vr = v.x, vi = v.y;
      for (int o = 32; o > 0; o >>= 1) { vr += __shfl_down(vr, o, 64); vi += __shfl_down(vi, o, 64); }
      if (lane == 0) { const int k = wave * 16 + kk; sx[k] = make_double2(syb[k].x - vr, syb[k].y - vi); }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < BS) X[((size_t)s * nrhs + q) * n_pad + jr + threadIdx.x] = sx[threadIdx.x];
    const cplx x = sx[lane];
#pragma unroll
    for (int k = 0; k < BACK_ROWS / 4; ++k) {
      const int i = i0 + k;
      if (i >= jr) break;
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
  {   // the checks of the entries this workgroup read, behind the arithmetic the next launch waits for
    double um2 = 0.0;
    bool badm = false;
#pragma unroll
    for (int k = 0; k < BACK_ROWS / 4; ++k) {
      if (i0 + k >= jr) break;
      const double m2 = u[k].x * u[k].x + u[k].y * u[k].y, d2 = dg[k].x * dg[k].x + dg[k].y * dg[k].y;
      if (!(m2 <= inv_rel2 * d2)) badm = true;
      um2 = nan_max(um2, m2 * d2);
    }
    block_max_publish(sqrt(um2), growth + 2 * (size_t)s + 1);
    if (badm && info[s] == 0) info[s] = -((i0 / NB) * NB + 1);
  }
}

// ---------------------------------------------------------------------------------------------
// Small systems (cfg 1: N = 72): the whole augmented system in LDS, one workgroup per system, ONE launch for factorisation,
// forward elimination, checks and back substitution - the blocked path above spends its time in per-panel launches there
// (4096 systems of N = 72: 5.2 of 6.8 ms in diagonal-block kernels that run one 64 x 64 block per workgroup).
// Same factorisation A = U^T U on the upper triangle (rows n .. of an identity-padded system are skipped), same acceptance tests
// and info codes; U is written back to the upper triangle.  n <= 128 rows, nrhs <= 8 and n + nrhs <= 128 (two 64-column lane slots; packed upper triangle of LDS).
// ---------------------------------------------------------------------------------------------
// 1 / d on the critical path of an elimination step: hardware reciprocal estimate + two Newton steps (4 FMAs) instead of the
// IEEE division sequence (~12 dependent instructions); relative error ~1e-16 for normal d
__device__ inline double fast_recip(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
constexpr int SMALL_N_MAX = 128;           // and n + nrhs <= 128 (two 64-column lane slots), packed store within the LDS
constexpr int SMALL_RHS_MAX = 8;
constexpr int SMALL_THREADS = 512;
// LDS of k_small_utu: packed upper triangle with the right-hand sides appended to each row, then 1/a_cc and 1/sqrt(a_cc) per row
// and two rows of multipliers
static inline size_t small_utu_lds(int n, int nrhs) { return ((size_t)n * (n + 1) / 2 + (size_t)n * nrhs + 4 * (size_t)n) * sizeof(cplx); }
// The matrix lives in registers during the elimination: wave w owns rows w, w + 8, ... (KR of them), lane l columns l and l + 64
// (TWO); a finished row (row c + 1 after step c) is published once to the packed LDS store, which the other waves read it from
// and which the back substitution and the write-back then use.  One barrier per step, no read-modify-write through LDS.
template <int KR, bool TWO>
__global__ void __launch_bounds__(SMALL_THREADS, (KR <= 9 ? 4 : 2)) k_small_utu(cplx* __restrict__ A, long long lda, long long sys_stride, int n, int n_pad, int nrhs,
                                                              int* __restrict__ info, unsigned long long* __restrict__ growth, double rel, int amax_ready) {
  // row r of the packed store: columns r .. n-1 of the matrix, then the nrhs right-hand sides; element (r, c) at off(r) + c, nc = n + nrhs
  extern __shared__ cplx sa[];
  __shared__ int bad_row;
  constexpr int NW = SMALL_THREADS / 64;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nc = n + nrhs;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar: the row tests below become scalar branches
  auto off = [&](int r) { return r * nc - (r * (r - 1)) / 2 - r; };
  cplx* ipiv = sa + (size_t)n * (n + 1) / 2 + (size_t)n * nrhs;            // 1 / a_cc
  cplx* isq = ipiv + n;                                                     // 1 / sqrt(a_cc)
  cplx* lrow = isq + n;                                                     // [2][n]: the multipliers a_cj / a_cc of the current row
  cplx* As = A + (size_t)s * sys_stride;
  if (tid == 0) bad_row = -1;
  const int j0 = lane, j1 = lane + 64;
  const long long g0 = j0 < n ? j0 : n_pad + (j0 - n), g1 = j1 < n ? j1 : n_pad + (j1 - n);     // global columns of the two slots
  cplx a0[KR], a1[KR];
  double am = 0.0;                               // (squares; the root is taken once)
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int i = w + NW * k;
    a0[k] = a1[k] = make_double2(0.0, 0.0);
    if (i < n) {
      const cplx* src = As + (size_t)i * lda;
      if (j0 >= i && j0 < nc) { a0[k] = src[g0]; if (j0 < n) am = nan_max(am, a0[k].x * a0[k].x + a0[k].y * a0[k].y); }
      if (TWO && j1 >= i && j1 < nc) { a1[k] = src[g1]; if (j1 < n) am = nan_max(am, a1[k].x * a1[k].x + a1[k].y * a1[k].y); }
    }
  }
  // A finished row i: its wave publishes it (packed store), 1 / a_ii (ipiv) and the multipliers a_ij / a_ii (lrow[i & 1]);
  // the reciprocal is computed here ONCE per row (plain 1 / |d|^2 form: the systems are equilibrated, |a_ii| = O(1); an
  // overflow would surface as inf / NaN in the growth test)
  auto publish = [&](int i, const cplx& r0, const cplx& r1) {
    cplx d;
    if (!TWO || i < 64) { d.x = lane_bcast(r0.x, i & 63); d.y = lane_bcast(r0.y, i & 63); }
    else { d.x = lane_bcast(r1.x, i & 63); d.y = lane_bcast(r1.y, i & 63); }
    const double rr = fast_recip(d.x * d.x + d.y * d.y);
    const cplx ip = make_double2(d.x * rr, -d.y * rr);
    cplx* ri = sa + off(i);
    cplx* lr = lrow + (i & 1) * n;
    if (j0 >= i && j0 < nc) { ri[j0] = r0; if (j0 < n) lr[j0] = cmul(r0, ip); }
    if (TWO && j1 >= i && j1 < nc) { ri[j1] = r1; if (j1 < n) lr[j1] = cmul(r1, ip); }
    if (lane == 0) ipiv[i] = ip;
  };
  if (w == 0) publish(0, a0[0], a1[0]);          // row 0 is final from the start
  if (!amax_ready) block_max_publish(sqrt(am), growth + 2 * (size_t)s);
  // Elimination in the D L^T form (row c stays unscaled: a_ij -= (a_ci / a_cc) a_cj); U = D^{-1/2} (D L^T) at the write-back.
  double um = 0.0;
  for (int c = 0; c < n; ++c) {
    __syncthreads();                            // row c has been published
    const cplx* rc = sa + off(c);
    const cplx* lr = lrow + (c & 1) * n;
    const cplx u0 = rc[(j0 >= c && j0 < nc) ? j0 : c];
    const cplx u1 = TWO ? rc[(j1 >= c && j1 < nc) ? j1 : c] : make_double2(0.0, 0.0);
    if (w == ((c + 1 + NW / 2) & (NW - 1))) {
      // acceptance tests on row c, once (by a wave that does not publish the next row): multipliers |a_cj| <= |piv| / rel;
      // growth: |a_cj| is the D L^T entry
      const cplx piv = rc[c];
      const double pa = fabs(piv.x) + fabs(piv.y);
      const bool in0 = j0 >= c && j0 < n, in1 = TWO && j1 >= c && j1 < n;
      const double v0 = in0 ? fabs(u0.x) + fabs(u0.y) : 0.0, v1 = in1 ? fabs(u1.x) + fabs(u1.y) : 0.0;
      if ((in0 && j0 > c && !(pa >= rel * v0)) || (in1 && j1 > c && !(pa >= rel * v1)) || !(pa > 0.0)) atomicMax(&bad_row, n - 1 - c);
      if (in0) um = nan_max(um, u0.x * u0.x + u0.y * u0.y);
      if (in1) um = nan_max(um, u1.x * u1.x + u1.y * u1.y);
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = w + NW * k;
      if (i > c && i < n) {
        const cplx f = lr[i];
        if (k < 64 / NW) a0[k] = cfnma(f, u0, a0[k]);         // (rows from 64 on have nothing in columns 0 .. 63)
        if (TWO) a1[k] = cfnma(f, u1, a1[k]);
        if (i == c + 1) publish(i, a0[k], a1[k]);             // this row is final now
      }
    }
  }
  __syncthreads();
  for (int r = tid; r < n; r += SMALL_THREADS) isq[r] = crecip(zsqrt(sa[off(r) + r]));
  um = sqrt(um);
  block_max_publish(um, growth + 2 * (size_t)s + 1);
  // back substitution (D L^T) x = y': x_c = (y'_c - sum_{j > c} a_cj x_j) / a_cc, column oriented, one barrier per step:
  // y'_c is final when step c starts; thread i < c takes a_ic x_c off y'_i; x_c = y'_c / a_cc is formed again at the write-back
  for (int c = n - 1; c > 0; --c) {
    __syncthreads();
    const cplx* rc = sa + off(c);
    const cplx ip = ipiv[c];
    for (int i = tid; i < c; i += SMALL_THREADS) {
      cplx* ri = sa + off(i);
      const cplx aic = ri[c];
      for (int q = 0; q < nrhs; ++q) ri[n + q] = cfnma(aic, cmul(rc[n + q], ip), ri[n + q]);
    }
  }
  __syncthreads();
  for (int r = w; r < n; r += SMALL_THREADS / 64) {
    cplx* dstg = As + (size_t)r * lda;
    const cplx* src = sa + off(r);
    const cplx sc = isq[r], ip = ipiv[r];
    for (int c = r + lane; c < nc; c += 64) {
      if (c < n) dstg[c] = cmul(src[c], sc);                  // U = D^{-1/2} (D L^T)
      else dstg[n_pad + (c - n)] = cmul(src[c], ip);         // the solution
    }
  }
  if (tid == 0 && bad_row >= 0 && info[s] == 0) info[s] = -(((n - 1 - bad_row) / NB) * NB + 1);
}

// ---------------------------------------------------------------------------------------------
// The diagonal 64 x 64 block of a panel, register-resident like k_small_utu (same elimination, same publication of finished
// rows): lane l of the wave that owns row i holds a_il and, in the second slot, column l of the identity carried through the
// elimination - [A11 | I] -> [D L^T | L^-1] - so the inverse the strip needs, U11^{-T} = D^{-1/2} L^{-1}, comes out of the lanes
// that the 64-column matrix block leaves idle.  Replaced an LDS form (64 steps of read-modify-write through LDS with a complex
// division per thread, then 64 two-barrier steps for the inverse; git history): 125 -> ~50 us per launch of one workgroup per CU
// (cfg 3: 56.4 -> 49.1 ms per 256-system step for strips + diagonal blocks; cfg 2: 61.9 -> 71.7 k systems/s, same box).
// Writes U11 into the upper triangle of the block and V = -U11^{-T} as V[k][i] (the A-operand order of the streaming zgemm: the strip is
// the pure product U12 = -V^T C, k_gemm3m_strip), and W = I + V beside it where k_back_step multiplies by the stored inverses.
// ---------------------------------------------------------------------------------------------
#ifdef BIEM_DIAG_TRACE
// diagnostic build only (tools/diag_trace.cpp): lane 0 of every wave of workgroup 0 stamps s_memtime at 4 points of each step
__device__ unsigned long long g_diag_trace[16][66][4];
#define BIEM_DT(step, i) { if (blockIdx.x == 0 && lane == 0) g_diag_trace[w][step][i] = __builtin_amdgcn_s_memtime(); }
#else
#define BIEM_DT(step, i)
#endif
constexpr int DIAG_RHS_MAX = 8;                                                          // right-hand sides a diagonal-block kernel solves with its block (rhs_gemv)
// The block's own part of the forward substitution, z_j = U11^{-T} y_j = D^{-1/2} L^{-1} y_j for up to 8 compact right-hand sides
// Y[s][q][row] (rows j .. j+63 have taken every earlier panel's term from the strip kernel's epilogue), from the packed L^-1 rows and
// 1 / sqrt(d) the kernel holds in LDS: wave = right-hand side, lane = row i, the sum over k <= i in ascending order.  Call behind a
// barrier that orders sy and isq; ys: [nrhs][64] of LDS.
__device__ __forceinline__ void diag_solve_rhs(cplx* __restrict__ Y, int nrhs, int n_pad, int s, int j, const cplx* sy, const cplx* isq, cplx* ys,
                                               int tid, int nthreads) {
  if (Y == nullptr) return;
  cplx* Ys = Y + (size_t)s * nrhs * n_pad + j;
  for (int e = tid; e < nrhs * NB; e += nthreads) ys[e] = Ys[(size_t)(e >> 6) * n_pad + (e & 63)];
  __syncthreads();
  const int lane = tid & 63;
  const cplx* row = sy + (lane * (lane + 1)) / 2;
  for (int q = tid >> 6; q < nrhs; q += nthreads >> 6) {
    cplx a = make_double2(0.0, 0.0);
    for (int k = 0; k < NB; ++k)
      if (k <= lane) a = cfma(row[k], ys[q * NB + k], a);
    Ys[(size_t)q * n_pad + lane] = cmul(a, isq[lane]);
  }
}

constexpr int DIAG_LDS_CPLX = 2 * (NB * (NB + 1) / 2) + 2 * NB + NB + 2 * NB + DIAG_RHS_MAX * NB;   // packed U rows, packed L^-1 rows, multipliers [2][64], 1 / sqrt(d), combined rows [2][64], y_j [8][64]
#ifndef BIEM_DIAG_THREADS
#define BIEM_DIAG_THREADS 1024
#endif
constexpr int DIAG_THREADS = BIEM_DIAG_THREADS;         // 16 waves x 4 rows: the step is bound by the instructions a wave issues for its rows
__global__ void __launch_bounds__(DIAG_THREADS) k_diag_utu_reg(cplx* __restrict__ A, long long lda, long long sys_stride, int j,
                                                                 cplx* __restrict__ Wt, long long w_stride, cplx* __restrict__ Vt, long long v_stride, int* __restrict__ info, double rel,
                                                                 unsigned long long* __restrict__ growth, cplx* __restrict__ Y, int nrhs, int n_pad) {
  extern __shared__ cplx sd[];
  __shared__ int bad;
  constexpr int NW = DIAG_THREADS / 64, KR = NB / NW;
  cplx* su = sd;                                   // (r, c), c >= r, at uoff(r) + c
  cplx* sy = su + NB * (NB + 1) / 2;               // (i, k), k <= i, at yoff(i) + k
  cplx* lrow = sy + NB * (NB + 1) / 2;             // [2][64] multipliers a_cj / a_cc of the current row
  cplx* isq = lrow + 2 * NB;                       // 1 / sqrt(d_r)
  auto uoff = [](int r) { return r * NB - (r * (r - 1)) / 2 - r; };
  auto yoff = [](int i) { return (i * (i + 1)) / 2; };
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar: the row tests below become scalar branches
  cplx* Ab = A + (size_t)s * sys_stride + (size_t)j * lda + j;
  if (tid == 0) bad = 0;
  BIEM_DT(64, 0)
  cplx a0[KR], y1[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int i = w + NW * k;
    a0[k] = lane >= i ? Ab[(size_t)i * lda + lane] : make_double2(0.0, 0.0);
    y1[k] = make_double2(lane == i ? 1.0 : 0.0, 0.0);
  }
  // A finished row i is published three times: packed rows su (D L^T) and sy (L^-1) for the write-back, and for the elimination ONE
  // combined vector comb[i & 1]: lane l <= i: (L^-1)_il (1 at l == i), lane l > i: a_il - the row-i operand of BOTH updates of a later
  // row r > i (its D L^T part lives in lanes >= r, its L^-1 part needs lanes <= i, and (L^-1)_il = 0 for l > i) - plus the multipliers
  // a_il / d_i in lrow[i & 1].  The step is LDS-bandwidth bound (tools/diag_trace.cpp: every wave reading the U row, the L^-1 row and a
  // broadcast multiplier per owned row = 96 reads of 1 KB per step, 650 of 1760 traced cycles): one row read instead of two, and waves /
  // rows that are finished read nothing.  (Multipliers taken from a vector through v_readlane instead of broadcast reads: slower,
  // 39 -> 48 us.)
  cplx* comb = isq + NB;                           // [2][64]
  auto publish = [&](int i, const cplx& r0, const cplx& r1) {
    cplx d;
    d.x = __shfl(r0.x, i, 64); d.y = __shfl(r0.y, i, 64);
    const double rr = fast_recip(d.x * d.x + d.y * d.y);
    const cplx ip = make_double2(d.x * rr, -d.y * rr);
    comb[(i & 1) * NB + lane] = make_double2(lane > i ? r0.x : r1.x, lane > i ? r0.y : r1.y);   // (by value: a conditional on the references selects an address and puts the rows into scratch)
    if (lane >= i) { su[uoff(i) + lane] = r0; lrow[(i & 1) * NB + lane] = cmul(r0, ip); }
    if (lane <= i) sy[yoff(i) + lane] = r1;
  };
  if (w == 0) publish(0, a0[0], y1[0]);
  double um = 0.0;
  BIEM_DT(64, 1)
  for (int c = 0; c < NB; ++c) {
    BIEM_DT(c, 0)
    __syncthreads();                            // row c has been published
    BIEM_DT(c, 1)
    const bool accept = w == ((c + 1 + NW / 2) & (NW - 1));   // acceptance tests on row c, once, by a wave that does not publish the next row
    if (accept) {
      const cplx* rc = su + uoff(c);
      const cplx piv = rc[c], ur = rc[lane >= c ? lane : c];
      const double pa = fabs(piv.x) + fabs(piv.y);
      if ((lane > c && !(pa >= rel * (fabs(ur.x) + fabs(ur.y)))) || !(pa > 0.0)) bad = 1;
      if (lane >= c) um = nan_max(um, ur.x * ur.x + ur.y * ur.y);
    }
    if (w + NW * (KR - 1) > c) {                // (a wave whose rows are all finished only takes the barriers)
    const cplx u0 = comb[(c & 1) * NB + lane];
    const cplx u1 = lane <= c ? u0 : make_double2(0.0, 0.0);
    const cplx* lr = lrow + (c & 1) * NB;
    // this wave's multipliers: all LDS reads issued together (inside the branches each would be waited for in turn)
    cplx fk[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) { const int i = w + NW * k; fk[k] = make_double2(0.0, 0.0); if (i > c) fk[k] = lr[i]; }
#ifdef BIEM_DIAG_TRACE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BIEM_DT(c, 2)
#endif
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = w + NW * k;
      if (i > c) {
        a0[k] = cfnma(fk[k], u0, a0[k]);
        y1[k] = cfnma(fk[k], u1, y1[k]);
        if (i == c + 1) { publish(i, a0[k], y1[k]); BIEM_DT(c, 3) }
      }
    }
    }
  }
  BIEM_DT(64, 2)
  __syncthreads();
  if (tid < NB) isq[tid] = crecip(zsqrt(su[uoff(tid) + tid]));
  block_max_publish(sqrt(um), growth + 2 * (size_t)s + 1);       // (its barrier also orders isq)
  // U11 = D^{-1/2} (D L^T) into the upper triangle of the block (lanes along the row)
  for (int r = w; r < NB; r += NW)
    if (lane >= r) Ab[(size_t)r * lda + lane] = cmul(su[uoff(r) + lane], isq[r]);
  // V[k][i] = -(U11^{-T})[i][k] = -L^-1[i][k] / sqrt(d_i), k <= i (lanes along i): the strip's A operand; W = I + V only where the
  // back substitution multiplies by the stored inverses (Wt != nullptr)
  cplx* Vo = Vt + (size_t)s * v_stride;
  cplx* Wo = Wt != nullptr ? Wt + (size_t)s * w_stride : nullptr;
  for (int k = w; k < NB; k += NW) {
    cplx xt = make_double2(0.0, 0.0);
    if (k <= lane) xt = cmul(sy[yoff(lane) + k], isq[lane]);
    Vo[k * NB + lane] = make_double2(-xt.x, -xt.y);
    if (Wo != nullptr) Wo[k * NB + lane] = k <= lane ? make_double2((k == lane ? 1.0 : 0.0) - xt.x, -xt.y) : make_double2(0.0, 0.0);
  }
  diag_solve_rhs(Y, nrhs, n_pad, s, j, sy, isq, comb + 2 * NB, tid, DIAG_THREADS);
  BIEM_DT(64, 3)
  if (tid == 0 && bad && info[s] == 0) info[s] = -(j + 1);
}

// ---------------------------------------------------------------------------------------------
// The same diagonal block, FOUR pivots per barrier: wave w owns the four consecutive rows 4w .. 4w+3.  tools/diag_trace.cpp showed
// the one-pivot-per-barrier form above to be a chain of latencies, not of work: per pivot a barrier, an LDS round trip, a lane
// broadcast of the pivot (another LDS round trip), a reciprocal (rcp + two Newton steps) and the multiplier products - about a
// dozen dependent FP64 instructions of ~20 cycles each plus ~400 cycles of LDS / barrier, ~1000 cycles where the arithmetic of a
// step needs 250.  Here a block of four finished rows is published at once: the waves behind it apply the four rows (rank-4
// update of their own four rows), and the wave that owns the next four rows then factors them on its own - the ten entries of its
// 4 x 4 diagonal sub-block are broadcast ONCE (ten independent lane broadcasts in flight together), every lane runs the 4 x 4
// elimination on them redundantly (pivots, reciprocals and the six multipliers inside the block as wave-uniform values: no further
// broadcast), and the vector updates of the rows follow.  16 barriers and 16 broadcast round trips instead of 64 each.
// Same arithmetic per entry as the form above (same order of the rank-1 updates), same acceptance tests, same outputs.
// ---------------------------------------------------------------------------------------------
constexpr int DIAGB_LDS_CPLX = 2 * (NB * (NB + 1) / 2) + NB + 2 * 2 * 4 * NB + 16 + DIAG_RHS_MAX * NB;   // packed U rows, packed L^-1 rows, 1 / sqrt(d), combined rows and multipliers [2][4][64] each, the 4 x 4 sub-block, y_j [8][64]
__global__ void __launch_bounds__(1024) k_diag_utu_blk(cplx* __restrict__ A, long long lda, long long sys_stride, int j,
                                                        cplx* __restrict__ Wt, long long w_stride, cplx* __restrict__ Vt, long long v_stride, int* __restrict__ info, double rel,
                                                        unsigned long long* __restrict__ growth, cplx* __restrict__ Y, int nrhs, int n_pad) {
  extern __shared__ cplx sd[];
  __shared__ int bad;
  constexpr int NW = 16, KR = 4;
  cplx* su = sd;                                   // (r, c), c >= r, at uoff(r) + c
  cplx* sy = su + NB * (NB + 1) / 2;               // (i, k), k <= i, at yoff(i) + k
  cplx* isq = sy + NB * (NB + 1) / 2;              // 1 / sqrt(d_r)
  cplx* cmb = isq + NB;                            // [2][4][64]: lane l <= i: (L^-1)_il, lane l > i: a_il of the published row i
  cplx* mul = cmb + 2 * 4 * NB;                    // [2][4][64]: a_il / d_i
  cplx* dsc = mul + 2 * 4 * NB;                    // [4][4]: the owner's 4 x 4 diagonal sub-block on its way to all lanes
  auto uoff = [](int r) { return r * NB - (r * (r - 1)) / 2 - r; };
  auto yoff = [](int i) { return (i * (i + 1)) / 2; };
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  cplx* Ab = A + (size_t)s * sys_stride + (size_t)j * lda + j;
  if (tid == 0) bad = 0;
  cplx a0[KR], y1[KR];
#pragma unroll
  for (int r = 0; r < KR; ++r) {
    const int i = 4 * w + r;
    a0[r] = lane >= i ? Ab[(size_t)i * lda + lane] : make_double2(0.0, 0.0);
    y1[r] = make_double2(lane == i ? 1.0 : 0.0, 0.0);
  }
  // in-wave factorisation of this wave's four rows (all earlier blocks applied), then their publication
  auto factor_block = [&]() {
    const int i0 = 4 * w;
    // the sub-block through LDS: four predicated writes, ten broadcast reads, one round trip (a wave's LDS operations complete in
    // order).  Twenty ds_bpermute with a single source lane took ~1000 cycles (tools/diag_trace.cpp).
    cplx D[KR][KR];
    const int cl = lane - i0;
#pragma unroll
    for (int r = 0; r < KR; ++r) if (cl >= r && cl < KR) dsc[r * KR + cl] = a0[r];
    // (lanes exchange data here without a workgroup barrier: the wave-scope fences keep hipcc from reading the entries before the
    // other lanes' stores, or forwarding this lane's own store - it did, and every system failed the pivot test)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r = 0; r < KR; ++r)
#pragma unroll
      for (int c = r; c < KR; ++c) D[r][c] = dsc[r * KR + c];
#ifdef BIEM_DIAG_TRACE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BIEM_DT(16 + w, 0)
#endif
    cplx ip[KR], m[KR][KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const double rr = fast_recip(D[r][r].x * D[r][r].x + D[r][r].y * D[r][r].y);
      const cplx dc = make_double2(D[r][r].x, -D[r][r].y);
      ip[r] = make_double2(dc.x * rr, dc.y * rr);
      // multipliers as (a conj d) / |d|^2: the product runs beside the reciprocal instead of behind it (two levels off the chain)
#pragma unroll
      for (int c = r + 1; c < KR; ++c) { const cplx t = cmul(D[r][c], dc); m[r][c] = make_double2(t.x * rr, t.y * rr); }
#pragma unroll
      for (int k = r + 1; k < KR; ++k)
#pragma unroll
        for (int c = k; c < KR; ++c) D[k][c] = cfnma(m[r][k], D[r][c], D[k][c]);
    }
#ifdef BIEM_DIAG_TRACE
    asm volatile("" :: "v"(ip[3].x), "v"(ip[3].y));
    BIEM_DT(16 + w, 1)
#endif
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const cplx yr = lane <= i0 + r ? y1[r] : make_double2(0.0, 0.0);
#pragma unroll
      for (int k = r + 1; k < KR; ++k) { a0[k] = cfnma(m[r][k], a0[r], a0[k]); y1[k] = cfnma(m[r][k], yr, y1[k]); }
    }
    cplx* cb = cmb + (w & 1) * 4 * NB;
    cplx* mb = mul + (w & 1) * 4 * NB;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const int i = i0 + r;
      cb[r * NB + lane] = make_double2(lane > i ? a0[r].x : y1[r].x, lane > i ? a0[r].y : y1[r].y);
      mb[r * NB + lane] = cmul(a0[r], ip[r]);
      if (lane >= i) su[uoff(i) + lane] = a0[r];
      if (lane <= i) sy[yoff(i) + lane] = y1[r];
    }
    BIEM_DT(16 + w, 2)
  };
  if (w == 0) factor_block();
  double um = 0.0;
  for (int b = 0; b < NW; ++b) {
    BIEM_DT(b, 0)
    __syncthreads();                            // rows 4b .. 4b+3 have been published
    BIEM_DT(b, 1)
    if (w == ((b + 1 + NW / 2) & (NW - 1))) {   // acceptance tests on the four rows, once, by a wave far from the chain
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const int c = 4 * b + r;
        const cplx* rc = su + uoff(c);
        const cplx piv = rc[c], ur = rc[lane >= c ? lane : c];
        const double pa = fabs(piv.x) + fabs(piv.y);
        if ((lane > c && !(pa >= rel * (fabs(ur.x) + fabs(ur.y)))) || !(pa > 0.0)) bad = 1;
        if (lane >= c) um = nan_max(um, ur.x * ur.x + ur.y * ur.y);
      }
    }
    if (w > b) {
      if (w == b + 1) __builtin_amdgcn_s_setprio(3);          // the next block's owner is the dependent chain
      const cplx* cb = cmb + (b & 1) * 4 * NB;
      const cplx* mb = mul + (b & 1) * 4 * NB;
      // (the reads of row r + 1 are issued before the arithmetic of row r: four exposed LDS round trips per block step otherwise)
      cplx nu = cb[lane], nf[KR];
#pragma unroll
      for (int k = 0; k < KR; ++k) nf[k] = mb[4 * w + k];
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const int c = 4 * b + r;
        const cplx u0 = nu;
        cplx fk[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) fk[k] = nf[k];
        if (r + 1 < KR) {
          nu = cb[(r + 1) * NB + lane];
#pragma unroll
          for (int k = 0; k < KR; ++k) nf[k] = mb[(r + 1) * NB + 4 * w + k];
        }
        const cplx u1 = lane <= c ? u0 : make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < KR; ++k) { a0[k] = cfnma(fk[k], u0, a0[k]); y1[k] = cfnma(fk[k], u1, y1[k]); }
      }
#ifdef BIEM_DIAG_TRACE
      asm volatile("" :: "v"(a0[0].x), "v"(a0[3].y), "v"(y1[3].x));
      BIEM_DT(b, 2)
#endif
      if (w == b + 1) { factor_block(); __builtin_amdgcn_s_setprio(0); }
    }
  }
  __syncthreads();
  if (tid < NB) isq[tid] = crecip(zsqrt(su[uoff(tid) + tid]));
  block_max_publish(sqrt(um), growth + 2 * (size_t)s + 1);       // (its barrier also orders isq)
  for (int r = w; r < NB; r += NW)
    if (lane >= r) Ab[(size_t)r * lda + lane] = cmul(su[uoff(r) + lane], isq[r]);
  // V = -U11^{-T} for the strip, W = I + V where the back substitution wants it (as in k_diag_utu_reg)
  cplx* Vo = Vt + (size_t)s * v_stride;
  cplx* Wo = Wt != nullptr ? Wt + (size_t)s * w_stride : nullptr;
  for (int k = w; k < NB; k += NW) {
    cplx xt = make_double2(0.0, 0.0);
    if (k <= lane) xt = cmul(sy[yoff(lane) + k], isq[lane]);
    Vo[k * NB + lane] = make_double2(-xt.x, -xt.y);
    if (Wo != nullptr) Wo[k * NB + lane] = k <= lane ? make_double2((k == lane ? 1.0 : 0.0) - xt.x, -xt.y) : make_double2(0.0, 0.0);
  }
  diag_solve_rhs(Y, nrhs, n_pad, s, j, sy, isq, dsc + 16, tid, 1024);
  if (tid == 0 && bad && info[s] == 0) info[s] = -(j + 1);
}

// The head of the stacked pass of panel p = J + 64 q of the group at row J (launch_gemm_stack): with V_p = -U11^{-T} of the panel's
// diagonal block in rows p - J .. of the slab (k_diag_utu_* writes it there), the blocks above it,
//   S_r[k][i] = -sum_m U[r + k, p + m] V_p[m][i]     for the finished panels r = J, J + 64, .. < p   (64 x 64 each, rows r - J .. of the slab),
// so that  -[S ; V]^T A[J : p+64, c]  is  U11^{-T} (C[p, c] - sum_r U[r, p]^T U[r, c]):  pending updates and solve in one product.
// One workgroup per block and system; thread (tk, ti) holds rows tk + 16 a, columns ti + 16 b of the block; m in steps of 16 through LDS.
__global__ void __launch_bounds__(256, 2) k_sym_slab(const cplx* __restrict__ A, long long lda, long long sys_stride, cplx* __restrict__ slab, int J, int p) {
  __shared__ cplx su[NB][17];
  __shared__ cplx sv[16][NB];
  const int s = blockIdx.y, r = blockIdx.x, tid = threadIdx.x, ti = tid & 15, tk = tid >> 4;
  const cplx* Ut = A + (size_t)s * sys_stride + (size_t)(J + r * NB) * lda + p;
  cplx* Ss = slab + (size_t)s * SYM_SLAB_CPLX;
  const cplx* V = Ss + (size_t)(p - J) * NB;
  cplx acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = make_double2(0.0, 0.0);
  // (V_p[m][i] = 0 for m > i: the column groups b < m0 / 16 of a step hold zeros and are skipped; the loops stay rolled - unrolled,
  // hipcc hoisted every LDS read of a step and spilled a thousand registers)
#pragma unroll 1
  for (int m0 = 0; m0 < NB; m0 += 16) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int e = tid + 256 * x;
      su[e >> 4][e & 15] = Ut[(size_t)(e >> 4) * lda + m0 + (e & 15)];
      sv[e >> 6][e & 63] = V[(m0 + (e >> 6)) * NB + (e & 63)];
    }
    __syncthreads();
#pragma unroll 2
    for (int m = 0; m < 16; ++m) {
      cplx u[4], v[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) u[a] = su[tk + 16 * a][m];
#pragma unroll
      for (int b = 0; b < 4; ++b) v[b] = sv[m][ti + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (16 * b + 15 >= m0) acc[a][b] = cfma(u[a], v[b], acc[a][b]);
    }
    __syncthreads();
  }
  cplx* So = Ss + (size_t)r * NB * NB;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) So[(tk + 16 * a) * NB + ti + 16 * b] = make_double2(-acc[a][b].x, -acc[a][b].y);
}

// ---------------------------------------------------------------------------------------------
// The form of a call (SymForm, dense.hpp): every rule and every switch that forces a form, in this one place.
// ---------------------------------------------------------------------------------------------
// The five switches (tests, A/B), read per call.  Of a value only its first letter counts; -1: not set.  A letter no rule names leaves
// the rule in place for BIEM_SYM_UPDATE, BIEM_SYM_GROUP and BIEM_DIAG_FORM; for BIEM_BACK_FORM it selects the row form (any value
// that starts with neither c nor s does); BIEM_NO_SMALL_PATH counts as soon as it is set, whatever its value.
// A sixth, BIEM_BACK_ROW=blocks, picks no form: inside the row form it runs the per-block launches (k_back_row) instead of the sweep.
// A seventh, BIEM_GEMM_NARROW=0|1, picks no form either: under the left-looking update it turns the narrow launch of the last tile column
// off, or drops its size rule (gemm_narrow_frags, kernels_gemm3m.hip).
struct SymEnv { int update, group, back, diag; bool no_small; int back_row; int narrow; };
static SymEnv sym_env() {
  auto first = [](const char* name) { const char* e = getenv(name); return e ? (int)(unsigned char)e[0] : -1; };
  const int nw = first("BIEM_GEMM_NARROW");
  return {first("BIEM_SYM_UPDATE"), first("BIEM_SYM_GROUP"), first("BIEM_BACK_FORM"), first("BIEM_DIAG_FORM"), getenv("BIEM_NO_SMALL_PATH") != nullptr,
          first("BIEM_BACK_ROW"), nw == '0' ? 0 : nw == '1' ? 1 : -1};
}

// the whole system fits LDS: one launch does everything (k_small_utu)
static bool small_rule(const SymEnv& e, int n_active, int nrhs) {
  return n_active > 0 && n_active <= SMALL_N_MAX && nrhs <= SMALL_RHS_MAX && n_active + nrhs <= 128 && small_utu_lds(n_active, nrhs) <= 160 * 1024 - 2048 &&
         !e.no_small;
}
// form of the bulk update: BIEM_SYM_UPDATE=left|right forces one; the rule and its measurements: gemm_left_fills_grid, kernels_gemm3m.hip
static bool left_rule(const SymEnv& e, int nb, int n_pad, int nrhs) {
  if (n_pad <= 4 * NB) return false;                               // one group: no bulk update at all
  if (e.update == 'l') return true;
  if (e.update == 'r') return false;
  return gemm_left_fills_grid(nb, n_pad, nrhs);
}
// Form of the panels b, c, d of a group: the stacked pass runs only where the bulk update is left-looking, and
// there from SYM_STACK_MIN_SYSTEMS systems per call.  What the passes save grows with the batch (14.0 ms per cfg 3 step at 256 systems),
// the three small head launches per panel cost the same few ms at any batch size (5.0 ms): they break even near 90 systems, and the
// form lost 1.2 % at 64 systems of cfg 4 and 2 % at 32 systems of cfg 3 (profiles/r06_other_shapes.txt) - so twice the break-even.
// BIEM_SYM_GROUP=twopass|stacked forces a form under the left-looking update (tests, A/B).
constexpr int SYM_STACK_MIN_SYSTEMS = 192;
static bool stacked_rule(const SymEnv& e, bool left, int nb) {
  if (!left) return false;
  if (e.group == 't') return false;
  if (e.group == 's') return true;
  return nb >= SYM_STACK_MIN_SYSTEMS;
}
// Back substitution.  Few systems: the row form has one workgroup per system and 64-row block (a quarter of the CUs busy at 64 systems);
// the column-block form spreads a system's rows over workgroups (cfg 4, N = 4064: 64 systems 6.1 -> 5.1 ms, 8 systems 5.7 -> 2.6 ms,
// one system per call 22.8 -> 20.6 ms; at 256+ systems the row form wins: it reads U once in long runs).  Fewer still (STEP, keep_w):
// every panel's W = I - U11^{-T} is kept and the back substitution multiplies by the stored inverses instead of solving with the
// diagonal blocks (k_back_step) - every workgroup of a block step forms x_b for itself from the 64 KB inverse: a latency trade that
// pays for a handful of systems (at 64 systems of cfg 4 the back substitution went from 4.4 to 11.5 ms with it).
// BIEM_BACK_FORM=row|col|step forces one: step the stored inverses, col the two-launch column form.  What the panel region cannot hold
// (SymAliases, dense.hpp) goes to the column form, which works on the augmented columns; no right-hand sides: the row form's pass for
// the checks alone.
constexpr int SYM_BACK_COL_MAX_SYSTEMS = 64, SYM_BACK_STEP_MAX_SYSTEMS = 8;
static SymForm::Back back_rule(const SymEnv& e, int nb, int nrhs) {
  const bool col_form = e.back >= 0 ? e.back == 'c' || e.back == 's' : nb <= SYM_BACK_COL_MAX_SYSTEMS;
  const bool keep_w = col_form && nrhs > 0 && nrhs <= SYM_STEP_RHS_MAX && (e.back >= 0 ? e.back == 's' : nb <= SYM_BACK_STEP_MAX_SYSTEMS);
  if (keep_w) return SymForm::BACK_STEP;
  return nrhs > SYM_ROW_RHS_MAX || (col_form && nrhs > 0) ? SymForm::BACK_COL : SymForm::BACK_ROW;
}

SymForm sym_form(int nb, int n_pad, int n_active, int nrhs) {
  const SymEnv e = sym_env();
  SymForm f;
  f.small = small_rule(e, n_active, nrhs);
  f.two = f.small && n_active + nrhs > 64;
  const int kr = (n_active + SMALL_THREADS / 64 - 1) / (SMALL_THREADS / 64);      // rows per wave; the instantiation that holds them
  f.kr = !f.small ? 0 : !f.two ? (kr <= 4 ? 4 : 8) : kr <= 8 ? 8 : kr <= 9 ? 9 : kr <= 12 ? 12 : 16;
  f.left = left_rule(e, nb, n_pad, nrhs);
  f.stacked = stacked_rule(e, f.left, nb);
  // Few right-hand sides do not ride in the matrix: the forward substitution works on the compact copy Y[s][q][row] the row-form back
  // substitution uses anyway - every diagonal-block kernel solves its own 64 entries, every strip tile takes its 64 columns' term from
  // the tile it has in registers.  U is read once for the solve (the back substitution); the update launches end at column n_pad.
  f.rhs_gemv = nrhs > 0 && nrhs <= 8;
  f.back = back_rule(e, nb, nrhs);
  f.diag_blk = e.diag != 's';        // BIEM_DIAG_FORM=step: one pivot per barrier (the A/B of the tests); default: four
  return f;
}
// the single decisions other units and the tests ask for
int sym_update_left(int nb, int n_pad, int nrhs) { return left_rule(sym_env(), nb, n_pad, nrhs) ? 1 : 0; }
bool sym_group_stacked(bool left, int nb) { return stacked_rule(sym_env(), left, nb); }
bool sym_small_path(int n_active, int nrhs) { return small_rule(sym_env(), n_active, nrhs); }
int sym_gemm_narrow(int nb, int n_pad, int n_active, int J) { return gemm_narrow_frags(nb, n_pad, n_active, J, sym_env().narrow); }

int sym_aliases(const SymForm& f, const DenseWork& w, void* d_work, int nb, int n_pad, int nrhs, SymAliases& a) {
  a = SymAliases{nullptr, nullptr, nullptr, 0, 0, 0, 0};
  if (f.small) return BIEM_OK;
  a.wall_stride = (long long)n_pad * NB;
  if (f.keep_w()) a.wall_bytes = (size_t)nb * a.wall_stride * sizeof(cplx);
  a.y_off = w.panels + a.wall_bytes;
  if (f.rhs_gemv || f.keep_w() || (f.back == SymForm::BACK_ROW && nrhs > 0)) a.y_bytes = (size_t)nb * nrhs * n_pad * sizeof(cplx);
  if (a.y_off + a.y_bytes > w.block) {
    set_error("biem_sym: %d right-hand sides of %d systems with n_pad=%d do not fit the panel region (back form %d)", nrhs, nb, n_pad, (int)f.back);
    return BIEM_ERR_ARG;
  }
  if (d_work != nullptr) {
    cplx* P = w.panels_at(d_work);
    if (f.keep_w()) { a.Wall = P; a.Xsol = P + a.wall_bytes / sizeof(cplx); }
    a.Y = f.keep_w() ? a.Xsol : P;
  }
  return BIEM_OK;
}

int sym_form_query(int nb, int n_pad, int n_active, int nrhs, int* form, size_t* work) {
  if (nb <= 0 || n_pad <= 0 || n_pad % NB || n_active < 1 || n_active > n_pad || nrhs < 0) {
    set_error("biem_sym_form: nb=%d, n_pad=%d (a multiple of %d), n_active=%d in 1 .. n_pad, nrhs=%d >= 0 expected", nb, n_pad, NB, n_active, nrhs);
    return BIEM_ERR_ARG;
  }
  const SymForm f = sym_form(nb, n_pad, n_active, nrhs);
  const DenseWork w = dense_work(nb, n_pad, nrhs);
  SymAliases a;
  if (const int rc = sym_aliases(f, w, nullptr, nb, n_pad, nrhs, a)) return rc;
  if (form) {
    const int v[BIEM_SYM_FORM_LEN] = {f.small, f.kr, f.two, f.left, f.stacked, f.rhs_gemv, (int)f.back, f.keep_w(), f.diag_blk};
    for (int i = 0; i < BIEM_SYM_FORM_LEN; ++i) form[i] = v[i];
  }
  if (work) {
    const size_t v[BIEM_SYM_WORK_LEN] = {w.panels, w.block, w.tri_map, w.growth, w.spare, w.slab, w.total, w.panels, a.wall_bytes, a.y_off, a.y_bytes};
    for (int i = 0; i < BIEM_SYM_WORK_LEN; ++i) work[i] = v[i];
  }
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// launch_sym_factor_solve: the operands of one call, and its three stages
// ---------------------------------------------------------------------------------------------
struct SymCall {
  int nb, n_pad, n_active, nrhs; cplx* A; long long lda, sys_stride; int* d_info; hipStream_t st; bool amax_ready;
  double nopiv, growth_max;                  // ldlt_thresholds
  cplx* Wt; int* tri_map; unsigned long long* growth; cplx* slab;     // DenseWork: the 64 x 64 block, the tile map, the growth slots, the slab
  SymAliases al;
};

static int sym_one_launch(const SymForm& f, const SymCall& c) {
  if (!c.amax_ready) launch_zero_int(c.st, (int*)c.growth, 4 * c.nb);   // max|A| is measured by the kernel
  ProfScope ps(PK_PANEL, c.st, 0.0);
  const size_t shm = small_utu_lds(c.n_active, c.nrhs);
#define BIEM_SMALL(KR, TWO)                                                                                                         \
  {                                                                                                                                  \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_small_utu<KR, TWO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));        \
    hipLaunchKernelGGL((k_small_utu<KR, TWO>), dim3(c.nb), dim3(SMALL_THREADS), shm, c.st, c.A, c.lda, c.sys_stride, c.n_active, c.n_pad, c.nrhs, \
                       c.d_info, c.growth, c.nopiv, c.amax_ready ? 1 : 0);                                                            \
  }
  if (!f.two) { if (f.kr == 4) BIEM_SMALL(4, false) else BIEM_SMALL(8, false) }
  else if (f.kr == 8) BIEM_SMALL(8, true)
  else if (f.kr == 9) BIEM_SMALL(9, true)
  else if (f.kr == 12) BIEM_SMALL(12, true)
  else BIEM_SMALL(16, true)
#undef BIEM_SMALL
  return BIEM_OK;
}

static int sym_factor(const SymForm& f, const SymCall& c) {
  const int nb = c.nb, n_pad = c.n_pad, nrhs = c.nrhs, n_cols = n_pad + nrhs;
  cplx* const A = c.A; const long long lda = c.lda, sys_stride = c.sys_stride; hipStream_t st = c.st;
  launch_tri_map(st, c.tri_map, n_pad);
  if (!c.amax_ready) {
    launch_zero_int(st, (int*)c.growth, 4 * nb);
    ProfScope ps(PK_SWAP, st, 0.0);
    hipLaunchKernelGGL(k_absmax_upper, dim3((n_pad + 7) / 8, nb), dim3(256), 0, st, A, lda, sys_stride, n_pad, c.growth);
  }
  int gemm_rc = BIEM_OK;
  auto keep = [&](int r) { if (r != BIEM_OK && gemm_rc == BIEM_OK) gemm_rc = r; };      // the first failure of an update launch is kept and returned
  auto gemm = [&](auto&&... a) { keep(launch_gemm_stream(a...)); };
  cplx* const Yf = f.rhs_gemv ? c.al.Y : nullptr;      // the compact copy the forward substitution works on
  const int f_cols = f.rhs_gemv ? n_pad : n_cols;      // the factorisation's last column
  if (f.rhs_gemv) hipLaunchKernelGGL(k_rhs_compact, dim3((n_pad + 255) / 256, nrhs, nb), dim3(256), 0, st, A, lda, sys_stride, Yf, nrhs, n_pad, 0);
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_diag_utu_reg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(DIAG_LDS_CPLX * sizeof(cplx))));
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_diag_utu_blk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(DIAGB_LDS_CPLX * sizeof(cplx))));
  // slab != nullptr: the panel p = j of the group at row J takes the stacked pass (below) - V goes to rows j - J .. of the slab
  auto panel = [&](int j, int J = 0, cplx* slab = nullptr) {
    // the strip's operand V = -U11^{-T} lives in the 64 x 64 block; a kept W = I + V goes to the panel region
    cplx* Wp = f.keep_w() ? c.al.Wall + (size_t)(j / NB) * NB * NB : nullptr;
    cplx* Vp = slab != nullptr ? slab + (size_t)(j - J) * NB : c.Wt;
    const long long w_stride = f.keep_w() ? c.al.wall_stride : 0, v_stride = slab != nullptr ? (long long)SYM_SLAB_CPLX : (long long)NB * NB;
    {
      ProfScope ps(PK_PANEL, st, 0.0);
      if (f.diag_blk) hipLaunchKernelGGL(k_diag_utu_blk, dim3(nb), dim3(1024), DIAGB_LDS_CPLX * sizeof(cplx), st, A, lda, sys_stride, j, Wp, w_stride, Vp, v_stride, c.d_info, c.nopiv, c.growth, Yf, nrhs, n_pad);
      else hipLaunchKernelGGL(k_diag_utu_reg, dim3(nb), dim3(DIAG_THREADS), DIAG_LDS_CPLX * sizeof(cplx), st, A, lda, sys_stride, j, Wp, w_stride, Vp, v_stride, c.d_info, c.nopiv, c.growth, Yf, nrhs, n_pad);
    }
    if (f_cols <= j + NB) return;
    if (slab != nullptr) {
      // the blocks S_r = -U[r, j] V of the finished panels of the group, then pending updates and solve as one product over K = j - J + 64
      {
        ProfScope ps(PK_PANEL, st, 8.0 * (double)nb * (j - J) * NB * NB);
        hipLaunchKernelGGL(k_sym_slab, dim3((j - J) / NB, nb), dim3(256), 0, st, A, lda, sys_stride, slab, J, j);
      }
      keep(launch_gemm_stack(st, nb, A, lda, sys_stride, slab, (long long)SYM_SLAB_CPLX, J, j, f_cols, Yf, nrhs, n_pad));
      return;
    }
    // U12 = U11^{-T} C = -V^T C in place over the 64 rows (every tile reads its own columns only); A operand V[k][i], i = row - j: the
    // base shifted by -j rows (only rows j .. j+63 are addressed)
    keep(launch_gemm_strip(st, nb, A, lda, sys_stride, c.Wt - j, v_stride, j, f_cols, Yf, nrhs, n_pad));
  };
  // The panels b, c, d of a group, two forms.  Two-pass: the panel's 64 rows take the group's pending updates in a C-streaming launch
  // (K = 64 q), then the strip solves them (K = 64) - every row is read and written twice.  Stacked (SymForm.stacked: under the left-
  // looking bulk update, large batches): only the diagonal tile takes the pending update; behind the diagonal block
  // the rest of the rows is ONE pure product over K = 64 (q + 1) (k_sym_slab, launch_gemm_stack) - no C slots, one set of stores per tile.
  // (Round 3 built a first fused form, U12 = C - [(X P^T) | W] [Q ; C] on the C-streaming kernel for every batch size: 2.5 % of panel +
  // in-group time at cfg 3, and a loss of 27 - 30 % where few systems are in flight - three more small launches per panel.  Since then
  // the strip became a pure product and the right-hand sides left the matrix; this form runs only where the launches are large.
  // DESIGN.md section 5 has both measurements.)
  cplx* const slab = f.stacked ? c.slab : nullptr;
  const int narrow_mode = sym_env().narrow;
  for (int J = 0; J < n_pad; J += 4 * NB) {
    const cplx* strip = A + (size_t)J * lda;        // both operands of this group's updates: rows J .. of the matrix itself
    if (f.left && J > 0) {
      // left-looking: the group's rows take every pending update of the finished rows 0 .. J-1 now, in one K = J pass (many right-hand
      // sides: tile columns of the same launch; few: not in the matrix at all)
      const int row_end = J + 4 * NB < n_pad ? J + 4 * NB : n_pad;
      // (the last tile column's identity padding is not multiplied where that pays: a narrow launch of its own, gemm_narrow_frags;
      // right-hand sides as tile columns behind it: the launch stays whole)
      const int nf = f_cols > n_pad ? 4 : gemm_narrow_frags(nb, n_pad, c.n_active, J, narrow_mode);
      keep(launch_gemm_left(st, nb, A, lda, sys_stride, J, row_end, f_cols, nf));
    }
    panel(J);
    for (int q = 1; q < 4; ++q) {
      const int jq = J + q * NB;
      if (jq >= n_pad) break;
      if (f.stacked) {
        // the diagonal tile alone takes the group's pending updates (K = 64 q); the rest of the rows waits for the stacked pass
        gemm(st, nb, A, lda, sys_stride, strip, lda, sys_stride, jq, jq + NB, jq, jq + NB, J, q * NB, PK_OTHER);
        panel(jq, J, slab);
        continue;
      }
      // the next panel's 64 rows: all pending updates of the group (K = 64 q), every column right of them incl. right-hand sides in the matrix
      gemm(st, nb, A, lda, sys_stride, strip, lda, sys_stride, jq, jq + NB, jq, f_cols, J, q * NB, PK_OTHER);
      panel(jq);
    }
    if (J + 4 * NB >= n_pad) break;
    if (f.left) continue;                            // no update after the group: the rows below take it when their own group starts
    gemm(st, nb, A, lda, sys_stride, strip, lda, sys_stride, J + 4 * NB, n_pad, J + 4 * NB, n_pad, J, 4 * NB, PK_GEMM, -1.0, nullptr, 0, 0, 0,
         c.tri_map, true);
    if (nrhs > 0 && !f.rhs_gemv) gemm(st, nb, A, lda, sys_stride, strip, lda, sys_stride, J + 4 * NB, n_pad, n_pad, n_cols, J, 4 * NB, PK_OTHER);
  }
  BIEM_LAUNCHCHK();
  return gemm_rc;
}

// back substitution, bottom block row first; its pass over U also takes the multiplier / growth checks of the strip entries
static int sym_back(const SymForm& f, const SymCall& c) {
  const int nb = c.nb, n_pad = c.n_pad, nrhs = c.nrhs;
  cplx* const A = c.A; const long long lda = c.lda, sys_stride = c.sys_stride; hipStream_t st = c.st;
  ProfScope ps(PK_BACK, st, 4.0 * (double)nb * n_pad * (double)n_pad * nrhs);
  const double inv_rel2 = 1.0 / (c.nopiv * c.nopiv);
  const dim3 compact_grid((n_pad + 255) / 256, nrhs, nb);
  if (f.back != SymForm::BACK_ROW) {
    // (these forms work on the augmented columns: the forward-substituted compact copy goes back there first)
    if (f.rhs_gemv) hipLaunchKernelGGL(k_rhs_compact, compact_grid, dim3(256), 0, st, A, lda, sys_stride, c.al.Y, nrhs, n_pad, 1);
    if (f.back == SymForm::BACK_STEP) {
      for (int jr = n_pad - BS; jr >= 0; jr -= BS)
        hipLaunchKernelGGL(k_back_step, dim3(jr > 0 ? (jr + BACK_ROWS - 1) / BACK_ROWS : 1, nb), dim3(256), 0, st, A, lda, sys_stride, A + n_pad, lda,
                           sys_stride, c.al.Wall, c.al.wall_stride, c.al.Xsol, n_pad, nrhs, jr, c.d_info, c.growth, inv_rel2);
      hipLaunchKernelGGL(k_rhs_compact, compact_grid, dim3(256), 0, st, A, lda, sys_stride, c.al.Xsol, nrhs, n_pad, 1);
    } else   // the column-block form on the augmented columns, same checks
      back_substitute_cols(st, nb, n_pad, nrhs, A, lda, sys_stride, A + n_pad, lda, sys_stride, c.d_info, c.growth, inv_rel2);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  // the row form on the compact copy; nrhs == 0: one pass for the checks alone; right-hand sides in groups of up to 8.  One launch per
  // group (k_back_sweep); BIEM_BACK_ROW=blocks: one launch per group and 64-row block (k_back_row), the same arithmetic
  cplx* const Y = c.al.Y;
  if (nrhs > 0 && !f.rhs_gemv) hipLaunchKernelGGL(k_rhs_compact, compact_grid, dim3(256), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, 0);
  const bool blocks = sym_env().back_row == 'b';
  int q0 = 0;
  do {
    const int nq = nrhs - q0 > 8 ? 8 : nrhs - q0;
    const int chk = q0 == 0 ? 1 : 0;
    const int NQ = nq <= 1 ? 1 : nq == 2 ? 2 : nq <= 4 ? 4 : 8;
    if (!blocks) {
#define BIEM_SWEEP(Q)                                                                                                                       \
      {                                                                                                                                      \
        BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_back_sweep<Q>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep_lds(Q)));        \
        hipLaunchKernelGGL(k_back_sweep<Q>, dim3(nb), dim3(1024), sweep_lds(Q), st, A, lda, sys_stride, Y, nrhs, n_pad, q0, nq, chk, c.d_info, \
                           c.growth, inv_rel2);                                                                                               \
      }
      if (NQ == 1) BIEM_SWEEP(1) else if (NQ == 2) BIEM_SWEEP(2) else if (NQ == 4) BIEM_SWEEP(4) else BIEM_SWEEP(8)
#undef BIEM_SWEEP
    } else
      for (int ib = n_pad / NB - 1; ib >= 0; --ib) {
        if (NQ == 1) hipLaunchKernelGGL(k_back_row<1>, dim3(nb), dim3(1024), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, q0, nq, ib, chk, c.d_info, c.growth, inv_rel2);
        else if (NQ == 2) hipLaunchKernelGGL(k_back_row<2>, dim3(nb), dim3(1024), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, q0, nq, ib, chk, c.d_info, c.growth, inv_rel2);
        else if (NQ == 4) hipLaunchKernelGGL(k_back_row<4>, dim3(nb), dim3(1024), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, q0, nq, ib, chk, c.d_info, c.growth, inv_rel2);
        else hipLaunchKernelGGL(k_back_row<8>, dim3(nb), dim3(1024), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, q0, nq, ib, chk, c.d_info, c.growth, inv_rel2);
      }
    q0 += nq;
  } while (q0 < nrhs);
  if (nrhs > 0) hipLaunchKernelGGL(k_rhs_compact, compact_grid, dim3(256), 0, st, A, lda, sys_stride, Y, nrhs, n_pad, 1);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_sym_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_info, void* d_work,
                            size_t work_bytes, hipStream_t st, bool amax_ready, int n_active) {
  if (nb <= 0 || n_pad <= 0) return BIEM_OK;
  if (n_active <= 0 || n_active > n_pad) n_active = n_pad;        // rows n_active .. n_pad-1: identity padding (the caller's promise)
  if (const int rc = check_factor_args("biem_sym", nb, n_pad, nrhs, lda, work_bytes)) return rc;
  const SymForm f = sym_form(nb, n_pad, n_active, nrhs);
  const DenseWork w = dense_work(nb, n_pad, nrhs);
  SymCall c{nb, n_pad, n_active, nrhs, (cplx*)d_A, lda, sys_stride, d_info, st, amax_ready, 0.0, 0.0,
            w.block_at(d_work), w.tri_map_at(d_work), w.growth_at(d_work), w.slab_at(d_work), SymAliases()};
  if (const int rc = sym_aliases(f, w, d_work, nb, n_pad, nrhs, c.al)) return rc;
  ldlt_thresholds(c.nopiv, c.growth_max);
  launch_zero_int(st, d_info, nb);
  if (f.small) {
    if (const int rc = sym_one_launch(f, c)) return rc;
  } else {
    if (const int rc = sym_factor(f, c)) return rc;
    if (const int rc = sym_back(f, c)) return rc;
  }
  launch_growth_check(st, nb, n_pad, c.growth, d_info, c.growth_max);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

#ifdef BIEM_DIAG_TRACE
extern "C" int biem_debug_diag(int reps, unsigned long long* trace_out, float* us_out) {
  const int n = 1024; const long long lda = n + 8;
  cplx *A = nullptr, *W = nullptr; int* info = nullptr; unsigned long long* growth = nullptr;
  if (hipMalloc((void**)&A, (size_t)n * lda * sizeof(cplx)) != hipSuccess || hipMalloc((void**)&W, NB * NB * sizeof(cplx)) != hipSuccess ||
      hipMalloc((void**)&info, 64) != hipSuccess || hipMalloc((void**)&growth, 64) != hipSuccess) return 1;
  std::vector<cplx> h((size_t)n * lda);
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) { const int a = r < c ? r : c, b = r < c ? c : r; h[(size_t)r * lda + c] = make_double2(r == c ? 3.0 : 0.3 * sin(0.37 * a + 1.1 * b), r == c ? 0.4 : 0.2 * cos(0.9 * a - 0.3 * b)); }
  hipMemcpy(A, h.data(), h.size() * sizeof(cplx), hipMemcpyHostToDevice);
  hipMemset(info, 0, 64); hipMemset(growth, 0, 64);
  hipFuncSetAttribute((const void*)k_diag_utu_reg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(DIAG_LDS_CPLX * sizeof(cplx)));
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const bool blk = sym_form(1, n, n, 0).diag_blk;      // (BIEM_DIAG_FORM=step as in production: the reg kernel)
  hipFuncSetAttribute((const void*)k_diag_utu_blk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(DIAGB_LDS_CPLX * sizeof(cplx)));
  for (int r = 0; r < 3; ++r) {
    if (blk) hipLaunchKernelGGL(k_diag_utu_blk, dim3(1), dim3(1024), DIAGB_LDS_CPLX * sizeof(cplx), 0, A, lda, 0, 64 * r, nullptr, 0, W, (long long)NB * NB, info, 0.01, growth, nullptr, 0, n);
    else hipLaunchKernelGGL(k_diag_utu_reg, dim3(1), dim3(DIAG_THREADS), DIAG_LDS_CPLX * sizeof(cplx), 0, A, lda, 0, 64 * r, nullptr, 0, W, (long long)NB * NB, info, 0.01, growth, nullptr, 0, n);
  }
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  for (int r = 0; r < reps; ++r) {
    if (blk) hipLaunchKernelGGL(k_diag_utu_blk, dim3(1), dim3(1024), DIAGB_LDS_CPLX * sizeof(cplx), 0, A, lda, 0, 64 * (3 + r % 12), nullptr, 0, W, (long long)NB * NB, info, 0.01, growth, nullptr, 0, n);
    else hipLaunchKernelGGL(k_diag_utu_reg, dim3(1), dim3(DIAG_THREADS), DIAG_LDS_CPLX * sizeof(cplx), 0, A, lda, 0, 64 * (3 + r % 12), nullptr, 0, W, (long long)NB * NB, info, 0.01, growth, nullptr, 0, n);
  }
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); *us_out = ms * 1e3f / reps;
  hipMemcpyFromSymbol(trace_out, HIP_SYMBOL(g_diag_trace), sizeof(unsigned long long) * 16 * 66 * 4);
  hipFree(A); hipFree(W); hipFree(info); hipFree(growth);
  return 0;
}
#endif

}  // namespace biem
