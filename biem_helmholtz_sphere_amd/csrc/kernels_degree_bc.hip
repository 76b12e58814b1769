// kernels_degree_bc.hip -- boundary coefficients that depend on the harmonic degree (gfx950):
//   alpha_{b,n} u + beta_{b,n} d_n u = 0 on ball b, e.g. a penetrable fluid sphere.
//
// Only the two places where alpha and beta enter are here: the per-ball tables and the projection of the incident field.  Fill,
// factorisations, density and the field kernels read the tables and never see where gj and gh came from; they are the kernels of
// kernels_fill.hip / kernels_fill_sym.hip / kernels_rhs.hip / kernels_lu.hip / kernels_uscat.hip, launched unchanged.
#include "common.hpp"

namespace biem {

// ---------------------------------------------------------------------------------------------
// per-ball tables  gj_n = alpha_n j_n + beta_n k j_n',  gh_n = alpha_n h_n + beta_n k h_n',  blc_n as k_ball_tables.
// The arithmetic per degree is k_ball_tables' own, so degree-constant coefficients give its table.
// one thread per (system, ball); alpha_n / beta_n [nb or 1][B][n_end], outputs tab[s][b][3][n_end] complex.
// ---------------------------------------------------------------------------------------------
__global__ void k_ball_tables_n(int d, int n_end, int nb, int B, const cplx* __restrict__ k, const double* __restrict__ eta,
                                const double* __restrict__ radii, int geom_batched, const cplx* __restrict__ alpha_n,
                                const cplx* __restrict__ beta_n, int ab_batched, cplx* __restrict__ tab, cplx* __restrict__ scratch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * B) return;
  int s = i / B, b = i % B;
  const cplx kk = k[s];
  const double et = eta[s];
  double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  const cplx* al = alpha_n + ((ab_batched ? (size_t)s * B : 0) + b) * n_end;
  const cplx* be = beta_n + ((ab_batched ? (size_t)s * B : 0) + b) * n_end;
  // orders up to kMaxRad: thread-local arrays; beyond (2-D only): 2 (n_end + 3) complex of global scratch per (system, ball)
  cplx Jl[kMaxRad + 3], Hl[kMaxRad + 3];
  cplx* J = scratch ? scratch + (size_t)i * 2 * (n_end + 3) : Jl;
  cplx* Hh = scratch ? J + (n_end + 3) : Hl;
  const cplx x = cscale(kk, rho);
  radial_jh(d, n_end, x, J, Hh);   // orders 0..n_end (one extra for the derivative); Im k = 0 takes the real routines
  const cplx ix = crecip(x);
  cplx* out = tab + (size_t)i * 3 * n_end;
  double rp = 1.0;               // rho^{d-1}
  for (int q = 0; q < d - 1; ++q) rp *= rho;
  cplx kd2 = make_double2(1.0, 0.0);   // k^{d-2}
  for (int q = 0; q < d - 2; ++q) kd2 = cmul(kd2, kk);
  for (int n = 0; n < n_end; ++n) {
    const cplx j = J[n], h = Hh[n];
    const cplx jp = csub(cscale(cmul(ix, j), (double)n), J[n + 1]);
    const cplx hp = csub(cscale(cmul(ix, h), (double)n), Hh[n + 1]);
    const cplx kjp = cmul(kk, jp), khp = cmul(kk, hp);
    cplx gj = cadd(cmul(al[n], j), cmul(be[n], kjp));
    cplx gh = cadd(cmul(al[n], h), cmul(be[n], khp));
    cplx blc = cscale(cmul(kd2, make_double2(et * j.x - kjp.y, et * j.y + kjp.x)), rp);
    out[n] = gj;
    out[n_end + n] = gh;
    out[2 * n_end + n] = blc;
  }
}

int launch_ball_tables_n(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                         int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_tab,
                         hipStream_t st) {
  if (p->n_end > kMaxRad && p->tree != TREE_A) { set_error("n_end=%d exceeds the built table size %d", p->n_end, kMaxRad); return BIEM_ERR_UNSUPPORTED; }
  int total = nb * B;
  if (total <= 0) return BIEM_OK;
  ProfScope ps(PK_TABLES, st);
  cplx* scratch = nullptr;
  if (p->n_end > kMaxRad) BIEM_HIPCHK(hipMallocAsync((void**)&scratch, (size_t)total * 2 * (p->n_end + 3) * sizeof(cplx), st));   // (2-D, large orders: stream-ordered)
  hipLaunchKernelGGL(k_ball_tables_n, dim3((total + 63) / 64), dim3(64), 0, st, p->d, p->n_end, nb, B, (const cplx*)d_k, d_eta, d_radii,
                     geom_batched, (const cplx*)d_alpha_n, (const cplx*)d_beta_n, ab_batched, (cplx*)d_tab, scratch);
  BIEM_LAUNCHCHK();
  if (scratch) BIEM_HIPCHK(hipFreeAsync(scratch, st));
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// The symmetric form scales by R = 1 / sqrt(gj gh) per (ball, degree).  A degree the ball does not scatter (gj_n = 0: a transparent
// sphere, k_b = k and density ratio 1) makes R infinite and the symmetric fill NaN; such a system is marked rejected, so the caller
// solves it with the pivoted LU, whose equilibrated form divides by gh only.  Every thread that finds one stores the same code.
// ---------------------------------------------------------------------------------------------
__global__ void k_flag_unscalable(int n_end, int B, int nb, const cplx* __restrict__ tab, int* __restrict__ info, int code) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // i = (s*B + b)*n_end + n
  if (i >= (long long)nb * B * n_end) return;
  const int n = (int)(i % n_end);
  const long long sb = i / n_end;
  const cplx* t = tab + (size_t)sb * 3 * n_end;
  const cplx r = crecip(zsqrt(cmul(t[n], t[n_end + n])));
  const cplx q = cmul(t[n], r);                                           // gj / sqrt(gj gh), the row factor of the symmetric fill
  if (!(isfinite(r.x) && isfinite(r.y) && isfinite(q.x) && isfinite(q.y))) info[sb / B] = code;
}

int launch_flag_unscalable(const biem_plan* p, int nb, int B, const double* d_tab, int* d_info, int code, hipStream_t st) {
  const long long total = (long long)nb * B * p->n_end;
  if (total <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_flag_unscalable, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p->n_end, B, nb, (const cplx*)d_tab, d_info, code);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// RHS projection with the degree known only after it:
//   f[row][h] = -( alpha_{n(h)} sum_q gu[row][q] W[q][h] + beta_{n(h)} sum_q gdn[row][q] W[q][h] )
// The two forms of k_rhs_project / k_rhs_project_few with two accumulators per row: one read of W[q][h] serves both sample sets, the
// coefficients of the row's ball enter in the epilogue.  RT rows of EACH set are staged, so at RT = 4 the LDS and the accumulator
// registers are those of the one-set kernels at RT = 8 (and row blocks go on grid.x: no limit of 65535 of them).  A null sample set is zero and costs neither loads nor multiply-adds.
// ---------------------------------------------------------------------------------------------
__device__ inline cplx degree_mix(const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n, int ab_batched, int n_end, int B,
                                  long long s, long long b, int n, cplx au, cplx ad) {
  const size_t o = ((ab_batched ? (size_t)s * B : 0) + (size_t)b) * n_end + n;
  const cplx t = cadd(cmul(alpha_n[o], au), cmul(beta_n[o], ad));
  return make_double2(-t.x, -t.y);
}

template <int RT>
__global__ void __launch_bounds__(256) k_rhs_project_n(int H, int Q, int rows, int B, int nrhs, int n_end, const cplx* __restrict__ gu,
                                                        const cplx* __restrict__ gd, const cplx* __restrict__ W,
                                                        const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n, int ab_batched,
                                                        const int* __restrict__ deg, cplx* __restrict__ f, long long sys_stride,
                                                        long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [2][RT][QC]: u_in samples, then d_n u_in samples
  constexpr int QC = 256;
  cplx* su = sg;
  cplx* sd = sg + RT * QC;
  int row0 = blockIdx.x * RT;
  int h = blockIdx.y * 256 + threadIdx.x;
  cplx au[RT], ad[RT];
  for (int r = 0; r < RT; ++r) au[r] = ad[r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      int r = i / QC, q = i % QC;
      const bool in = row0 + r < rows && q < qn;
      if (gu) su[i] = in ? gu[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
      if (gd) sd[i] = in ? gd[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (h < H) {
      for (int q = 0; q < qn; ++q) {
        cplx w = W[(size_t)(q0 + q) * H + h];
        if (gu) {
#pragma unroll
          for (int r = 0; r < RT; ++r) au[r] = cfma(su[r * QC + q], w, au[r]);
        }
        if (gd) {
#pragma unroll
          for (int r = 0; r < RT; ++r) ad[r] = cfma(sd[r * QC + q], w, ad[r]);
        }
      }
    }
  }
  if (h < H) {
    const int n = deg[h];
    for (int r = 0; r < RT; ++r) {
      int row = row0 + r;
      if (row >= rows) break;
      long long b = row % B, sr = row / B, rr = sr % nrhs, s = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      f[s * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride] =
          degree_mix(alpha_n, beta_n, ab_batched, n_end, B, s, b, n, au[r], ad[r]);
    }
  }
}

// Few rows: a workgroup takes 16 harmonics and splits the quadrature points over its 16 lane groups, as k_rhs_project_few does; the
// partial sums of both sets are reduced through LDS in a fixed order (deterministic).
template <int RT>
__global__ void __launch_bounds__(256) k_rhs_project_n_few(int H, int Q, int rows, int B, int nrhs, int n_end, const cplx* __restrict__ gu,
                                                            const cplx* __restrict__ gd, const cplx* __restrict__ W,
                                                            const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n,
                                                            int ab_batched, const int* __restrict__ deg, cplx* __restrict__ f,
                                                            long long sys_stride, long long elem_stride, long long rhs_stride,
                                                            const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [2][RT][QC]; afterwards the partial sums [2][16 slices][RT][16]  (RT * 256 complex per set either way)
  constexpr int QC = 256;
  cplx* su = sg;
  cplx* sd = sg + RT * QC;
  const int row0 = blockIdx.x * RT;
  const int hl = threadIdx.x & 15, qs = threadIdx.x >> 4;
  const int h = blockIdx.y * 16 + hl, hc = h < H ? h : H - 1;
  cplx au[RT], ad[RT];
  for (int r = 0; r < RT; ++r) au[r] = ad[r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    const int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      const int r = i / QC, q = i % QC;
      const bool in = row0 + r < rows && q < qn;
      if (gu) su[i] = in ? gu[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
      if (gd) sd[i] = in ? gd[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int q = qs; q < qn; q += 16) {
      const cplx w = W[(size_t)(q0 + q) * H + hc];
      if (gu) {
#pragma unroll
        for (int r = 0; r < RT; ++r) au[r] = cfma(su[r * QC + q], w, au[r]);
      }
      if (gd) {
#pragma unroll
        for (int r = 0; r < RT; ++r) ad[r] = cfma(sd[r * QC + q], w, ad[r]);
      }
    }
  }
  __syncthreads();
  for (int r = 0; r < RT; ++r) {
    su[(qs * RT + r) * 16 + hl] = au[r];
    sd[(qs * RT + r) * 16 + hl] = ad[r];
  }
  __syncthreads();
  if (threadIdx.x < RT * 16) {
    const int r = threadIdx.x >> 4, row = row0 + r;
    cplx tu = make_double2(0.0, 0.0), td = make_double2(0.0, 0.0);
    for (int z = 0; z < 16; ++z) {
      const cplx vu = su[(z * RT + r) * 16 + hl], vd = sd[(z * RT + r) * 16 + hl];
      tu.x += vu.x; tu.y += vu.y;
      td.x += vd.x; td.y += vd.y;
    }
    if (row < rows && h < H) {
      long long b = row % B, sr = row / B, rr = sr % nrhs, sy = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      f[sy * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride] =
          degree_mix(alpha_n, beta_n, ab_batched, n_end, B, sy, b, deg[h], tu, td);
    }
  }
}

int launch_rhs_project_n(const biem_plan* p, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn, const double* d_alpha_n,
                         const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride, long long elem_stride,
                         long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) {
  if (nrhs < 1) { set_error("biem_rhs_project_n: nrhs < 1"); return BIEM_ERR_ARG; }
  int rows = nb * nrhs * B;
  if (rows <= 0) return BIEM_OK;
  constexpr int RT = 4;
  // (row blocks on grid.x, which holds 2^31 - 1: any rows an int counts; harmonic blocks, H / 16 at most, on grid.y)
  size_t shm = (size_t)2 * RT * 256 * sizeof(cplx);
  const int sets = (d_gu ? 1 : 0) + (d_gdn ? 1 : 0);
  ProfScope ps(PK_RHS, st, 8.0 * sets * (double)rows * p->Q * p->H);
  if ((long long)((p->H + 255) / 256) * ((rows + RT - 1) / RT) < 128) {
    hipLaunchKernelGGL(k_rhs_project_n_few<RT>, dim3((rows + RT - 1) / RT, (p->H + 15) / 16), dim3(256), shm, st, p->H, p->Q, rows, B,
                       nrhs, p->n_end, (const cplx*)d_gu, (const cplx*)d_gdn, (const cplx*)p->d_W, (const cplx*)d_alpha_n,
                       (const cplx*)d_beta_n, ab_batched, p->d_deg, (cplx*)d_f, sys_stride, elem_stride, rhs_stride,
                       slot_order ? p->d_hpos : nullptr, split);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  hipLaunchKernelGGL(k_rhs_project_n<RT>, dim3((rows + RT - 1) / RT, (p->H + 255) / 256), dim3(256), shm, st, p->H, p->Q, rows, B,
                     nrhs, p->n_end, (const cplx*)d_gu, (const cplx*)d_gdn, (const cplx*)p->d_W, (const cplx*)d_alpha_n,
                     (const cplx*)d_beta_n, ab_batched, p->d_deg, (cplx*)d_f, sys_stride, elem_stride, rhs_stride,
                     slot_order ? p->d_hpos : nullptr, split);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
