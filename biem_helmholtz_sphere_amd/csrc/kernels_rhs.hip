// kernels_rhs.hip -- right-hand-side projection, the R W^H transform of the symmetric path and the density scaling (gfx950).
//
// Replaces the span _biem.py:627-639 of the reference.
#include "common.hpp"

namespace biem {

// ---------------------------------------------------------------------------------------------
// RHS projection  f[row][h] = sum_q g[row][q] W[q][h]   (ush.expand, _biem.py:627-639)
// block = RT rows x 256 columns; g rows staged in LDS, W streamed coalesced along h.
// ---------------------------------------------------------------------------------------------
template <int RT>
__global__ void __launch_bounds__(256) k_rhs_project(int H, int Q, int rows, int B, int nrhs, const cplx* __restrict__ g,
                                                      const cplx* __restrict__ W, cplx* __restrict__ f, long long sys_stride,
                                                      long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [RT][QC]
  constexpr int QC = 256;
  int row0 = blockIdx.y * RT;
  int h = blockIdx.x * 256 + threadIdx.x;
  cplx acc[RT];
  for (int r = 0; r < RT; ++r) acc[r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      int r = i / QC, q = i % QC;
      sg[i] = (row0 + r < rows && q < qn) ? g[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (h < H) {
      for (int q = 0; q < qn; ++q) {
        cplx w = W[(size_t)(q0 + q) * H + h];
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = cfma(sg[r * QC + q], w, acc[r]);
      }
    }
  }
  if (h < H) {
    for (int r = 0; r < RT; ++r) {
      int row = row0 + r;
      if (row >= rows) break;
      long long b = row % B, sr = row / B, rr = sr % nrhs, s = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      f[(long long)s * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride] = acc[r];
    }
  }
}

// Few rows (one system per call: B nrhs rows): the form above leaves the whole sum over q to (H / 256) x (rows / RT) workgroups - 4 at cfg 3,
// 435 us.  Here a workgroup takes 16 harmonics and splits the quadrature points over its 16 lane groups (partial sums reduced through
// LDS in a fixed order: deterministic), so H / 16 workgroups per row block share the stream of W.
template <int RT>
__global__ void __launch_bounds__(256) k_rhs_project_few(int H, int Q, int rows, int B, int nrhs, const cplx* __restrict__ g,
                                                          const cplx* __restrict__ W, cplx* __restrict__ f, long long sys_stride,
                                                          long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [RT][QC]; afterwards the partial sums [16 slices][RT][16]
  constexpr int QC = 256;
  const int row0 = blockIdx.y * RT;
  const int hl = threadIdx.x & 15, qs = threadIdx.x >> 4;
  const int h = blockIdx.x * 16 + hl, hc = h < H ? h : H - 1;
  cplx acc[RT];
  for (int r = 0; r < RT; ++r) acc[r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    const int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      const int r = i / QC, q = i % QC;
      sg[i] = (row0 + r < rows && q < qn) ? g[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int q = qs; q < qn; q += 16) {
      const cplx w = W[(size_t)(q0 + q) * H + hc];
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = cfma(sg[r * QC + q], w, acc[r]);
    }
  }
  __syncthreads();
  for (int r = 0; r < RT; ++r) sg[(qs * RT + r) * 16 + hl] = acc[r];
  __syncthreads();
  if (threadIdx.x < RT * 16) {
    const int r = threadIdx.x >> 4, row = row0 + r;
    cplx t = make_double2(0.0, 0.0);
    for (int z = 0; z < 16; ++z) { const cplx v = sg[(z * RT + r) * 16 + hl]; t.x += v.x; t.y += v.y; }
    if (row < rows && h < H) {
      long long b = row % B, sr = row / B, rr = sr % nrhs, sy = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      f[(long long)sy * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride] = t;
    }
  }
}

int launch_rhs_project(const biem_plan* p, int nb, int B, int nrhs, const double* d_g, double* d_f, long long sys_stride,
                       long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) {
  if (nrhs < 1) { set_error("biem_rhs_project: nrhs < 1"); return BIEM_ERR_ARG; }
  int rows = nb * nrhs * B;
  if (rows <= 0) return BIEM_OK;
  constexpr int RT = 8;
  size_t shm = (size_t)RT * 256 * sizeof(cplx);
  ProfScope ps(PK_RHS, st, 8.0 * (double)rows * p->Q * p->H);
  if ((long long)((p->H + 255) / 256) * ((rows + RT - 1) / RT) < 128) {
    hipLaunchKernelGGL(k_rhs_project_few<RT>, dim3((p->H + 15) / 16, (rows + RT - 1) / RT), dim3(256), shm, st, p->H, p->Q, rows, B,
                       nrhs, (const cplx*)d_g, (const cplx*)p->d_W, (cplx*)d_f, sys_stride, elem_stride, rhs_stride,
                       slot_order ? p->d_hpos : nullptr, split);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  hipLaunchKernelGGL(k_rhs_project<RT>, dim3((p->H + 255) / 256, (rows + RT - 1) / RT), dim3(256), shm, st, p->H, p->Q, rows, B,
                     nrhs, (const cplx*)d_g, (const cplx*)p->d_W, (cplx*)d_f, sys_stride, elem_stride, rhs_stride,
                     slot_order ? p->d_hpos : nullptr, split);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// right-hand sides / solutions of the complex-symmetric form (the matrix itself comes from kernels_fill_sym.hip):
//   f~ = R W^H f  before the factorisation,   x = W R^-1 x~  after it,   R = diag(1 / sqrt(gj gh)) per (ball, degree).
// The right-hand-side columns hold a ball's harmonics in the internal slot order (biem_rhs_project with the plan's hpos: h of
// unit u in slot u, its partner p in slot U + spos[u]), so both transforms work in place on the two slots of a unit.
// ---------------------------------------------------------------------------------------------
__device__ inline cplx sym_r(const cplx* __restrict__ tball, int n_end, int n) {   // 1 / sqrt(gj gh)
  return crecip(zsqrt(cmul(tball[n], tball[n_end + n])));
}

__global__ void __launch_bounds__(256) k_sym_rhs(int H, int U, int n_end, int B, int nrhs, int n_pad, const int* __restrict__ units,
                                                  const int* __restrict__ spos, const int* __restrict__ deg, const cplx* __restrict__ tab,
                                                  cplx* __restrict__ A, long long lda, long long sys_stride, int inverse, SplitMap sm) {
  const int s = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;                 // (unit over all balls, rhs)
  if (t >= B * U * nrhs) return;
  const int q = t % nrhs, ru = t / nrhs, br = ru / U, ur = ru - br * U;
  const int rh = units[2 * ur], rp = units[2 * ur + 1];
  const cplx* ts = tab + ((size_t)s * B + br) * 3 * n_end;
  cplx* F = A + (size_t)s * sys_stride + n_pad + q;
  cplx* pc = F + sm.rhs_off(br, H, ur, lda);
  cplx* psn = F + sm.rhs_off(br, H, U + (rp != rh ? spos[ur] : 0), lda);
  const double q2 = 0.70710678118654752440;
  if (!inverse) {
    const cplx r = sym_r(ts, n_end, deg[rh]);
    const cplx fh = *pc;
    if (rp == rh) { *pc = cmul(fh, r); return; }
    const cplx fp = *psn;
    const cplx a = make_double2((fh.x + fp.x) * q2, (fh.y + fp.y) * q2), d = make_double2((fh.x - fp.x) * q2, (fh.y - fp.y) * q2);
    *pc = cmul(a, r);
    *psn = cmul(make_double2(-d.y, d.x), r);                    // i (f_h - f_p) / sqrt2
  } else {
    const cplx g = zsqrt(cmul(ts[deg[rh]], ts[n_end + deg[rh]]));      // 1 / r
    const cplx yh = cmul(*pc, g);
    if (rp == rh) { *pc = yh; return; }
    const cplx yp = cmul(*psn, g);                              // x_h = (y_c - i y_s)/sqrt2, x_p = (y_c + i y_s)/sqrt2
    *pc = make_double2((yh.x + yp.y) * q2, (yh.y - yp.x) * q2);
    *psn = make_double2((yh.x - yp.y) * q2, (yh.y + yp.x) * q2);
  }
}

int launch_sym_rhs(const biem_plan* p, int nb, int B, int nrhs, int n_pad, const double* d_tab, double* d_rhs, long long lda,
                   long long sys_stride, bool inverse_on_solution, hipStream_t st, const SplitMap& split) {
  const int U = (int)(p->units.size() / 2);
  if (nb <= 0 || B <= 0 || nrhs <= 0) return BIEM_OK;
  if (nb > 65535) { set_error("biem symmetric path: at most 65535 systems per call"); return BIEM_ERR_ARG; }
  ProfScope ps(PK_SWAP, st, 0.0);   // class 4: row interchanges in the LU, these transforms in the symmetric path
  // the kernel addresses the right-hand sides as column n_pad of its pointer argument: it gets the device address n_pad entries in front
  // of them (formed as a number: where the columns are an array of their own there is no such object, and none is touched)
  cplx* base = reinterpret_cast<cplx*>(reinterpret_cast<uintptr_t>(d_rhs) - (uintptr_t)n_pad * sizeof(cplx));
  hipLaunchKernelGGL(k_sym_rhs, dim3((B * U * nrhs + 255) / 256, nb), dim3(256), 0, st, p->H, U, p->n_end, B, nrhs, n_pad, p->d_units,
                     p->d_spos, p->d_deg, (const cplx*)d_tab, base, lda, sys_stride, inverse_on_solution ? 1 : 0, split);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// density = x / (gh * blc)   (reference scaling of the unknown; single-ball shortcut _biem.py:673-690 with x = f)
// ---------------------------------------------------------------------------------------------
__global__ void k_density(int H, int n_end, int B, int nrhs, long long total, const int* __restrict__ deg, const cplx* __restrict__ x,
                          long long sys_stride, long long elem_stride, long long rhs_stride, const cplx* __restrict__ tab,
                          cplx* __restrict__ dens, const int* __restrict__ hpos, SplitMap sm) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // i = ((s*nrhs + r)*B + b)*H + h
  if (i >= total) return;
  int h = (int)(i % H);
  long long srb = i / H;
  long long b = srb % B, sr = srb / B, r = sr % nrhs, s = sr / nrhs;
  int n = deg[h];
  const cplx* t = tab + (size_t)(s * B + b) * 3 * n_end;
  cplx v = x[s * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + r * rhs_stride];
  dens[i] = cmul(v, crecip(cmul(t[n_end + n], t[2 * n_end + n])));
}

int launch_density(const biem_plan* p, int nb, int B, int nrhs, const double* d_x, long long sys_stride, long long elem_stride,
                   long long rhs_stride, const double* d_tab, double* d_density, hipStream_t st, bool slot_order, const SplitMap& split) {
  if (nrhs < 1) { set_error("biem_density: nrhs < 1"); return BIEM_ERR_ARG; }
  long long total = (long long)nb * nrhs * B * p->H;
  if (total <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_density, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p->H, p->n_end, B, nrhs, total, p->d_deg,
                     (const cplx*)d_x, sys_stride, elem_stride, rhs_stride, (const cplx*)d_tab, (cplx*)d_density, slot_order ? p->d_hpos : nullptr, split);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
