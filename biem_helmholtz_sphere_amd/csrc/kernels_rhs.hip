// kernels_rhs.hip -- right-hand-side projection of boundary samples (one or two sets), the R W^H transform of the symmetric path with
// the test of its scaling, and the density scaling (gfx950).
//
// Replaces the span _biem.py:627-639 of the reference.
#include "common.hpp"
#include <climits>

namespace biem {

// ---------------------------------------------------------------------------------------------
// RHS projection  P[g][row][h] = sum_q g[row][q] W[q][h]   (ush.expand, _biem.py:627-639), one text for SETS sets of samples:
//   SETS == 1:  f = P[g0]                                        (plain coefficients: the samples arrive mixed)
//   SETS == 2:  f = -(alpha_{n(h)} P[g0] + beta_{n(h)} P[g1])     (the degree of a harmonic is known only after the projection, so the
//               coefficients of the row's ball enter in the epilogue; a null set is zero and costs neither loads nor multiply-adds)
// block = RT rows of EACH set x 256 columns, RT = 8 / SETS: 8 staged rows (32 KiB of LDS) and 8 accumulators per lane either way; the
// rows are staged in LDS, W is streamed coalesced along h, and one read of W[q][h] serves both sets.
// Grid: flat (flat_block below), so the row blocks are bounded by what one grid dimension holds and not by the 65535 of grid.y.
// ---------------------------------------------------------------------------------------------
__device__ inline cplx degree_mix(const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n, int ab_batched, int n_end, int B,
                                  long long s, long long b, int n, cplx au, cplx ad) {
  const size_t o = ((ab_batched ? (size_t)s * B : 0) + (size_t)b) * n_end + n;
  const cplx t = cadd(cmul(alpha_n[o], au), cmul(beta_n[o], ad));
  return make_double2(-t.x, -t.y);
}

// (row block, harmonic block) of a workgroup of the flat grid.  One set: the harmonic block runs fastest; two sets: the row block does -
// the orders the kernels had on two grid dimensions and are measured in (two sets, harmonic block fastest: 1.6 % slower at H = 400).
// (The division runs on the vector unit; readfirstlane returns the wave-uniform quotient to a scalar register - without it the
// few-rows kernels hold 4 more VGPRs and one set loses a wave per SIMD.)
template <int SETS>
__device__ inline void flat_block(unsigned n_hblocks, unsigned n_rblocks, unsigned& rb, unsigned& hb) {
  const unsigned inner = SETS == 1 ? n_hblocks : n_rblocks, outer = __builtin_amdgcn_readfirstlane(blockIdx.x / inner);
  const unsigned rest = blockIdx.x - outer * inner;
  rb = SETS == 1 ? outer : rest;
  hb = SETS == 1 ? rest : outer;
}

template <int SETS>
__global__ void __launch_bounds__(256) k_rhs_project(int H, int Q, int rows, int B, int nrhs, int n_end, const cplx* __restrict__ g0,
                                                      const cplx* __restrict__ g1, const cplx* __restrict__ W,
                                                      const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n, int ab_batched,
                                                      const int* __restrict__ deg, cplx* __restrict__ f, long long sys_stride,
                                                      long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [SETS][RT][QC]
  constexpr int RT = 8 / SETS, QC = 256;
  auto set = [&](int t) { return t == 0 ? g0 : g1; };
  unsigned rb, hb;
  flat_block<SETS>((unsigned)(H + 255) / 256, (unsigned)(rows + RT - 1) / RT, rb, hb);
  const int row0 = (int)rb * RT;
  const int h = (int)hb * 256 + threadIdx.x;
  cplx acc[SETS][RT];
#pragma unroll
  for (int t = 0; t < SETS; ++t)
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[t][r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      int r = i / QC, q = i % QC;
      const bool in = row0 + r < rows && q < qn;
#pragma unroll
      for (int t = 0; t < SETS; ++t)
        if (SETS == 1 || set(t)) sg[t * RT * QC + i] = in ? set(t)[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (h < H) {
      for (int q = 0; q < qn; ++q) {
        cplx w = W[(size_t)(q0 + q) * H + h];
#pragma unroll
        for (int t = 0; t < SETS; ++t)
          if (SETS == 1 || set(t)) {
#pragma unroll
            for (int r = 0; r < RT; ++r) acc[t][r] = cfma(sg[(t * RT + r) * QC + q], w, acc[t][r]);
          }
      }
    }
  }
  if (h < H) {
    for (int r = 0; r < RT; ++r) {
      int row = row0 + r;
      if (row >= rows) break;
      long long b = row % B, sr = row / B, rr = sr % nrhs, s = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      cplx& out = f[s * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride];
      if constexpr (SETS == 1) out = acc[0][r];
      else out = degree_mix(alpha_n, beta_n, ab_batched, n_end, B, s, b, deg[h], acc[0][r], acc[1][r]);
    }
  }
}

// Few rows (one system per call: B nrhs rows): the form above leaves the whole sum over q to (H / 256) x (rows / RT) workgroups - 4 at cfg 3,
// 435 us.  Here a workgroup takes 16 harmonics and splits the quadrature points over its 16 lane groups (partial sums of every set reduced
// through LDS in a fixed order: deterministic), so H / 16 workgroups per row block share the stream of W.
template <int SETS>
__global__ void __launch_bounds__(256) k_rhs_project_few(int H, int Q, int rows, int B, int nrhs, int n_end, const cplx* __restrict__ g0,
                                                          const cplx* __restrict__ g1, const cplx* __restrict__ W,
                                                          const cplx* __restrict__ alpha_n, const cplx* __restrict__ beta_n, int ab_batched,
                                                          const int* __restrict__ deg, cplx* __restrict__ f, long long sys_stride,
                                                          long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  extern __shared__ cplx sg[];   // [SETS][RT][QC]; afterwards the partial sums [SETS][16 slices][RT][16]  (RT * 256 complex per set either way)
  constexpr int RT = 8 / SETS, QC = 256;
  auto set = [&](int t) { return t == 0 ? g0 : g1; };
  unsigned rb, hb;
  flat_block<SETS>((unsigned)(H + 15) / 16, (unsigned)(rows + RT - 1) / RT, rb, hb);
  const int row0 = (int)rb * RT;
  const int hl = threadIdx.x & 15, qs = threadIdx.x >> 4;
  const int h = (int)hb * 16 + hl, hc = h < H ? h : H - 1;
  cplx acc[SETS][RT];
#pragma unroll
  for (int t = 0; t < SETS; ++t)
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[t][r] = make_double2(0.0, 0.0);
  for (int q0 = 0; q0 < Q; q0 += QC) {
    const int qn = min(QC, Q - q0);
    __syncthreads();
    for (int i = threadIdx.x; i < RT * QC; i += 256) {
      const int r = i / QC, q = i % QC;
      const bool in = row0 + r < rows && q < qn;
#pragma unroll
      for (int t = 0; t < SETS; ++t)
        if (SETS == 1 || set(t)) sg[t * RT * QC + i] = in ? set(t)[(size_t)(row0 + r) * Q + q0 + q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int q = qs; q < qn; q += 16) {
      const cplx w = W[(size_t)(q0 + q) * H + hc];
#pragma unroll
      for (int t = 0; t < SETS; ++t)
        if (SETS == 1 || set(t)) {
#pragma unroll
          for (int r = 0; r < RT; ++r) acc[t][r] = cfma(sg[(t * RT + r) * QC + q], w, acc[t][r]);
        }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < SETS; ++t)
#pragma unroll
    for (int r = 0; r < RT; ++r) sg[t * RT * QC + (qs * RT + r) * 16 + hl] = acc[t][r];
  __syncthreads();
  if (threadIdx.x < RT * 16) {
    const int r = threadIdx.x >> 4, row = row0 + r;
    cplx sum[SETS];
#pragma unroll
    for (int t = 0; t < SETS; ++t) sum[t] = make_double2(0.0, 0.0);
    for (int z = 0; z < 16; ++z) {
#pragma unroll
      for (int t = 0; t < SETS; ++t) { const cplx v = sg[t * RT * QC + (z * RT + r) * 16 + hl]; sum[t].x += v.x; sum[t].y += v.y; }
    }
    if (row < rows && h < H) {
      long long b = row % B, sr = row / B, rr = sr % nrhs, sy = sr / nrhs;     // row = (s*nrhs + rr)*B + b
      cplx& out = f[sy * sys_stride + sm.rhs_off((int)b, H, hpos ? hpos[h] : h, elem_stride) + rr * rhs_stride];
      if constexpr (SETS == 1) out = sum[0];
      else out = degree_mix(alpha_n, beta_n, ab_batched, n_end, B, sy, b, deg[h], sum[0], sum[1]);
    }
  }
}

// The one launcher: the form rule, the shared-memory size, the profile scope and the slot order are decided here for both SETS.
// The full form runs from 128 workgroups on (1017 rows of one set, 509 of two, at H <= 256); below, the few-rows form.
template <int SETS>
static int launch_project(const char* who, const biem_plan* p, int nb, int B, int nrhs, const double* d_g0, const double* d_g1,
                          const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) {
  if (nrhs < 1) { set_error("%s: nrhs < 1", who); return BIEM_ERR_ARG; }
  int rows = nb * nrhs * B;
  if (rows <= 0) return BIEM_OK;
  constexpr int RT = 8 / SETS;
  const size_t shm = (size_t)SETS * RT * 256 * sizeof(cplx);
  const int sets = SETS == 1 ? 1 : (d_g0 ? 1 : 0) + (d_g1 ? 1 : 0);
  ProfScope ps(PK_RHS, st, 8.0 * sets * (double)rows * p->Q * p->H);
  const long long row_blocks = (rows + RT - 1) / RT;
  const bool few = (long long)((p->H + 255) / 256) * row_blocks < 128;
  const long long blocks = row_blocks * (few ? (p->H + 15) / 16 : (p->H + 255) / 256);
  if (blocks > INT_MAX) { set_error("%s: %lld workgroups exceed one grid dimension", who, blocks); return BIEM_ERR_ARG; }
  hipLaunchKernelGGL(few ? &k_rhs_project_few<SETS> : &k_rhs_project<SETS>, dim3((unsigned)blocks), dim3(256), shm, st, p->H, p->Q, rows, B,
                     nrhs, p->n_end, (const cplx*)d_g0, (const cplx*)d_g1, (const cplx*)p->d_W, (const cplx*)d_alpha_n,
                     (const cplx*)d_beta_n, ab_batched, p->d_deg, (cplx*)d_f, sys_stride, elem_stride, rhs_stride,
                     slot_order ? p->d_hpos : nullptr, split);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_rhs_project(const biem_plan* p, int nb, int B, int nrhs, const double* d_g, double* d_f, long long sys_stride,
                       long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) {
  return launch_project<1>("biem_rhs_project", p, nb, B, nrhs, d_g, nullptr, nullptr, nullptr, 0, d_f, sys_stride, elem_stride, rhs_stride, st,
                           slot_order, split);
}

int launch_rhs_project_n(const biem_plan* p, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn, const double* d_alpha_n,
                         const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride, long long elem_stride,
                         long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) {
  return launch_project<2>("biem_rhs_project_n", p, nb, B, nrhs, d_gu, d_gdn, d_alpha_n, d_beta_n, ab_batched, d_f, sys_stride, elem_stride,
                           rhs_stride, st, slot_order, split);
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

// A degree the ball does not scatter (gj_n = 0: a transparent sphere, k_b = k and density ratio 1) makes R infinite and the symmetric
// fill NaN; such a system is marked rejected, so the caller solves it with the pivoted LU, whose equilibrated form divides by gh only.
// Every thread that finds one stores the same code.
__global__ void k_flag_unscalable(int n_end, int B, int nb, const cplx* __restrict__ tab, int* __restrict__ info, int code) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // i = (s*B + b)*n_end + n
  if (i >= (long long)nb * B * n_end) return;
  const int n = (int)(i % n_end);
  const long long sb = i / n_end;
  const cplx* t = tab + (size_t)sb * 3 * n_end;
  const cplx r = sym_r(t, n_end, n);
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
