// kernels_power.hip -- extinction and absorbed power per ball from quantities the solve already has (gfx950).
//
// Real k, outgoing coefficients c_h = density_h blc_n(rho) (what k_uscat_coef forms), U_h / V_h the projections of u_in / d_n u_in on
// the surface of the ball onto Y_h (biem_rhs_project of the unweighted samples), power = (1/k) Im oint conj(u) d_n u dS:
//   P_ext = -(rho^{d-1} / k) sum_h Im[ conj(U_h) k c_h h_n'(k rho) + conj(c_h h_n(k rho)) V_h ]
//   P_abs = rho^{d-1} k (k rho)^{2-2d} sum_h Im(alpha_n conj beta_n) |c_h|^2 / |gj_n|^2          (Wronskian j y' - y j' = x^{1-d})
// Only coefficients enter, never harmonics: every tree the plans cover, the chains d >= 5 included.
#include "common.hpp"

namespace biem {

// One wave per (ball, right-hand side, system) = (blockIdx.x, .y, .z).  Lane 0 runs the radial recurrences at k rho into LDS, the
// lanes then form the per-degree factors (k h_n' = k ((n / x) h_n - h_{n+1}); the absorption weight Im(alpha_n conj beta_n), exactly 0
// where the pair is lossless - no division there, so gj_n = 0 of a lossless ball is harmless - and NaN where a lossy degree has gj_n
// zero or not finite; 1 / gj_n by a scaled division) and stride over the harmonics.  The absorbed term is w |c_h / gj_n|^2, the quotient
// first: c_h and gj_n both fall like j_n(k rho), and their squares leave the fp64 range (|gj_n| < 1e-154: tree a from degree 283 at
// k rho = 60) long before they do.  wave_sum adds in a fixed order: no atomics, two calls agree bit for bit.
// alpha / beta: [nb or 1][B] (per_degree = 0) or [nb or 1][B][n_end]; tab [nb][B][3][n_end] (gj, gh, blc); density, pu, pv
// [nb][nrhs][B][H]; out [nb][nrhs][B][2] = (P_ext, P_abs).
__global__ void __launch_bounds__(64) k_power(int d, int H, int n_end, const int* __restrict__ deg, int B, int nrhs,
                                               const cplx* __restrict__ k, const double* __restrict__ radii, int geom_batched,
                                               const cplx* __restrict__ alpha, const cplx* __restrict__ beta, int ab_batched, int per_degree,
                                               const cplx* __restrict__ tab, const cplx* __restrict__ dens, const cplx* __restrict__ pu,
                                               const cplx* __restrict__ pv, double* __restrict__ out) {
  __shared__ cplx sJ[kMaxRad + 3], sH[kMaxRad + 3];     // radial_jh: n_end + 1 entries (+ its order shift for d >= 4)
  __shared__ cplx sHp[kMaxRad];                         // k h_n'(k rho)
  __shared__ double sA[kMaxRad];                        // Im(alpha_n conj beta_n)
  __shared__ cplx sIg[kMaxRad];                         // 1 / gj_n of a lossy degree
  const int b = blockIdx.x, r = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  const double kr = k[s].x;
  const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  const double x = kr * rho, ix = 1.0 / x;
  const cplx* t = tab + ((size_t)s * B + b) * 3 * n_end;
  if (lane == 0) radial_jh(d, n_end, make_double2(x, 0.0), sJ, sH);
  __syncthreads();
  const size_t ab0 = (ab_batched ? (size_t)s * B : 0) + b;
  for (int n = lane; n < n_end; n += 64) {
    sHp[n] = cscale(csub(cscale(sH[n], (double)n * ix), sH[n + 1]), kr);
    const cplx a = per_degree ? alpha[ab0 * n_end + n] : alpha[ab0];
    const cplx be = per_degree ? beta[ab0 * n_end + n] : beta[ab0];
    const double w = a.y * be.x - a.x * be.y;           // Im(alpha conj beta)
    double v = 0.0;
    cplx ig = make_double2(0.0, 0.0);
    if (w != 0.0) {
      const cplx gj = t[n];
      const double m = fmax(fabs(gj.x), fabs(gj.y));
      v = nan("");
      if (isfinite(m) && m > 0.0) {                     // (scaled by the larger component: no underflow of the squares)
        const double xs = gj.x / m, ys = gj.y / m, den = (xs * xs + ys * ys) * m;
        ig = make_double2(xs / den, -ys / den);
        v = w;
      }
    }
    sA[n] = v;
    sIg[n] = ig;
  }
  __syncthreads();
  const size_t row = (((size_t)s * nrhs + r) * B + b) * H;
  double pe = 0.0, pa = 0.0;
  for (int h = lane; h < H; h += 64) {
    const int n = deg[h];
    const cplx c = cmul(dens[row + h], t[2 * n_end + n]);
    const cplx U = pu[row + h], V = pv[row + h];
    const cplx dc = cmul(c, sHp[n]), vc = cmul(c, sH[n]);          // k c h_n', c h_n
    pe += (U.x * dc.y - U.y * dc.x) + (vc.x * V.y - vc.y * V.x);   // Im[conj(U) k c h_n'] + Im[conj(c h_n) V]
    const double w = sA[n];
    if (w != 0.0) {
      const cplx q = cmul(c, sIg[n]);
      pa += w * (q.x * q.x + q.y * q.y);
    }
  }
  pe = wave_sum(pe);
  pa = wave_sum(pa);
  if (lane == 0) {
    double rp = 1.0, ixp = 1.0;                         // rho^{d-1}, (k rho)^{2-2d}
    for (int q = 0; q < d - 1; ++q) { rp *= rho; ixp *= ix * ix; }
    double* o = out + (((size_t)s * nrhs + r) * B + b) * 2;
    o[0] = -(rp / kr) * pe;
    o[1] = rp * kr * ixp * pa;
  }
}

int launch_power(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_radii, int geom_batched,
                 const double* d_alpha, const double* d_beta, int ab_batched, bool per_degree, const double* d_tab,
                 const double* d_density, const double* d_pu, const double* d_pv, double* d_out, hipStream_t st) {
  // the kernel's radial arrays: n_end + 1 orders plus the order shift of radial_jh (d >= 4)
  if (p->n_end > kMaxRad || p->n_end + 1 + (p->d >= 4 ? radial_shift(p->d) : 0) > kMaxRad + 3) {
    set_error("biem_power: n_end=%d exceeds the built table size %d", p->n_end, kMaxRad);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (nb <= 0 || B <= 0 || nrhs <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_power, dim3(B, nrhs, nb), dim3(64), 0, st, p->d, p->H, p->n_end, p->d_deg, B, nrhs, (const cplx*)d_k, d_radii,
                     geom_batched, (const cplx*)d_alpha, (const cplx*)d_beta, ab_batched, per_degree ? 1 : 0, (const cplx*)d_tab,
                     (const cplx*)d_density, (const cplx*)d_pu, (const cplx*)d_pv, d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
