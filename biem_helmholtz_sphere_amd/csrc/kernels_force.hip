// kernels_force.hip -- time-averaged radiation force on each ball from quantities the solve already has (gfx950).
//
// Real k, kind = outer.  With c_h = density_h blc_n(rho), gj_n = alpha_n j_n + beta_n k j_n' and the Wronskian Wr = i (k rho)^{1-d} the
// boundary condition fixes both traces of the total field on the ball's own surface:
//   s_h = c_h k Wr / gj_n ,   u_h = -beta_n s_h  (u on r = rho) ,   v_h = alpha_n s_h  (d_n u)
// and the radiation stress tensor integrated over that surface is, with T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega (the plan's coupling
// table, nonzero only for |n - n'| = 1) and lambda_n = n (n + d - 2),
//   Phi_i = -(rho^{d-1} / (2 k^2)) Re sum_{h',h} T^i_{h'h} [ conj(u_h') u_h (k^2 - (lambda_n + lambda_n' - (d-1)) / (2 rho^2))
//                                                          + conj(v_h') v_h + (1/rho) (lambda_n - lambda_n' + d - 1) conj(v_h') u_h ]
// in the normalisation of the powers.  Neither the incident field nor a harmonic enters: every tree the plans cover.
#include "common.hpp"

namespace biem {

namespace {
constexpr double kForceCancel = 64.0 * 2.220446049250313e-16;   // |gj| below this fraction of its two terms counts as 0 (kernels_uinterior.hip)
}

// One wave per (ball, right-hand side, system) = (blockIdx.x, .y, .z).  Lane 0 runs the recurrence of j_n at k rho into LDS, the lanes
// then form the per-degree factors of u_h and v_h (sU = -beta_n blc_n k Wr / gj_n, sV = alpha_n blc_n k Wr / gj_n; a degree whose gj_n
// is zero - to the rounding of its two terms - or not finite gets 0 and a mark) and stride over the rows h' of the table once, the inner loops
// over the row's entries component by component into d accumulators (statically indexed: registers, no scratch).  A marked degree with a nonzero coefficient makes the whole ball NaN (the rule of
// uinterior: the traces of a degree the ball does not scatter are not determined by the density).  wave_sum adds in a fixed order: no
// atomics, two calls agree bit for bit.
// alpha / beta: [nb or 1][B] (per_degree = 0) or [nb or 1][B][n_end]; tab [nb][B][3][n_end] (gj, gh, blc); density [nb][nrhs][B][H];
// fptr [H d + 1], fcol, fval: the entries of (row h', component i); out [nb][nrhs][B][d].
__global__ void __launch_bounds__(64) k_force(int d, int H, int n_end, int nj, const int* __restrict__ deg, const uint32_t* __restrict__ fptr,
                                               const int* __restrict__ fcol, const cplx* __restrict__ fval, int B, int nrhs,
                                               const cplx* __restrict__ k, const double* __restrict__ radii, int geom_batched,
                                               const cplx* __restrict__ alpha, const cplx* __restrict__ beta, int ab_batched, int per_degree,
                                               const cplx* __restrict__ tab, const cplx* __restrict__ dens, double* __restrict__ out) {
  // LDS sized by the launch (a fixed kMaxRad layout would hold a CU to 9 waves): j_n, n_end + 1 entries plus radial_jh's order shift
  // for d >= 4 (nj in all), the two factors and the marks
  extern __shared__ cplx smem[];
  cplx* sJ = smem;
  cplx* sU = sJ + nj;
  cplx* sV = sU + n_end;
  int* sBad = reinterpret_cast<int*>(sV + n_end);
  const int b = blockIdx.x, r = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  const double kr = k[s].x;
  const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  const double x = kr * rho, ix = 1.0 / x;
  const cplx* t = tab + ((size_t)s * B + b) * 3 * n_end;
  if (lane == 0) radial_jh(d, n_end, make_double2(x, 0.0), sJ, nullptr);
  __syncthreads();
  double ixp = 1.0;                                     // (k rho)^{1-d}
  for (int q = 0; q < d - 1; ++q) ixp *= ix;
  const cplx kwr = make_double2(0.0, kr * ixp);         // k Wr
  const size_t ab0 = (ab_batched ? (size_t)s * B : 0) + b;
  for (int n = lane; n < n_end; n += 64) {
    const cplx a = per_degree ? alpha[ab0 * n_end + n] : alpha[ab0];
    const cplx be = per_degree ? beta[ab0 * n_end + n] : beta[ab0];
    const cplx j = sJ[n];
    const cplx kjp = cscale(csub(cscale(j, (double)n * ix), sJ[n + 1]), kr);        // k j_n'(k rho)
    const cplx gj = t[n];
    const cplx f = cmul(cmul(t[2 * n_end + n], kwr), crecip(gj));
    const cplx fu = cmul(be, f), fv = cmul(a, f);
    const bool ok = zabs1(gj) > kForceCancel * (zabs1(cmul(a, j)) + zabs1(cmul(be, kjp))) && isfinite(fu.x) && isfinite(fu.y) &&
                    isfinite(fv.x) && isfinite(fv.y);
    sU[n] = ok ? make_double2(-fu.x, -fu.y) : make_double2(0.0, 0.0);
    sV[n] = ok ? fv : make_double2(0.0, 0.0);
    sBad[n] = ok ? 0 : 1;
  }
  __syncthreads();
  const size_t row = (((size_t)s * nrhs + r) * B + b) * H;
  double bad = 0.0;
  for (int h = lane; h < H; h += 64) {
    const int n = deg[h];
    if (sBad[n]) {
      const cplx c = cmul(dens[row + h], t[2 * n_end + n]);
      if (c.x != 0.0 || c.y != 0.0) bad += 1.0;         // (NaN compares unequal: counted)
    }
  }
  bad = wave_sum(bad);
  double rp = 1.0;                                      // rho^{d-1}
  for (int q = 0; q < d - 1; ++q) rp *= rho;
  const double k2 = kr * kr, irho = 1.0 / rho, hr2 = 0.5 * irho * irho, dm1 = (double)(d - 1);
  double* o = out + (((size_t)s * nrhs + r) * B + b) * d;
  // one pass over the rows, an accumulator per component: the loop over the components is unrolled to the largest dimension a plan
  // has and guarded by i < d, so acc[] is indexed statically and stays in registers
  double acc[kChainDimMax];
#pragma unroll
  for (int i = 0; i < kChainDimMax; ++i) acc[i] = 0.0;
  for (int hp = lane; hp < H; hp += 64) {
    const uint32_t* fp = fptr + (size_t)hp * d;
    if (fp[0] == fp[d]) continue;
    const int np_ = deg[hp];
    const cplx dp = dens[row + hp];
    const cplx up = cmul(dp, sU[np_]), vp = cmul(dp, sV[np_]);
    const double lp = (double)np_ * (double)(np_ + d - 2);
#pragma unroll
    for (int i = 0; i < kChainDimMax; ++i) {
      double a = 0.0;
      for (uint32_t e = (i < d ? fp[i] : 0u), e1 = (i < d ? fp[i + 1] : 0u); e < e1; ++e) {
        const int h = fcol[e];
        const int n = deg[h];
        const cplx dh = dens[row + h];
        const cplx u = cmul(dh, sU[n]), v = cmul(dh, sV[n]);
        const double l = (double)n * (double)(n + d - 2);
        // conj(u') u (k^2 - (l + l' - (d-1)) / (2 rho^2)) + conj(v') v + (1/rho) (l - l' + d - 1) conj(v') u
        const cplx uu = cmulc(u, up), vv = cmulc(v, vp), vu = cmulc(u, vp);
        const double wu = k2 - (l + lp - dm1) * hr2, wv = (l - lp + dm1) * irho;
        const cplx br = make_double2(uu.x * wu + vv.x + vu.x * wv, uu.y * wu + vv.y + vu.y * wv);
        const cplx T = fval[e];
        a += T.x * br.x - T.y * br.y;                   // Re(T [..])
      }
      acc[i] += a;
    }
  }
#pragma unroll
  for (int i = 0; i < kChainDimMax; ++i) {
    const double tot = wave_sum(acc[i]);               // (d is uniform: the whole wave takes part or none of it)
    if (i < d && lane == 0) o[i] = bad != 0.0 ? nan("") : -(rp / (2.0 * k2)) * tot;
  }
}

int launch_force(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_radii, int geom_batched,
                 const double* d_alpha, const double* d_beta, int ab_batched, bool per_degree, const double* d_tab,
                 const double* d_density, double* d_out, hipStream_t st) {
  // the kernel's radial array: n_end + 1 orders plus the order shift of radial_jh (d >= 4)
  if (p->n_end > kMaxRad || p->n_end + 1 + (p->d >= 4 ? radial_shift(p->d) : 0) > kMaxRad + 3) {
    set_error("biem_force: n_end=%d exceeds the built table size %d", p->n_end, kMaxRad);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (!p->force_uploaded) { set_error("biem_force: the plan's force coupling table is not on the device"); return BIEM_ERR_ARG; }
  if (nb <= 0 || B <= 0 || nrhs <= 0) return BIEM_OK;
  const int nj = p->n_end + 1 + (p->d >= 4 ? radial_shift(p->d) : 0);
  const size_t lds = (size_t)(nj + 2 * p->n_end) * sizeof(cplx) + (size_t)p->n_end * sizeof(int);
  hipLaunchKernelGGL(k_force, dim3(B, nrhs, nb), dim3(64), lds, st, p->d, p->H, p->n_end, nj, p->d_deg, p->d_fptr_comp, p->d_fcol,
                     (const cplx*)p->d_fval, B, nrhs, (const cplx*)d_k, d_radii, geom_batched, (const cplx*)d_alpha, (const cplx*)d_beta,
                     ab_batched, per_degree ? 1 : 0, (const cplx*)d_tab, (const cplx*)d_density, d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
