// rhs_translate.hpp -- the geometry and the radial row of one (system, source, ball) of the translated right-hand sides: what the
// single-harmonic kernels (kernels_rhs_ms.hip) and the expansion kernels (kernels_rhs_ex.hip) both start from.
#pragma once
#include "common.hpp"

namespace biem {

// the centre, the source and the system of table row `row` = (sr - sr0) B + b, sr = s nrhs + r
struct MsRow { long long s; int r, b; };
__device__ inline MsRow ms_row(long long row, long long sr0, int B, int nrhs) {
  const long long sr = sr0 + row / B;
  return {sr / nrhs, (int)(sr % nrhs), (int)(row % B)};
}
// t = c_b - s_r (the sign of a pair table's c_b - c_b'; k_ps_geometry has s - c); flip: t = s_r - c_b
__device__ inline void ms_displacement(const MsRow& w, int d, int B, int nrhs, const double* __restrict__ centers, int geom_batched,
                                       const double* __restrict__ src, int src_batched, double* t, double* dist, bool flip = false) {
  const double* c = centers + ((geom_batched ? w.s * B : 0) + w.b) * d;
  const double* x = src + ((src_batched ? w.s * nrhs : 0) + w.r) * d;
  double r2 = 0.0;
  for (int i = 0; i < d; ++i) { t[i] = flip ? x[i] - c[i] : c[i] - x[i]; r2 += t[i] * t[i]; }
  *dist = sqrt(r2);
}
// the radial row of a table at z = k |t|, orders 0 .. nmax, by one lane.  REG: the regular functions alone (sH is not written); at
// |t| = 0 they are j_l(0) = delta_{l0} j_0(0), written as such - the recurrences divide by z
template <bool REG>
__device__ inline void ms_radial_row(int d, int nmax, cplx kk, double dist, cplx* sJ, cplx* sH) {
  if (REG && dist == 0.0) {
    const double z0 = radial_z0_at_zero(d);
    for (int n = 0; n <= nmax; ++n) sJ[n] = make_double2(n == 0 ? z0 : 0.0, 0.0);
    return;
  }
  radial_jh(d, nmax, cscale(kk, dist), sJ, REG ? nullptr : sH);
}
// |t| = 0 has no direction: any fixed unit vector does (its harmonics are finite, and only degree 0 meets a nonzero radial value)
__device__ inline void ms_unit_if_zero(int d, double dist, double* t) {
  if (dist == 0.0) { t[0] = 1.0; for (int i = 1; i < d; ++i) t[i] = 0.0; }
}

__device__ inline double ms_sign_even(int e) { return ((e / 2) & 1) ? -1.0 : 1.0; }      // i^e for even e (either sign)

}  // namespace biem
