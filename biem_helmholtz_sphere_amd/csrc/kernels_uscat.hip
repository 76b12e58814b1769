// kernels_uscat.hip -- K6: scattered-field evaluation (reference biem_u, _biem.py:822-977).
//   near : u(x) = sum_b sum_h density[b][h] blc_n(rho_b) h_n(k |x - c_b|) Y_h(dir(x - c_b))     (_biem.py:896-966)
//   far  : no radial factor, times (-i)^n e^{-i k x.c_b} / (i k)^{(d-1)/2}; Y is still taken at dir(x - c_b),
//          exactly as the reference does (_biem.py:885,930-959)
//   NaN fill where the point is inside a ball (outer) / outside (inner)                          (_biem.py:971-976)
//   kind = "inner": the points left valid lie INSIDE the spheres (r <= rho), where the layer potentials of a density Y_h on
//   |y| = rho expand in the regular functions: slc_in = i k^{d-2} rho^{d-1} h_n(k rho) j_n(k r), dlc_in = i k^{d-1} rho^{d-1}
//   h_n'(k rho) j_n(k r) (j and h exchange roles across the sphere; potential_coef(x_abs = r, y_abs = rho) of the un-vendored
//   ultrasphere presumably selects it - parity unpinned, no reference fixture has kind = "inner").  The exterior form is
//   singular at r -> 0 and is not the potential there.  tests: jump relation u(rho+) - u(rho-) = density . Y, regularity at
//   r = 0, Helmholtz residual inside the ball.
#include "fast_layout.hpp"   // BIEM_FAST_LAYOUT / TABLES / STAGE, BIEM_FIELD_HARMONICS, BIEM_GRAD_HARMONICS, the launchers' LDS size and dispatch

namespace biem {

constexpr int kMaxRadU = 320;
static_assert(kMaxRadU == kMaxRad, "one table order for every translation unit (common.hpp)");

// c[s][b][h] = density * blc_{n(h)}(rho_b) (inner: the interior coefficient with h_n, h_n' at k rho): one wave per (system, ball)
__global__ void __launch_bounds__(64) k_uscat_coef(int d, int H, int n_end, const int* __restrict__ deg, int B, int inner,
                                                    const cplx* __restrict__ k, const double* __restrict__ eta,
                                                    const double* __restrict__ radii, int geom_batched,
                                                    const cplx* __restrict__ dens, cplx* __restrict__ c, cplx* __restrict__ scratch) {
  __shared__ cplx sJl[kMaxRadU + 3], sHl[kMaxRadU + 3];
  __shared__ cplx sBl[kMaxRadU];
  int b = blockIdx.x, s = blockIdx.y;
  // orders beyond kMaxRadU (2-D only): 3 (n_end + 3) complex of global scratch per block (written by thread 0, read after the barrier)
  cplx* sJ = scratch ? scratch + ((size_t)s * gridDim.x + b) * 3 * (n_end + 3) : sJl;
  cplx* sH = scratch ? sJ + (n_end + 3) : sHl;
  cplx* sB = scratch ? sH + (n_end + 3) : sBl;
  const cplx kk = k[s];
  const double et = eta[s];
  double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  if (threadIdx.x == 0) {
    const cplx x = cscale(kk, rho), ix = crecip(x);
    radial_jh(d, n_end, x, sJ, sH);
    double rp = 1.0; for (int q = 0; q < d - 1; ++q) rp *= rho;
    cplx kd2 = make_double2(1.0, 0.0); for (int q = 0; q < d - 2; ++q) kd2 = cmul(kd2, kk);
    for (int n = 0; n < n_end; ++n) {
      const cplx j = inner ? sH[n] : sJ[n];
      const cplx kjp = cmul(kk, csub(cscale(cmul(ix, j), (double)n), inner ? sH[n + 1] : sJ[n + 1]));
      sB[n] = cscale(cmul(kd2, make_double2(et * j.x - kjp.y, et * j.y + kjp.x)), rp);   // blc = k^{d-2} rho^{d-1} (eta j + i k j')
    }
  }
  __syncthreads();
  size_t base = ((size_t)s * B + b) * H;
  for (int h = threadIdx.x; h < H; h += 64) c[base + h] = cmul(dens[base + h], sB[deg[h]]);
}

__global__ void __launch_bounds__(256) k_uscat(int tree, int d, int H, int n_end, const int* __restrict__ labels,
                                                const int* __restrict__ deg, int nb, int B, int P, const cplx* __restrict__ k,
                                                const double* __restrict__ centers, const double* __restrict__ radii,
                                                int geom_batched, const cplx* __restrict__ c, const double* __restrict__ pts,
                                                int flags, cplx* __restrict__ out) {
  __shared__ cplx sJ[4][kMaxRadU + 3], sH[4][kMaxRadU + 3];
  __shared__ int sBad;
  extern __shared__ cplx sBall[];   // [B]
  const int p = blockIdx.x, s = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool far = (flags & BIEM_USCAT_FAR_FIELD) != 0, per_ball = (flags & BIEM_USCAT_PER_BALL) != 0;
  const bool inner = (flags & BIEM_USCAT_KIND_INNER) != 0, pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  if (threadIdx.x == 0) sBad = 0;
  double x[4];
  for (int i = 0; i < d; ++i) x[i] = pb ? pts[((size_t)i * P + p) * nb + s] : pts[(size_t)i * P + p];
  const cplx kk = k[s];
  __syncthreads();
  for (int bb = 0; bb < B; bb += 4) {
    const int b = bb + wave;
    const bool act = b < B;
    double rel[4] = {0, 0, 0, 0}, r = 1.0, xc = 0.0;
    if (act) {
      const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
      double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
      double r2 = 0.0;
      for (int i = 0; i < d; ++i) { rel[i] = x[i] - cb[i]; r2 += rel[i] * rel[i]; xc += x[i] * cb[i]; }
      r = sqrt(r2);
      if (lane == 0 && !far) {
        if ((!inner && r < rho) || (inner && r > rho)) atomicOr(&sBad, 1);
        if (r > 0.0) radial_jh(d, n_end - 1, cscale(kk, r), sJ[wave], sH[wave]);
        else {   // centre of a ball (inner kind): z_n(0) = delta_{n0} sqrt(pi/2) 2^{1-d/2} / Gamma(d/2); the exterior form has no value there
          const double z0 = radial_z0_at_zero(d);
          const double qn = __longlong_as_double(0x7ff8000000000000LL);
          for (int n = 0; n < n_end; ++n) { sJ[wave][n] = make_double2(n == 0 ? z0 : 0.0, 0.0); sH[wave][n] = make_double2(qn, qn); }
        }
      }
    }
    __syncthreads();
    if (act) {
      Dir dir = make_dir(tree, rel);
      const cplx* cs = c + ((size_t)s * B + b) * H;
      double ar = 0.0, ai = 0.0;
      for (int h = lane; h < H; h += 64) {
        double yr, yi;
        harmonic_single(tree, labels[3 * h], labels[3 * h + 1], labels[3 * h + 2], dir, &yr, &yi);
        int n = deg[h];
        cplx rad;
        if (far) {
          // (-i)^n
          int q = n & 3;
          rad = q == 0 ? make_double2(1, 0) : q == 1 ? make_double2(0, -1) : q == 2 ? make_double2(-1, 0) : make_double2(0, 1);
        } else {
          rad = inner ? sJ[wave][n] : sH[wave][n];
        }
        cplx v = cmul(cmul(cs[h], rad), make_double2(yr, yi));
        ar += v.x; ai += v.y;
      }
      ar = wave_sum(ar); ai = wave_sum(ai);
      if (lane == 0) {
        cplx v = make_double2(ar, ai);
        if (far) {
          // e^{-i k x.c_b} / (i k)^{(d-1)/2} = exp(-i k x.c_b - p log(i k)),  p = (d-1)/2, principal branch (k > 0 real:
          // |k|^{-p} e^{-i (k x.c_b + pi p / 2)})
          const double pw = 0.5 * (d - 1);
          const cplx lik = zlog(make_double2(-kk.y, kk.x));                    // log(i k)
          v = cmul(v, zexp(make_double2(kk.y * xc - pw * lik.x, -kk.x * xc - pw * lik.y)));
        }
        sBall[b] = v;
      }
    }
    __syncthreads();
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const bool bad = !far && sBad;
  if (per_ball) {
    for (int b = threadIdx.x; b < B; b += 256)
      out[((size_t)p * nb + s) * B + b] = bad ? make_double2(qnan, 0.0) : sBall[b];
  } else if (threadIdx.x == 0) {
    double ar = 0.0, ai = 0.0;
    for (int b = 0; b < B; ++b) { ar += sBall[b].x; ai += sBall[b].y; }
    out[(size_t)p * nb + s] = bad ? make_double2(qnan, 0.0) : make_double2(ar, ai);
  }
}

// ---------------------------------------------------------------------------------------------
// Near field (both kinds) and the far field, trees a (2-D), ba (3-D; bpa is ba in permuted axes), bba (4-D; bpbpa likewise) and
// caa: ONE POINT PER LANE.
// The generic kernel above spends one workgroup per (point, system), evaluates every harmonic from scratch (an O(n) Legendre
// recurrence and a sin / cos per harmonic) and leaves 63 lanes idle while lane 0 runs the radial recurrences: 2.0e6
// point-systems/s at cfg 3 (16 balls, H = 400) - the 100 x 100 plot grid of the reference's second hot loop took as long as the
// solve.  Here a lane owns a point and walks the harmonics by recurrence, all in registers:
//   h_n(k r): upward three-term recurrence from h_0, h_1 (the outgoing function is the dominant solution: stable), restarted
//             for every order m (n_end^2 / 2 extra steps - cheaper than an n_end-entry array per lane);
//   Pbar_n^m: the normalised recurrence of pbar_single with its square-root coefficients tabulated once per workgroup in LDS;
//   e^{i m phi}: rotation by (cos phi, sin phi) = (u1, u2) / |(u1, u2)| - no trigonometric call at all;
//   the +m and -m harmonics of a degree share Pbar and h;  the ball's coefficients c[h] = density * blc sit in LDS in (n, m)
//   order (every lane reads the same entry: a broadcast).
// ---------------------------------------------------------------------------------------------
constexpr int kFastNendMax3 = 48;          // LDS: 2 n_end^2 doubles of recurrence coefficients + n_end^2 complex of c
constexpr int kFastNendMax2 = kMaxRadU;    // 2-D: 2 n_end - 1 complex of c
constexpr int kFastNendMax4 = 14;          // 4-D (bba): c in a dense [n][l][m] store, n_end^2 (2 n_end - 1) complex = 85 KB at 14
constexpr int kFastNendMaxCaa = 12;        // 4-D (caa): c in a dense [n][m1][m2] store, n_end (2 n_end - 1)^2 complex = 101 KB at 12
// INNER (kind = "inner", near field): the radial factor is the regular function j_n(k r), whose upward recurrence is unstable
// for n > |k r|: each lane computes j_0 .. j_{n_end-1} once per ball by the backward recurrence of radial_jh into its own LDS row
// (64-thread workgroups; odd row stride: conflict-free 16-byte reads) and the harmonic loops read it by degree.
template <int TREE, bool FAR, bool INNER>
__global__ void __launch_bounds__(256) k_uscat_fast(int d, int H, int n_end, const int* __restrict__ labels, int nb, int B, int P,
                                                     const cplx* __restrict__ k, const double* __restrict__ centers,
                                                     const double* __restrict__ radii, int geom_batched, const cplx* __restrict__ c,
                                                     const double* __restrict__ pts, int flags, cplx* __restrict__ out) {
  BIEM_FAST_LAYOUT()
  const int js = (n_end + 2) | 1;           // INNER: row stride of the per-lane j_n store (radial_jh wants n_end + 1 slots at d = 4)
  const int s = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
  cplx* sJl = sC + nC + (size_t)tid * js;
  const int p = blockIdx.x * T + tid, pc = p < P ? p : P - 1;
  const bool per_ball = (flags & BIEM_USCAT_PER_BALL) != 0, pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  BIEM_FAST_TABLES()
  double x[4];
  for (int i = 0; i < d; ++i) x[i] = pb ? pts[((size_t)i * P + pc) * nb + s] : pts[(size_t)i * P + pc];
  const cplx kk = k[s];
  bool bad = false;
  double tr = 0.0, ti = 0.0;
  const double dd2 = (double)(d - 2);
  for (int b = 0; b < B; ++b) {
    __syncthreads();                       // the previous ball's coefficients are no longer read (and the tables are written)
    const cplx* cs = c + ((size_t)s * B + b) * H;
    BIEM_FAST_STAGE()
    __syncthreads();
    const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
    const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
    double u[4] = {0.0, 0.0, 0.0, 0.0}, r2 = 0.0;
    for (int i = 0; i < d; ++i) { u[i] = x[i] - cb[i]; r2 += u[i] * u[i]; }
    const double r = sqrt(r2);
    if (!FAR && (INNER ? r > rho : r < rho)) bad = true;
    // h_0, h_1 at k r (r = 0 only inside a ball: the value is discarded).  Far field: the radial factor is (-i)^n, i.e. the
    // "recurrence" h_{n+1} = -i h_n from h_0 = 1 (advance() below)
    cplx h0 = make_double2(1.0, 0.0), h1 = make_double2(0.0, -1.0), ix = make_double2(0.0, 0.0);
    if (INNER) {
      if (r > 0.0) radial_jh(d, n_end - 1, cscale(kk, r), (zc*)sJl, nullptr);
      else {                                // centre of the ball: z_n(0) = delta_{n0} sqrt(pi/2) 2^{1-d/2} / Gamma(d/2)
        const double z0 = radial_z0_at_zero(d);
        for (int n = 0; n < n_end; ++n) sJl[n] = make_double2(n == 0 ? z0 : 0.0, 0.0);
      }
    } else if (!FAR) {
      zc J2[4], H2[4];
      radial_jh(d, 1, cscale(kk, r > 0.0 ? r : rho), J2, H2);
      h0 = H2[0]; h1 = H2[1];
      ix = crecip(cscale(kk, r > 0.0 ? r : rho));
    }
    // next of (h_{q-1}, h_q): h_{q+1} = ((2 q + d - 2) / x) h_q - h_{q-1}
    auto advance = [&](const cplx& hprev, const cplx& hcur, double two_q) -> cplx {
      if (FAR) return make_double2(hcur.y, -hcur.x);
      return csub(cmul(cscale(ix, two_q + dd2), hcur), hprev);
    };
    auto radial = [&](int n, const cplx& hup) -> cplx { if (INNER) return sJl[n]; return hup; };   // the radial factor of degree n
    BIEM_FIELD_HARMONICS()                 // the harmonic loops (fast_layout.hpp, shared with k_uinterior_fast): defines ar, ai
    ar *= kInvSqrt2Pi; ai *= kInvSqrt2Pi;
    if (FAR) {
      // e^{-i k x.c_b} / (i k)^{(d-1)/2}, as in the generic kernel
      double xc = 0.0;
      for (int i = 0; i < d; ++i) xc += x[i] * cb[i];
      const double pw = 0.5 * (d - 1);
      const cplx lik = zlog(make_double2(-kk.y, kk.x));
      const cplx v = cmul(make_double2(ar, ai), zexp(make_double2(kk.y * xc - pw * lik.x, -kk.x * xc - pw * lik.y)));
      ar = v.x; ai = v.y;
    }
    if (per_ball) { if (p < P) out[((size_t)p * nb + s) * B + b] = make_double2(ar, ai); }
    else { tr += ar; ti += ai; }
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (p >= P) return;
  if (per_ball) {
    if (bad) for (int b = 0; b < B; ++b) out[((size_t)p * nb + s) * B + b] = make_double2(qnan, 0.0);
  } else out[(size_t)p * nb + s] = bad ? make_double2(qnan, 0.0) : make_double2(tr, ti);
}

// ---------------------------------------------------------------------------------------------
// Gradient of the near field, trees a, ba, bba, caa (bpa / bpbpa in permuted axes), both kinds: ONE POINT PER LANE, the loops of
// k_uscat_fast with the derivative of every factor carried along its recurrence and d complex sums instead of one.
//   Write a term as z_n(k r) Y_h(u / r) = [z_n(k r) / r^n] S_h(u) with the solid harmonic S_h(u) = r^n Y_h(u / r), a homogeneous
//   polynomial of degree n in the Cartesian components.  With z_n'(x) = (n / x) z_n - z_{n+1}:
//       grad (z_n Y_h) = -k z_{n+1}(k r) Y_h(e) e + (z_n(k r) / r) (grad S_h)(e),      e = u / r,
//   and both S_h and grad S_h are evaluated ON THE UNIT SPHERE by recurrences in the components of e that never divide:
//     e^{i m phi} sin^m      -> w^m, w = e_a + i e_b (the last two components), gradient m w^{m-1} (1, i);
//     Pbar_l^m(c) / sin^m    -> Q_l^m(c), the same three-term recurrence (tables ra, rb) started from the constant Q_m^m; below the
//                               root (bba) in the homogeneous form L_l = t^{l-m} Q_l^m(e_1 / t), t^2 = e_1^2 + e_2^2 + e_3^2,
//                               L_l = ra (e_1 L_{l-1} - rb t^2 L_{l-2}) with gradient a_l (0,1,0,0) + b_l (0, e_1, e_2, e_3);
//     Gegenbauer / Jacobi    -> polynomials in e_0 (bba) or in xx = e_0^2 + e_1^2 - e_2^2 - e_3^2 (caa): value and derivative.
//   So a point whose offset lies on a coordinate axis of the tree (sin theta = 0 at any node) is an ordinary point: no branch, no
//   guard, the same instructions.  At the centre of a ball (inner kind) only z_1 / r -> k z_0(0) / d survives; e is then arbitrary
//   (grad S_1 is constant).
//   Per innermost step three radial weights (alpha_n = -k z_{n+1}, beta_n = z_n / r): W1 = P (alpha + (n - n0) beta),
//   W2 = beta P', W3 = beta P, each times the coefficients of the sign combinations that share them.
// out[i][p][s] (or [i][p][s][b]): component i in the plan's (canonical) axes.
// ---------------------------------------------------------------------------------------------
template <int TREE, bool INNER>
__global__ void __launch_bounds__(256) k_uscat_grad_fast(int d, int H, int n_end, const int* __restrict__ labels, int nb, int B, int P,
                                                          const cplx* __restrict__ k, const double* __restrict__ centers,
                                                          const double* __restrict__ radii, int geom_batched,
                                                          const cplx* __restrict__ c, const double* __restrict__ pts, int flags,
                                                          cplx* __restrict__ out) {
  constexpr int D = TREE == TREE_A ? 2 : TREE == TREE_BA ? 3 : 4;   // = d (a compile-time extent keeps x, e, g in registers)
  BIEM_FAST_LAYOUT()
  const int js = (n_end + 3) | 1;           // INNER: j_0 .. j_{n_end} per lane (radial_jh wants n_end + 2 slots at d = 4)
  const int s = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
  cplx* sJl = sC + nC + (size_t)tid * js;
  const int p = blockIdx.x * T + tid, pc = p < P ? p : P - 1;
  const bool per_ball = (flags & BIEM_USCAT_PER_BALL) != 0, pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  const size_t cstride = (size_t)P * nb * (per_ball ? B : 1);      // between the components of the output
  (void)ra; (void)rb; (void)cmm; (void)ga; (void)gia; (void)g0; (void)jA; (void)jB; (void)jC; (void)jN; (void)K2; (void)ms;
  BIEM_FAST_TABLES()
  double x[4];
  for (int i = 0; i < D; ++i) x[i] = pb ? pts[((size_t)i * P + pc) * nb + s] : pts[(size_t)i * P + pc];
  const cplx kk = k[s];
  bool bad = false;
  cplx tot[4];
  for (int i = 0; i < 4; ++i) tot[i] = make_double2(0.0, 0.0);
  const double dd2 = (double)(d - 2);
  const cplx zero = make_double2(0.0, 0.0);
  for (int b = 0; b < B; ++b) {
    __syncthreads();                       // the previous ball's coefficients are no longer read (and the tables are written)
    const cplx* cs = c + ((size_t)s * B + b) * H;
    BIEM_FAST_STAGE()
    __syncthreads();
    const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * D;
    const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
    double u[4] = {0.0, 0.0, 0.0, 0.0}, r2 = 0.0;
    for (int i = 0; i < D; ++i) { u[i] = x[i] - cb[i]; r2 += u[i] * u[i]; }
    const double r = sqrt(r2);
    if (INNER ? r > rho : r < rho) bad = true;
    // e = u / r; at r = 0 (a masked point of the outer kind, the centre of the inner kind) any unit vector does
    double invr = r > 0.0 ? 1.0 / r : 1.0;
    double e[4] = {1.0, 0.0, 0.0, 0.0};
    if (r > 0.0) for (int i = 0; i < 4; ++i) e[i] = u[i] / r;
    cplx kneg = make_double2(-kk.x, -kk.y);                       // alpha_n = kneg z_{n+1}
    cplx h0 = zero, h1 = zero, ix = zero;
    if (INNER) {
      if (r > 0.0) radial_jh(d, n_end, cscale(kk, r), (zc*)sJl, nullptr);
      else {                                // centre: z_{n+1}(0) = 0 and z_n / r -> delta_{n1} k z_0(0) / d, kept in place of z_1 (invr = 1)
        const double z0 = radial_z0_at_zero(d) / (double)d;
        for (int n = 0; n <= n_end; ++n) sJl[n] = n == 1 ? cscale(kk, z0) : zero;
        kneg = zero;
      }
    } else {
      const double ra0 = r > 0.0 ? r : rho;                       // (r = 0 only inside a ball: the value is discarded)
      zc J2[4], H2[4];
      radial_jh(d, 1, cscale(kk, ra0), J2, H2);
      h0 = H2[0]; h1 = H2[1];
      ix = crecip(cscale(kk, ra0));
    }
    // next of (h_{q-1}, h_q): h_{q+1} = ((2 q + d - 2) / x) h_q - h_{q-1}
    auto advance = [&](const cplx& hprev, const cplx& hcur, double two_q) -> cplx {
      return csub(cmul(cscale(ix, two_q + dd2), hcur), hprev);
    };
    // (alpha_n, beta_n) = (-k z_{n+1}, z_n / r) from the pair (h_n, h_{n+1}) of the upward recurrence, or from the lane's j_n row
    auto radial2 = [&](int n, const cplx& hn, const cplx& hn1, cplx& al, cplx& be) {
      if (INNER) { al = cmul(kneg, sJl[n + 1]); be = cscale(sJl[n], invr); }
      else { al = cmul(kneg, hn1); be = cscale(hn, invr); }
    };
    BIEM_GRAD_HARMONICS()                  // the harmonic loops (fast_layout.hpp, shared with k_uinterior_grad_fast): defines g[4]
    for (int i = 0; i < D; ++i) {
      g[i] = cscale(g[i], kInvSqrt2Pi);
      if (per_ball) { if (p < P) out[i * cstride + ((size_t)p * nb + s) * B + b] = g[i]; }
      else { tot[i].x += g[i].x; tot[i].y += g[i].y; }
    }
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (p >= P) return;
  for (int i = 0; i < D; ++i) {
    if (per_ball) {
      if (bad) for (int b = 0; b < B; ++b) out[i * cstride + ((size_t)p * nb + s) * B + b] = make_double2(qnan, 0.0);
    } else out[i * cstride + (size_t)p * nb + s] = bad ? make_double2(qnan, 0.0) : tot[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Chain trees (any depth): one workgroup of 4 waves per (point, system), a wave per ball as in k_uscat, but the harmonics come from
// node tables: lane 0 runs the radial functions and the angles, the lanes fill F_j[L][L1] (one lane per (node j, L1): the Gegenbauer
// degree recurrence once) and the phases e^{i m phi}, then every harmonic is d - 2 LDS lookups and one phase.
// ---------------------------------------------------------------------------------------------
constexpr int kChainRadU = 64;                  // radial orders per wave (n_end + 1 + shift)
constexpr int kChainTabU = 1024;                // node-table doubles per wave ((d - 2) n_end^2)
__global__ void __launch_bounds__(256) k_uscat_chain(int d, int H, int n_end, const int* __restrict__ labels,
                                                      const int* __restrict__ deg, int nb, int B, int P, const cplx* __restrict__ k,
                                                      const double* __restrict__ centers, const double* __restrict__ radii,
                                                      int geom_batched, const cplx* __restrict__ c, const double* __restrict__ pts,
                                                      int flags, cplx* __restrict__ out) {
  __shared__ cplx sJ[4][kChainRadU], sH[4][kChainRadU], sPh[4][kChainRadU];
  __shared__ double sF[4][kChainTabU];
  __shared__ double sC[4][kChainDimMax], sS[4][kChainDimMax], sPhi[4];
  __shared__ int sBad;
  extern __shared__ cplx sBall[];   // [B]
  const int p = blockIdx.x, s = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool far = (flags & BIEM_USCAT_FAR_FIELD) != 0, per_ball = (flags & BIEM_USCAT_PER_BALL) != 0;
  const bool inner = (flags & BIEM_USCAT_KIND_INNER) != 0, pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  const int np = d - 2, lw = d - 1;
  if (threadIdx.x == 0) sBad = 0;
  const cplx kk = k[s];
  __syncthreads();
  for (int bb = 0; bb < B; bb += 4) {
    const int b = bb + wave;
    const bool act = b < B;
    double xc = 0.0;
    if (act && lane == 0) {
      const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
      const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
      double rel[kChainDimMax];
      double r2 = 0.0;
      for (int i = 0; i < d; ++i) {
        const double xi = pb ? pts[((size_t)i * P + p) * nb + s] : pts[(size_t)i * P + p];
        rel[i] = xi - cb[i]; r2 += rel[i] * rel[i]; xc += xi * cb[i];
      }
      const double r = sqrt(r2);
      double phi;
      chain_angles(d, rel, sC[wave], sS[wave], &phi);
      sPhi[wave] = phi;
      if (!far) {
        if ((!inner && r < rho) || (inner && r > rho)) atomicOr(&sBad, 1);
        if (r > 0.0) radial_jh(d, n_end - 1, cscale(kk, r), sJ[wave], sH[wave]);
        else {   // centre of a ball (inner kind): z_n(0) = delta_{n0} z_0(0); the exterior form has no value there
          const double z0 = radial_z0_at_zero(d);
          const double qn = __longlong_as_double(0x7ff8000000000000LL);
          for (int n = 0; n < n_end; ++n) { sJ[wave][n] = make_double2(n == 0 ? z0 : 0.0, 0.0); sH[wave][n] = make_double2(qn, qn); }
        }
      }
    }
    __syncthreads();
    if (act) {
      for (int i = lane; i < np * n_end; i += 64) {
        const int j = i / n_end, L1 = i - j * n_end;
        const double lam = (double)L1 + 0.5 * (d - j - 2), cj = sC[wave][j], sn = sS[wave][j];
        double sl = 1.0;
        for (int q = 0; q < L1; ++q) sl *= sn;
        double p0 = sl / sqrt(sqrt(kPi) * exp(lgamma(lam + 0.5) - lgamma(lam + 1.0))), p1 = 0.0, aprev = 0.0;
        double* F = sF[wave] + ((size_t)j * n_end) * n_end + L1;
        for (int L = L1; L < n_end; ++L) {
          const int kq = L - L1;
          if (kq > 0) {
            const double aq = 0.5 * sqrt((double)kq * ((double)kq + 2.0 * lam - 1.0) / (((double)kq + lam - 1.0) * ((double)kq + lam)));
            const double p2 = (cj * p0 - aprev * p1) / aq;
            p1 = p0; p0 = p2; aprev = aq;
          }
          F[(size_t)L * n_end] = p0;
        }
      }
      for (int m = lane; m < n_end; m += 64) {
        double sn, cs;
        sincos((double)m * sPhi[wave], &sn, &cs);
        sPh[wave][m] = make_double2(cs, sn);
      }
    }
    __syncthreads();
    if (act) {
      const cplx* cs = c + ((size_t)s * B + b) * H;
      double ar = 0.0, ai = 0.0;
      for (int h = lane; h < H; h += 64) {
        const int* lb = labels + (size_t)h * lw;
        const int m = lb[lw - 1], am = m < 0 ? -m : m;
        double amp = kInvSqrt2Pi;
        for (int j = 0; j < np; ++j) amp *= sF[wave][((size_t)j * n_end + lb[j]) * n_end + (j + 1 < np ? lb[j + 1] : am)];
        const cplx ph = sPh[wave][am];
        const int n = deg[h];
        cplx rad;
        if (far) {
          const int q = n & 3;
          rad = q == 0 ? make_double2(1, 0) : q == 1 ? make_double2(0, -1) : q == 2 ? make_double2(-1, 0) : make_double2(0, 1);
        } else {
          rad = inner ? sJ[wave][n] : sH[wave][n];
        }
        const cplx v = cmul(cmul(cs[h], rad), make_double2(amp * ph.x, m < 0 ? -amp * ph.y : amp * ph.y));
        ar += v.x; ai += v.y;
      }
      ar = wave_sum(ar); ai = wave_sum(ai);
      if (lane == 0) {
        cplx v = make_double2(ar, ai);
        if (far) {
          const double pw = 0.5 * (d - 1);
          const cplx lik = zlog(make_double2(-kk.y, kk.x));                    // log(i k)
          v = cmul(v, zexp(make_double2(kk.y * xc - pw * lik.x, -kk.x * xc - pw * lik.y)));
        }
        sBall[b] = v;
      }
    }
    __syncthreads();
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const bool bad = !far && sBad;
  if (per_ball) {
    for (int b = threadIdx.x; b < B; b += 256)
      out[((size_t)p * nb + s) * B + b] = bad ? make_double2(qnan, 0.0) : sBall[b];
  } else if (threadIdx.x == 0) {
    double ar = 0.0, ai = 0.0;
    for (int b = 0; b < B; ++b) { ar += sBall[b].x; ai += sBall[b].y; }
    out[(size_t)p * nb + s] = bad ? make_double2(qnan, 0.0) : make_double2(ar, ai);
  }
}

// The field of a plan in three host steps, so that biem_uscat_hess (kernels_ladder.hip) can put its coefficient ladder between the
// second and the third: what the kernels do not cover at this plan (uscat_covered), c = density * blc (uscat_form_coef), the field of
// a coefficient set (uscat_eval_coef: the per-lane / generic / chain choice and the BIEM_USCAT_GENERIC switch).
int uscat_covered(const biem_plan* p, int nb, int B, int flags) {
  // orders beyond the LDS tables: 2-D only, through the per-lane kernel (its only table is the ball's 2 n_end - 1 coefficients)
  const bool big = p->n_end > kMaxRadU;
  if (big && (p->tree != TREE_A || (size_t)(2 * p->n_end - 1) * sizeof(cplx) > 150 * 1024 ||
              ((flags & BIEM_USCAT_KIND_INNER) && !(flags & BIEM_USCAT_FAR_FIELD)) || nb > 65535)) {
    set_error("biem_uscat: n_end=%d too large for this tree / kind", p->n_end); return BIEM_ERR_UNSUPPORTED;
  }
  if (p->tree == TREE_CHAIN && (p->n_end + 1 + kRadShiftMax > kChainRadU || (p->d - 2) * p->n_end * p->n_end > kChainTabU || nb > 65535 ||
                                (size_t)B * sizeof(cplx) > 64 * 1024)) {
    set_error("biem_uscat: chain tree d=%d n_end=%d (%d balls) exceeds the field kernel's tables", p->d, p->n_end, B); return BIEM_ERR_UNSUPPORTED;
  }
  return BIEM_OK;
}

int uscat_form_coef(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                    const double* d_density, int flags, cplx* c, hipStream_t st) {
  const bool big = p->n_end > kMaxRadU;
  cplx* scratch = nullptr;
  if (big) BIEM_HIPCHK(hipMallocAsync((void**)&scratch, (size_t)nb * B * 3 * (p->n_end + 3) * sizeof(cplx), st));
  hipLaunchKernelGGL(k_uscat_coef, dim3(B, nb), dim3(64), 0, st, p->d, p->H, p->n_end, p->d_deg, B,
                     (flags & BIEM_USCAT_KIND_INNER) && !(flags & BIEM_USCAT_FAR_FIELD) ? 1 : 0, (const cplx*)d_k, d_eta, d_radii,
                     geom_batched, (const cplx*)d_density, c, scratch);
  BIEM_LAUNCHCHK();
  if (scratch) BIEM_HIPCHK(hipFreeAsync(scratch, st));
  return BIEM_OK;
}

int launch_uscat(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                 const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                 double* d_out, void* d_work, size_t work_bytes, hipStream_t st) {
  if (nb <= 0 || B <= 0 || P <= 0) return BIEM_OK;
  int rc = uscat_covered(p, nb, B, flags);
  if (rc != BIEM_OK) return rc;
  size_t need = (size_t)nb * B * p->H * sizeof(cplx);
  if (work_bytes < need) { set_error("biem_uscat: workspace too small"); return BIEM_ERR_ARG; }
  cplx* c = (cplx*)d_work;
  if ((rc = uscat_form_coef(p, nb, B, d_k, d_eta, d_radii, geom_batched, d_density, flags, c, st)) != BIEM_OK) return rc;
  return uscat_eval_coef(p, nb, B, P, d_k, d_centers, d_radii, geom_batched, c, d_points, flags, d_out, st);
}

int uscat_eval_coef(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_centers, const double* d_radii,
                    int geom_batched, const cplx* c, const double* d_points, int flags, double* d_out, hipStream_t st) {
  const bool big = p->n_end > kMaxRadU;
  if (p->tree == TREE_CHAIN) {
    hipLaunchKernelGGL(k_uscat_chain, dim3(P, nb), dim3(256), (size_t)B * sizeof(cplx), st, p->d, p->H, p->n_end, p->d_labels,
                       p->d_deg, nb, B, P, (const cplx*)d_k, d_centers, d_radii, geom_batched, (const cplx*)c, d_points, flags, (cplx*)d_out);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  // the far field does not depend on the kind; the near field of kind inner reads j_n from a per-lane LDS row (INNER)
  const bool far = (flags & BIEM_USCAT_FAR_FIELD) != 0;
  const bool inner = !far && (flags & BIEM_USCAT_KIND_INNER);
  const int ne = p->n_end;
  const bool fast_tree = (p->tree == TREE_BA && ne <= kFastNendMax3) || (p->tree == TREE_A && (big || ne <= kFastNendMax2)) ||
                         (p->tree == TREE_BBA && ne <= kFastNendMax4) || (p->tree == TREE_CAA && ne <= kFastNendMaxCaa);
  if (fast_tree && !getenv("BIEM_USCAT_GENERIC") && nb <= 65535) {
    const int T = inner ? 64 : 256;
    const size_t shm = fast_layout_lds_bytes(p->tree, ne, T, inner ? (ne + 2) | 1 : 0);   // (the kernel's js)
    if (shm <= 160 * 1024) {
#define BIEM_USCAT_FAST(TREE, FARF, INNERF)                                                                                      \
  {                                                                                                                              \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_uscat_fast<TREE, FARF, INNERF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
    hipLaunchKernelGGL((k_uscat_fast<TREE, FARF, INNERF>), dim3((P + T - 1) / T, nb), dim3(T), shm, st, p->d, p->H, ne, p->d_labels, nb, \
                       B, P, (const cplx*)d_k, d_centers, d_radii, geom_batched, (const cplx*)c, d_points, flags, (cplx*)d_out); \
  }
#define BIEM_USCAT_FAST_TREE(TREE)                                                                                               \
  { if (far) BIEM_USCAT_FAST(TREE, true, false) else if (inner) BIEM_USCAT_FAST(TREE, false, true) else BIEM_USCAT_FAST(TREE, false, false) }
      BIEM_FAST_TREE_DISPATCH(p->tree, BIEM_USCAT_FAST_TREE)
#undef BIEM_USCAT_FAST_TREE
#undef BIEM_USCAT_FAST
      BIEM_LAUNCHCHK();
      return BIEM_OK;
    }
  }
  hipLaunchKernelGGL(k_uscat, dim3(P, nb), dim3(256), (size_t)B * sizeof(cplx), st, p->tree, p->d, p->H, p->n_end, p->d_labels,
                     p->d_deg, nb, B, P, (const cplx*)d_k, d_centers, d_radii, geom_batched, (const cplx*)c, d_points, flags, (cplx*)d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// Gradient of the near field: the per-lane kernels only.  Whatever they do not cover (chain trees, orders above the per-lane
// ceilings, a workgroup's tables beyond the LDS) is BIEM_ERR_UNSUPPORTED - there is no generic gradient kernel to fall through to.
int launch_uscat_grad(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                      double* d_out, void* d_work, size_t work_bytes, hipStream_t st) {
  if (flags & BIEM_USCAT_FAR_FIELD) { set_error("biem_uscat_grad: the far-field pattern has no gradient in space (BIEM_USCAT_FAR_FIELD)"); return BIEM_ERR_ARG; }
  const int ne = p->n_end, cap = uscat_fast_nend_max(p->tree);
  if (cap == 0) {
    set_error("biem_uscat_grad: built for the trees a, ba (bpa), bba (bpbpa) and caa; chain trees (d=%d) are not covered", p->d);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (ne > cap) {
    set_error("biem_uscat_grad: n_end=%d above the per-lane ceiling %d of this tree (a %d, ba %d, bba %d, caa %d)", ne, cap,
              kFastNendMax2, kFastNendMax3, kFastNendMax4, kFastNendMaxCaa);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (nb > 65535) { set_error("biem_uscat_grad: more than 65535 systems in one call (%d)", nb); return BIEM_ERR_UNSUPPORTED; }
  if (nb <= 0 || B <= 0 || P <= 0) return BIEM_OK;
  const bool inner = (flags & BIEM_USCAT_KIND_INNER) != 0;
  const int T = inner ? 64 : 256;
  const size_t shm = fast_layout_lds_bytes(p->tree, ne, T, inner ? (ne + 3) | 1 : 0);   // (the kernel's js)
  if (shm > 160 * 1024) {
    set_error("biem_uscat_grad: n_end=%d needs %zu bytes of LDS per workgroup (limit %d)", ne, shm, 160 * 1024);
    return BIEM_ERR_UNSUPPORTED;
  }
  size_t need = (size_t)nb * B * p->H * sizeof(cplx);
  if (work_bytes < need) { set_error("biem_uscat_grad: workspace too small"); return BIEM_ERR_ARG; }
  cplx* c = (cplx*)d_work;
  hipLaunchKernelGGL(k_uscat_coef, dim3(B, nb), dim3(64), 0, st, p->d, p->H, ne, p->d_deg, B, inner ? 1 : 0, (const cplx*)d_k, d_eta,
                     d_radii, geom_batched, (const cplx*)d_density, c, (cplx*)nullptr);
  BIEM_LAUNCHCHK();
#define BIEM_USCAT_GRAD(TREE, INNERF)                                                                                            \
  {                                                                                                                              \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_uscat_grad_fast<TREE, INNERF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
    hipLaunchKernelGGL((k_uscat_grad_fast<TREE, INNERF>), dim3((P + T - 1) / T, nb), dim3(T), shm, st, p->d, p->H, ne, p->d_labels, nb, \
                       B, P, (const cplx*)d_k, d_centers, d_radii, geom_batched, (const cplx*)c, d_points, flags, (cplx*)d_out); \
  }
#define BIEM_USCAT_GRAD_TREE(TREE) { if (inner) BIEM_USCAT_GRAD(TREE, true) else BIEM_USCAT_GRAD(TREE, false) }
  BIEM_FAST_TREE_DISPATCH(p->tree, BIEM_USCAT_GRAD_TREE)
#undef BIEM_USCAT_GRAD_TREE
#undef BIEM_USCAT_GRAD
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// the per-lane order ceiling of a tree (0: no per-lane kernel), for the launchers of other translation units
int uscat_fast_nend_max(int tree) {
  return tree == TREE_A ? kFastNendMax2 : tree == TREE_BA ? kFastNendMax3 : tree == TREE_BBA ? kFastNendMax4 :
         tree == TREE_CAA ? kFastNendMaxCaa : 0;
}

}  // namespace biem
