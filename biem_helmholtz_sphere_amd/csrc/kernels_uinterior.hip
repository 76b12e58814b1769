// kernels_uinterior.hip -- the total field INSIDE penetrable fluid balls and its gradient (5e), gfx950.
//   u_b(y) = sum_h a_{b,h} j_n(k_b |y - c_b|) Y_h(dir(y - c_b)),      |y - c_b| < rho_b
// The coefficients follow algebraically from the solved density.  Row (b, h) of the system says that the regular local coefficient
// of the exterior total field at ball b is I = -s gh_n / gj_n with s = density blc_n(rho_b) (what k_uscat_coef forms); continuity of u
// and of (1 / density) d_n u across the sphere, with the unscaled pair alpha^_n = -k_b j_n'(k_b rho), beta^_n = delta j_n(k_b rho), gives
//   a_{b,h} = -s delta k W(x) / gj_n,    W(x) = j_n h_n' - j_n' h_n = i / x^{d-1},    gj_n = alpha^_n j_n(x) + beta^_n k j_n'(x),    x = k rho
// with nothing divided by j_n(k_b rho).  No second solve, no matrix, no matvec.
#include <atomic>
#include "fast_layout.hpp"

namespace biem {

namespace {
__device__ inline bool cfinite(cplx a) { return isfinite(a.x) && isfinite(a.y); }
__device__ inline cplx cnan() { const double q = __longlong_as_double(0x7ff8000000000000LL); return make_double2(q, q); }
constexpr double kInteriorCancel = 64.0 * 2.220446049250313e-16;   // |gj| below this fraction of its two terms: no correct digit left
}  // namespace

// a[s][b][h] = density[s][b][h] F_n,  F_n = -blc_n delta k W / gj_n: one wave per (system, ball), like k_uscat_coef.
// The pair (alpha^_n, beta^_n) is scaled by 1 / sigma_n, sigma_n = max(|alpha^_n|, |k beta^_n|) (the scale of fluid_inclusion_bc), in gj and
// in the numerator alike, so the quotient neither under- nor overflows while j_n(k rho) and j_n(k_b rho) are normal numbers each.
// Not finite (k_b NaN: an impenetrable ball; gj_n = 0: a degree the ball does not scatter, whose interior field the density does not
// determine) is written as NaN: the field kernel's sums then give NaN inside that ball.  gj_n counts as 0 when its two terms cancel to
// rounding (kInteriorCancel): the transparent sphere k_b = k, delta = 1 leaves rounding noise there, not a value.
__global__ void __launch_bounds__(64) k_interior_coef(int d, int H, int n_end, const int* __restrict__ deg, int B,
                                                       const cplx* __restrict__ k, const double* __restrict__ eta,
                                                       const double* __restrict__ radii, int geom_batched,
                                                       const cplx* __restrict__ kint, const cplx* __restrict__ delta, int fluid_batched,
                                                       const cplx* __restrict__ dens, cplx* __restrict__ a) {
  __shared__ cplx sJ[kMaxRad + 3], sH[kMaxRad + 3], sJz[kMaxRad + 3];
  __shared__ cplx sF[kMaxRad];
  const int b = blockIdx.x, s = blockIdx.y;
  const cplx kk = k[s];
  const double et = eta[s];
  const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  const cplx kb = kint[(fluid_batched ? (size_t)s * B : 0) + b];
  const cplx dl = delta[(fluid_batched ? (size_t)s * B : 0) + b];
  if (threadIdx.x == 0) {
    const cplx x = cscale(kk, rho), z = cscale(kb, rho);
    const bool fluid = cfinite(z) && cfinite(dl) && (z.x != 0.0 || z.y != 0.0);
    if (!fluid) {
      for (int n = 0; n < n_end; ++n) sF[n] = cnan();
    } else {
      radial_jh(d, n_end, x, sJ, sH);          // orders 0 .. n_end (one extra for the derivative)
      radial_jh(d, n_end, z, sJz, nullptr);
      const cplx ix = crecip(x), iz = crecip(z);
      double rp = 1.0; for (int q = 0; q < d - 1; ++q) rp *= rho;
      cplx kd2 = make_double2(1.0, 0.0); for (int q = 0; q < d - 2; ++q) kd2 = cmul(kd2, kk);
      cplx xw = make_double2(1.0, 0.0); for (int q = 0; q < d - 1; ++q) xw = cmul(xw, x);
      const cplx ixw = crecip(xw);
      const cplx dkw = cmul(cmul(dl, kk), make_double2(-ixw.y, ixw.x));     // delta k W,  W = i / x^{d-1}
      for (int n = 0; n < n_end; ++n) {
        const cplx j = sJ[n];
        const cplx kjp = cmul(kk, csub(cscale(cmul(ix, j), (double)n), sJ[n + 1]));
        const cplx blc = cscale(cmul(kd2, make_double2(et * j.x - kjp.y, et * j.y + kjp.x)), rp);   // as k_uscat_coef
        const cplx jz = sJz[n];
        const cplx kjpz = cmul(kb, csub(cscale(cmul(iz, jz), (double)n), sJz[n + 1]));              // k_b j_n'(k_b rho) = -alpha^_n
        const cplx bj = cmul(dl, jz);                                                               // beta^_n
        const double sg = fmax(zabs1(kjpz), zabs1(cmul(kk, bj)));
        const double is = 1.0 / sg;
        const cplx t1 = cmul(j, cscale(kjpz, is)), t2 = cmul(cscale(bj, is), kjp);
        const cplx gj = csub(t2, t1);                                                               // gj_n / sigma_n
        cplx f = cmul(cmul(blc, crecip(gj)), cscale(dkw, -is));
        if (!(zabs1(gj) > kInteriorCancel * (zabs1(t1) + zabs1(t2))) || !cfinite(f)) f = cnan();
        sF[n] = f;
      }
    }
  }
  __syncthreads();
  const size_t base = ((size_t)s * B + b) * H;
  for (int h = threadIdx.x; h < H; h += 64) {
    cplx v = cmul(dens[base + h], sF[deg[h]]);
    if (!cfinite(v)) v = cnan();
    a[base + h] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// The field, ONE POINT PER LANE: the skeleton of k_uscat_fast<TREE, false, true> (workgroup-uniform loop over the balls, the ball's
// coefficients staged in LDS, j_n by radial_jh's backward recurrence into the lane's own LDS row) around that kernel's harmonic loops
// (BIEM_FIELD_HARMONICS, fast_layout.hpp: one text for both; the upward recurrence of the exterior kind is a constant zero here and
// folds away), with three differences:
//   - the argument of j_n is k_b r with the ball's own complex wavenumber;
//   - a lane contributes only for the ball that contains its point (r < rho: exactly where k_uscat_fast masks);
//   - a ball that holds no point of the workgroup is not staged, and a wave none of whose lanes lies in it skips its radial and
//     harmonic loops.  Both barriers of a ball are reached by every wave or by none (the vote is workgroup-wide).
// out[p][s]; NaN where no ball contains the point, and inside a ball with a NaN coefficient (the sums carry it) or a NaN k_b.
// ---------------------------------------------------------------------------------------------
template <int TREE>
__global__ void __launch_bounds__(64) k_uinterior_fast(int d, int H, int n_end, const int* __restrict__ labels, int nb, int B, int P,
                                                        const double* __restrict__ centers, const double* __restrict__ radii,
                                                        int geom_batched, const cplx* __restrict__ kint, int fluid_batched,
                                                        const cplx* __restrict__ a, const double* __restrict__ pts, int flags,
                                                        cplx* __restrict__ out) {
  BIEM_FAST_LAYOUT()
  const int js = (n_end + 2) | 1;           // row stride of the per-lane j_n store (radial_jh wants n_end + 1 slots at d = 4); odd: conflict-free
  const int s = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
  cplx* sJl = sC + nC + (size_t)tid * js;
  const int p = blockIdx.x * T + tid, pc = p < P ? p : P - 1;
  const bool pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  (void)ra; (void)rb; (void)cmm; (void)ga; (void)gia; (void)g0; (void)jA; (void)jB; (void)jC; (void)jN; (void)K2; (void)ms;
  BIEM_FAST_TABLES()
  double x[4];
  for (int i = 0; i < d; ++i) x[i] = pb ? pts[((size_t)i * P + pc) * nb + s] : pts[(size_t)i * P + pc];
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  double tr = qnan, ti = 0.0;               // no ball contains the point
  for (int b = 0; b < B; ++b) {
    const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
    const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
    double u[4] = {0.0, 0.0, 0.0, 0.0}, r2 = 0.0;
    for (int i = 0; i < d; ++i) { u[i] = x[i] - cb[i]; r2 += u[i] * u[i]; }
    const double r = sqrt(r2);
    const bool in = p < P && r < rho;
    // (a barrier: the previous ball's coefficients are no longer read, and the tables are written)
    if (!__syncthreads_or(in ? 1 : 0)) continue;
    const cplx* cs = a + ((size_t)s * B + b) * H;
    BIEM_FAST_STAGE()
    __syncthreads();
    if (__ballot(in) == 0ull) continue;     // (after both barriers)
    if (in) {
      const cplx kb = kint[(fluid_batched ? (size_t)s * B : 0) + b];
      double br = qnan, bi = 0.0;           // (a NaN k_b)
      if (isfinite(kb.x) && isfinite(kb.y)) {
        if (r > 0.0) radial_jh(d, n_end - 1, cscale(kb, r), (zc*)sJl, nullptr);
        else {                                // centre of the ball: z_n(0) = delta_{n0} sqrt(pi/2) 2^{1-d/2} / Gamma(d/2)
          const double z0 = radial_z0_at_zero(d);
          for (int n = 0; n < n_end; ++n) sJl[n] = make_double2(n == 0 ? z0 : 0.0, 0.0);
        }
        // the radial part BIEM_FIELD_HARMONICS asks for: no upward recurrence here, the factor comes from the lane's j_n row
        const cplx zero = make_double2(0.0, 0.0), h0 = zero, h1 = zero;
        auto advance = [&](const cplx&, const cplx&, double) -> cplx { return zero; };
        auto radial = [&](int n, const cplx&) -> cplx { return sJl[n]; };
        BIEM_FIELD_HARMONICS()
        ar *= kInvSqrt2Pi; ai *= kInvSqrt2Pi;
        if (!(isfinite(ar) && isfinite(ai))) { ar = qnan; ai = 0.0; }
        br = ar; bi = ai;
      }
      tr = br; ti = bi;
    }
  }
  if (p < P) out[(size_t)p * nb + s] = make_double2(tr, ti);
}

// ---------------------------------------------------------------------------------------------
// The gradient of that field, ONE POINT PER LANE: the skeleton of k_uinterior_fast (containment vote, staging only the
// balls that hold a point of the workgroup, both barriers reached by every wave or by none) around the harmonic loops of
// k_uscat_grad_fast<TREE, true> (BIEM_GRAD_HARMONICS: the solid-harmonic form, which never divides by a sine, so the centre of a ball
// and the axes of the tree are ordinary points).  The radial weights carry the ball's own complex wavenumber,
//   alpha_n = -k_b j_{n+1}(k_b r),   beta_n = j_n(k_b r) / r,
// from j_0 .. j_{n_end} in the lane's LDS row; at r = 0 only j_1 / r -> k_b z_0(0) / d survives and alpha = 0.
// out[i][p][s], component i in the plan's (canonical) axes; NaN in every component wherever k_uinterior_fast writes NaN: a NaN
// coefficient enters at least one of the d sums, and one sum that is not finite poisons all components of that ball.
// ---------------------------------------------------------------------------------------------
template <int TREE>
__global__ void __launch_bounds__(64) k_uinterior_grad_fast(int d, int H, int n_end, const int* __restrict__ labels, int nb, int B, int P,
                                                             const double* __restrict__ centers, const double* __restrict__ radii,
                                                             int geom_batched, const cplx* __restrict__ kint, int fluid_batched,
                                                             const cplx* __restrict__ a, const double* __restrict__ pts, int flags,
                                                             cplx* __restrict__ out) {
  constexpr int D = TREE == TREE_A ? 2 : TREE == TREE_BA ? 3 : 4;   // = d (a compile-time extent keeps x, e, g in registers)
  BIEM_FAST_LAYOUT()
  const int js = (n_end + 3) | 1;           // j_0 .. j_{n_end} per lane (radial_jh wants n_end + 2 slots at d = 4); odd: conflict-free
  const int s = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
  cplx* sJl = sC + nC + (size_t)tid * js;
  const int p = blockIdx.x * T + tid, pc = p < P ? p : P - 1;
  const bool pb = (flags & BIEM_USCAT_POINTS_BATCHED) != 0;
  const size_t cstride = (size_t)P * nb;    // between the components of the output
  (void)d; (void)ra; (void)rb; (void)cmm; (void)ga; (void)gia; (void)g0; (void)jA; (void)jB; (void)jC; (void)jN; (void)K2; (void)ms;
  BIEM_FAST_TABLES()
  double x[4];
  for (int i = 0; i < D; ++i) x[i] = pb ? pts[((size_t)i * P + pc) * nb + s] : pts[(size_t)i * P + pc];
  const cplx zero = make_double2(0.0, 0.0), qnan = cnan();
  cplx tot[4] = {qnan, qnan, qnan, qnan};   // no ball contains the point
  for (int b = 0; b < B; ++b) {
    const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * D;
    const double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
    double u[4] = {0.0, 0.0, 0.0, 0.0}, r2 = 0.0;
    for (int i = 0; i < D; ++i) { u[i] = x[i] - cb[i]; r2 += u[i] * u[i]; }
    const double r = sqrt(r2);
    const bool in = p < P && r < rho;
    // (a barrier: the previous ball's coefficients are no longer read, and the tables are written)
    if (!__syncthreads_or(in ? 1 : 0)) continue;
    const cplx* cs = a + ((size_t)s * B + b) * H;
    BIEM_FAST_STAGE()
    __syncthreads();
    if (__ballot(in) == 0ull) continue;     // (after both barriers)
    if (in) {
      const cplx kb = kint[(fluid_batched ? (size_t)s * B : 0) + b];
      for (int i = 0; i < D; ++i) tot[i] = qnan;
      if (cfinite(kb)) {
        // e = u / r; at the centre any unit vector does (grad S_1 is constant)
        const double invr = r > 0.0 ? 1.0 / r : 1.0;
        double e[4] = {1.0, 0.0, 0.0, 0.0};
        if (r > 0.0) for (int i = 0; i < 4; ++i) e[i] = u[i] / r;
        cplx kneg = make_double2(-kb.x, -kb.y);                     // alpha_n = kneg j_{n+1}
        if (r > 0.0) radial_jh(D, n_end, cscale(kb, r), (zc*)sJl, nullptr);
        else {                                // centre: j_{n+1}(0) = 0 and j_n / r -> delta_{n1} k_b z_0(0) / d, kept in place of j_1 (invr = 1)
          const double z0 = radial_z0_at_zero(D) / (double)D;
          for (int n = 0; n <= n_end; ++n) sJl[n] = n == 1 ? cscale(kb, z0) : zero;
          kneg = zero;
        }
        // the radial part BIEM_GRAD_HARMONICS asks for: no upward recurrence here, the weights come from the lane's j_n row
        const cplx h0 = zero, h1 = zero;
        auto advance = [&](const cplx&, const cplx&, double) -> cplx { return zero; };
        auto radial2 = [&](int n, const cplx&, const cplx&, cplx& al, cplx& be) {
          al = cmul(kneg, sJl[n + 1]); be = cscale(sJl[n], invr);
        };
        BIEM_GRAD_HARMONICS()
        bool fin = true;
        for (int i = 0; i < D; ++i) { g[i] = cscale(g[i], kInvSqrt2Pi); fin = fin && cfinite(g[i]); }
        if (fin) for (int i = 0; i < D; ++i) tot[i] = g[i];
      }
    }
  }
  if (p < P) for (int i = 0; i < D; ++i) out[i * cstride + (size_t)p * nb + s] = tot[i];
}

namespace {
// what the per-lane kernel covers: 0 and a message otherwise
int interior_cap(const biem_plan* p, const char* who) {
  const int cap = uscat_fast_nend_max(p->tree);
  if (cap == 0) {
    set_error("%s: built for the trees a, ba (bpa), bba (bpbpa) and caa; chain trees (d=%d) are not covered", who, p->d);
    return 0;
  }
  if (p->n_end > cap) {
    set_error("%s: n_end=%d above the per-lane ceiling %d of this tree (a %d, ba %d, bba %d, caa %d)", who, p->n_end, cap,
              uscat_fast_nend_max(TREE_A), uscat_fast_nend_max(TREE_BA), uscat_fast_nend_max(TREE_BBA), uscat_fast_nend_max(TREE_CAA));
    return 0;
  }
  return cap;
}
}  // namespace

int launch_interior_coef(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                         int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched, const double* d_density,
                         double* d_a, hipStream_t st) {
  static_assert(kMaxRad >= 320, "the coefficient kernel's LDS tables hold every per-lane order");
  if (!interior_cap(p, "biem_interior_coef")) return BIEM_ERR_UNSUPPORTED;
  if (nb > 65535) { set_error("biem_interior_coef: more than 65535 systems in one call (%d)", nb); return BIEM_ERR_UNSUPPORTED; }
  if (nb <= 0 || B <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_interior_coef, dim3(B, nb), dim3(64), 0, st, p->d, p->H, p->n_end, p->d_deg, B, (const cplx*)d_k, d_eta, d_radii,
                     geom_batched, (const cplx*)d_kint, (const cplx*)d_delta, fluid_batched, (const cplx*)d_density, (cplx*)d_a);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

namespace {
// the field (grad = false: out[P][nb]) or its gradient (out[d][P][nb]) at points, after the coefficients
int interior_field(bool grad, const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                   const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                   const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                   hipStream_t st) {
  const char* who = grad ? "biem_uinterior_grad" : "biem_uinterior";
  if (flags & ~BIEM_USCAT_POINTS_BATCHED) {
    set_error("%s: flags=%d; only BIEM_USCAT_POINTS_BATCHED applies to the interior field", who, flags); return BIEM_ERR_ARG;
  }
  if (!interior_cap(p, who)) return BIEM_ERR_UNSUPPORTED;
  if (nb > 65535) { set_error("%s: more than 65535 systems in one call (%d)", who, nb); return BIEM_ERR_UNSUPPORTED; }
  const int ne = p->n_end, T = 64;
  const size_t shm = fast_layout_lds_bytes(p->tree, ne, T, grad ? (ne + 3) | 1 : (ne + 2) | 1);   // (the kernels' js: the gradient reads j_{n_end} too)
  // The kernel's own LDS (what the compiler reserves beside the dynamic part) counts against the same 160 KiB per workgroup.  Without
  // it 2-D n_end = 153 passed this check with 163600 bytes and failed later in hipFuncSetAttribute.  Read once per kernel.
  const void* kern = nullptr;
#define BIEM_UINTERIOR_PICK(TREE) kern = grad ? (const void*)k_uinterior_grad_fast<TREE> : (const void*)k_uinterior_fast<TREE>;
  BIEM_FAST_TREE_DISPATCH(p->tree, BIEM_UINTERIOR_PICK)
#undef BIEM_UINTERIOR_PICK
  static std::atomic<long> own_lds[2][4] = {{{-1}, {-1}, {-1}, {-1}}, {{-1}, {-1}, {-1}, {-1}}};
  std::atomic<long>& own = own_lds[grad ? 1 : 0][p->tree];
  if (own.load() < 0) {
    hipFuncAttributes fa;
    BIEM_HIPCHK(hipFuncGetAttributes(&fa, kern));
    own.store((long)fa.sharedSizeBytes);
  }
  if (shm + (size_t)own.load() > 160 * 1024) {
    set_error("%s: n_end=%d needs %zu bytes of LDS per workgroup (limit %d)", who, ne, shm + (size_t)own.load(), 160 * 1024);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (nb <= 0 || B <= 0 || P <= 0) return BIEM_OK;
  const size_t need = (size_t)nb * B * p->H * sizeof(cplx);
  if (work_bytes < need) { set_error("%s: workspace too small", who); return BIEM_ERR_ARG; }
  cplx* a = (cplx*)d_work;
  const int rc = launch_interior_coef(p, nb, B, d_k, d_eta, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density,
                                      (double*)a, st);
  if (rc != BIEM_OK) return rc;
#define BIEM_UINTERIOR(KERNEL, TREE)                                                                                             \
  {                                                                                                                              \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)KERNEL<TREE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));           \
    hipLaunchKernelGGL((KERNEL<TREE>), dim3((P + T - 1) / T, nb), dim3(T), shm, st, p->d, p->H, ne, p->d_labels, nb, B, P,       \
                       d_centers, d_radii, geom_batched, (const cplx*)d_kint, fluid_batched, (const cplx*)a, d_points, flags,    \
                       (cplx*)d_out);                                                                                            \
  }
#define BIEM_UINTERIOR_TREE(TREE) { if (grad) BIEM_UINTERIOR(k_uinterior_grad_fast, TREE) else BIEM_UINTERIOR(k_uinterior_fast, TREE) }
  BIEM_FAST_TREE_DISPATCH(p->tree, BIEM_UINTERIOR_TREE)
#undef BIEM_UINTERIOR_TREE
#undef BIEM_UINTERIOR
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}
}  // namespace

int launch_uinterior(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                     const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                     const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                     hipStream_t st) {
  return interior_field(false, p, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density,
                        d_points, flags, d_out, d_work, work_bytes, st);
}

int launch_uinterior_grad(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                          const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                          const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                          hipStream_t st) {
  return interior_field(true, p, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density,
                        d_points, flags, d_out, d_work, work_bytes, st);
}

}  // namespace biem
