// kernels_ladder.hip -- Hessian of the scattered field by a coefficient ladder (gfx950), and the field and gradient of a
// multipole source by the same ladder.
//
// For z = h (outer) or z = j (kind inner) in every dimension, with T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega (the plan's force
// coupling table, plan_build_force):
//   d/dx_i [ z_n(k r) Y_h(e) ] = k [ z_{n-1}(k r) P_{n-1}(e_i Y_h) - z_{n+1}(k r) P_{n+1}(e_i Y_h) ],   P_{n'}(e_i Y_h) = sum_{h' of degree n'} T^i_{h'h} Y_h'
// so a derivative of a multipole expansion is a multipole expansion about the same centre, one degree longer, with the coefficients
//   (D_i c)_{h'} = k sgn(n_h - n_h') sum_h T^i_{h'h} c_h .
// The Hessian is the value kernels of biem_uscat (kernels_uscat.hip, untouched) applied to D_j D_i c in a plan two degrees longer.
#include "common.hpp"
#include <string>

namespace biem {

// out[s][b][h'] = k_s sum_e sgn(deg[col_e] - deg[h']) T_e in[s][b][col_e] over the entries e of (row h', component comp) whose column
// has a degree < n_src: one wave per (ball, system) = (blockIdx.x, .y), the lanes stride over the rows.  Every row is written (zeros
// included), each by one lane in the order of the table: no atomics, two calls agree bit for bit.  in and out must not overlap.
__global__ void __launch_bounds__(64) k_coef_ladder(int d, int H, int comp, int n_src, const int* __restrict__ deg,
                                                     const uint32_t* __restrict__ fptr, const int* __restrict__ fcol,
                                                     const cplx* __restrict__ fval, int B, const cplx* __restrict__ k,
                                                     const cplx* __restrict__ in, cplx* __restrict__ out) {
  const int b = blockIdx.x, s = blockIdx.y;
  const cplx kk = k[s];
  const size_t row = ((size_t)s * B + b) * H;
  for (int hp = threadIdx.x; hp < H; hp += 64) {
    const int np_ = deg[hp];
    cplx up = make_double2(0.0, 0.0), dn = make_double2(0.0, 0.0);     // columns one degree above the row, one below
    for (uint32_t e = fptr[(size_t)hp * d + comp], e1 = fptr[(size_t)hp * d + comp + 1]; e < e1; ++e) {
      const int h = fcol[e];
      const int n = deg[h];
      if (n >= n_src) continue;
      const cplx t = cmul(fval[e], in[row + h]);
      if (n > np_) up = cadd(up, t); else dn = cadd(dn, t);
    }
    out[row + hp] = cmul(kk, csub(up, dn));
  }
}

size_t uscat_hess_workspace_bytes(const biem_plan* p, int nb, int B) { return (size_t)(p->d + 2) * nb * B * p->H * sizeof(cplx); }

static void ladder(const biem_plan* p, int nb, int B, int comp, int n_src, const double* d_k, const cplx* in, cplx* out, hipStream_t st) {
  hipLaunchKernelGGL(k_coef_ladder, dim3(B, nb), dim3(64), 0, st, p->d, p->H, comp, n_src, p->d_deg, p->d_fptr_comp, p->d_fcol,
                     (const cplx*)p->d_fval, B, (const cplx*)d_k, in, out);
}

// Workspace: c, g_0 .. g_{d-1}, then the buffer of the pair in flight - d + 2 coefficient sets.  Every launch is on `st`, so the
// field kernel of one pair has read the pair buffer before the ladder of the next pair writes it.
int launch_uscat_hess(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                      double* d_out, void* d_work, size_t work_bytes, hipStream_t st) {
  if (flags & BIEM_USCAT_FAR_FIELD) { set_error("biem_uscat_hess: the far-field pattern has no Hessian in space (BIEM_USCAT_FAR_FIELD)"); return BIEM_ERR_ARG; }
  if (p->n_end < 3) { set_error("biem_uscat_hess: the plan has n_end=%d; it is the plan of order n_end + 2 of the density, at least 3", p->n_end); return BIEM_ERR_ARG; }
  if (!p->force_uploaded) { set_error("biem_uscat_hess: the plan's force coupling table is not on the device"); return BIEM_ERR_ARG; }
  if (nb > 65535) { set_error("biem_uscat_hess: more than 65535 systems in one call (%d)", nb); return BIEM_ERR_UNSUPPORTED; }
  if (nb <= 0 || B <= 0 || P <= 0) return BIEM_OK;
  int rc = uscat_covered(p, nb, B, flags);
  if (rc != BIEM_OK) {
    const std::string why = last_error();
    set_error("biem_uscat_hess: the field of the plan of order n_end=%d is not built (%s)", p->n_end, why.c_str());
    return rc == BIEM_ERR_UNSUPPORTED ? rc : BIEM_ERR_ARG;
  }
  if (work_bytes < uscat_hess_workspace_bytes(p, nb, B)) { set_error("biem_uscat_hess: workspace too small"); return BIEM_ERR_ARG; }
  const int d = p->d, n_src = p->n_end - 2;
  const size_t set = (size_t)nb * B * p->H;
  cplx* c = (cplx*)d_work;
  cplx* g = c + set;
  cplx* pair = g + (size_t)d * set;
  if ((rc = uscat_form_coef(p, nb, B, d_k, d_eta, d_radii, geom_batched, d_density, flags, c, st)) != BIEM_OK) return rc;
  for (int i = 0; i < d; ++i) ladder(p, nb, B, i, n_src, d_k, c, g + (size_t)i * set, st);
  BIEM_LAUNCHCHK();
  const size_t per = (size_t)P * nb * ((flags & BIEM_USCAT_PER_BALL) ? B : 1) * 2;      // doubles of one component pair of the result
  int q = 0;
  for (int i = 0; i < d; ++i)
    for (int j = i; j < d; ++j, ++q) {
      ladder(p, nb, B, j, n_src + 1, d_k, g + (size_t)i * set, pair, st);
      BIEM_LAUNCHCHK();
      if ((rc = uscat_eval_coef(p, nb, B, P, d_k, d_centers, d_radii, geom_batched, pair, d_points, flags, d_out + (size_t)q * per, st)) != BIEM_OK) return rc;
    }
  return BIEM_OK;
}

// ---- the field of an outgoing multipole h_n'(k |x - s|) Y_h'((x - s)^) itself: the scattered field of one fictitious ball per system at
// s, radius 0, with the unit coefficient set delta_{h, idx}; its gradient: one ladder step per component, then the value kernels
// (launch_uscat_hess's route taken once).  The regular wave j_n' Y_h' about s (BIEM_USCAT_KIND_INNER): the kind-inner value kernels on the
// same unit set, the fictitious ball of infinite radius - kind inner masks r > rho only, so every point is an ordinary one, x = s included.
// A whole expansion about s (biem_expansion_field): the caller's coefficient set in place of the unit one, everything else unchanged.
// c[s][h] = delta_{h, idx[s]}; an index outside [0, H) leaves the set zero.  idx null: c = coef
__global__ void __launch_bounds__(256) k_unit_coef(int H, long long count, const int* __restrict__ idx, const cplx* __restrict__ coef,
                                                    cplx* __restrict__ c, double* __restrict__ radii, double radius) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const long long s = i / H;
    const int h = (int)(i - s * H);
    c[i] = idx ? make_double2(idx[s] == h ? 1.0 : 0.0, 0.0) : coef[i];
    if (h == 0) radii[s] = radius;
  }
}

// workspace: the unit set, one laddered set, the radii (zero; regular: infinite) of the fictitious balls
size_t multipole_field_workspace_bytes(const biem_plan* p, int nb) {
  return nb <= 0 ? 0 : 2 * align256((size_t)nb * p->H * sizeof(cplx)) + align256((size_t)nb * sizeof(double));
}

int launch_multipole_field(const char* who, const biem_plan* p, int nb, int P, const double* d_k, const double* d_src, const int* d_idx,
                           const double* d_coef, const double* d_points, int flags, int grad, double* d_out, void* d_work, size_t work_bytes,
                           hipStream_t st) {
  if (flags & ~(BIEM_USCAT_POINTS_BATCHED | BIEM_USCAT_KIND_INNER)) { set_error("%s: flags other than BIEM_USCAT_POINTS_BATCHED and BIEM_USCAT_KIND_INNER (%d)", who, flags); return BIEM_ERR_ARG; }
  if (grad && p->n_end < 2) { set_error("%s: the gradient needs the plan of order n' + 2 of the source's degree n', at least 2 (n_end=%d)", who, p->n_end); return BIEM_ERR_ARG; }
  if (grad && !p->force_uploaded) { set_error("%s: the plan's force coupling table is not on the device", who); return BIEM_ERR_ARG; }
  if (nb > 65535) { set_error("%s: more than 65535 systems in one call (%d)", who, nb); return BIEM_ERR_UNSUPPORTED; }
  if (nb <= 0 || P <= 0) return BIEM_OK;
  int rc = uscat_covered(p, nb, 1, flags);
  if (rc != BIEM_OK) {
    const std::string why = last_error();
    set_error("%s: the field of the plan of order n_end=%d is not built (%s)", who, p->n_end, why.c_str());
    return rc == BIEM_ERR_UNSUPPORTED ? rc : BIEM_ERR_ARG;
  }
  if (work_bytes < multipole_field_workspace_bytes(p, nb)) { set_error("%s: workspace too small", who); return BIEM_ERR_ARG; }
  const size_t set = align256((size_t)nb * p->H * sizeof(cplx));
  cplx* c = (cplx*)d_work;
  cplx* g = (cplx*)((char*)d_work + set);
  double* radii = (double*)((char*)d_work + 2 * set);
  const long long count = (long long)nb * p->H;
  hipLaunchKernelGGL(k_unit_coef, dim3((unsigned)((count + 255) / 256 < 65536 ? (count + 255) / 256 : 65536)), dim3(256), 0, st, p->H, count, d_idx, (const cplx*)d_coef, c, radii,
                     (flags & BIEM_USCAT_KIND_INNER) ? (double)INFINITY : 0.0);
  BIEM_LAUNCHCHK();
  if (!grad) return uscat_eval_coef(p, nb, 1, P, d_k, d_src, radii, 1, c, d_points, flags, d_out, st);
  const size_t per = (size_t)P * nb * 2;                     // doubles of one component of the result
  for (int i = 0; i < p->d; ++i) {
    // (the set's entries are of degrees the caller keeps below n_end - 1 - others are not read -: the step stays inside the plan)
    ladder(p, nb, 1, i, p->n_end - 1, d_k, c, g, st);
    BIEM_LAUNCHCHK();
    if ((rc = uscat_eval_coef(p, nb, 1, P, d_k, d_src, radii, 1, g, d_points, flags, d_out + (size_t)i * per, st)) != BIEM_OK) return rc;
  }
  return BIEM_OK;
}

}  // namespace biem
