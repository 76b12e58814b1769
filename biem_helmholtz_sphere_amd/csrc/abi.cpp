// abi.cpp -- extern "C" entry points of libbiem_mi355.so (declared in include/biem_mi355.h).
#include "common.hpp"
#include <cstdlib>
#include <cstring>
#include <new>

using namespace biem;

namespace biem {
Profiler& profiler() { static thread_local Profiler p; return p; }
hipEvent_t Profiler::get() {
  hipEvent_t e = nullptr;
  if (!pool.empty()) { e = pool.back(); pool.pop_back(); return e; }
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace biem

// (the *_AS forms: a body shared by two entry points reports under the name of the one that was called)
#define NEED_AS(who, p, what) do { if (!(p)) { set_error("%s: null %s", who, what); return BIEM_ERR_ARG; } } while (0)
#define NEED_DEV_AS(who, pl) do { NEED_AS(who, pl, "plan"); if ((pl)->device < 0) { set_error("%s: plan not uploaded to a device (biem_plan_upload)", who); return BIEM_ERR_ARG; } } while (0)
#define NEED(p, what) NEED_AS(__func__, p, what)
#define NEED_DEV(pl) NEED_DEV_AS(__func__, pl)

extern "C" {

int biem_version(void) { return 200; }   // 0.2.0

// hash of the sources this library was built from (set by _build.py; the loader compares it with the checkout's)
#ifndef BIEM_SRC_HASH
#define BIEM_SRC_HASH "unknown"
#endif
extern const char biem_src_hash_marker[] = "BIEM_SRC_HASH=" BIEM_SRC_HASH ";";
const char* biem_build_id(void) { return BIEM_SRC_HASH; }

const char* biem_last_error(void) { return last_error(); }

int biem_device_count(int* n) {
  NEED(n, "n");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess || c <= 0) { *n = 0; set_error("no HIP device visible: %s", hipGetErrorString(e)); return BIEM_ERR_NO_DEVICE; }
  *n = c;
  return BIEM_OK;
}

int biem_plan_create_host(int tree, int n_end, biem_plan** plan) {
  NEED(plan, "plan");
  biem_plan* p = new (std::nothrow) biem_plan();
  if (!p) { set_error("out of host memory"); return BIEM_ERR_ALLOC; }
  int rc = BIEM_OK;
  try {
    rc = plan_build_host(p, tree, n_end);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory building tables for n_end=%d", n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) { delete p; *plan = nullptr; return rc; }
  *plan = p;
  return BIEM_OK;
}

int biem_plan_upload(biem_plan* plan) { NEED(plan, "plan"); return plan_upload(plan); }

int biem_plan_create_chain_host(int d, int n_end, biem_plan** plan) {
  NEED(plan, "plan");
  biem_plan* p = new (std::nothrow) biem_plan();
  if (!p) { set_error("out of host memory"); return BIEM_ERR_ALLOC; }
  int rc = BIEM_OK;
  try {
    rc = plan_build_chain_host(p, d, n_end);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory building chain tables for d=%d n_end=%d", d, n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) { delete p; *plan = nullptr; return rc; }
  *plan = p;
  return BIEM_OK;
}

int biem_plan_create_chain(int d, int n_end, biem_plan** plan) {
  int n = 0;
  int rc = biem_device_count(&n);
  if (rc != BIEM_OK) return rc;
  rc = biem_plan_create_chain_host(d, n_end, plan);
  if (rc != BIEM_OK) return rc;
  rc = plan_upload(*plan);
  if (rc != BIEM_OK) { plan_free(*plan); *plan = nullptr; }
  return rc;
}

int biem_plan_create(int tree, int n_end, biem_plan** plan) {
  int n = 0;
  int rc = biem_device_count(&n);
  if (rc != BIEM_OK) return rc;
  rc = biem_plan_create_host(tree, n_end, plan);
  if (rc != BIEM_OK) return rc;
  rc = plan_upload(*plan);
  if (rc != BIEM_OK) { plan_free(*plan); *plan = nullptr; }
  return rc;
}

int biem_plan_destroy(biem_plan* plan) { if (plan) plan_free(plan); return BIEM_OK; }

int biem_plan_info(const biem_plan* plan, int* d, int* n_harm, int* n_quad, int* n_harm2, long long* n_terms) {
  NEED(plan, "plan");
  if (d) *d = plan->d;
  if (n_harm) *n_harm = plan->H;
  if (n_quad) *n_quad = plan->Q;
  if (n_harm2) *n_harm2 = plan->H2;
  if (n_terms) *n_terms = (long long)plan->coef.size();
  return BIEM_OK;
}

int biem_plan_labels(const biem_plan* plan, int* h_labels, int* h_deg) {
  NEED(plan, "plan");
  if (plan->lw != 3) { set_error("biem_plan_labels: this plan's labels have %d entries; use biem_plan_labels_n", plan->lw); return BIEM_ERR_UNSUPPORTED; }
  if (h_labels) memcpy(h_labels, plan->labels.data(), plan->labels.size() * sizeof(int));
  if (h_deg) memcpy(h_deg, plan->deg.data(), plan->deg.size() * sizeof(int));
  return BIEM_OK;
}

int biem_plan_labels_n(const biem_plan* plan, int width, int* h_labels, int* h_deg) {
  NEED(plan, "plan");
  if (width < plan->lw) { set_error("biem_plan_labels_n: width %d < the plan's label width %d", width, plan->lw); return BIEM_ERR_ARG; }
  if (h_labels)
    for (int h = 0; h < plan->H; ++h)
      for (int j = 0; j < width; ++j) h_labels[(size_t)h * width + j] = j < plan->lw ? plan->labels[(size_t)h * plan->lw + j] : 0;
  if (h_deg) memcpy(h_deg, plan->deg.data(), plan->deg.size() * sizeof(int));
  return BIEM_OK;
}

int biem_plan_symmetric_order(const biem_plan* plan, int* h_partner, int* h_slot) {
  NEED(plan, "plan");
  const int U = (int)(plan->units.size() / 2);
  for (int u = 0; u < U; ++u) {
    const int h = plan->units[2 * u], p = plan->units[2 * u + 1];
    if (h_partner) { h_partner[h] = p; h_partner[p] = h; }
  }
  if (h_slot) memcpy(h_slot, plan->hpos.data(), plan->hpos.size() * sizeof(int));
  return BIEM_OK;
}

int biem_plan_split_order(const biem_plan* plan, int B, int* n_cos, int* nE, int* nO, int* npE, int* npO, int* h_row) {
  NEED(plan, "plan");
  if (B < 1) { set_error("biem_plan_split_order: B < 1"); return BIEM_ERR_ARG; }
  const int H = plan->H, U = (int)(plan->units.size() / 2);
  const SplitMap m = make_split_map(B, H, U);
  if (n_cos) *n_cos = U;
  if (nE) *nE = B * U;
  if (nO) *nO = B * (H - U);
  if (npE) *npE = m.npE;
  if (npO) *npO = m.npO;
  if (h_row)
    for (int b = 0; b < B; ++b)
      for (int slot = 0; slot < H; ++slot) h_row[(size_t)b * H + slot] = m.row_of(b, H, slot);
  return BIEM_OK;
}

int biem_plan_fill_info(const biem_plan* plan, int* n_units, int* n_phases, int* reduced_ok, int* lds_rows, int* gather_ok) {
  NEED(plan, "plan");
  if (n_units) *n_units = plan->E;
  if (n_phases) *n_phases = plan->NP;
  if (reduced_ok) *reduced_ok = plan->red_lists_ok ? 1 : 0;
  if (lds_rows) *lds_rows = plan->rchunk_rows_max;
  if (gather_ok) *gather_ok = (plan->pair_lists_ok && plan->qchunk.size() > 1) ? 1 : 0;
  return BIEM_OK;
}

int biem_plan_quadrature(const biem_plan* plan, double* h_y, double* h_w) {
  NEED(plan, "plan");
  if (h_y) memcpy(h_y, plan->qy.data(), plan->qy.size() * sizeof(double));
  if (h_w) memcpy(h_w, plan->qw.data(), plan->qw.size() * sizeof(double));
  return BIEM_OK;
}

int biem_plan_projection(const biem_plan* plan, double* h_W) {
  NEED(plan, "plan"); NEED(h_W, "h_W");
  memcpy(h_W, plan->W.data(), plan->W.size() * sizeof(double));
  return BIEM_OK;
}

int biem_plan_terms(const biem_plan* plan, long long* h_ptr, double* h_coef, int* h_tidx) {
  NEED(plan, "plan");
  if (!plan->lists_built) { set_error("biem_plan_terms: a 2-D plan of order n_end > %d holds no term lists (one Graf term per entry, evaluated directly)", kLists2dMax); return BIEM_ERR_UNSUPPORTED; }
  if (h_ptr) for (size_t i = 0; i < plan->ptr.size(); ++i) h_ptr[i] = (long long)plan->ptr[i];
  if (h_coef) memcpy(h_coef, plan->coef.data(), plan->coef.size() * sizeof(double));
  if (h_tidx) memcpy(h_tidx, plan->tidx.data(), plan->tidx.size() * sizeof(int));
  return BIEM_OK;
}

int biem_plan_force_terms(biem_plan* plan, long long* n_entries, long long* h_ptr, int* h_col, int* h_comp, double* h_val) {
  NEED(plan, "plan");
  int rc = BIEM_OK;
  try {
    rc = plan_build_force(plan);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory building the force coupling table for n_end=%d", plan->n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) return rc;
  if (n_entries) *n_entries = (long long)plan->fcol.size();
  if (h_ptr) for (size_t i = 0; i < plan->fptr.size(); ++i) h_ptr[i] = (long long)plan->fptr[i];
  if (h_col) memcpy(h_col, plan->fcol.data(), plan->fcol.size() * sizeof(int));
  if (h_comp) memcpy(h_comp, plan->fcomp.data(), plan->fcomp.size() * sizeof(int));
  if (h_val) memcpy(h_val, plan->fval.data(), plan->fval.size() * sizeof(double));
  return BIEM_OK;
}

int biem_radial(int d, int nmax, int count, const double* d_x, double* d_out, void* stream) {
  NEED(d_x, "d_x"); NEED(d_out, "d_out");
  return launch_radial(d, nmax, count, d_x, d_out, (hipStream_t)stream);
}

int biem_radial_complex(int d, int nmax, int count, const double* d_z, double* d_out, void* stream) {
  NEED(d_z, "d_z"); NEED(d_out, "d_out");
  return launch_radial_c(d, nmax, count, d_z, d_out, (hipStream_t)stream);
}

int biem_harmonics(const biem_plan* plan, int count, const double* d_u, double* d_Y, void* stream) {
  NEED_DEV(plan); NEED(d_u, "d_u"); NEED(d_Y, "d_Y");
  return launch_harmonics(plan, count, d_u, d_Y, (hipStream_t)stream);
}

int biem_ball_tables(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                     int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_tab, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_radii, "d_radii"); NEED(d_alpha, "d_alpha"); NEED(d_beta, "d_beta"); NEED(d_tab, "d_tab");
  return launch_ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, (hipStream_t)stream);
}

int biem_rhs_project(const biem_plan* plan, int nb, int B, int nrhs, const double* d_g, double* d_f, long long sys_stride,
                     long long elem_stride, long long rhs_stride, void* stream) {
  NEED_DEV(plan); NEED(d_g, "d_g"); NEED(d_f, "d_f");
  return launch_rhs_project(plan, nb, B, nrhs, d_g, d_f, sys_stride, elem_stride, rhs_stride, (hipStream_t)stream);
}

int biem_ball_tables_n(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_tab, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_radii, "d_radii"); NEED(d_alpha_n, "d_alpha_n"); NEED(d_beta_n, "d_beta_n"); NEED(d_tab, "d_tab");
  return launch_ball_tables_n(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha_n, d_beta_n, ab_batched, d_tab, (hipStream_t)stream);
}

int biem_rhs_project_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn, const double* d_alpha_n,
                       const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride, long long elem_stride,
                       long long rhs_stride, void* stream) {
  NEED_DEV(plan); NEED(d_alpha_n, "d_alpha_n"); NEED(d_beta_n, "d_beta_n"); NEED(d_f, "d_f");
  return launch_rhs_project_n(plan, nb, B, nrhs, d_gu, d_gdn, d_alpha_n, d_beta_n, ab_batched, d_f, sys_stride, elem_stride, rhs_stride,
                              (hipStream_t)stream);
}

int biem_flag_unscalable(const biem_plan* plan, int nb, int B, const double* d_tab, int* d_info, int code, void* stream) {
  NEED_DEV(plan); NEED(d_tab, "d_tab"); NEED(d_info, "d_info");
  return launch_flag_unscalable(plan, nb, B, d_tab, d_info, code, (hipStream_t)stream);
}

size_t biem_fill_workspace_bytes(const biem_plan* plan, int nb, int B) { return plan ? fill_workspace_bytes(plan, nb, B) : 0; }

int biem_fill(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_centers, int geom_batched,
              const double* d_tab, int scaling, double* d_A, long long lda, long long sys_stride, int n_pad, void* d_work,
              size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_A, "d_A");
  if (B > 1) NEED(d_work, "d_work");
  if (scaling == BIEM_FILL_SYMMETRIC)
    return launch_fill_sym(plan, nb, B, d_k, d_centers, geom_batched, d_tab, d_A, lda, sys_stride, n_pad, d_work, work_bytes, (hipStream_t)stream);
  return launch_fill(plan, nb, B, d_k, d_centers, geom_batched, d_tab, scaling, d_A, lda, sys_stride, n_pad, d_work, work_bytes,
                     (hipStream_t)stream);
}

int biem_lu_npad(int N) { return lu_npad(N); }
size_t biem_lu_workspace_bytes(int nb, int n_pad, int nrhs) { return lu_workspace_bytes(nb, n_pad, nrhs); }

int biem_lu_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info,
                         void* d_work, size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_ipiv, "d_ipiv"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  // BIEM_LU_DISCARD_FACTORS=1 (tests): solve exactly as the fused path does, without storing the multipliers back
  const char* e = getenv("BIEM_LU_DISCARD_FACTORS");
  return launch_lu_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream,
                                !(e && e[0] == '1'));
}

int biem_ldlt_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info,
                           void* d_work, size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_ipiv, "d_ipiv"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  const char* e = getenv("BIEM_LU_DISCARD_FACTORS");
  return launch_lu_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream,
                                !(e && e[0] == '1'), /*symmetric=*/true);
}

int biem_lu_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info, void* d_work,
                   size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_ipiv, "d_ipiv"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  return launch_lu_factor_solve(nb, n_pad, 0, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream, true, false);
}

int biem_ldlt_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info, void* d_work,
                     size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_ipiv, "d_ipiv"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  return launch_lu_factor_solve(nb, n_pad, 0, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream, true, true);
}

int biem_lu_solve(int nb, int n_pad, int nrhs, const double* d_LU, long long lda, long long sys_stride, const int* d_ipiv, double* d_B,
                  long long ldb, long long b_stride, void* stream) {
  NEED(d_LU, "d_LU"); NEED(d_ipiv, "d_ipiv"); NEED(d_B, "d_B");
  return launch_lu_solve(nb, n_pad, nrhs, d_LU, lda, sys_stride, d_ipiv, d_B, ldb, b_stride, (hipStream_t)stream);
}

int biem_sym_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_info, void* d_work,
                          size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  return launch_sym_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_info, d_work, work_bytes, (hipStream_t)stream, false);
}

int biem_sym_factor_solve_n(int nb, int n_pad, int n_active, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_info,
                            void* d_work, size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  if (n_active < 1 || n_active > n_pad) { set_error("%s: n_active=%d outside 1 .. n_pad=%d", __func__, n_active, n_pad); return BIEM_ERR_ARG; }
  return launch_sym_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_info, d_work, work_bytes, (hipStream_t)stream, false, n_active);
}

int biem_sym_update_form(int nb, int n_pad, int nrhs) { return sym_update_left(nb, n_pad, nrhs); }
int biem_sym_form(int nb, int n_pad, int n_active, int nrhs, int* form, size_t* work) { return sym_form_query(nb, n_pad, n_active, nrhs, form, work); }

int biem_density(const biem_plan* plan, int nb, int B, int nrhs, const double* d_x, long long sys_stride, long long elem_stride,
                 long long rhs_stride, const double* d_tab, double* d_density, void* stream) {
  NEED_DEV(plan); NEED(d_x, "d_x"); NEED(d_tab, "d_tab"); NEED(d_density, "d_density");
  return launch_density(plan, nb, B, nrhs, d_x, sys_stride, elem_stride, rhs_stride, d_tab, d_density, (hipStream_t)stream);
}

size_t biem_uscat_workspace_bytes(const biem_plan* plan, int nb, int B) {
  return plan ? (size_t)nb * B * plan->H * sizeof(cplx) : 0;
}

int biem_uscat(const biem_plan* plan, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags, double* d_out,
               void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  NEED(d_density, "d_density"); NEED(d_points, "d_points"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  return launch_uscat(plan, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_density, d_points, flags, d_out, d_work,
                      work_bytes, (hipStream_t)stream);
}

int biem_uscat_grad(const biem_plan* plan, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                    const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags, double* d_out,
                    void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  NEED(d_density, "d_density"); NEED(d_points, "d_points"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  return launch_uscat_grad(plan, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_density, d_points, flags, d_out, d_work,
                           work_bytes, (hipStream_t)stream);
}

// ---- Hessian of the scattered field (kernels_ladder.hip) ----
size_t biem_uscat_hess_workspace_bytes(const biem_plan* plan, int nb, int B) { return plan ? uscat_hess_workspace_bytes(plan, nb, B) : 0; }

int biem_uscat_hess(biem_plan* plan, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                    const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags, double* d_out,
                    void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  NEED(d_density, "d_density"); NEED(d_points, "d_points"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  int rc = BIEM_OK;
  try {
    rc = plan_build_force(plan);             // (the first call of this plan: builds and uploads the coupling table)
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory building the force coupling table for n_end=%d", __func__, plan->n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) return rc;
  return launch_uscat_hess(plan, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_density, d_points, flags, d_out, d_work,
                           work_bytes, (hipStream_t)stream);
}

// ---- total field inside penetrable fluid balls (kernels_uinterior.hip) ----
int biem_interior_coef(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched, const double* d_density,
                       double* d_a, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_radii, "d_radii"); NEED(d_kint, "d_kint"); NEED(d_delta, "d_delta");
  NEED(d_density, "d_density"); NEED(d_a, "d_a");
  return launch_interior_coef(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density, d_a,
                              (hipStream_t)stream);
}

size_t biem_uinterior_workspace_bytes(const biem_plan* plan, int nb, int B) {
  return plan ? (size_t)nb * B * plan->H * sizeof(cplx) : 0;
}

int biem_uinterior(const biem_plan* plan, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                   const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                   const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                   void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  NEED(d_kint, "d_kint"); NEED(d_delta, "d_delta"); NEED(d_density, "d_density"); NEED(d_points, "d_points"); NEED(d_out, "d_out");
  NEED(d_work, "d_work");
  return launch_uinterior(plan, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density,
                          d_points, flags, d_out, d_work, work_bytes, (hipStream_t)stream);
}

int biem_uinterior_grad(const biem_plan* plan, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                        const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                        const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                        void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  NEED(d_kint, "d_kint"); NEED(d_delta, "d_delta"); NEED(d_density, "d_density"); NEED(d_points, "d_points"); NEED(d_out, "d_out");
  NEED(d_work, "d_work");
  return launch_uinterior_grad(plan, nb, B, P, d_k, d_eta, d_centers, d_radii, geom_batched, d_kint, d_delta, fluid_batched, d_density,
                               d_points, flags, d_out, d_work, work_bytes, (hipStream_t)stream);
}

// ---- whole path -----------------------------------------------------------------------------
namespace {
struct SolveLayout {
  int N, n_pad, chunk;
  long long lda, sys_stride;
  size_t off_tab, off_A, off_T, off_P, off_ipiv, off_info2, total;
  SplitMap split;                          // on: the split form of flat layouts (n_pad = npE + npO, lda and sys_stride with it)
};
// Flat layouts of at least this many unknowns take the split form; below, the step is bound by the per-panel launches, whose number
// does not fall.  (Not 392 or below: rejection codes of small flat systems are pinned in unsplit row numbers by the tests.)
constexpr int SYM_SPLIT_MIN_N = 1024;
thread_local int g_last_split[2] = {0, 0};   // npE, npO of the last symmetric solve on this thread; 0, 0: unsplit
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// degree-dependent boundary coefficients of the *_n entries: alpha_n / beta_n [nb or 1][B][n_end] in place of alpha / beta [nb or 1][B],
// the unmixed samples gu / gdn [nb][nrhs][B][Q] (either may be null: zero) in place of g
struct DegreeBc { const double* alpha_n; const double* beta_n; const double* gu; const double* gdn; };
// One size serves both forms (the caller asks for it before the geometry is looked at): every region is as large as the larger form needs,
// so the offsets are the same whichever runs; n_pad, lda and sys_stride are those of the form asked for.
SolveLayout make_layout(const biem_plan* p, int nb, int B, int nrhs, int chunk, bool split = false) {
  SolveLayout L;
  L.N = B * p->H;
  const int ldr = ((nrhs + 7) / 8) * 8;     // right-hand side columns; rows stay 128-byte aligned (8 complex128)
  const int np_plain = lu_npad(L.N);
  const SplitMap sm = make_split_map(B, p->H, (int)(p->units.size() / 2));
  const int np_split = sm.npE + sm.npO, np_max = np_split > np_plain ? np_split : np_plain;
  L.split = split ? sm : SplitMap();
  L.n_pad = split ? np_split : np_plain;
  L.lda = L.n_pad + ldr;
  L.sys_stride = (long long)L.n_pad * L.lda;
  const size_t sys_max = (size_t)np_max * (np_max + ldr);
  if (chunk <= 0) {
    // resident matrices per chunk: as many as fit ~24 GiB, at most nb
    size_t per = sys_max * 16 + (size_t)B * B * p->H2 * 16 + lu_workspace_bytes(1, np_max, nrhs);
    size_t fit = ((size_t)24 << 30) / (per ? per : 1);
    chunk = (int)(fit < 1 ? 1 : (fit > (size_t)nb ? (size_t)nb : fit));
  }
  if (chunk > nb) chunk = nb;
  if (chunk > 32768) chunk = 32768;            // grid y / z dimensions of the per-system kernels
  L.chunk = chunk;
  size_t o = 0;
  L.off_tab = o; o = align256(o + (size_t)nb * B * 3 * p->n_end * 16);
  L.off_A = o; o = align256(o + (size_t)chunk * sys_max * 16);
  L.off_T = o; o = align256(o + fill_workspace_bytes(p, chunk, B));
  L.off_P = o; o = align256(o + lu_workspace_bytes(chunk, np_max, nrhs));
  L.off_ipiv = o; o = align256(o + (size_t)chunk * np_max * sizeof(int));
  L.off_info2 = o; o = align256(o + (size_t)chunk * sizeof(int));     // the O block's codes of the split form
  L.total = o;
  return L;
}
}  // namespace

size_t biem_solve_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int chunk) {
  if (!plan || nb <= 0 || B <= 0 || nrhs < 1) return 0;
  return make_layout(plan, nb, B, nrhs, chunk).total;
}

// Flat layouts (every centre with the same last coordinate): A~ = diag(E, O) in the split order, factored as two blocks.  Whether this
// call takes the split form: `split` is set, or left off (SplitMap()).  The conditions that cost nothing come first; the centres come
// to the host only for calls that pass them (one small copy, one wait).
static int flat_layout_split(const biem_plan* plan, int B, int nrhs, const double* d_centers, int geom_batched, hipStream_t st, SplitMap& split) {
  split = SplitMap();
  const int H = plan->H, d = plan->d;
  const char* e = getenv("BIEM_SYM_SPLIT");
  const SplitMap sm = make_split_map(B, H, (int)(plan->units.size() / 2));
  if ((e && e[0] == '0') || geom_batched || plan->tree == TREE_CAA || !fill_sym_red_form(plan, B) || sym_small_path(B * H, nrhs) ||
      !((e && e[0] == '1') || B * H >= SYM_SPLIT_MIN_N) || sm.U >= H || ((nrhs + 7) / 8) * 8 > sm.npO)
    return BIEM_OK;
  std::vector<double> hc((size_t)B * d);
  BIEM_HIPCHK(hipMemcpyAsync(hc.data(), d_centers, hc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BIEM_HIPCHK(hipStreamSynchronize(st));
  const double z0 = hc[d - 1] + 0.0;      // (-0.0 + 0.0 = 0.0; == also takes the two zeros as equal, and no NaN as equal to anything)
  for (int b = 0; b < B; ++b) if (!(hc[(size_t)b * d + d - 1] == z0)) return BIEM_OK;
  split = sm;
  return BIEM_OK;
}

// The symmetric factorisation of a chunk of c systems as a list of diagonal blocks of the one allocation: the whole matrix, or E then O
// of the split form.  One stream and one workspace: the blocks run one after the other.  Each block's growth slots are preset first -
// max |A~| >= 1 (its diagonal is exactly 1), so 1 is a valid, conservative reference (a system is handed to the pivoted LU when
// max |u_ii u_ic| exceeds GROWTH_MAX = 200 x this lower bound); saves a pass over the matrix.  Two blocks: the first one's codes are
// the caller's array, the second one's stand beside them and are merged (the first nonzero wins, in the split layout's row numbers).
struct SymBlock { size_t view; int n_pad, n_active; int* info; };       // view: the block's first entry, in doubles from A
static int factor_sym_blocks(int c, int nrhs, double* A, long long lda, long long sys_stride, const SymBlock* blocks, int n_blocks, void* Pw,
                             hipStream_t st) {
  for (int i = 0; i < n_blocks; ++i) {
    const SymBlock& b = blocks[i];
    int rc = lu_growth_init(Pw, c, b.n_pad, 1.0, st);
    if (rc) return rc;
    rc = launch_sym_factor_solve(c, b.n_pad, nrhs, A + b.view, lda, sys_stride, b.info, Pw, lu_workspace_bytes(c, b.n_pad, nrhs), st, true, b.n_active);
    if (rc) return rc;
  }
  return n_blocks == 2 ? launch_split_info_merge(c, blocks[0].n_pad, blocks[1].n_pad, blocks[0].info, blocks[1].info, st) : BIEM_OK;
}

static int solve_impl(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
               const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream,
               bool symmetric, const DegreeBc* bcn = nullptr) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii");
  if (bcn) { NEED(bcn->alpha_n, "d_alpha_n"); NEED(bcn->beta_n, "d_beta_n"); }
  else { NEED(d_alpha, "d_alpha"); NEED(d_beta, "d_beta"); NEED(d_g, "d_g"); }
  NEED(d_density, "d_density"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  if (nb <= 0 || B <= 0) return BIEM_OK;
  if (nrhs < 1) { set_error("biem_solve: nrhs < 1"); return BIEM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const int H = plan->H, d = plan->d, Q = plan->Q;
  SplitMap flat = SplitMap();              // (off: the pivoted LU has no split form)
  if (symmetric) {
    g_last_split[0] = g_last_split[1] = 0;
    if (const int rc = flat_layout_split(plan, B, nrhs, d_centers, geom_batched, st, flat)) return rc;
  }
  const bool split = flat.on();
  SolveLayout L = make_layout(plan, nb, B, nrhs, chunk, split);
  if (work_bytes < L.total) { set_error("biem_solve: workspace too small (%zu < %zu)", work_bytes, L.total); return BIEM_ERR_ARG; }
  const SplitMap& sm = L.split;
  if (split) { g_last_split[0] = sm.npE; g_last_split[1] = sm.npO; }
  char* w = (char*)d_work;
  double* tab = (double*)(w + L.off_tab);
  double* A = (double*)(w + L.off_A);
  void* T = w + L.off_T;
  void* Pw = w + L.off_P;
  int* ipiv = (int*)(w + L.off_ipiv);
  int* info_O = (int*)(w + L.off_info2);
  int rc = bcn ? launch_ball_tables_n(plan, nb, B, d_k, d_eta, d_radii, geom_batched, bcn->alpha_n, bcn->beta_n, ab_batched, tab, st)
               : launch_ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, tab, st);
  if (rc) return rc;
  for (int s0 = 0; s0 < nb; s0 += L.chunk) {
    const int c = (nb - s0 < L.chunk) ? nb - s0 : L.chunk;
    const double* ks = d_k + 2 * (size_t)s0;   // complex128 per system
    const double* cen = d_centers + (geom_batched ? (size_t)s0 * B * d : 0);
    const double* tb = tab + (size_t)s0 * B * 3 * plan->n_end * 2;
    // right-hand side into column n_pad of the augmented matrix (padded rows: zero via fill_pad? -> set explicitly below)
    // small systems are solved in one LDS-resident launch that never reads the padding rows / columns: they are not written then
    const bool small = symmetric && sym_small_path(L.N, nrhs);
    // blocks of ball pairs with the same displacement and the same (radius, alpha, beta) on either side are contracted once
    const FillDedupe dd = {d_radii, d_alpha, d_beta};
    if (split)
      // E's right-hand-side columns lie inside the O rows' matrix columns: they are cleared for all rows BEFORE the fill writes O
      launch_clear_cols(st, A + (size_t)sm.npE * 2, L.lda, L.lda - L.n_pad, (long long)L.n_pad * c);
    if (symmetric)
      // (degree-dependent coefficients: every pair on its own - the classes are keyed on one (alpha, beta) per ball)
      rc = launch_fill_sym(plan, c, B, ks, cen, geom_batched, tb, A, L.lda, L.sys_stride, L.n_pad, T, fill_workspace_bytes(plan, c, B), st, small,
                           (!geom_batched && !ab_batched && !bcn) ? &dd : nullptr, sm);
    else
      rc = launch_fill(plan, c, B, ks, cen, geom_batched, tb, BIEM_FILL_EQUILIBRATED, A, L.lda, L.sys_stride, L.n_pad, T,
                       fill_workspace_bytes(plan, c, B), st);
    if (rc) return rc;
    if (!small)
      launch_clear_cols(st, A + (size_t)L.n_pad * 2, L.lda, L.lda - L.n_pad, (long long)L.n_pad * c);
    const size_t g0 = (size_t)s0 * nrhs * B * Q * 2;
    if (bcn) {
      const size_t ab0 = ab_batched ? (size_t)s0 * B * plan->n_end * 2 : 0;
      rc = launch_rhs_project_n(plan, c, B, nrhs, bcn->gu ? bcn->gu + g0 : nullptr, bcn->gdn ? bcn->gdn + g0 : nullptr, bcn->alpha_n + ab0,
                                bcn->beta_n + ab0, ab_batched, A + (size_t)L.n_pad * 2, L.sys_stride, L.lda, 1, st, symmetric, sm);
    } else {
      rc = launch_rhs_project(plan, c, B, nrhs, d_g + g0, A + (size_t)L.n_pad * 2, L.sys_stride, L.lda, 1, st, symmetric, sm);
    }
    if (rc) return rc;
    if (symmetric) {
      rc = launch_sym_rhs(plan, c, B, nrhs, L.n_pad, tb, A, L.lda, L.sys_stride, false, st, sm);
      if (rc) return rc;
      // the existing factorisation on the whole matrix, or on two views of the one allocation, E then O
      const SymBlock whole[1] = {{0, L.n_pad, L.N, d_info + s0}};
      const SymBlock halves[2] = {{0, sm.npE, B * sm.U, d_info + s0},
                                  {2 * ((size_t)sm.npE * L.lda + sm.npE), sm.npO, B * (H - sm.U), info_O}};
      rc = factor_sym_blocks(c, nrhs, A, L.lda, L.sys_stride, split ? halves : whole, split ? 2 : 1, Pw, st);
    } else
      rc = launch_lu_factor_solve(c, L.n_pad, nrhs, A, L.lda, L.sys_stride, ipiv, d_info + s0, Pw, lu_workspace_bytes(c, L.n_pad, nrhs), st,
                                  /*keep_multipliers=*/false, false, false);   // the fused path only needs the solution
    if (rc) return rc;
    if (symmetric && bcn) {
      // a degree with gj = 0 (a ball that does not scatter it) has no symmetric scaling: rejected here whatever the factorisation reported
      rc = launch_flag_unscalable(plan, c, B, tb, d_info + s0, -(L.n_pad + 2), st);
      if (rc) return rc;
    }
    if (symmetric) {
      rc = launch_sym_rhs(plan, c, B, nrhs, L.n_pad, tb, A, L.lda, L.sys_stride, true, st, sm);
      if (rc) return rc;
    }
    rc = launch_density(plan, c, B, nrhs, A + (size_t)L.n_pad * 2, L.sys_stride, L.lda, 1, tb, d_density + (size_t)s0 * nrhs * B * H * 2, st, symmetric, sm);
    if (rc) return rc;
  }
  return BIEM_OK;
}

int biem_solve(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
               const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream) {
  return solve_impl(plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_g, d_density, d_info,
                    chunk, d_work, work_bytes, stream, false);
}

int biem_solve_ldlt(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                    const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
                    const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream) {
  return solve_impl(plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_g, d_density, d_info,
                    chunk, d_work, work_bytes, stream, true);
}

int biem_last_solve_split(int* npE, int* npO) {
  if (npE) *npE = g_last_split[0];
  if (npO) *npO = g_last_split[1];
  return BIEM_OK;
}

int biem_solve_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                 const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                 const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                 void* stream) {
  const DegreeBc bcn = {d_alpha_n, d_beta_n, d_gu, d_gdn};
  return solve_impl(plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, nullptr, nullptr, ab_batched, nullptr, d_density, d_info,
                    chunk, d_work, work_bytes, stream, false, &bcn);
}

int biem_solve_ldlt_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                      const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                      void* stream) {
  const DegreeBc bcn = {d_alpha_n, d_beta_n, d_gu, d_gdn};
  return solve_impl(plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, nullptr, nullptr, ab_batched, nullptr, d_density, d_info,
                    chunk, d_work, work_bytes, stream, true, &bcn);
}

// ---- factor now, solve later: the symmetric path split at the factorisation -------------------------------------------------
int biem_sym_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_info, void* d_work, size_t work_bytes,
                    void* stream) {
  NEED(d_A, "d_A"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  return launch_sym_factor_solve(nb, n_pad, 0, d_A, lda, sys_stride, d_info, d_work, work_bytes, (hipStream_t)stream, false);
}

int biem_sym_solve(int nb, int n_pad, int nrhs, const double* d_U, long long lda, long long sys_stride, double* d_B, long long ldb,
                   long long b_stride, void* stream) {
  NEED(d_U, "d_U"); NEED(d_B, "d_B");
  return launch_sym_solve(nb, n_pad, nrhs, d_U, lda, sys_stride, d_B, ldb, b_stride, (hipStream_t)stream);
}

namespace {
struct FactorLayout {
  int N, n_pad, chunk;
  size_t off_T, off_P, total;
};
FactorLayout make_factor_layout(const biem_plan* p, int nb, int B, int chunk) {
  FactorLayout L;
  L.N = B * p->H;
  L.n_pad = lu_npad(L.N);
  if (chunk <= 0) {
    // fill and factorisation workspace of ~4 GiB at most: the factors themselves are the caller's, all of them resident
    const size_t per = fill_workspace_bytes(p, 1, B) + lu_workspace_bytes(1, L.n_pad, 0);
    const size_t fit = ((size_t)4 << 30) / (per ? per : 1);
    chunk = (int)(fit < 1 ? 1 : (fit > (size_t)nb ? (size_t)nb : fit));
  }
  if (chunk > nb) chunk = nb;
  if (chunk < 1) chunk = 1;
  L.chunk = chunk;
  size_t o = 0;
  L.off_T = o; o = align256(o + fill_workspace_bytes(p, chunk, B));
  L.off_P = o; o = align256(o + lu_workspace_bytes(chunk, L.n_pad, 0));
  L.total = o;
  return L;
}
inline long long solve_ldx(int nrhs) { return ((long long)nrhs + 7) / 8 * 8; }   // rows of the right-hand sides 128-byte aligned
}  // namespace

size_t biem_factor_workspace_bytes(const biem_plan* plan, int nb, int B, int chunk) {
  if (!plan || nb <= 0 || B <= 0) return 0;
  return make_factor_layout(plan, nb, B, chunk).total;
}

static int factor_impl(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_F,
                       long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes,
                       void* stream, bool per_degree, const char* who) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_centers, "d_centers"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, d_alpha, "d_alpha"); NEED_AS(who, d_beta, "d_beta"); NEED_AS(who, d_F, "d_F"); NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_info, "d_info"); NEED_AS(who, d_work, "d_work");
  if (nb < 0 || nb > 65535 || B < 0) { set_error("%s: 0 .. 65535 systems per call and B >= 0 (got nb=%d, B=%d)", who, nb, B); return BIEM_ERR_ARG; }
  if (nb == 0 || B == 0) return BIEM_OK;
  const FactorLayout L = make_factor_layout(plan, nb, B, chunk);
  if (lda < L.n_pad || sys_stride < (long long)L.n_pad * lda) {
    set_error("%s: lda=%lld < n_pad=%d or sys_stride=%lld < n_pad * lda", who, lda, L.n_pad, sys_stride);
    return BIEM_ERR_ARG;
  }
  if (work_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, L.total); return BIEM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)d_work;
  void* T = w + L.off_T;
  void* Pw = w + L.off_P;
  const int d = plan->d;
  int rc = per_degree ? launch_ball_tables_n(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, st)
                      : launch_ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, st);
  if (rc) return rc;
  const FillDedupe dd = {d_radii, d_alpha, d_beta};
  for (int s0 = 0; s0 < nb; s0 += L.chunk) {
    const int c = (nb - s0 < L.chunk) ? nb - s0 : L.chunk;
    const double* ks = d_k + 2 * (size_t)s0;
    const double* cen = d_centers + (geom_batched ? (size_t)s0 * B * d : 0);
    const double* tb = d_tab + (size_t)s0 * B * 3 * plan->n_end * 2;
    double* A = d_F + 2 * (size_t)s0 * sys_stride;
    // identity padding written (no_padding = false) even where the one-launch path factors the active rows only: the solve runs
    // over all n_pad rows and finds U = I there
    rc = launch_fill_sym(plan, c, B, ks, cen, geom_batched, tb, A, lda, sys_stride, L.n_pad, T, fill_workspace_bytes(plan, c, B), st, false,
                         (!geom_batched && !ab_batched && !per_degree) ? &dd : nullptr);
    if (rc) return rc;
    const SymBlock whole[1] = {{0, L.n_pad, L.N, d_info + s0}};      // (growth preset as in biem_solve_ldlt)
    rc = factor_sym_blocks(c, 0, A, lda, sys_stride, whole, 1, Pw, st);
    if (rc) return rc;
    if (per_degree) {     // a degree with gj = 0 has no symmetric scaling (biem_solve_ldlt_n)
      rc = launch_flag_unscalable(plan, c, B, tb, d_info + s0, -(L.n_pad + 2), st);
      if (rc) return rc;
    }
  }
  return BIEM_OK;
}

int biem_factor_ldlt(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                     const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_F,
                     long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes,
                     void* stream) {
  return factor_impl(plan, nb, B, d_k, d_eta, d_centers, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_F, lda, sys_stride, d_tab,
                     d_info, chunk, d_work, work_bytes, stream, false, "biem_factor_ldlt");
}

int biem_factor_ldlt_n(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                       double* d_F, long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work,
                       size_t work_bytes, void* stream) {
  return factor_impl(plan, nb, B, d_k, d_eta, d_centers, d_radii, geom_batched, d_alpha_n, d_beta_n, ab_batched, d_F, lda, sys_stride, d_tab,
                     d_info, chunk, d_work, work_bytes, stream, true, "biem_factor_ldlt_n");
}

size_t biem_solve_factored_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs) {
  if (!plan || nb <= 0 || B <= 0 || nrhs <= 0) return 0;
  return (size_t)nb * lu_npad(B * plan->H) * solve_ldx(nrhs) * sizeof(cplx);
}

static int solve_factored_impl(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                               const double* d_tab, const double* d_g, double* d_density, void* d_work, size_t work_bytes, void* stream,
                               const DegreeBc* bcn, int ab_batched, const char* who) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_F, "d_F"); NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_work, "d_work");
  if (bcn) { NEED_AS(who, bcn->alpha_n, "d_alpha_n"); NEED_AS(who, bcn->beta_n, "d_beta_n"); }
  else NEED_AS(who, d_g, "d_g");
  if (nb < 0 || nb > 65535 || nrhs < 0 || nrhs > 65535 || B < 0) {
    set_error("%s: 0 .. 65535 systems / right-hand sides per call and B >= 0 (got nb=%d, nrhs=%d, B=%d)", who, nb, nrhs, B);
    return BIEM_ERR_ARG;
  }
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  const int n_pad = lu_npad(B * plan->H);
  if (lda < n_pad || sys_stride < (long long)n_pad * lda) {
    set_error("%s: lda=%lld < n_pad=%d or sys_stride=%lld < n_pad * lda", who, lda, n_pad, sys_stride);
    return BIEM_ERR_ARG;
  }
  const size_t need = biem_solve_factored_workspace_bytes(plan, nb, B, nrhs);
  if (work_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, need); return BIEM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  // right-hand sides X[s][row][q] (row-major, ldx columns), rows in the slot order of the symmetric form; padding rows zero
  double* X = (double*)d_work;
  const long long ldx = solve_ldx(nrhs), xs = (long long)n_pad * ldx;
  double* Xaug = X - 2 * (size_t)n_pad;      // X seen as the augmented columns n_pad .. of a matrix with leading dimension ldx
  BIEM_HIPCHK(hipMemsetAsync(X, 0, need, st));
  int rc = bcn ? launch_rhs_project_n(plan, nb, B, nrhs, bcn->gu, bcn->gdn, bcn->alpha_n, bcn->beta_n, ab_batched, X, xs, ldx, 1, st, true)
               : launch_rhs_project(plan, nb, B, nrhs, d_g, X, xs, ldx, 1, st, true);
  if (rc) return rc;
  rc = launch_sym_rhs(plan, nb, B, nrhs, n_pad, d_tab, Xaug, ldx, xs, false, st);
  if (rc) return rc;
  rc = launch_sym_solve(nb, n_pad, nrhs, d_F, lda, sys_stride, X, ldx, xs, st);
  if (rc) return rc;
  rc = launch_sym_rhs(plan, nb, B, nrhs, n_pad, d_tab, Xaug, ldx, xs, true, st);
  if (rc) return rc;
  return launch_density(plan, nb, B, nrhs, X, xs, ldx, 1, d_tab, d_density, st, true);
}

int biem_solve_factored(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                        const double* d_tab, const double* d_g, double* d_density, void* d_work, size_t work_bytes, void* stream) {
  return solve_factored_impl(plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, d_g, d_density, d_work, work_bytes, stream, nullptr, 0,
                             "biem_solve_factored");
}

int biem_solve_factored_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                          const double* d_tab, const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_gu,
                          const double* d_gdn, double* d_density, void* d_work, size_t work_bytes, void* stream) {
  const DegreeBc bcn = {d_alpha_n, d_beta_n, d_gu, d_gdn};
  return solve_factored_impl(plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, nullptr, d_density, d_work, work_bytes, stream, &bcn, ab_batched,
                             "biem_solve_factored_n");
}

// ---- extinction and absorbed power (kernels_power.hip) ----
static int power_impl(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
                      int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab,
                      const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream, bool per_degree,
                      const char* who) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, d_alpha, per_degree ? "d_alpha_n" : "d_alpha"); NEED_AS(who, d_beta, per_degree ? "d_beta_n" : "d_beta");
  NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_pu, "d_pu"); NEED_AS(who, d_pv, "d_pv");
  NEED_AS(who, d_out, "d_out");
  if (nb < 0 || nb > 65535 || nrhs < 0 || nrhs > 65535 || B < 0) {
    set_error("%s: 0 .. 65535 systems / right-hand sides per call and B >= 0 (got nb=%d, nrhs=%d, B=%d)", who, nb, nrhs, B);
    return BIEM_ERR_ARG;
  }
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  hipStream_t st = (hipStream_t)stream;
  // the powers are defined for a lossless exterior: the wavenumbers come to the host for that test (one small copy, one wait)
  std::vector<double> hk((size_t)nb * 2);
  BIEM_HIPCHK(hipMemcpyAsync(hk.data(), d_k, hk.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BIEM_HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < nb; ++s)
    if (hk[2 * (size_t)s + 1] != 0.0) { set_error("%s: system %d has Im k = %g; the powers need a real wavenumber", who, s, hk[2 * (size_t)s + 1]); return BIEM_ERR_ARG; }
  return launch_power(plan, nb, B, nrhs, d_k, d_radii, geom_batched, d_alpha, d_beta, ab_batched, per_degree, d_tab, d_density, d_pu,
                      d_pv, d_out, st);
}

int biem_power(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
               int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab,
               const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream) {
  return power_impl(plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, d_density, d_pu, d_pv, d_out,
                    stream, false, "biem_power");
}

int biem_power_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
                 int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_tab,
                 const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream) {
  return power_impl(plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, d_alpha_n, d_beta_n, ab_batched, d_tab, d_density, d_pu, d_pv,
                    d_out, stream, true, "biem_power_n");
}

// ---- radiation force (kernels_force.hip) ----
static int force_impl(biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
                      int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab,
                      const double* d_density, double* d_out, void* stream, bool per_degree, const char* who) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, d_alpha, per_degree ? "d_alpha_n" : "d_alpha"); NEED_AS(who, d_beta, per_degree ? "d_beta_n" : "d_beta");
  NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_out, "d_out");
  if (nb < 0 || nb > 65535 || nrhs < 0 || nrhs > 65535 || B < 0) {
    set_error("%s: 0 .. 65535 systems / right-hand sides per call and B >= 0 (got nb=%d, nrhs=%d, B=%d)", who, nb, nrhs, B);
    return BIEM_ERR_ARG;
  }
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  hipStream_t st = (hipStream_t)stream;
  // the force is defined for a lossless exterior: the wavenumbers come to the host for that test (one small copy, one wait)
  std::vector<double> hk((size_t)nb * 2);
  BIEM_HIPCHK(hipMemcpyAsync(hk.data(), d_k, hk.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BIEM_HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < nb; ++s)
    if (hk[2 * (size_t)s + 1] != 0.0) { set_error("%s: system %d has Im k = %g; the force needs a real wavenumber", who, s, hk[2 * (size_t)s + 1]); return BIEM_ERR_ARG; }
  int rc = BIEM_OK;
  try {
    rc = plan_build_force(plan);             // (the first call of this plan: builds and uploads the coupling table)
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory building the force coupling table for n_end=%d", who, plan->n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) return rc;
  return launch_force(plan, nb, B, nrhs, d_k, d_radii, geom_batched, d_alpha, d_beta, ab_batched, per_degree, d_tab, d_density, d_out, st);
}

int biem_force(biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
               const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab, const double* d_density, double* d_out,
               void* stream) {
  return force_impl(plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, d_density, d_out, stream,
                    false, "biem_force");
}

int biem_force_n(biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                 const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_tab, const double* d_density,
                 double* d_out, void* stream) {
  return force_impl(plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, d_alpha_n, d_beta_n, ab_batched, d_tab, d_density, d_out, stream,
                    true, "biem_force_n");
}

int biem_profile_begin(void) {
  Profiler& p = profiler();
  for (auto& r : p.recs) { p.pool.push_back(r.a); p.pool.push_back(r.b); }
  p.recs.clear();
  for (int i = 0; i < PK_COUNT; ++i) { p.work[i] = 0.0; p.launches[i] = 0; }
  p.on = true;
  return BIEM_OK;
}

int biem_profile_end(double* ms, double* work, long long* launches) {
  Profiler& p = profiler();
  p.on = false;
  double acc[PK_COUNT] = {0};
  for (auto& r : p.recs) {
    (void)hipEventSynchronize(r.b);
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) acc[r.cls] += t;
    p.pool.push_back(r.a); p.pool.push_back(r.b);
  }
  p.recs.clear();
  for (int i = 0; i < PK_COUNT; ++i) {
    if (ms) ms[i] = acc[i];
    if (work) work[i] = p.work[i];
    if (launches) launches[i] = p.launches[i];
  }
  return BIEM_OK;
}

int biem_bench_mfma_f64(int iters, double* tflops, void* stream) {
  NEED(tflops, "tflops");
  return bench_mfma_f64(iters, tflops, (hipStream_t)stream);
}
int biem_bench_mfma_f64_ex(int iters, int variant, double* tflops, void* stream) {
  NEED(tflops, "tflops");
  if (iters <= 0 || (variant != 0 && variant != 1)) { set_error("biem_bench_mfma_f64_ex: iters > 0, variant 0 or 1"); return BIEM_ERR_ARG; }
  return bench_mfma_f64(iters, tflops, (hipStream_t)stream, variant);
}

}  // extern "C"
