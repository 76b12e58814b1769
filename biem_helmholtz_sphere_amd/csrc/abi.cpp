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

#define NEED(p, what) NEED_AS(__func__, p, what)
#define NEED_DEV(pl) NEED_DEV_AS(__func__, pl)

// the first call of a plan that needs it builds and uploads the force coupling table
static int build_force_table(const char* who, biem_plan* plan) {
  try {
    return plan_build_force(plan);
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory building the force coupling table for n_end=%d", who, plan->n_end);
    return BIEM_ERR_ALLOC;
  }
}

// BIEM_LU_DISCARD_FACTORS=1 (tests): solve exactly as the fused path does, without storing the multipliers back
static bool keep_lu_factors() { const char* e = getenv("BIEM_LU_DISCARD_FACTORS"); return !(e && e[0] == '1'); }

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

int biem_plan_entry_terms(int tree, int n_end, int h_col, int h_row, int capacity, int* n_terms, double* h_coef, int* h_tidx) {
  NEED(n_terms, "n_terms");
  std::vector<double> coef;
  std::vector<int> tidx;
  int rc = BIEM_OK;
  try {
    rc = plan_entry_terms(tree, n_end, h_col, h_row, coef, tidx);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory building the integral tables for n_end=%d", n_end);
    rc = BIEM_ERR_ALLOC;
  }
  if (rc != BIEM_OK) return rc;
  *n_terms = (int)coef.size();
  if ((int)coef.size() > capacity) { set_error("biem_plan_entry_terms: the entry has %d terms, capacity %d", (int)coef.size(), capacity); return BIEM_ERR_ARG; }
  if (h_coef) memcpy(h_coef, coef.data(), coef.size() * sizeof(double));
  if (h_tidx) memcpy(h_tidx, tidx.data(), tidx.size() * sizeof(int));
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
  return ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false}, d_tab, (hipStream_t)stream);
}

int biem_rhs_project(const biem_plan* plan, int nb, int B, int nrhs, const double* d_g, double* d_f, long long sys_stride,
                     long long elem_stride, long long rhs_stride, void* stream) {
  NEED_DEV(plan); NEED(d_g, "d_g"); NEED(d_f, "d_f");
  return RhsSource::samples(d_g).launch(plan, nb, B, nrhs, {nullptr, nullptr, 0, false}, nullptr, d_f, sys_stride, elem_stride, rhs_stride,
                                        (hipStream_t)stream);
}

int biem_ball_tables_n(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_tab, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_radii, "d_radii"); NEED(d_alpha_n, "d_alpha_n"); NEED(d_beta_n, "d_beta_n"); NEED(d_tab, "d_tab");
  return ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true}, d_tab, (hipStream_t)stream);
}

int biem_rhs_project_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn, const double* d_alpha_n,
                       const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride, long long elem_stride,
                       long long rhs_stride, void* stream) {
  NEED_DEV(plan); NEED(d_alpha_n, "d_alpha_n"); NEED(d_beta_n, "d_beta_n"); NEED(d_f, "d_f");
  return RhsSource::samples_n(d_gu, d_gdn).launch(plan, nb, B, nrhs, {d_alpha_n, d_beta_n, ab_batched, true}, nullptr, d_f, sys_stride,
                                                  elem_stride, rhs_stride, (hipStream_t)stream);
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
  return launch_lu_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream, keep_lu_factors());
}

int biem_ldlt_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info,
                           void* d_work, size_t work_bytes, void* stream) {
  NEED(d_A, "d_A"); NEED(d_ipiv, "d_ipiv"); NEED(d_info, "d_info"); NEED(d_work, "d_work");
  return launch_lu_factor_solve(nb, n_pad, nrhs, d_A, lda, sys_stride, d_ipiv, d_info, d_work, work_bytes, (hipStream_t)stream, keep_lu_factors(),
                                /*symmetric=*/true);
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
int biem_gemm_narrow_frags(int nb, int n_pad, int n_active, int J) { return sym_gemm_narrow(nb, n_pad, n_active, J); }

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
  if (const int rc = build_force_table(__func__, plan)) return rc;
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

// ---- whole path (solve_path.cpp) ----
size_t biem_solve_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int chunk) {
  return (!plan || nb <= 0 || B <= 0 || nrhs < 1) ? 0 : solve_workspace_bytes(plan, nb, B, nrhs, chunk);
}

int biem_solve(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
               const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream) {
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false},
                    RhsSource::samples(d_g), d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, false);
}

int biem_solve_ldlt(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                    const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
                    const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream) {
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false},
                    RhsSource::samples(d_g), d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, true);
}

int biem_last_solve_split(int* npE, int* npO) { last_solve_split(npE, npO); return BIEM_OK; }

int biem_solve_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                 const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                 const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                 void* stream) {
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true},
                    RhsSource::samples_n(d_gu, d_gdn), d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, false);
}

int biem_solve_ldlt_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                      const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                      void* stream) {
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true},
                    RhsSource::samples_n(d_gu, d_gdn), d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, true);
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

size_t biem_factor_workspace_bytes(const biem_plan* plan, int nb, int B, int chunk) {
  return (!plan || nb <= 0 || B <= 0) ? 0 : factor_workspace_bytes(plan, nb, B, chunk);
}

int biem_factor_ldlt(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                     const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_F,
                     long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes,
                     void* stream) {
  return factor_path(__func__, plan, nb, B, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false}, d_F, lda,
                     sys_stride, d_tab, d_info, chunk, d_work, work_bytes, (hipStream_t)stream);
}

int biem_factor_ldlt_n(const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                       double* d_F, long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work,
                       size_t work_bytes, void* stream) {
  return factor_path(__func__, plan, nb, B, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true}, d_F, lda,
                     sys_stride, d_tab, d_info, chunk, d_work, work_bytes, (hipStream_t)stream);
}

size_t biem_solve_factored_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs) {
  return (!plan || nb <= 0 || B <= 0 || nrhs <= 0) ? 0 : solve_factored_workspace_bytes(plan, nb, B, nrhs);
}

int biem_solve_factored(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                        const double* d_tab, const double* d_g, double* d_density, void* d_work, size_t work_bytes, void* stream) {
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {nullptr, nullptr, 0, false}, RhsSource::samples(d_g),
                             d_density, d_work, work_bytes, (hipStream_t)stream);
}

int biem_solve_factored_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                          const double* d_tab, const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_gu,
                          const double* d_gdn, double* d_density, void* d_work, size_t work_bytes, void* stream) {
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha_n, d_beta_n, ab_batched, true},
                             RhsSource::samples_n(d_gu, d_gdn), d_density, d_work, work_bytes, (hipStream_t)stream);
}

// ---- right-hand sides in closed form on their own: the source's limits, its workspace, then its launcher (natural order, unsplit) ----
static int closed_form_rhs(const char* who, RhsSource src, const biem_plan* plan, int nb, int B, int nrhs, const double* d_tab, double* d_f,
                           long long sys_stride, long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, hipStream_t st) {
  if (const int rc = src.check(who, plan, nb, nrhs)) return rc;
  const size_t need = src.work_bytes(plan, nb, B, nrhs);
  if (work_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, need); return BIEM_ERR_ARG; }
  src.work = d_work;
  return src.launch(plan, nb, B, nrhs, {nullptr, nullptr, 0, false}, d_tab, d_f, sys_stride, elem_stride, rhs_stride, st);
}

// ---- plane-wave incidence in closed form (kernels_rhs_pw.hip): the third source of right-hand sides ----
size_t biem_rhs_plane_wave_workspace_bytes(const biem_plan* plan, int nb, int nrhs, int dirs_batched) {
  return plan ? rhs_plane_wave_workspace_bytes(plan, nb, nrhs, dirs_batched) : 0;
}

int biem_rhs_plane_wave(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                        const double* d_tab, const double* d_dirs, int dirs_batched, double* d_f, long long sys_stride,
                        long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_dirs, "d_dirs"); NEED(d_f, "d_f"); NEED(d_work, "d_work");
  return closed_form_rhs(__func__, RhsSource::plane_waves(d_dirs, dirs_batched, d_k, d_centers, geom_batched), plan, nb, B, nrhs, d_tab, d_f,
                         sys_stride, elem_stride, rhs_stride, d_work, work_bytes, (hipStream_t)stream);
}

int biem_solve_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_dirs, int dirs_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream) {
  NEED(d_dirs, "d_dirs");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::plane_waves(d_dirs, dirs_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work,
                    work_bytes, (hipStream_t)stream, false);
}

int biem_solve_ldlt_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                       const double* d_dirs, int dirs_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                       void* stream) {
  NEED(d_dirs, "d_dirs");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::plane_waves(d_dirs, dirs_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work,
                    work_bytes, (hipStream_t)stream, true);
}

int biem_solve_factored_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k, const double* d_centers, int geom_batched, const double* d_alpha,
                           const double* d_beta, int ab_batched, int per_degree, const double* d_dirs, int dirs_batched,
                           double* d_density, void* d_work, size_t work_bytes, void* stream) {
  NEED(d_dirs, "d_dirs");
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha, d_beta, ab_batched, per_degree != 0},
                             RhsSource::plane_waves(d_dirs, dirs_batched, d_k, d_centers, geom_batched), d_density, d_work,
                             work_bytes, (hipStream_t)stream);
}

// ---- point-source incidence in closed form (kernels_rhs_ps.hip): the fourth source of right-hand sides ----
size_t biem_rhs_point_source_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int src_batched, int geom_batched) {
  return plan ? rhs_point_source_workspace_bytes(plan, nb, B, nrhs, src_batched, geom_batched) : 0;
}

int biem_rhs_point_source(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                          const double* d_tab, const double* d_src, int src_batched, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_src, "d_src"); NEED(d_f, "d_f"); NEED(d_work, "d_work");
  return closed_form_rhs(__func__, RhsSource::point_sources(d_src, src_batched, d_k, d_centers, geom_batched), plan, nb, B, nrhs, d_tab, d_f,
                         sys_stride, elem_stride, rhs_stride, d_work, work_bytes, (hipStream_t)stream);
}

int biem_solve_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_src, int src_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream) {
  NEED(d_src, "d_src");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::point_sources(d_src, src_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work, work_bytes,
                    (hipStream_t)stream, false);
}

int biem_solve_ldlt_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                       const double* d_src, int src_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                       void* stream) {
  NEED(d_src, "d_src");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::point_sources(d_src, src_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work, work_bytes,
                    (hipStream_t)stream, true);
}

int biem_solve_factored_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k, const double* d_centers, int geom_batched, const double* d_alpha,
                           const double* d_beta, int ab_batched, int per_degree, const double* d_src, int src_batched,
                           double* d_density, void* d_work, size_t work_bytes, void* stream) {
  NEED(d_src, "d_src");
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha, d_beta, ab_batched, per_degree != 0},
                             RhsSource::point_sources(d_src, src_batched, d_k, d_centers, geom_batched), d_density, d_work, work_bytes,
                             (hipStream_t)stream);
}

// ---- multipole incidence in closed form (kernels_rhs_ms.hip): the fifth source; the _ps entries with d_idx after src_batched ----
size_t biem_rhs_multipole_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int src_batched, int geom_batched) {
  return plan ? rhs_multipole_workspace_bytes(plan, nb, B, nrhs, src_batched, geom_batched) : 0;
}

int biem_rhs_multipole(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                          const double* d_tab, const double* d_src, int src_batched, const int* d_idx, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_src, "d_src"); NEED(d_idx, "d_idx"); NEED(d_f, "d_f"); NEED(d_work, "d_work");
  return closed_form_rhs(__func__, RhsSource::multipole_sources(d_src, d_idx, src_batched, d_k, d_centers, geom_batched), plan, nb, B, nrhs, d_tab, d_f,
                         sys_stride, elem_stride, rhs_stride, d_work, work_bytes, (hipStream_t)stream);
}

int biem_solve_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_src, int src_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream) {
  NEED(d_src, "d_src"); NEED(d_idx, "d_idx");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::multipole_sources(d_src, d_idx, src_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work, work_bytes,
                    (hipStream_t)stream, false);
}

int biem_solve_ldlt_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                       const double* d_src, int src_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                       void* stream) {
  NEED(d_src, "d_src"); NEED(d_idx, "d_idx");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::multipole_sources(d_src, d_idx, src_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work, work_bytes,
                    (hipStream_t)stream, true);
}

int biem_solve_factored_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k, const double* d_centers, int geom_batched, const double* d_alpha,
                           const double* d_beta, int ab_batched, int per_degree, const double* d_src, int src_batched, const int* d_idx,
                           double* d_density, void* d_work, size_t work_bytes, void* stream) {
  NEED(d_src, "d_src"); NEED(d_idx, "d_idx");
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha, d_beta, ab_batched, per_degree != 0},
                             RhsSource::multipole_sources(d_src, d_idx, src_batched, d_k, d_centers, geom_batched), d_density, d_work, work_bytes,
                             (hipStream_t)stream);
}

// ---- regular-wave incidence in closed form (kernels_rhs_ms.hip, REG): the sixth source; the _ms entries with origins for sources ----
size_t biem_rhs_regular_wave_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int origin_batched, int geom_batched) {
  return plan ? rhs_multipole_workspace_bytes(plan, nb, B, nrhs, origin_batched, geom_batched) : 0;
}

int biem_rhs_regular_wave(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                          const double* d_tab, const double* d_origin, int origin_batched, const int* d_idx, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_origin, "d_origin"); NEED(d_idx, "d_idx"); NEED(d_f, "d_f"); NEED(d_work, "d_work");
  return closed_form_rhs(__func__, RhsSource::regular_waves(d_origin, d_idx, origin_batched, d_k, d_centers, geom_batched), plan, nb, B, nrhs, d_tab,
                         d_f, sys_stride, elem_stride, rhs_stride, d_work, work_bytes, (hipStream_t)stream);
}

int biem_solve_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_origin, int origin_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work,
                  size_t work_bytes, void* stream) {
  NEED(d_origin, "d_origin"); NEED(d_idx, "d_idx");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::regular_waves(d_origin, d_idx, origin_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work,
                    work_bytes, (hipStream_t)stream, false);
}

int biem_solve_ldlt_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                       const double* d_origin, int origin_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work,
                       size_t work_bytes, void* stream) {
  NEED(d_origin, "d_origin"); NEED(d_idx, "d_idx");
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    RhsSource::regular_waves(d_origin, d_idx, origin_batched, d_k, d_centers, geom_batched), d_density, d_info, chunk, d_work,
                    work_bytes, (hipStream_t)stream, true);
}

int biem_solve_factored_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k, const double* d_centers, int geom_batched, const double* d_alpha,
                           const double* d_beta, int ab_batched, int per_degree, const double* d_origin, int origin_batched, const int* d_idx,
                           double* d_density, void* d_work, size_t work_bytes, void* stream) {
  NEED(d_origin, "d_origin"); NEED(d_idx, "d_idx");
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha, d_beta, ab_batched, per_degree != 0},
                             RhsSource::regular_waves(d_origin, d_idx, origin_batched, d_k, d_centers, geom_batched), d_density, d_work,
                             work_bytes, (hipStream_t)stream);
}

// ---- incident fields by their expansion coefficients (kernels_rhs_ex.hip): the seventh source; whole coefficient vectors against the
//      columns the _ms / _rw entries take one at a time ----
#define NEED_EX(who)                                                                                                                      \
  NEED_AS(who, d_origin, "d_origin"); NEED_AS(who, d_coef, "d_coef"); NEED_DEV_AS(who, list_plan);                                         \
  if (list_plan != plan) NEED_AS(who, d_map, "d_map")
#define EX_SOURCE RhsSource::expansion(regular != 0, d_origin, origin_batched, n_origin, d_coef, coef_batched, list_plan, d_map, n_in, d_k, d_centers, geom_batched)

size_t biem_rhs_expansion_workspace_bytes(const biem_plan* list_plan, int nb, int B, int n_origin) {
  return list_plan ? rhs_expansion_workspace_bytes(list_plan, nb, B, n_origin) : 0;
}

int biem_rhs_expansion(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                       const double* d_tab, const double* d_origin, int origin_batched, int n_origin, const double* d_coef, int coef_batched,
                       const biem_plan* list_plan, const int* d_map, int n_in, int regular, double* d_f, long long sys_stride,
                       long long elem_stride, long long rhs_stride, int stage, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_centers, "d_centers"); NEED(d_tab, "d_tab"); NEED(d_f, "d_f"); NEED(d_work, "d_work");
  NEED_EX(__func__);
  const RhsSource src = EX_SOURCE;
  if (const int rc = src.check(__func__, plan, nb, nrhs)) return rc;
  const size_t need = src.work_bytes(plan, nb, B, nrhs);
  if (work_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", __func__, work_bytes, need); return BIEM_ERR_ARG; }
  return launch_rhs_expansion(plan, list_plan, d_map, n_in, regular != 0, nb, B, nrhs, d_k, d_centers, geom_batched, d_tab, d_origin, origin_batched,
                              n_origin, d_coef, coef_batched, d_f, sys_stride, elem_stride, rhs_stride, (hipStream_t)stream, false, SplitMap(), stage,
                              d_work);
}

int biem_solve_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_origin, int origin_batched, int n_origin, const double* d_coef, int coef_batched, const biem_plan* list_plan,
                  const int* d_map, int n_in, int regular, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream) {
  NEED_EX(__func__);
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    EX_SOURCE, d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, false);
}

int biem_solve_ldlt_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                       const double* d_origin, int origin_batched, int n_origin, const double* d_coef, int coef_batched,
                       const biem_plan* list_plan, const int* d_map, int n_in, int regular, double* d_density, int* d_info, int chunk,
                       void* d_work, size_t work_bytes, void* stream) {
  NEED_EX(__func__);
  return solve_path(__func__, plan, nb, B, nrhs, d_k, d_eta, d_centers, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, per_degree != 0},
                    EX_SOURCE, d_density, d_info, chunk, d_work, work_bytes, (hipStream_t)stream, true);
}

int biem_solve_factored_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k, const double* d_centers, int geom_batched, const double* d_alpha,
                           const double* d_beta, int ab_batched, int per_degree, const double* d_origin, int origin_batched, int n_origin,
                           const double* d_coef, int coef_batched, const biem_plan* list_plan, const int* d_map, int n_in, int regular,
                           double* d_density, void* d_work, size_t work_bytes, void* stream) {
  NEED_EX(__func__);
  return solve_factored_path(__func__, plan, nb, B, nrhs, d_F, lda, sys_stride, d_tab, {d_alpha, d_beta, ab_batched, per_degree != 0}, EX_SOURCE,
                             d_density, d_work, work_bytes, (hipStream_t)stream);
}
#undef EX_SOURCE
#undef NEED_EX

// ---- outgoing coefficients of the whole cluster about an origin (kernels_cluster.hip) ----
size_t biem_cluster_coefficients_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs) {
  return plan ? cluster_coefficients_workspace_bytes(plan, nb, B, nrhs) : 0;
}

int biem_cluster_coefficients(const biem_plan* plan, int nb, int B, int nrhs, int n_src, const double* d_k, const double* d_eta,
                              const double* d_centers, const double* d_radii, int geom_batched, const double* d_origin, int origin_batched,
                              const double* d_density, double* d_out, int stage, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_eta, "d_eta"); NEED(d_centers, "d_centers"); NEED(d_radii, "d_radii"); NEED(d_origin, "d_origin");
  NEED(d_density, "d_density"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  return launch_cluster_coefficients(plan, nb, B, nrhs, n_src, d_k, d_eta, d_centers, d_radii, geom_batched, d_origin, origin_batched, d_density,
                                     d_out, stage, d_work, work_bytes, (hipStream_t)stream);
}

// the field of the source itself (kernels_ladder.hip): what .uin, utotal and the powers of a closed-form call evaluate
size_t biem_multipole_field_workspace_bytes(const biem_plan* plan, int nb) { return plan ? multipole_field_workspace_bytes(plan, nb) : 0; }

int biem_multipole_field(biem_plan* plan, int nb, int P, const double* d_k, const double* d_src, const int* d_idx, const double* d_points,
                         int flags, int grad, double* d_out, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_src, "d_src"); NEED(d_idx, "d_idx"); NEED(d_points, "d_points"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  if (grad) { if (const int rc = build_force_table(__func__, plan)) return rc; }
  return launch_multipole_field(__func__, plan, nb, P, d_k, d_src, d_idx, nullptr, d_points, flags, grad, d_out, d_work, work_bytes, (hipStream_t)stream);
}

int biem_expansion_field(biem_plan* plan, int nb, int P, const double* d_k, const double* d_origin, const double* d_coef, const double* d_points,
                         int flags, int grad, double* d_out, void* d_work, size_t work_bytes, void* stream) {
  NEED_DEV(plan); NEED(d_k, "d_k"); NEED(d_origin, "d_origin"); NEED(d_coef, "d_coef"); NEED(d_points, "d_points"); NEED(d_out, "d_out"); NEED(d_work, "d_work");
  if (grad) { if (const int rc = build_force_table(__func__, plan)) return rc; }
  return launch_multipole_field(__func__, plan, nb, P, d_k, d_origin, nullptr, d_coef, d_points, flags, grad, d_out, d_work, work_bytes, (hipStream_t)stream);
}

// ---- extinction and absorbed power (kernels_power.hip), radiation force (kernels_force.hip) ----
// both are defined for a lossless exterior: the wavenumbers come to the host for that test (one small copy, one wait)
static int require_real_k(const char* who, const char* what, const double* d_k, int nb, hipStream_t st) {
  std::vector<double> hk((size_t)nb * 2);
  BIEM_HIPCHK(hipMemcpyAsync(hk.data(), d_k, hk.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  BIEM_HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < nb; ++s)
    if (hk[2 * (size_t)s + 1] != 0.0) { set_error("%s: system %d has Im k = %g; the %s a real wavenumber", who, s, hk[2 * (size_t)s + 1], what); return BIEM_ERR_ARG; }
  return BIEM_OK;
}

static int power_impl(const char* who, const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta,
                      const double* d_radii, int geom_batched, const BoundaryCoef& bc, const double* d_tab, const double* d_density,
                      const double* d_pu, const double* d_pv, double* d_out, hipStream_t st) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, bc.alpha, bc.alpha_name()); NEED_AS(who, bc.beta, bc.beta_name());
  NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_pu, "d_pu"); NEED_AS(who, d_pv, "d_pv");
  NEED_AS(who, d_out, "d_out");
  if (const int rc = check_counts(who, nb, nrhs, B)) return rc;
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  if (const int rc = require_real_k(who, "powers need", d_k, nb, st)) return rc;
  return launch_power(plan, nb, B, nrhs, d_k, d_radii, geom_batched, bc.alpha, bc.beta, bc.batched, bc.per_degree, d_tab, d_density, d_pu,
                      d_pv, d_out, st);
}

int biem_power(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
               int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab,
               const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream) {
  return power_impl(__func__, plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false}, d_tab, d_density,
                    d_pu, d_pv, d_out, (hipStream_t)stream);
}

int biem_power_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
                 int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_tab,
                 const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream) {
  return power_impl(__func__, plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true}, d_tab, d_density,
                    d_pu, d_pv, d_out, (hipStream_t)stream);
}

static int force_impl(const char* who, biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii,
                      int geom_batched, const BoundaryCoef& bc, const double* d_tab, const double* d_density, double* d_out, hipStream_t st) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, bc.alpha, bc.alpha_name()); NEED_AS(who, bc.beta, bc.beta_name());
  NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_out, "d_out");
  if (const int rc = check_counts(who, nb, nrhs, B)) return rc;
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  if (const int rc = require_real_k(who, "force needs", d_k, nb, st)) return rc;
  if (const int rc = build_force_table(who, plan)) return rc;
  return launch_force(plan, nb, B, nrhs, d_k, d_radii, geom_batched, bc.alpha, bc.beta, bc.batched, bc.per_degree, d_tab, d_density, d_out, st);
}

int biem_force(biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
               const double* d_alpha, const double* d_beta, int ab_batched, const double* d_tab, const double* d_density, double* d_out,
               void* stream) {
  return force_impl(__func__, plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, {d_alpha, d_beta, ab_batched, false}, d_tab, d_density,
                    d_out, (hipStream_t)stream);
}

int biem_force_n(biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                 const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_tab, const double* d_density,
                 double* d_out, void* stream) {
  return force_impl(__func__, plan, nb, B, nrhs, d_k, d_eta, d_radii, geom_batched, {d_alpha_n, d_beta_n, ab_batched, true}, d_tab, d_density,
                    d_out, (hipStream_t)stream);
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
