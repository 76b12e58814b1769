// common.hpp -- small helpers shared by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "plan.hpp"
#include "../../include/biem_mi355.h"

namespace biem {

typedef double2 cplx;  // .x = re, .y = im

constexpr int kMaxRad = 320;   // max table order handled per thread-local/LDS radial array (every translation unit: one value)

__host__ __device__ inline cplx cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline cplx cadd(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__host__ __device__ inline cplx csub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__host__ __device__ inline cplx cscale(cplx a, double s) { return make_double2(a.x * s, a.y * s); }
// a + b*c
__host__ __device__ inline cplx cfma(cplx b, cplx c, cplx a) {
  return make_double2(fma(b.x, c.x, fma(-b.y, c.y, a.x)), fma(b.x, c.y, fma(b.y, c.x, a.y)));
}
// a - b*c
__host__ __device__ inline cplx cfnma(cplx b, cplx c, cplx a) {
  return make_double2(fma(-b.x, c.x, fma(b.y, c.y, a.x)), fma(-b.x, c.y, fma(-b.y, c.x, a.y)));
}
// 1/a with scaling (Smith) so that huge/tiny components do not overflow prematurely
__host__ __device__ inline cplx crecip(cplx a) {
  if (fabs(a.x) >= fabs(a.y)) {
    double r = a.y / a.x, den = a.x + a.y * r;
    return make_double2(1.0 / den, -r / den);
  } else {
    double r = a.x / a.y, den = a.x * r + a.y;
    return make_double2(r / den, -1.0 / den);
  }
}
__host__ __device__ inline cplx cdiv(cplx a, cplx b) { return cmul(a, crecip(b)); }
// accumulating forms of the gradient kernels (BIEM_GRAD_HARMONICS, fast_layout.hpp)
__device__ __forceinline__ void cacc(cplx& acc, const cplx& a, const cplx& b) {           // acc += a b
  acc.x += a.x * b.x - a.y * b.y; acc.y += a.x * b.y + a.y * b.x;
}
__device__ __forceinline__ void cacc_conj(cplx& acc, const cplx& a, const cplx& b) {          // acc += a conj(b)
  acc.x += a.x * b.x + a.y * b.y; acc.y += a.y * b.x - a.x * b.y;
}
__device__ __forceinline__ void cacc_real(cplx& acc, const cplx& a, double s) { acc.x += a.x * s; acc.y += a.y * s; }
__device__ __forceinline__ cplx cmulc(const cplx& a, const cplx& b) {                     // a conj(b)
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// sum over the 64 lanes of a wave in a fixed order (no atomics: two runs give the same bits); the total is in lane 0
__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

#define BIEM_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { biem::set_error("%s failed: %s", #x, hipGetErrorString(e_)); return BIEM_ERR_HIP; } } while (0)
#define BIEM_LAUNCHCHK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { biem::set_error("kernel launch failed at %s:%d: %s", __FILE__, __LINE__, hipGetErrorString(e_)); return BIEM_ERR_HIP; } } while (0)

// (a body shared by several entry points reports under the name of the one that was called: `who`)
#define NEED_AS(who, p, what) do { if (!(p)) { biem::set_error("%s: null %s", who, what); return BIEM_ERR_ARG; } } while (0)
#define NEED_DEV_AS(who, pl) do { NEED_AS(who, pl, "plan"); if ((pl)->device < 0) { biem::set_error("%s: plan not uploaded to a device (biem_plan_upload)", who); return BIEM_ERR_ARG; } } while (0)

const char* last_error();

// ---- optional HIP-event profiler (thread-local; off unless biem_profile_begin was called on this thread) ----
enum ProfClass { PK_TABLES = 0, PK_FILL, PK_RHS, PK_PANEL, PK_SWAP, PK_TRSM, PK_GEMM, PK_BACK, PK_OTHER, PK_COUNT };
struct Profiler {
  bool on = false;
  struct Rec { hipEvent_t a, b; int cls; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  double work[PK_COUNT] = {0};          // algorithmic flops (GEMM/TRSM/PANEL) or bytes (FILL) per class
  long long launches[PK_COUNT] = {0};
  hipEvent_t get();
};
Profiler& profiler();
struct ProfScope {
  Profiler& p; hipStream_t st; hipEvent_t a = nullptr; int cls;
  ProfScope(int cls_, hipStream_t st_, double work = 0.0) : p(profiler()), st(st_), cls(cls_) {
    if (!p.on) return;
    a = p.get();
    (void)hipEventRecord(a, st);
    p.work[cls] += work; p.launches[cls] += 1;
  }
  ~ProfScope() {
    if (!p.on || !a) return;
    hipEvent_t b = p.get();
    (void)hipEventRecord(b, st);
    p.recs.push_back({a, b, cls});
  }
};

// ---- split layout of the symmetric path (flat sphere layouts) ----
// With every centre in one plane of constant last coordinate, A~ couples no cosine slot to a sine slot: it is diag(E, O) after the
// permutation that collects the balls' cosine runs (U slots each) in rows [0, npE) and their sine runs (H - U each) in rows
// [npE, npE + npO), both padded to whole 64-row tiles.  E's right-hand sides stand at column npE of the E rows (inside the E x O rectangle
// nobody reads as matrix), O's at column n_pad = npE + npO as in the unsplit layout.  U == 0: the unsplit layout (row b H + slot).
struct SplitMap {
  int U, npE, npO;                        // (SplitMap(): all zero)
  __host__ __device__ bool on() const { return U != 0; }
  __host__ __device__ int row_of(int b, int H, int slot) const {
    return U == 0 ? b * H + slot : slot < U ? b * U + slot : npE + b * (H - U) + (slot - U);
  }
  // offset of (b, slot)'s first right-hand side relative to column n_pad of row 0 (where the unsplit layout keeps them all)
  __host__ __device__ long long rhs_off(int b, int H, int slot, long long lda) const {
    return (long long)row_of(b, H, slot) * lda - ((U != 0 && slot < U) ? npO : 0);
  }
};
inline int roundup64(int v) { return (v + 63) / 64 * 64; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }   // regions of a workspace start on 256-byte boundaries
inline SplitMap make_split_map(int B, int H, int U) { SplitMap m; m.U = U; m.npE = roundup64(B * U); m.npO = roundup64(B * (H - U)); return m; }

// launch wrappers implemented in the .hip files (all stream-ordered, no syncs)
int launch_radial(int d, int nmax, int count, const double* d_x, double* d_out, hipStream_t st);
int launch_radial_c(int d, int nmax, int count, const double* d_z, double* d_out, hipStream_t st);
int launch_harmonics(const biem_plan* p, int count, const double* d_u, double* d_Y, hipStream_t st);
int launch_ball_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_tab, hipStream_t st);
// projection of boundary samples (kernels_rhs.hip), any number of rows nb nrhs B an int counts.
// slot_order: harmonic h of a ball goes to / comes from the plan's internal slot hpos[h] (symmetric path) instead of position h
int launch_rhs_project(const biem_plan* p, int nb, int B, int nrhs, const double* d_g, double* d_f, long long sys_stride,
                       long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order = false, const SplitMap& split = SplitMap());
// degree-dependent boundary coefficients: alpha_n / beta_n [nb or 1][B][n_end] complex; the tables are laid out as
// launch_ball_tables' (the same kernel text) and feed the same fill / solve / density launches
int launch_ball_tables_n(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                         int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_tab, hipStream_t st);
// f = -(alpha_n P[gu] + beta_n P[gdn]); a null sample set is zero; strides and slot order as launch_rhs_project
int launch_rhs_project_n(const biem_plan* p, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn, const double* d_alpha_n,
                         const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride, long long elem_stride,
                         long long rhs_stride, hipStream_t st, bool slot_order = false, const SplitMap& split = SplitMap());
// plane-wave incidence in closed form (kernels_rhs_pw.hip): f = -C_d i^n gj_n conj(Y_h(p^_r)) e^{i k p^_r.c_b} from the ball tables, written
// where launch_rhs_project writes.  d_dirs: unit vectors in the plan's axes, [nrhs][d] or (dirs_batched) [nb][nrhs][d]; d_work:
// rhs_plane_wave_workspace_bytes (the harmonics of the directions).  At most 65535 systems and right-hand sides (RhsSource::check).
size_t rhs_plane_wave_workspace_bytes(const biem_plan* p, int nb, int nrhs, int dirs_batched);
int launch_rhs_plane_wave(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                          const double* d_tab, const double* d_dirs, int dirs_batched, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work);
// complex [batch][rows][cols] -> [batch][cols][rows], 32 x 32 tiles through LDS (kernels_rhs_pw.hip); batches <= 65535, rows <= 32 x 65535
int launch_transpose_rows(int cols, int rows, int batches, const double* d_in, double* d_out, hipStream_t st);
// point-source incidence in closed form (kernels_rhs_ps.hip): the monopole h_0(k |x - s_r|), f = -C_d gj_n h_n(k |t|) conj(Y_h(t^)),
// t = s_r - c_b, from the ball tables, written where launch_rhs_project writes.  d_src: source positions in the plan's axes, [nrhs][d] or
// (src_batched) [nb][nrhs][d]; d_work: rhs_point_source_workspace_bytes.  |t| > rho_b is the caller's to ensure (not tested: finite
// nonsense on or inside a sphere, non-finite values at t = 0).  At most 65535 systems and right-hand sides and n_end <= kMaxRad: both
// are RhsSource::check's to refuse before anything is launched.
size_t rhs_point_source_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int src_batched, int geom_batched);
int launch_rhs_point_source(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                            const double* d_tab, const double* d_src, int src_batched, double* d_f, long long sys_stride,
                            long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work);
// multipole incidence in closed form (kernels_rhs_ms.hip): the outgoing multipole h_n'(k |x - s_r|) Y_h'((x - s_r)^), h' = d_idx[r] an index
// into the plan's harmonic axis; f = -gj_n (S|R)_{h'->h}(c_b - s_r) from the ball tables and the plan's term lists (tree a: Graf's one term),
// written where launch_rhs_project writes.  d_src as launch_rhs_point_source's, d_idx [nrhs] or (src_batched) [nb][nrhs]; d_work:
// rhs_multipole_workspace_bytes, the table rows of one slice of (systems x right-hand sides).  |t| > rho_b and 0 <= h' < H are the caller's
// to ensure (an index outside gives NaN); the count and order limits and a plan without term lists are RhsSource::check's to refuse.
size_t rhs_multipole_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int src_batched, int geom_batched);
int launch_rhs_multipole(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                         const double* d_tab, const double* d_src, int src_batched, const int* d_idx, double* d_f, long long sys_stride,
                         long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work,
                         bool regular = false);
// regular: the regular wave j_n'(k |x - o_r|) Y_h'((x - o_r)^) about the origins d_src instead, f = -gj_n (R|R)_{h'->h}(c_b - o_r): the same
// kernels with the regular radial row, workspace and limits as above.  The origin is unrestricted; o_r = c_b gives (R|R)(0) = identity.
// The two pieces the cluster coefficients (kernels_cluster.hip) share with it: (system, right-hand side) pairs per table slice under the
// byte cap (BIEM_RHS_TABLE_BYTES), and the regular table rows T[row][H2] = C_d j_n''(k |t|) Y_l(t^) of the rows sr0 B .. of (pairs x balls),
// t = c_b - src (flip: src - c_b)
long long rhs_table_slice_pairs(const biem_plan* p, int nb, int B, int nrhs);
int launch_regular_tables(const biem_plan* p, int B, int nrhs, long long sr0, long long rows, const double* d_k, const double* d_centers,
                          int geom_batched, const double* d_src, int src_batched, int flip, double* d_T, hipStream_t st);
// the same rows with the outgoing radial function (regular == false): T[row][H2] = C_d h_n''(k |t|) Y_l(t^)
int launch_translation_tables(const biem_plan* p, bool regular, int B, int nrhs, long long sr0, long long rows, const double* d_k,
                              const double* d_centers, int geom_batched, const double* d_src, int src_batched, int flip, double* d_T,
                              hipStream_t st);
// incident fields by their expansion coefficients (kernels_rhs_ex.hip): u_in = sum_h' p_h' z_n'(k |x - o|) Y_h'((x - o)^), z = j (regular) or h,
// f = -gj_n sum_{n(h') < n_in} p_h' (X|R)_{h'->h}(c_b - o), written where launch_rhs_project writes for the solve plan p.  lp: the LIST plan of
// the same tree, of order max(n_in, n_end) (p itself where n_in <= n_end): its term lists, table labels and harmonic axis, along which
// d_coef [nrhs][H(lp)] or (coef_batched) [nb][nrhs][H(lp)] lies; d_map [H(p)]: the position of every harmonic of p on that axis (null with
// lp == p).  d_origin [n_origin][d] or (origin_batched) [nb][n_origin][d], n_origin 1 (one origin for all right-hand sides of a system: the
// table rows are formed once) or nrhs.  d_work: rhs_expansion_workspace_bytes, the table rows of one slice.  stage: 0; 1 / 2 the table
// rows / the contraction alone (timing; 1 then 2 is 0 only for a call of one table slice - the workspace holds one).  The count and order limits are RhsSource::check's to refuse (on lp).
size_t rhs_expansion_workspace_bytes(const biem_plan* lp, int nb, int B, int n_origin);
int launch_rhs_expansion(const biem_plan* p, const biem_plan* lp, const int* d_map, int n_in, bool regular, int nb, int B, int nrhs,
                         const double* d_k, const double* d_centers, int geom_batched, const double* d_tab, const double* d_origin,
                         int origin_batched, int n_origin, const double* d_coef, int coef_batched, double* d_f, long long sys_stride,
                         long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, int stage,
                         void* d_work);
// outgoing coefficients of the whole cluster about an origin (kernels_cluster.hip): A[s][r][h''] = sum_b sum_h (R|R)_{h->h''}(o_s - c_b) c[s][r][b][h],
// c = density * blc.  d_density [nb][nrhs][B][H] in the plan's layout (degrees >= n_src are not read), d_origin [d] or (origin_batched) [nb][d],
// d_out [nb][nrhs][H]; kind outer.  stage: 0 both, 1 the table rows only, 2 the contraction only (timing; slices then walk one stage)
size_t cluster_coefficients_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs);
int launch_cluster_coefficients(const biem_plan* p, int nb, int B, int nrhs, int n_src, const double* d_k, const double* d_eta,
                                const double* d_centers, const double* d_radii, int geom_batched, const double* d_origin, int origin_batched,
                                const double* d_density, double* d_out, int stage, void* d_work, size_t work_bytes, hipStream_t st);
// d_info[s] = code for every system with a (ball, degree) whose symmetric scaling 1 / sqrt(gj gh) is not finite (gj = 0); others untouched
// (biem_flag_unscalable exposes it for tests)
int launch_flag_unscalable(const biem_plan* p, int nb, int B, const double* d_tab, int* d_info, int code, hipStream_t st);
// extinction and absorbed power per (system, right-hand side, ball) from the density, the projections pu / pv of u_in / d_n u_in
// [nb][nrhs][B][H] and the ball tables (kernels_power.hip); alpha / beta [nb or 1][B], per_degree: [nb or 1][B][n_end]; real k only
int launch_power(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_radii, int geom_batched,
                 const double* d_alpha, const double* d_beta, int ab_batched, bool per_degree, const double* d_tab,
                 const double* d_density, const double* d_pu, const double* d_pv, double* d_out, hipStream_t st);
// radiation force per (system, right-hand side, ball), out [nb][nrhs][B][d] (kernels_force.hip); operands as launch_power, the plan's
// force coupling table uploaded (plan_build_force)
int launch_force(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_radii, int geom_batched,
                 const double* d_alpha, const double* d_beta, int ab_batched, bool per_degree, const double* d_tab,
                 const double* d_density, double* d_out, hipStream_t st);
size_t fill_workspace_bytes(const biem_plan* p, int nb, int B);
int launch_fill(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched,
                const double* d_tab, int scaling, double* d_A, long long lda, long long sys_stride, int n_pad,
                void* d_work, size_t work_bytes, hipStream_t st);
int launch_density(const biem_plan* p, int nb, int B, int nrhs, const double* d_x, long long sys_stride, long long elem_stride,
                   long long rhs_stride, const double* d_tab, double* d_density, hipStream_t st, bool slot_order = false,
                   const SplitMap& split = SplitMap());
// the complex-symmetric form A~ = R W^H M W R^-1 in the plan's internal slot order, written only where the U^T U factorisation in row
// form (launch_sym_factor_solve) reads it (UPPER triangle + diagonal 64 x 64 tiles); fill_sym_bytes = those bytes per system
// FillDedupe (optional): per-ball radii [B], alpha [B], beta [B] (complex) shared by all systems of the call.  Ball pairs with the
// same displacement vector (to the rounding of the subtraction) and the same (radius, alpha, beta) on either side have IDENTICAL blocks of A~ (translation invariance of
// (S|R)): the block is contracted once and stored to every such pair (lattices of equal spheres: cfg 3 has 24 distinct blocks
// among its 120 pairs).  nullptr: every pair on its own (batched geometry or per-system alpha / beta).
struct FillDedupe { const double* radii; const double* alpha; const double* beta; };
int launch_fill_sym(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched, const double* d_tab,
                    double* d_A, long long lda, long long sys_stride, int n_pad, void* d_work, size_t work_bytes, hipStream_t st, bool no_padding = false,
                    const FillDedupe* dedupe = nullptr, const SplitMap& split = SplitMap());
double fill_sym_bytes(int n_pad);
// whether launch_fill_sym runs k_fill_red for this plan and B balls (the one fill form with a split mode)
bool fill_sym_red_form(const biem_plan* p, int B);
// info[s] = first nonzero of (E's code, O's code) in unsplit terms: row codes of O shifted by npE, either growth code -> -(n_pad + 1)
int launch_split_info_merge(int nb, int npE, int npO, int* d_info, const int* d_info_O, hipStream_t st);
int launch_uscat(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                 const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                 double* d_out, void* d_work, size_t work_bytes, hipStream_t st);
int launch_uscat_grad(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                      double* d_out, void* d_work, size_t work_bytes, hipStream_t st);
// the host steps of launch_uscat (kernels_uscat.hip): what biem_uscat refuses at this plan (BIEM_ERR_UNSUPPORTED, nothing launched),
// c[nb][B][H] = density * blc, and the field of a coefficient set c at the points (out and flags as launch_uscat)
int uscat_covered(const biem_plan* p, int nb, int B, int flags);
int uscat_form_coef(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                    const double* d_density, int flags, cplx* c, hipStream_t st);
int uscat_eval_coef(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_centers, const double* d_radii,
                    int geom_batched, const cplx* c, const double* d_points, int flags, double* d_out, hipStream_t st);
// Hessian of the near field (kernels_ladder.hip): p is the plan of order n_end + 2 with its force coupling table uploaded, the density
// in that plan's layout (degrees < n_end(p) - 2 are read); out[d (d + 1) / 2][P][nb] ([..][B] per ball), the pairs i <= j row-major
size_t uscat_hess_workspace_bytes(const biem_plan* p, int nb, int B);
int launch_uscat_hess(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                      const double* d_radii, int geom_batched, const double* d_density, const double* d_points, int flags,
                      double* d_out, void* d_work, size_t work_bytes, hipStream_t st);
// the field of the outgoing multipole h_n'(k |x - s|) Y_h'((x - s)^) at the points (kernels_ladder.hip): d_src [nb][d], d_idx [nb] into the
// plan's harmonic axis; out [P][nb], or (grad) its Cartesian gradient [d][P][nb] - p is then a plan of order n' + 2 or more with its force
// coupling table uploaded.  flags: BIEM_USCAT_POINTS_BATCHED, and BIEM_USCAT_KIND_INNER for the regular wave j_n' Y_h' about d_src (the
// kind-inner value kernels on the unit coefficient, the fictitious ball unbounded: every point is an ordinary one, x = d_src included)
// The field of a whole coefficient vector about d_src instead (biem_expansion_field, `who`): d_idx null and d_coef [nb][H] along the
// plan's harmonic axis, copied where the unit set is written; the gradient reads its degrees < n_end - 1.  One body for both.
size_t multipole_field_workspace_bytes(const biem_plan* p, int nb);
int launch_multipole_field(const char* who, const biem_plan* p, int nb, int P, const double* d_k, const double* d_src, const int* d_idx,
                           const double* d_coef, const double* d_points, int flags, int grad, double* d_out, void* d_work, size_t work_bytes,
                           hipStream_t st);
// per-lane order ceiling of a tree (kernels_uscat.hip: kFastNendMax*; 0 for the chain trees)
int uscat_fast_nend_max(int tree);
// total field inside penetrable fluid balls (kernels_uinterior.hip).  d_kint / d_delta [nb or 1][B] complex; the coefficient step
// a[s][b][h] on its own, and the field at points (out[P][nb], NaN outside every ball); workspace: the coefficients, nb B H complex
int launch_interior_coef(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                         int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched, const double* d_density,
                         double* d_a, hipStream_t st);
int launch_uinterior(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                     const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                     const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                     hipStream_t st);
// its Cartesian gradient, out[d][P][nb] in the plan's axes: the arguments and the workspace of launch_uinterior
int launch_uinterior_grad(const biem_plan* p, int nb, int B, int P, const double* d_k, const double* d_eta, const double* d_centers,
                          const double* d_radii, int geom_batched, const double* d_kint, const double* d_delta, int fluid_batched,
                          const double* d_density, const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes,
                          hipStream_t st);
int lu_npad(int N);
size_t lu_workspace_bytes(int nb, int n_pad, int nrhs);
int launch_lu_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_ipiv,
                           int* d_info, void* d_work, size_t work_bytes, hipStream_t st, bool keep_multipliers = true,
                           bool symmetric = false, bool amax_ready = false);
// complex-symmetric A = U^T U in row form on the upper triangle (kernels_sym.hip), fused with the solve of the augmented columns
// (the form of a call is decided in one place, sym_form in kernels_sym.hip; these read single decisions of it)
int sym_update_left(int nb, int n_pad, int nrhs);  // form of the bulk update launch_sym_factor_solve runs for this call: 1 left-looking, 0 right-looking
bool sym_small_path(int n_active, int nrhs);      // whether launch_sym_factor_solve takes its one-launch LDS-resident path
int sym_gemm_narrow(int nb, int n_pad, int n_active, int J);   // column groups the left-looking band at row J multiplies in its last tile column (4: all)
// the whole form and the workspace layout of a call as numbers (biem_sym_form); host only
__attribute__((visibility("hidden"))) int sym_form_query(int nb, int n_pad, int n_active, int nrhs, int* form, size_t* work);
// (n_active: rows n_active .. n_pad-1 are identity padding; systems of at most 128 active rows run in one LDS-resident launch)
int launch_sym_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_info, void* d_work,
                            size_t work_bytes, hipStream_t st, bool amax_ready = false, int n_active = 0);
// zero `width` complex columns from d_A on in `rows` consecutive rows of lda complex (right-hand-side columns of a chunk's systems)
void launch_clear_cols(hipStream_t st, double* d_A, long long lda, int width, long long rows);
// where the symmetric factorisation keeps max |A|, max |U| per system inside its workspace (unsigned 64-bit patterns of doubles)
unsigned long long* lu_growth_slots(void* d_work, int nb, int n_pad);
// preset the slots for a caller that knows (a lower bound of) max |A|: growth[s] = (amax, 0); then pass amax_ready = true
int lu_growth_init(void* d_work, int nb, int n_pad, double amax, hipStream_t st);
// right-hand-side columns (slot order): f~ = R W^H f in place; inverse_on_solution: x = W R^-1 x~.  d_rhs: the first right-hand-side entry
// of the first system (column n_pad of an augmented matrix, or an array of its own), rows lda complex apart
int launch_sym_rhs(const biem_plan* p, int nb, int B, int nrhs, int n_pad, const double* d_tab, double* d_rhs, long long lda,
                   long long sys_stride, bool inverse_on_solution, hipStream_t st, const SplitMap& split = SplitMap());
// solve with a stored U^T U factor (upper triangle, identity-padded): forward U^T y = f, back U x = y, B row-major [n_pad][ldb] per system
int launch_sym_solve(int nb, int n_pad, int nrhs, const double* d_U, long long lda, long long sys_stride, double* d_B, long long ldb,
                     long long b_stride, hipStream_t st);
int launch_lu_solve(int nb, int n_pad, int nrhs, const double* d_LU, long long lda, long long sys_stride, const int* d_ipiv, double* d_B,
                    long long ldb, long long b_stride, hipStream_t st);
int bench_mfma_f64(int iters, double* tflops, hipStream_t st, int variant = 0);

// ---- the whole-path driver (solve_path.cpp) as the entry points of abi.cpp see it, and what both files check with ----
// boundary coefficients: alpha / beta [nb or 1][B] complex, or per degree (the *_n entries) [nb or 1][B][n_end]; batched: one set per system
struct BoundaryCoef {
  const double* alpha; const double* beta; int batched; bool per_degree;
  const char* alpha_name() const { return per_degree ? "d_alpha_n" : "d_alpha"; }
  const char* beta_name() const { return per_degree ? "d_beta_n" : "d_beta"; }
};
// The source of the right-hand sides of a call, made by its named constructors only.  A new incident field is one more kind, one more
// constructor and one more case in work_bytes / check / launch (solve_path.cpp).
//   SAMPLES        boundary samples g [nb][nrhs][B][Q] complex of plain coefficients, projected by launch_rhs_project
//   SAMPLES_N      the unmixed samples gu / gdn of per-degree coefficients (either may be null: zero), launch_rhs_project_n
//   PLANE_WAVES    plane waves along pts = dirs in closed form (launch_rhs_plane_wave: no samples)
//   POINT_SOURCES  point sources at pts = src in closed form (launch_rhs_point_source)
//   MULTIPOLE_SOURCES  outgoing multipoles at pts = src of the harmonics idx in closed form (launch_rhs_multipole)
//   REGULAR_WAVES  regular waves about the origins pts of the harmonics idx in closed form (launch_rhs_multipole, regular)
//   REGULAR_EXPANSION / MULTIPOLE_EXPANSION  whole coefficient vectors `coef` of regular / outgoing waves about the origins pts
//                  (launch_rhs_expansion): the columns the two kinds above take one at a time, contracted
// The closed forms read the wavenumbers, centres and ball tables of the call and keep their harmonics in `work`, work_bytes() of them:
// the caller's workspace, or (set by the whole path) the tail of its own.
struct RhsSource {
  enum Kind { SAMPLES, SAMPLES_N, PLANE_WAVES, POINT_SOURCES, MULTIPOLE_SOURCES, REGULAR_WAVES, REGULAR_EXPANSION, MULTIPOLE_EXPANSION };
  Kind kind;
  const double* g[2] = {nullptr, nullptr};                 // samples: g, or gu and gdn
  const double* pts = nullptr; int pts_batched = 0;        // closed forms: [nrhs][d], or (pts_batched) [nb][nrhs][d], in the plan's axes
  const int* idx = nullptr;                                // multipoles: the harmonic of every source, [nrhs] or (pts_batched) [nb][nrhs]
  const double* k = nullptr; const double* centers = nullptr; int geom_batched = 0;
  // expansions: the coefficient vectors [nrhs][H(lists)] or (coef_batched) [nb][nrhs][H(lists)], the list plan, the map of the solve
  // plan's harmonics onto its axis (null: the same plan), the order of the coefficients and the origins per system (pts: 1 or nrhs)
  const double* coef = nullptr; int coef_batched = 0; const biem_plan* lists = nullptr; const int* map = nullptr; int n_in = 0, n_origin = 0;
  void* work = nullptr;

  static RhsSource samples(const double* g) { RhsSource s(SAMPLES); s.g[0] = g; return s; }
  static RhsSource samples_n(const double* gu, const double* gdn) { RhsSource s(SAMPLES_N); s.g[0] = gu; s.g[1] = gdn; return s; }
  static RhsSource plane_waves(const double* dirs, int batched, const double* k, const double* centers, int geom_batched) {
    return RhsSource(PLANE_WAVES, dirs, batched, k, centers, geom_batched);
  }
  static RhsSource point_sources(const double* src, int batched, const double* k, const double* centers, int geom_batched) {
    return RhsSource(POINT_SOURCES, src, batched, k, centers, geom_batched);
  }

  static RhsSource multipole_sources(const double* src, const int* idx, int batched, const double* k, const double* centers, int geom_batched) {
    RhsSource s(MULTIPOLE_SOURCES, src, batched, k, centers, geom_batched);
    s.idx = idx;
    return s;
  }
  static RhsSource regular_waves(const double* origin, const int* idx, int batched, const double* k, const double* centers, int geom_batched) {
    RhsSource s(REGULAR_WAVES, origin, batched, k, centers, geom_batched);
    s.idx = idx;
    return s;
  }

  static RhsSource expansion(bool regular, const double* origin, int batched, int n_origin, const double* coef, int coef_batched,
                             const biem_plan* lists, const int* map, int n_in, const double* k, const double* centers, int geom_batched) {
    RhsSource s(regular ? REGULAR_EXPANSION : MULTIPOLE_EXPANSION, origin, batched, k, centers, geom_batched);
    s.coef = coef; s.coef_batched = coef_batched; s.lists = lists; s.map = map; s.n_in = n_in; s.n_origin = n_origin;
    return s;
  }

  bool expanded() const { return kind == REGULAR_EXPANSION || kind == MULTIPOLE_EXPANSION; }   // a coefficient vector against the columns
  // columns of the translation operator: the order limits, the term lists and the table rows of `table_plan`
  bool translated() const { return kind == MULTIPOLE_SOURCES || kind == REGULAR_WAVES || expanded(); }
  const biem_plan* table_plan(const biem_plan* p) const { return expanded() && lists ? lists : p; }
  bool closed_form() const { return kind == PLANE_WAVES || kind == POINT_SOURCES || translated(); }
  // the same source for the systems s0 .. of the call
  RhsSource at(const biem_plan* p, int s0, int nrhs, int B) const {
    RhsSource s = *this;
    for (const double*& x : s.g) if (x) x += (size_t)s0 * nrhs * B * p->Q * 2;
    if (pts && pts_batched) s.pts += (size_t)s0 * (expanded() ? n_origin : nrhs) * p->d;
    if (coef && coef_batched) s.coef += (size_t)s0 * nrhs * table_plan(p)->H * 2;
    if (idx && pts_batched) s.idx += (size_t)s0 * nrhs;
    if (k) s.k += 2 * (size_t)s0;
    if (centers && geom_batched) s.centers += (size_t)s0 * B * p->d;
    return s;
  }
  size_t work_bytes(const biem_plan* p, int nb, int B, int nrhs) const {
    return kind == PLANE_WAVES ? rhs_plane_wave_workspace_bytes(p, nb, nrhs, pts_batched)
         : kind == POINT_SOURCES ? rhs_point_source_workspace_bytes(p, nb, B, nrhs, pts_batched, geom_batched)
         : expanded() ? rhs_expansion_workspace_bytes(table_plan(p), nb, B, n_origin)
         : translated() ? rhs_multipole_workspace_bytes(p, nb, B, nrhs, pts_batched, geom_batched) : 0;
  }
  // what the closed forms cannot take (grid dimensions; the thread-local radial table of a (source, ball) pair): refused under the
  // caller's name `who` before anything is launched
  int check(const char* who, const biem_plan* p, int nb, int nrhs) const;
  // f of the nb systems this source starts at: strides, slot order and split as launch_rhs_project; bc is read by SAMPLES_N, the ball
  // tables d_tab of the nb systems by the closed forms
  int launch(const biem_plan* p, int nb, int B, int nrhs, const BoundaryCoef& bc, const double* d_tab, double* d_f, long long sys_stride,
             long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order = false, const SplitMap& split = SplitMap()) const;

 private:
  explicit RhsSource(Kind kd, const double* pts_ = nullptr, int batched = 0, const double* k_ = nullptr, const double* centers_ = nullptr,
                     int geom_batched_ = 0)
      : kind(kd), pts(pts_), pts_batched(batched), k(k_), centers(centers_), geom_batched(geom_batched_) {}
};

inline long long rhs_ld(long long nrhs) { return (nrhs + 7) / 8 * 8; }   // right-hand-side columns; rows stay 128-byte aligned (8 complex128)

inline int check_counts(const char* who, int nb, int nrhs, int B) {
  if (nb >= 0 && nb <= 65535 && nrhs >= 0 && nrhs <= 65535 && B >= 0) return BIEM_OK;
  set_error("%s: 0 .. 65535 systems / right-hand sides per call and B >= 0 (got nb=%d, nrhs=%d, B=%d)", who, nb, nrhs, B);
  return BIEM_ERR_ARG;
}

// the one place that picks the per-degree launcher of the ball tables
int ball_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                const BoundaryCoef& bc, double* d_tab, hipStream_t st);

size_t solve_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int chunk);
size_t factor_workspace_bytes(const biem_plan* p, int nb, int B, int chunk);
size_t solve_factored_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs);
void last_solve_split(int* npE, int* npO);

// tables -> fill -> right-hand side -> factor and solve -> density; symmetric: U^T U (LDL^T entries), else the pivoted LU
int solve_path(const char* who, const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const BoundaryCoef& bc, const RhsSource& src, double* d_density, int* d_info, int chunk,
               void* d_work, size_t work_bytes, hipStream_t st, bool symmetric);
// the same path cut at the factorisation: factors and tables stay with the caller, right-hand sides come later
int factor_path(const char* who, const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                const double* d_radii, int geom_batched, const BoundaryCoef& bc, double* d_F, long long lda, long long sys_stride,
                double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes, hipStream_t st);
int solve_factored_path(const char* who, const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                        const double* d_tab, const BoundaryCoef& bc, const RhsSource& src, double* d_density, void* d_work, size_t work_bytes,
                        hipStream_t st);

}  // namespace biem
