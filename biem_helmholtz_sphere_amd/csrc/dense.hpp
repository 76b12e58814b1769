// dense.hpp -- private to the dense-solver units kernels_gemm3m.hip (the trailing-update zgemm), kernels_lu.hip (pivoted LU and the L D L^T
// column form), kernels_sym.hip (the U^T U row form production runs) and kernels_trisolve.hip (stored-factor solves, column-form back
// substitution, growth bookkeeping): the constants and device inlines more than one of them uses, and the host functions through which
// a unit reaches another unit's kernels - a kernel is launched only by the unit that defines it (no relocatable device code).
#pragma once
#include "common.hpp"
#include <cstdlib>

namespace biem {

constexpr int NB = 64;    // panel width
constexpr int BS = 64;    // back-substitution block
static inline long long ldp_of(int n_pad) { return (long long)n_pad; }
typedef double v4d __attribute__((ext_vector_type(4)));   // (k_bench_mfma)

// ---------------------------------------------------------------------------------------------
// a-posteriori element growth of the symmetric factorisation (bounded multipliers alone do not bound it):
// growth[s][0] = max |a_ij| over the part of A the factorisation reads, growth[s][1] = max |u_ij|, both as cabs1 = |re| + |im|.
// Bit patterns of non-negative doubles order like unsigned integers and every NaN pattern lies above the finite ones, so a
// 64-bit atomicMax keeps the maximum and a NaN sticks.  k_growth_check marks a system (info = -(n_pad + 1)) whose factor U grew
// by more than GROWTH_MAX over A, or holds a non-finite entry; the caller re-solves it with the pivoted LU.
// ---------------------------------------------------------------------------------------------
constexpr double GROWTH_MAX = 2.0e2;     // (1e3 with multipliers <= 2 in round 1, 2e2 with multipliers <= 10 in round 2; see NOPIV_REL for round 3)
__device__ inline double cabs1(cplx v) { return fabs(v.x) + fabs(v.y); }
__device__ inline double nan_max(double a, double b) { return !(b <= a) ? b : a; }       // NaN in b wins; NaN in a stays
__device__ inline void block_max_publish(double m, unsigned long long* dst) {              // 1-D blocks of whole waves
  __shared__ double sm_max[16];
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = sm_max[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = nan_max(m, sm_max[i]);
    // most workgroups cannot raise the maximum: a plain read filters them out (the slot only grows, so a stale value is safe)
    if (!(m <= __longlong_as_double((long long)*(volatile unsigned long long*)dst))) atomicMax(dst, (unsigned long long)__double_as_longlong(m));
  }
}

// symmetric path: smallest accepted |diagonal| / |entry of its row|: every multiplier <= 10 (partial pivoting: <= 1).  It is the growth
// check (GROWTH_MAX) that bounds the error; with it in place the limit of 2 of round 1 only sent close-sphere systems at low k
// to the pivoted LU that the symmetric path solves to the same 1e-13 (profiles/r02_ldlt_fallback_survey.txt: a third -> a ninth of them)
// Round 3: multipliers <= 100.  The rejections of the close-sphere survey all sit at the first unknown of the second sphere (its
// monopole after the first sphere's elimination: pivot 1 - coupling^2) at LOW wavenumbers, with multipliers of 11 .. 77 (they
// saturate near 76 as k -> 0 for two unit spheres 0.04 apart) and a measured growth of 8 .. 45; the factorisation without
// interchanges solves every one of them to 4e-15 .. 1e-14 of the pivoted LU (NumPy emulation of this factorisation on the symmetric
// form, cond 33 .. 614).  It is the a-posteriori growth limit (200) that bounds the error; a limit of 10 on the multipliers only
// cost a fill and a pivoted LU (3 x the time) for systems the symmetric path solves to rounding.
constexpr double NOPIV_REL = 0.01;

// value of lane i (WAVE-UNIFORM i) in every lane: two v_readlane_b32 through the scalar file instead of the LDS crossbar round trip
// of ds_bpermute (__shfl) - these broadcasts sit on the dependent chain of the elimination / substitution steps
__device__ inline double lane_bcast(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}
constexpr int SYM_SLAB_CPLX = 4 * NB * NB;   // [S_J ; S_{J+64} ; S_{J+128} ; V_p] of the stacked pass: up to 256 rows of 64 per system
constexpr int BACK_ROWS = 16;   // rows per workgroup (4 per wave)
constexpr int RHS_UPD_ROWS = 64;  // rows per workgroup of k_rhs_update

// ---------------------------------------------------------------------------------------------
// The one workspace of the dense factorisations: lu_workspace_bytes(nb, n_pad, nrhs) bytes at d_work serve the pivoted LU, the
// L D L^T column form and the U^T U row form.  Regions in this order, byte offsets from d_work (dense_work fills them; a region ends
// where the next one starts):
//   panels   four 64-column panels per system, column-major with ldp = n_pad (two K = 128 blocks = one K = 256 update):
//            PANEL_COLS * n_pad complex per system.  The row form factors in place and needs no panels: it hands the region out
//            again under other names (SymAliases below)
//   block    64 x 64 complex per system: I - L11^{-1} of the MFMA triangular solve (LU), U11^{-1} (column form), V = -U11^{-T} (row form)
//   tri_map  the tile map of the triangular updates: one int per lower-triangle tile of the largest trailing matrix, T (T + 1) / 2
//            with T = n_pad / 64, rounded up to 64 ints
//   growth   two doubles per system as 64-bit patterns: max |A| over what the symmetric factorisation reads, max |U| (see above)
//   spare    64 complex per system that NO code reads or writes (an earlier row form kept a vector per system there); its bytes stay,
//            because biem_lu_workspace_bytes is public and the slab's place is counted from the end
//   slab     [S ; S ; S ; V] of a group of the row form's stacked pass: SYM_SLAB_CPLX complex per system
// nrhs does not enter today; it stays an argument of the public size.
// ---------------------------------------------------------------------------------------------
constexpr int PANEL_COLS = 4 * NB;           // columns of n_pad complex per system in the panel region
struct DenseWork {
  size_t panels, block, tri_map, growth, spare, slab, total;
  cplx* panels_at(void* w) const { return (cplx*)((char*)w + panels); }
  cplx* block_at(void* w) const { return (cplx*)((char*)w + block); }
  int* tri_map_at(void* w) const { return (int*)((char*)w + tri_map); }
  unsigned long long* growth_at(void* w) const { return (unsigned long long*)((char*)w + growth); }
  cplx* slab_at(void* w) const { return (cplx*)((char*)w + slab); }
};
inline DenseWork dense_work(int nb, int n_pad, int nrhs) {
  (void)nrhs;
  const size_t T = (size_t)n_pad / NB;
  DenseWork w;
  w.panels = 0;
  w.block = w.panels + (size_t)nb * PANEL_COLS * (size_t)ldp_of(n_pad) * sizeof(cplx);
  w.tri_map = w.block + (size_t)nb * NB * NB * sizeof(cplx);
  w.growth = w.tri_map + ((T * (T + 1) / 2 + 63) / 64) * 64 * sizeof(int);
  w.spare = w.growth + (size_t)nb * 2 * sizeof(double);
  w.slab = w.spare + (size_t)nb * NB * sizeof(cplx);
  w.total = w.slab + (size_t)nb * SYM_SLAB_CPLX * sizeof(cplx);
  return w;
}

// ---------------------------------------------------------------------------------------------
// The form of one call of launch_sym_factor_solve, decided once by sym_form (kernels_sym.hip, with the rules and their measurements);
// the launcher's three stages switch on it and decide nothing themselves.  With `small` the other fields are not used.
// ---------------------------------------------------------------------------------------------
struct SymForm {
  bool small; int kr; bool two;     // the one-launch LDS-resident path and its instantiation k_small_utu<kr, two>
  bool left;                        // bulk update left-looking (launch_gemm_left before a group), else the K = 256 update after it
  bool stacked;                     // panels b, c, d of a group in one stacked product pass, else in-group update + strip
  bool rhs_gemv;                    // the right-hand sides ride in the compact copy Y[s][q][row], else as columns of the matrix
  enum Back { BACK_ROW = 0, BACK_COL = 1, BACK_STEP = 2 } back;   // back substitution: k_back_sweep (k_back_row) / back_substitute_cols / k_back_step
  bool keep_w() const { return back == BACK_STEP; }               // every panel's W = I - U11^{-T} is kept for k_back_step
  bool diag_blk;                    // diagonal kernel k_diag_utu_blk (four pivots per barrier), else k_diag_utu_reg
};
// What the row form keeps in the panel region (nullptr: not used by this form):
//   Wall  keep_w: the kept W blocks, n_pad x 64 complex per system (wall_stride), system after system
//   Xsol  keep_w: behind them the solutions of k_back_step, nrhs x n_pad per system
//   Y     the compact copy Y[s][q][row], nrhs x n_pad per system, of the forward substitution (rhs_gemv) and of the row-form back
//         substitution: at the region's start, or at Xsol where the W blocks are kept
// Capacity: Wall takes NB of the PANEL_COLS columns per system, so keep_w holds PANEL_COLS - NB right-hand sides and the row form's
// copy PANEL_COLS; sym_form sends more to the form that needs no copy.
constexpr int SYM_ROW_RHS_MAX = PANEL_COLS, SYM_STEP_RHS_MAX = PANEL_COLS - NB;
struct SymAliases { cplx *Wall, *Xsol, *Y; long long wall_stride; size_t wall_bytes, y_off, y_bytes; };

#pragma GCC visibility push(hidden)   // between the units of one library: none of these is exported
// ---- kernels_sym.hip
SymForm sym_form(int nb, int n_pad, int n_active, int nrhs);
// the aliases of form f at d_work (which may be null: offsets and sizes only); BIEM_ERR_ARG if one would leave the panel region
int sym_aliases(const SymForm& f, const DenseWork& w, void* d_work, int nb, int n_pad, int nrhs, SymAliases& a);
// ---- kernels_gemm3m.hip
// C[row_begin:row_end, col_begin:col_end] -= P[0:kd]^T (rows of the region) * M[brow:brow+kd, cols of the region]
int launch_gemm_stream(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* Pw, long long ldp,
                       long long p_stride, int row_begin, int row_end, int col_begin, int col_end, int brow, int kd,
                       int prof_class = PK_GEMM, double prof_work = -1.0, cplx* pout = nullptr, long long pout_ld = 0,
                       long long pout_stride = 0, int pcol_tx = 0, const int* tri_map = nullptr, bool upper = false);
// the K-long left-looking update of the row form: A[J:row_end, J:col_end] -= U[0:J, J:row_end]^T U[0:J, J:col_end]
// nf < 4: col_end ends the last matrix tile column, of which only the column groups 0 .. nf-1 are multiplied (gemm_narrow_frags)
int launch_gemm_left(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, int J, int row_end, int col_end, int nf = 4);
// the rule of that split for the band at row J: the column groups to multiply, 4 = the launch stays whole (mode: BIEM_GEMM_NARROW, -1 unset)
int gemm_narrow_frags(int nb, int n_pad, int n_active, int J, int mode);
// the strip of panel j of the symmetric factorisation as a pure product: A[j:j+64, j+64:col_end] = -V^T A[j:j+64, j+64:col_end] (pass V - j);
// with Y (compact Y[s][q][row], y_ld rows per right-hand side, nrhs <= 8) also Y[.., c] -= U[j:j+64, c]^T Y[.., j:j+64] for the strip's columns
int launch_gemm_strip(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* V, long long v_stride, int j, int col_end,
                      cplx* Y = nullptr, int nrhs = 0, int y_ld = 0);
// the stacked pass of panel p of the group at row J: A[p:p+64, p+64:col_end] = -slab^T A[J:p+64, p+64:col_end], slab = [S_J ; .. ; V_p] of
// (p - J + 64) x 64 per system; Y as in launch_gemm_strip
int launch_gemm_stack(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* slab, long long slab_stride, int J, int p,
                      int col_end, cplx* Y = nullptr, int nrhs = 0, int y_ld = 0);
void launch_tri_map(hipStream_t st, int* tri_map, int n_pad);   // tile map of the triangular updates of an n_pad system
// sym_form's default rule for the bulk update: whether the smallest launch of the left-looking form has a tile for every CU
bool gemm_left_fills_grid(int nb, int n_pad, int nrhs);
// ---- kernels_trisolve.hip
void launch_zero_int(hipStream_t st, int* p, int n);
void launch_growth_check(hipStream_t st, int nb, int n_pad, const unsigned long long* growth, int* d_info, double limit);
// right-hand-side columns of the rows from row_begin down: f[i] -= P[0:kd, i]^T f[jg : jg + kd] (with its PK_OTHER profile scope)
void launch_rhs_update(hipStream_t st, int nb, int nrhs, cplx* A, long long lda, long long sys_stride, const cplx* Pw, long long ldp,
                       long long p_stride, int n_pad, int row_begin, int jg, int kd);
// column-form back substitution U x = y on F, bottom block first; with d_info the pass also checks the strip entries it reads
void back_substitute_cols(hipStream_t st, int nb, int n_pad, int nrhs, const cplx* A, long long lda, long long sys_stride, cplx* F,
                          long long ldf, long long f_stride, int* d_info = nullptr, unsigned long long* growth = nullptr, double inv_rel2 = 0.0);
// ---- kernels_lu.hip
int check_factor_args(const char* who, int nb, int n_pad, int nrhs, long long lda, size_t work_bytes);   // shared by the two factorisations; who: biem_lu / biem_sym
// BIEM_LDLT_PIVOT_REL / BIEM_LDLT_GROWTH_MAX (tests): acceptance threshold of the diagonal pivots (multipliers <= 1 / threshold; 1e30
// rejects every system) and accepted max |U| / max |A|; a value that does not parse to something positive is the default
void ldlt_thresholds(double& nopiv_rel, double& growth_max);
#pragma GCC visibility pop

}  // namespace biem
