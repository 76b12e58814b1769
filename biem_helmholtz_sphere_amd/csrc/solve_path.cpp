// solve_path.cpp -- the whole path behind biem_solve*, biem_factor_ldlt* and biem_solve_factored*: tables -> fill -> right-hand side ->
// factor / solve -> density, over chunks of resident systems.  Host code only; every decision of the path is taken once, here.
#include "common.hpp"
#include <climits>
#include <cstdlib>

namespace biem {
namespace {
// Flat layouts of at least this many unknowns take the split form; below, the step is bound by the per-panel launches, whose number
// does not fall.  (Not 392 or below: rejection codes of small flat systems are pinned in unsplit row numbers by the tests.)
constexpr int SYM_SPLIT_MIN_N = 1024;
thread_local int g_last_split[2] = {0, 0};   // npE, npO of the last symmetric solve on this thread; 0, 0: unsplit

// systems resident per chunk: the number asked for, or (chunk <= 0) as many as fit the budget; at most nb and cap, at least 1
int resident_chunk(int chunk, size_t budget_bytes, size_t per_system_bytes, int nb, int cap) {
  if (chunk <= 0) {
    const size_t fit = budget_bytes / (per_system_bytes ? per_system_bytes : 1);
    chunk = (int)(fit < 1 ? 1 : (fit > (size_t)nb ? (size_t)nb : fit));
  }
  if (chunk > nb) chunk = nb;
  if (chunk > cap) chunk = cap;
  return chunk < 1 ? 1 : chunk;
}

// the systems s0 .. s0 + c of a call and where their wavenumbers, centres and ball tables start
struct Chunk { int s0, c; const double* k; const double* centers; const double* tab; };
template <class Body>
int for_each_chunk(const biem_plan* p, int nb, int B, int chunk, const double* d_k, const double* d_centers, int geom_batched,
                   const double* d_tab, Body body) {
  for (int s0 = 0; s0 < nb; s0 += chunk) {
    const Chunk ch = {s0, (nb - s0 < chunk) ? nb - s0 : chunk, d_k + 2 * (size_t)s0,   // complex128 per system
                      d_centers + (geom_batched ? (size_t)s0 * B * p->d : 0), d_tab + (size_t)s0 * B * 3 * p->n_end * 2};
    if (const int rc = body(ch)) return rc;
  }
  return BIEM_OK;
}

struct SolveLayout {
  int N, n_pad, chunk;
  long long lda, sys_stride;
  size_t off_tab, off_A, off_T, off_P, off_ipiv, off_info2, total;
};
// One size serves both forms (the caller asks for it before the geometry is looked at): every region is as large as the larger form needs,
// so the offsets are the same whichever runs; n_pad, lda and sys_stride are those of the form asked for (split: n_pad = npE + npO).
SolveLayout make_layout(const biem_plan* p, int nb, int B, int nrhs, int chunk, bool split = false) {
  SolveLayout L;
  L.N = B * p->H;
  const int ldr = (int)rhs_ld(nrhs);
  const int np_plain = lu_npad(L.N);
  const SplitMap sm = make_split_map(B, p->H, (int)(p->units.size() / 2));
  const int np_split = sm.npE + sm.npO, np_max = np_split > np_plain ? np_split : np_plain;
  L.n_pad = split ? np_split : np_plain;
  L.lda = L.n_pad + ldr;
  L.sys_stride = (long long)L.n_pad * L.lda;
  const size_t sys_max = (size_t)np_max * (np_max + ldr);
  // resident matrices per chunk: as many as fit ~24 GiB; 32768: grid y / z dimensions of the per-system kernels
  L.chunk = chunk = resident_chunk(chunk, (size_t)24 << 30, sys_max * 16 + (size_t)B * B * p->H2 * 16 + lu_workspace_bytes(1, np_max, nrhs), nb, 32768);
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

struct FactorLayout {
  int N, n_pad, chunk;
  size_t off_T, off_P, total;
};
FactorLayout make_factor_layout(const biem_plan* p, int nb, int B, int chunk) {
  FactorLayout L;
  L.N = B * p->H;
  L.n_pad = lu_npad(L.N);
  // fill and factorisation workspace of ~4 GiB at most: the factors themselves are the caller's, all of them resident
  L.chunk = chunk = resident_chunk(chunk, (size_t)4 << 30, fill_workspace_bytes(p, 1, B) + lu_workspace_bytes(1, L.n_pad, 0), nb, INT_MAX);
  size_t o = 0;
  L.off_T = o; o = align256(o + fill_workspace_bytes(p, chunk, B));
  L.off_P = o; o = align256(o + lu_workspace_bytes(chunk, L.n_pad, 0));
  L.total = o;
  return L;
}

// Flat layouts (every centre with the same last coordinate): A~ = diag(E, O) in the split order, factored as two blocks.  Whether this
// call takes the split form: `split` is set, or left off (SplitMap()).  The conditions that cost nothing come first; the centres come
// to the host only for calls that pass them (one small copy, one wait).
int flat_layout_split(const biem_plan* plan, int B, int nrhs, const double* d_centers, int geom_batched, hipStream_t st, SplitMap& split) {
  split = SplitMap();
  const int H = plan->H, d = plan->d;
  const char* e = getenv("BIEM_SYM_SPLIT");
  const SplitMap sm = make_split_map(B, H, (int)(plan->units.size() / 2));
  if ((e && e[0] == '0') || geom_batched || plan->tree == TREE_CAA || !fill_sym_red_form(plan, B) || sym_small_path(B * H, nrhs) ||
      !((e && e[0] == '1') || B * H >= SYM_SPLIT_MIN_N) || sm.U >= H || rhs_ld(nrhs) > sm.npO)
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
int factor_sym_blocks(int c, int nrhs, double* A, long long lda, long long sys_stride, const SymBlock* blocks, int n_blocks, void* Pw,
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

// the caller's factor array (n_pad rows of lda per system) and workspace, as biem_factor_ldlt* write and biem_solve_factored* read them
int check_factor_room(const char* who, long long lda, long long sys_stride, int n_pad, size_t work_bytes, size_t need) {
  if (lda < n_pad || sys_stride < (long long)n_pad * lda) { set_error("%s: lda=%lld < n_pad=%d or sys_stride=%lld < n_pad * lda", who, lda, n_pad, sys_stride); return BIEM_ERR_ARG; }
  if (work_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, need); return BIEM_ERR_ARG; }
  return BIEM_OK;
}

// blocks of ball pairs with the same displacement and the same (radius, alpha, beta) on either side are contracted once: the classes are
// keyed on one (alpha, beta) per ball, shared by all systems (degree-dependent coefficients: every pair on its own)
inline bool fill_may_dedupe(int geom_batched, const BoundaryCoef& bc) { return !geom_batched && !bc.batched && !bc.per_degree; }

// a degree with gj = 0 (a ball that does not scatter it) has no symmetric scaling: rejected whatever the factorisation reported
int flag_unscalable(const biem_plan* p, int c, int B, const BoundaryCoef& bc, const double* tab, int* info, int n_pad, hipStream_t st) {
  return bc.per_degree ? launch_flag_unscalable(p, c, B, tab, info, -(n_pad + 2), st) : BIEM_OK;
}

// Where the right-hand sides of c systems live: f is the first entry of the first system, row r of system s at f + 2 (s sys_stride + r ld)
// (complex128); the columns n_pad .. of an augmented matrix, or an array of their own.  Rows in the slot order of the symmetric form.
struct RhsView { double* f; long long sys_stride, ld; int n_pad; SplitMap split; };
// load: the right-hand sides of the systems s0 .. s0 + c from their source, then f~ = R W^H f; unload: x = W R^-1 x~, then the density
int rhs_load(const biem_plan* p, int s0, int c, int B, int nrhs, const BoundaryCoef& bc, const RhsSource& src, const double* tab,
             const RhsView& v, bool symmetric, hipStream_t st) {
  const size_t ab0 = (bc.per_degree && bc.batched) ? (size_t)s0 * B * p->n_end * 2 : 0;
  const BoundaryCoef bcs = {bc.alpha + ab0, bc.beta + ab0, bc.batched, bc.per_degree};   // (read by the per-degree projection only)
  const int rc = src.at(p, s0, nrhs, B).launch(p, c, B, nrhs, bcs, tab, v.f, v.sys_stride, v.ld, 1, st, symmetric, v.split);
  return (rc || !symmetric) ? rc : launch_sym_rhs(p, c, B, nrhs, v.n_pad, tab, v.f, v.ld, v.sys_stride, false, st, v.split);
}
int rhs_unload(const biem_plan* p, int c, int B, int nrhs, const double* tab, const RhsView& v, bool symmetric, double* density, hipStream_t st) {
  const int rc = symmetric ? launch_sym_rhs(p, c, B, nrhs, v.n_pad, tab, v.f, v.ld, v.sys_stride, true, st, v.split) : BIEM_OK;
  return rc ? rc : launch_density(p, c, B, nrhs, v.f, v.sys_stride, v.ld, 1, tab, density, st, symmetric, v.split);
}
}  // namespace

int ball_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                const BoundaryCoef& bc, double* d_tab, hipStream_t st) {
  return bc.per_degree ? launch_ball_tables_n(p, nb, B, d_k, d_eta, d_radii, geom_batched, bc.alpha, bc.beta, bc.batched, d_tab, st)
                       : launch_ball_tables(p, nb, B, d_k, d_eta, d_radii, geom_batched, bc.alpha, bc.beta, bc.batched, d_tab, st);
}

int RhsSource::check(const char* who, const biem_plan* p, int nb, int nrhs) const {
  if (!closed_form()) return BIEM_OK;
  if (nb > 65535 || nrhs > 65535) { set_error("%s: at most 65535 systems / right-hand sides per call (got nb=%d, nrhs=%d)", who, nb, nrhs); return BIEM_ERR_ARG; }
  if (kind == POINT_SOURCES && p->n_end > kMaxRad) {
    set_error("%s: n_end=%d exceeds the built table size %d of the point-source right-hand side", who, p->n_end, kMaxRad);
    return BIEM_ERR_UNSUPPORTED;
  }
  if (translated()) {
    // tree a: the radial row of a (source, ball) pair in LDS, orders < 2 n_end - 1; every other tree: the term lists, built up to half that.
    // Expansions: the same limits on the plan whose lists and labels they read
    const biem_plan* t = table_plan(p);
    const char* what = kind == REGULAR_WAVES ? "regular-wave" : kind == MULTIPOLE_SOURCES ? "multipole" : "expansion";
    if (t->tree == TREE_A ? t->n_end > kMaxRad : 2 * t->n_end > kMaxRad) {
      set_error("%s: n_end=%d exceeds the built table size %d of the %s right-hand side", who, t->n_end, t->tree == TREE_A ? kMaxRad : kMaxRad / 2, what);
      return BIEM_ERR_UNSUPPORTED;
    }
    if (t->tree != TREE_A && (!t->lists_built || t->ptr.empty() || !t->d_ptr)) {
      set_error("%s: the plan has no translation term lists", who);
      return BIEM_ERR_UNSUPPORTED;
    }
  }
  return BIEM_OK;
}

int RhsSource::launch(const biem_plan* p, int nb, int B, int nrhs, const BoundaryCoef& bc, const double* d_tab, double* d_f, long long sys_stride,
                      long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split) const {
  switch (kind) {
    case SAMPLES:
      return launch_rhs_project(p, nb, B, nrhs, g[0], d_f, sys_stride, elem_stride, rhs_stride, st, slot_order, split);
    case SAMPLES_N:
      return launch_rhs_project_n(p, nb, B, nrhs, g[0], g[1], bc.alpha, bc.beta, bc.batched, d_f, sys_stride, elem_stride, rhs_stride, st,
                                  slot_order, split);
    case PLANE_WAVES:
      return launch_rhs_plane_wave(p, nb, B, nrhs, k, centers, geom_batched, d_tab, pts, pts_batched, d_f, sys_stride, elem_stride,
                                   rhs_stride, st, slot_order, split, work);
    case POINT_SOURCES:
      return launch_rhs_point_source(p, nb, B, nrhs, k, centers, geom_batched, d_tab, pts, pts_batched, d_f, sys_stride, elem_stride,
                                     rhs_stride, st, slot_order, split, work);
    case MULTIPOLE_SOURCES:
    case REGULAR_WAVES:
      return launch_rhs_multipole(p, nb, B, nrhs, k, centers, geom_batched, d_tab, pts, pts_batched, idx, d_f, sys_stride, elem_stride,
                                  rhs_stride, st, slot_order, split, work, kind == REGULAR_WAVES);
    case REGULAR_EXPANSION:
    case MULTIPOLE_EXPANSION:
      return launch_rhs_expansion(p, table_plan(p), map, n_in, kind == REGULAR_EXPANSION, nb, B, nrhs, k, centers, geom_batched, d_tab, pts,
                                  pts_batched, n_origin, coef, coef_batched, d_f, sys_stride, elem_stride, rhs_stride, st, slot_order, split, 0,
                                  work);
  }
  return BIEM_ERR_ARG;
}

size_t solve_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int chunk) { return make_layout(p, nb, B, nrhs, chunk).total; }
size_t factor_workspace_bytes(const biem_plan* p, int nb, int B, int chunk) { return make_factor_layout(p, nb, B, chunk).total; }
size_t solve_factored_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs) {
  return (size_t)nb * lu_npad(B * p->H) * rhs_ld(nrhs) * sizeof(cplx);
}
void last_solve_split(int* npE, int* npO) {
  if (npE) *npE = g_last_split[0];
  if (npO) *npO = g_last_split[1];
}

int solve_path(const char* who, const biem_plan* plan, int nb, int B, int nrhs, const double* d_k, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const BoundaryCoef& bc, const RhsSource& source, double* d_density, int* d_info, int chunk,
               void* d_work, size_t work_bytes, hipStream_t st, bool symmetric) {
  RhsSource src = source;
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_centers, "d_centers"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, bc.alpha, bc.alpha_name()); NEED_AS(who, bc.beta, bc.beta_name());
  if (src.kind == RhsSource::SAMPLES) NEED_AS(who, src.g[0], "d_g");
  NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_info, "d_info"); NEED_AS(who, d_work, "d_work");
  if (nb <= 0 || B <= 0) return BIEM_OK;
  if (nrhs < 1) { set_error("%s: nrhs < 1", who); return BIEM_ERR_ARG; }
  if (const int rc = src.check(who, plan, nb, nrhs)) return rc;
  const int H = plan->H;
  SplitMap sm = SplitMap();                // (off: the pivoted LU has no split form)
  if (symmetric) {
    g_last_split[0] = g_last_split[1] = 0;
    if (const int rc = flat_layout_split(plan, B, nrhs, d_centers, geom_batched, st, sm)) return rc;
  }
  const bool split = sm.on();
  const SolveLayout L = make_layout(plan, nb, B, nrhs, chunk, split);
  const size_t need = L.total + src.work_bytes(plan, nb, B, nrhs);    // (a source in closed form keeps its harmonics at the tail)
  if (work_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, need); return BIEM_ERR_ARG; }
  if (split) { g_last_split[0] = sm.npE; g_last_split[1] = sm.npO; }
  char* w = (char*)d_work;
  src.work = w + L.total;
  double* tab = (double*)(w + L.off_tab);
  double* A = (double*)(w + L.off_A);
  void* T = w + L.off_T;
  void* Pw = w + L.off_P;
  int* ipiv = (int*)(w + L.off_ipiv);
  int* info_O = (int*)(w + L.off_info2);
  if (const int rc = ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, bc, tab, st)) return rc;
  // small systems are solved in one LDS-resident launch that never reads the padding rows / columns: they are not written then
  const bool small = symmetric && sym_small_path(L.N, nrhs);
  const FillDedupe dd = {d_radii, bc.alpha, bc.beta};
  const RhsView rhs = {A + (size_t)L.n_pad * 2, L.sys_stride, L.lda, L.n_pad, sm};   // column n_pad of the augmented matrix
  return for_each_chunk(plan, nb, B, L.chunk, d_k, d_centers, geom_batched, tab, [&](const Chunk& ch) {
    const int c = ch.c;
    int* info = d_info + ch.s0;
    int rc;
    if (split)
      // E's right-hand-side columns lie inside the O rows' matrix columns: they are cleared for all rows BEFORE the fill writes O
      launch_clear_cols(st, A + (size_t)sm.npE * 2, L.lda, L.lda - L.n_pad, (long long)L.n_pad * c);
    if (symmetric)
      rc = launch_fill_sym(plan, c, B, ch.k, ch.centers, geom_batched, ch.tab, A, L.lda, L.sys_stride, L.n_pad, T, fill_workspace_bytes(plan, c, B), st,
                           small, fill_may_dedupe(geom_batched, bc) ? &dd : nullptr, sm);
    else
      rc = launch_fill(plan, c, B, ch.k, ch.centers, geom_batched, ch.tab, BIEM_FILL_EQUILIBRATED, A, L.lda, L.sys_stride, L.n_pad, T,
                       fill_workspace_bytes(plan, c, B), st);
    if (rc) return rc;
    if (!small) launch_clear_cols(st, rhs.f, L.lda, L.lda - L.n_pad, (long long)L.n_pad * c);
    if ((rc = rhs_load(plan, ch.s0, c, B, nrhs, bc, src, ch.tab, rhs, symmetric, st))) return rc;
    if (symmetric) {
      // the existing factorisation on the whole matrix, or on two views of the one allocation, E then O
      const SymBlock whole[1] = {{0, L.n_pad, L.N, info}};
      const SymBlock halves[2] = {{0, sm.npE, B * sm.U, info}, {2 * ((size_t)sm.npE * L.lda + sm.npE), sm.npO, B * (H - sm.U), info_O}};
      rc = factor_sym_blocks(c, nrhs, A, L.lda, L.sys_stride, split ? halves : whole, split ? 2 : 1, Pw, st);
      if (!rc) rc = flag_unscalable(plan, c, B, bc, ch.tab, info, L.n_pad, st);
    } else
      rc = launch_lu_factor_solve(c, L.n_pad, nrhs, A, L.lda, L.sys_stride, ipiv, info, Pw, lu_workspace_bytes(c, L.n_pad, nrhs), st,
                                  /*keep_multipliers=*/false, false, false);   // the fused path only needs the solution
    if (rc) return rc;
    return rhs_unload(plan, c, B, nrhs, ch.tab, rhs, symmetric, d_density + (size_t)ch.s0 * nrhs * B * H * 2, st);
  });
}

int factor_path(const char* who, const biem_plan* plan, int nb, int B, const double* d_k, const double* d_eta, const double* d_centers,
                const double* d_radii, int geom_batched, const BoundaryCoef& bc, double* d_F, long long lda, long long sys_stride,
                double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes, hipStream_t st) {
  NEED_DEV_AS(who, plan); NEED_AS(who, d_k, "d_k"); NEED_AS(who, d_eta, "d_eta"); NEED_AS(who, d_centers, "d_centers"); NEED_AS(who, d_radii, "d_radii");
  NEED_AS(who, bc.alpha, "d_alpha"); NEED_AS(who, bc.beta, "d_beta"); NEED_AS(who, d_F, "d_F"); NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_info, "d_info"); NEED_AS(who, d_work, "d_work");
  if (nb < 0 || nb > 65535 || B < 0) { set_error("%s: 0 .. 65535 systems per call and B >= 0 (got nb=%d, B=%d)", who, nb, B); return BIEM_ERR_ARG; }
  if (nb == 0 || B == 0) return BIEM_OK;
  const FactorLayout L = make_factor_layout(plan, nb, B, chunk);
  if (const int rc = check_factor_room(who, lda, sys_stride, L.n_pad, work_bytes, L.total)) return rc;
  void* T = (char*)d_work + L.off_T;
  void* Pw = (char*)d_work + L.off_P;
  if (const int rc = ball_tables(plan, nb, B, d_k, d_eta, d_radii, geom_batched, bc, d_tab, st)) return rc;
  const FillDedupe dd = {d_radii, bc.alpha, bc.beta};
  return for_each_chunk(plan, nb, B, L.chunk, d_k, d_centers, geom_batched, d_tab, [&](const Chunk& ch) {
    double* A = d_F + 2 * (size_t)ch.s0 * sys_stride;
    // identity padding written (no_padding = false) even where the one-launch path factors the active rows only: the solve runs
    // over all n_pad rows and finds U = I there
    int rc = launch_fill_sym(plan, ch.c, B, ch.k, ch.centers, geom_batched, ch.tab, A, lda, sys_stride, L.n_pad, T, fill_workspace_bytes(plan, ch.c, B), st,
                             false, fill_may_dedupe(geom_batched, bc) ? &dd : nullptr);
    if (rc) return rc;
    const SymBlock whole[1] = {{0, L.n_pad, L.N, d_info + ch.s0}};      // (growth preset as in the fused solve)
    rc = factor_sym_blocks(ch.c, 0, A, lda, sys_stride, whole, 1, Pw, st);
    return rc ? rc : flag_unscalable(plan, ch.c, B, bc, ch.tab, d_info + ch.s0, L.n_pad, st);
  });
}

int solve_factored_path(const char* who, const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                        const double* d_tab, const BoundaryCoef& bc, const RhsSource& source, double* d_density, void* d_work, size_t work_bytes,
                        hipStream_t st) {
  RhsSource src = source;
  NEED_DEV_AS(who, plan); NEED_AS(who, d_F, "d_F"); NEED_AS(who, d_tab, "d_tab"); NEED_AS(who, d_density, "d_density"); NEED_AS(who, d_work, "d_work");
  if (src.closed_form()) { NEED_AS(who, src.k, "d_k"); NEED_AS(who, src.centers, "d_centers"); }
  else if (src.kind == RhsSource::SAMPLES_N) { NEED_AS(who, bc.alpha, bc.alpha_name()); NEED_AS(who, bc.beta, bc.beta_name()); }
  else NEED_AS(who, src.g[0], "d_g");
  if (const int rc = check_counts(who, nb, nrhs, B)) return rc;
  if (nb == 0 || nrhs == 0 || B == 0) return BIEM_OK;
  if (const int rc = src.check(who, plan, nb, nrhs)) return rc;
  const int n_pad = lu_npad(B * plan->H);
  const size_t need = solve_factored_workspace_bytes(plan, nb, B, nrhs);
  if (const int rc = check_factor_room(who, lda, sys_stride, n_pad, work_bytes, need + src.work_bytes(plan, nb, B, nrhs))) return rc;
  src.work = (char*)d_work + need;                                 // (a source in closed form keeps its harmonics at the tail)
  // right-hand sides X[s][row][q] (row-major, ldx columns), rows in the slot order of the symmetric form; padding rows zero
  const long long ldx = rhs_ld(nrhs);
  const RhsView X = {(double*)d_work, (long long)n_pad * ldx, ldx, n_pad, SplitMap()};
  BIEM_HIPCHK(hipMemsetAsync(X.f, 0, need, st));
  int rc = rhs_load(plan, 0, nb, B, nrhs, bc, src, d_tab, X, true, st);
  if (rc) return rc;
  rc = launch_sym_solve(nb, n_pad, nrhs, d_F, lda, sys_stride, X.f, X.ld, X.sys_stride, st);
  return rc ? rc : rhs_unload(plan, nb, B, nrhs, d_tab, X, true, d_density, st);
}

}  // namespace biem
