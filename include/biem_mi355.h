/*
 * biem_mi355.h  --  C ABI of libbiem_mi355.so: the biem() dense assembly-and-solve hot path on MI355X.
 *
 * The reference (ultrasphere-dev/biem-helmholtz-sphere v1.2.0) is pure Python and has no FFI; the
 * boundary it offers for this path is the Python signature of biem() (src/biem_helmholtz_sphere/
 * _biem.py:453-469).  Every entry point below replaces a span of that function (or of biem_u) and
 * cites it.  The host layer (biem_helmholtz_sphere_amd/_biem.py) binds these with ctypes; what a
 * maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++/torch types; all sizes are int / long long / size_t; complex128 = 2 doubles.
 *   - pointers named d_* are DEVICE pointers (HIP, gfx950) owned by the caller; h_* are host pointers.
 *   - every function returns a status (0 = BIEM_OK) and never throws; text via biem_last_error().
 *   - all device work is enqueued on the caller-supplied hipStream_t (passed as void*), nothing
 *     synchronises unless stated; the library keeps no global mutable state (error text is
 *     thread-local).  Workspaces are caller-allocated; sizes come from the *_bytes functions.
 *   - `nb` = number of independent (k, eta, incidence) systems in the call (the batch "..." of
 *     _biem.py:80-91), B = balls, H = harmonics of degree < n_end per ball, N = B*H,
 *     Npad = N rounded up (biem_lu_npad) - the LU works on an identity-padded Npad x Npad system.
 *   - order of the harm axis: see biem_plan_labels (this project's choice; the reference's order is
 *     decided inside un-vendored ush.flatten_harmonics and is not pinned by any fixture).
 */
#ifndef BIEM_MI355_H
#define BIEM_MI355_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define BIEM_OK 0
#define BIEM_ERR_ARG 1          /* bad argument (shape, null pointer, flag) */
#define BIEM_ERR_HIP 2          /* a HIP runtime call failed */
#define BIEM_ERR_UNSUPPORTED 3  /* coordinate tree / size not built */
#define BIEM_ERR_ALLOC 4
#define BIEM_ERR_NO_DEVICE 5    /* no gfx950 device visible */

/* coordinate trees (ultrasphere.create_from_branching_types strings) */
#define BIEM_TREE_A 0    /* "a"   d=2 */
#define BIEM_TREE_BA 1   /* "ba"  d=3, polar axis x0 */
#define BIEM_TREE_BBA 2  /* "bba" d=4 */
#define BIEM_TREE_CAA 3  /* "caa" d=4, Hopf-type: x0 = r cos t0 cos t1, x1 = r cos t0 sin t1, x2 = r sin t0 cos t2, x3 = r sin t0 sin t2 */

/* fill scalings */
#define BIEM_FILL_REFERENCE 0    /* A = blc_{n'} * { diag(alpha h + beta k h') | (S|R)^T (alpha j + beta k j') }  (_biem.py:745-792) */
#define BIEM_FILL_EQUILIBRATED 1 /* M = I + (S|R)^T (alpha j+beta k j')_row / (alpha h+beta k h')_col : what the LU factors */
#define BIEM_FILL_SYMMETRIC 2    /* A~ = R W^H M W R^-1, complex symmetric (W: unitary map to real harmonics, R = diag(1/sqrt(gj gh))):
                                    what the symmetric path factors.  Rows / columns of a ball in the internal slot order of
                                    biem_plan_symmetric_order; ONLY the upper triangle and the diagonal 64 x 64 tiles are written
                                    (n_pad must be a multiple of 64, lda >= n_pad); everything else is left untouched.  That is the input of
                                    biem_sym_factor_solve (row form, upper triangle) ONLY: biem_ldlt_factor / biem_ldlt_factor_solve read the
                                    LOWER triangle, which this fill does not write */

/* uscat flags */
#define BIEM_USCAT_FAR_FIELD 1
#define BIEM_USCAT_PER_BALL 2
#define BIEM_USCAT_KIND_INNER 4
#define BIEM_USCAT_POINTS_BATCHED 8 /* points carry their own batch axis (expand_x=False, _biem.py:879-883) */

typedef struct biem_plan biem_plan; /* opaque: host+device tables of one (tree, n_end) */

int biem_version(void);
/* hash of the csrc/ + include/ sources the library was built from (the Python loader rebuilds a library whose hash differs) */
const char* biem_build_id(void);
const char* biem_last_error(void);
/* number of visible HIP devices; BIEM_ERR_NO_DEVICE if none */
int biem_device_count(int* n);

/* ---- plan: k- and geometry-independent tables (replaces the table side of ush.expand /
 *      ush.harmonics_translation_coef / ush.index_array_harmonics, _biem.py:627,651,697,720) ---- */
/* host-only tables (no GPU needed): labels, quadrature, projection matrix, translation terms */
int biem_plan_create_host(int tree, int n_end, biem_plan** plan);
/* upload the tables to the current HIP device (idempotent) */
int biem_plan_upload(biem_plan* plan);
/* = create_host + upload */
int biem_plan_create(int tree, int n_end, biem_plan** plan);
/* the standard chain tree "b" * (d - 2) + "a" of dimension d (3 <= d <= 10; d = 3, 4 give the labels and rules of ba / bba through
 * the generic chain code): harmonics Y = prod_j sin^{l_{j+1}} t_j Gbar_{l_j - l_{j+1}}^{(l_{j+1} + (d-j-2)/2)}(cos t_j) e^{i m phi} / sqrt(2 pi)
 * (Gbar: orthonormal Gegenbauer, no Condon-Shortley phase), boundary rule = n_end-point Gauss-Jacobi((d-j-3)/2, (d-j-3)/2) per polar
 * node x 2 n_end azimuths.  Orders whose tables pass a 16-bit index or LDS limit fail with BIEM_ERR_UNSUPPORTED naming it. */
int biem_plan_create_chain_host(int d, int n_end, biem_plan** plan);
int biem_plan_create_chain(int d, int n_end, biem_plan** plan);
int biem_plan_destroy(biem_plan* plan);
/* d, H (degree < n_end), Q quadrature points per ball, H2 (degree < 2 n_end - 1), number of translation terms */
int biem_plan_info(const biem_plan* plan, int* d, int* n_harm, int* n_quad, int* n_harm2, long long* n_terms);
/* h_labels[H][3]: a:(m,0,0)  ba:(n,m,0)  bba:(n,l,m)  caa:(n,m1,m2);  h_deg[H]: degree n */
/* (a chain plan - biem_plan_create_chain - has wider labels: BIEM_ERR_UNSUPPORTED, nothing is written) */
int biem_plan_labels(const biem_plan* plan, int* h_labels, int* h_deg);
/* h_labels[H][width], width >= the plan's label width (3; chain plans: d - 1), entries beyond it 0.  Chain labels:
 * (n = l_0 >= l_1 >= ... >= l_{d-3} >= |m|, m) in n-major order (l_1 from 0 to n, then the next entry, ..., m from -l to l) */
int biem_plan_labels_n(const biem_plan* plan, int width, int* h_labels, int* h_deg);
/* the real-harmonic form used by the symmetric path: h_partner[h] = p with conj Y_h = Y_p (p == h: a real harmonic); h_slot[h] =
 * internal position of harmonic h among its ball's H unknowns in that path: for a unit (h <= p) the "cosine" combination
 * (Y_h + Y_p)/sqrt2 sits in slot h_slot[h], the "sine" combination i (Y_p - Y_h)/sqrt2 in slot h_slot[p] */
int biem_plan_symmetric_order(const biem_plan* plan, int* h_partner /*[H]*/, int* h_slot /*[H]*/);
/* the split layout of the symmetric path for B balls (host information).  For the chain trees (a, ba, bba, b...ba) the cosine slots
 * are even and the sine slots odd under reflection of the LAST coordinate, so with every centre at the same last coordinate A~ couples
 * no cosine slot to a sine slot: it is diag(E, O) once the balls' cosine runs (n_cos slots each) are collected in rows [0, nE) and their
 * sine runs in rows [npE, npE + nO); npE, npO = nE, nO rounded up to whole 64-row tiles.  h_row[b][slot] = row of unknown (b, slot).
 * Any output may be null. */
int biem_plan_split_order(const biem_plan* plan, int B, int* n_cos, int* nE, int* nO, int* npE, int* npO, int* h_row /*[B][H]*/);
/* which forms of the symmetric fill this plan's tables admit (host information, no device needed): n_units = label units E of the
 * reduced pair table (a degree < 2 n_end - 1 label and its conjugate partner share an entry), n_phases = distinct azimuthal phases,
 * reduced_ok = 1 if every term list is of one kind and one phase and a wave's lists fit LDS (the default fill kernel), lds_rows =
 * term rows (64 lanes each) of its largest chunk, gather_ok = 1 if the gather form it replaced fits */
int biem_plan_fill_info(const biem_plan* plan, int* n_units, int* n_phases, int* reduced_ok, int* lds_rows, int* gather_ok);
/* unit vectors y[Q][d] and weights w[Q] of the boundary-data rule (ush.expand(n=n_end)) */
int biem_plan_quadrature(const biem_plan* plan, double* h_y, double* h_w);
/* projection matrix W[Q][H] (complex128, host copy):  f_h = sum_q W[q][h] g(y_q),  W = w_q conj(Y_h(y_q)) */
int biem_plan_projection(const biem_plan* plan, double* h_W);
/* translation terms in CSR over entries e = h*H + h' (row h = test index, column h' = unknown):
 * (S|R)_{h'->h}(t) = sum_{p in [ptr[e],ptr[e+1])} coef[p] * T[tidx[p]],  T[l] = C_d h_{n''}(k|t|) Y_l(t^), l over labels of degree < 2 n_end - 1 */
int biem_plan_terms(const biem_plan* plan, long long* h_ptr /*[H*H+1]*/, double* h_coef, int* h_tidx);
/* the term list of ONE entry (row h_row, column h_col: the slice [ptr[e], ptr[e+1]) of biem_plan_terms at e = h_row*H + h_col) of
 * tree bba (2) or caa (3) at order n_end (1 .. 64), by the code the plan build runs but without building a plan (host only; a plan at
 * n_end 22 holds hundreds of millions of terms).  *n_terms = terms of the entry; they are written while n_terms <= capacity, otherwise
 * BIEM_ERR_ARG and nothing is written.  The integral tables of the last (tree, n_end) are kept between calls. */
int biem_plan_entry_terms(int tree, int n_end, int h_col, int h_row, int capacity, int* n_terms, double* h_coef, int* h_tidx);
/* coupling table of the radiation force, T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega, in CSR over the rows h': entry p in
 * [ptr[h'], ptr[h'+1]) is T^{comp[p]}_{h', col[p]} = val[p] (complex128), ordered by (component, column) within a row.  Hermitian in
 * (h', h), entries only where |n - n'| = 1.  Built on the first request (this call or biem_force; host work only unless the plan is
 * uploaded, then its device mirror too), so plans that never compute a force keep their build time and memory.  Any array may be null;
 * n_entries alone sizes the others. */
int biem_plan_force_terms(biem_plan* plan, long long* n_entries, long long* h_ptr /*[H+1]*/, int* h_col, int* h_comp, double* h_val);

/* ---- special functions on the device, exposed for parity tests (ultrasphere.shn1 / potential_coef) ---- */
/* z[i][0..nmax] (j) and [nmax+1 .. 2nmax+1] (y): d-dimensional spherical Bessel functions at x[i] */
int biem_radial(int d, int nmax, int count, const double* d_x, double* d_out /*[count][2][nmax+1]*/, void* stream);
/* complex arguments z[i] (complex128): out[i][0][n] = z_n regular, out[i][1][n] = h_n = j_n + i y_n outgoing (complex128);
 * h is computed directly (closed forms / modified Bessel functions), never as the cancelling sum j + i y */
int biem_radial_complex(int d, int nmax, int count, const double* d_z /*[count] c128*/, double* d_out /*[count][2][nmax+1] c128*/,
                        void* stream);
/* Y[p][h] (complex128) at directions d_u[p][d] (need not be normalised) for all labels of degree < n_end */
int biem_harmonics(const biem_plan* plan, int count, const double* d_u, double* d_Y /*[count][H] c128*/, void* stream);

/* ---- wavenumbers: every d_k below is [nb] COMPLEX128 (re, im interleaved), the reference's k of dtype result_type(k, complex)
 *      (gui.py:296-301 passes complex k); systems with Im k == 0 take the real-argument special functions. ---- */
/* ---- per-ball tables (ush.harmonics_regular_singular_component + potential_coef, _biem.py:723-789) ----
 * d_tab[nb][B][3][n_end] complex128: [0] gj = alpha j_n + beta k j_n', [1] gh = alpha h_n + beta k h_n', [2] blc_n = dlc - i eta slc
 * geometry arrays are [nb][B]... when geom_batched != 0, else [B]... shared by all systems; alpha/beta likewise (ab_batched). */
int biem_ball_tables(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_eta,
                     const double* d_radii, int geom_batched, const double* d_alpha /*c128*/, const double* d_beta /*c128*/,
                     int ab_batched, double* d_tab, void* stream);

/* ---- right-hand side (ush.expand, _biem.py:627-639): the incident field stays a Python callable; only its samples
 *      g[s][r][b][q] = (-alpha u_in - beta d_n u_in)(c_b + rho_b y_q) cross the ABI; r = 0..nrhs-1 are right-hand sides that
 *      share system s (incidences on which k, eta, the geometry and alpha/beta do not depend: factor once, solve many).
 *      f element (s, r, b, h) is written to d_f[s*sys_stride + (b*H + h)*elem_stride + r*rhs_stride]  (complex128 units).
 *      The nb*nrhs*B rows run in blocks of 8 on one flat grid dimension (biem_rhs_project_n: blocks of 4), not on a dimension of 65535. ---- */
int biem_rhs_project(const biem_plan* plan, int nb, int B, int nrhs, const double* d_g /*[nb][nrhs][B][Q] c128*/, double* d_f,
                     long long sys_stride, long long elem_stride, long long rhs_stride, void* stream);

/* ---- matrix fill (ush.harmonics_translation_coef + the where/create_diagonal/moveaxis block, _biem.py:694-792) ----
 * Writes the N x N matrix of every system, row-major [b][h][b'][h'] with leading dimension lda (complex128 units),
 * system s at d_A + 2*s*sys_stride doubles.  When lda > N / rows_pad > N the caller gets an identity-padded
 * Npad x Npad block (columns >= Npad are left untouched: that is where the LU keeps right-hand sides).
 * d_tab from biem_ball_tables.  Workspace: biem_fill_workspace_bytes. */
size_t biem_fill_workspace_bytes(const biem_plan* plan, int nb, int B);
int biem_fill(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_centers /*[nb or 1][B][d]*/,
              int geom_batched, const double* d_tab, int scaling, double* d_A, long long lda, long long sys_stride,
              int n_pad, void* d_work, size_t work_bytes, void* stream);

/* ---- dense complex LU (batch_tensorsolve.btensorsolve -> linalg.solve, _biem.py:797) ----
 * Right-looking blocked LU with partial (row) pivoting in groups of four 64-column panels; trailing updates are 3M zgemm
 * (K = 64 / 128 inside a group, one K = 256 update per group) on v_mfma_f64_4x4x4_4b_f64.
 * The system is the augmented row-major [A | F]: Npad rows, Npad + nrhs columns, leading dimension lda >= Npad + nrhs.
 * biem_lu_factor_solve overwrites F with the solution (forward elimination rides in the trailing update, then a
 * blocked back substitution); A is overwritten by U and the un-permuted multipliers. */
int biem_lu_npad(int N);
size_t biem_lu_workspace_bytes(int nb, int n_pad, int nrhs);   /* panels of a group + 64 x 64 block per system + tile map of the symmetric path + its 256 x 64 slab per system */
int biem_lu_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride,
                         int* d_ipiv /*[nb][n_pad]*/, int* d_info /*[nb]*/, void* d_work, size_t work_bytes, void* stream);

/* Factor now, solve later (the reference's btensorsolve has no such split: linalg.solve factors again for every call, _biem.py:797).
 * biem_lu_factor leaves in A the factor U (on and above the diagonal) and the multipliers (below), d_ipiv the interchanges:
 * row j was exchanged with row ipiv[j] >= j when column j was eliminated; the multipliers of a 64-column panel are stored in the
 * row order that panel's own interchanges left (LINPACK style: later interchanges are NOT applied to earlier multipliers), which
 * is what biem_lu_solve expects.  biem_lu_solve overwrites B (row-major [Npad][ldb] per system, nrhs <= ldb columns, system s at
 * d_B + 2*s*b_stride doubles; rows N..Npad-1 of an identity-padded system must hold zeros) with the solutions; it needs no
 * workspace and may be called any number of times.  d_info as in biem_lu_factor_solve. */
int biem_lu_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_ipiv /*[nb][n_pad]*/, int* d_info /*[nb]*/,
                   void* d_work, size_t work_bytes /* biem_lu_workspace_bytes(nb, n_pad, 0) */, void* stream);
int biem_lu_solve(int nb, int n_pad, int nrhs, const double* d_LU, long long lda, long long sys_stride, const int* d_ipiv,
                  double* d_B, long long ldb, long long b_stride, void* stream);
/* the same split for complex-symmetric systems (see biem_ldlt_factor_solve below): A <- L (unit lower, below the diagonal) and
 * U = D L^T (on and above), ipiv = identity; solve with biem_lu_solve.  d_info[s] < 0: rejected, use biem_lu_factor. */
int biem_ldlt_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_ipiv, int* d_info, void* d_work,
                     size_t work_bytes, void* stream);

/* Complex-SYMMETRIC systems (A = A^T, not Hermitian): A = L D L^T with the diagonal as pivots, no interchanges.  Same layout,
 * workspace and kernels as biem_lu_factor_solve; a panel's U rows are its transposed multipliers and the K = 256 updates run
 * over the lower triangle of tiles only (half the flops).  Only the lower triangle (and the diagonal 64 x 64 blocks) of A is
 * read.  d_info[s] = -(row+1), `row` = first row of the 64-column panel in which a diagonal entry was below 0.01 x the largest
 * entry of its (updated) column, i.e. a multiplier exceeded 100 (partial pivoting guarantees 1; 10 until round 2; or NaN);
 * d_info[s] = -(Npad+1): a-posteriori growth check failed, max |U| > 200 max |A| (|.| = |re| + |im|, A = the part read) or a
 * non-finite entry in U: the result of that system is not to be trusted and the caller re-solves it with biem_lu_factor_solve. */
int biem_ldlt_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride,
                           int* d_ipiv /*[nb][n_pad], identity on return*/, int* d_info /*[nb]*/, void* d_work, size_t work_bytes,
                           void* stream);

/* The same systems in ROW form, which is what biem_solve_ldlt runs: A = U^T U, U upper triangular (the complex-symmetric analogue
 * of Cholesky: U = D^{1/2} L^T with the L, D above; principal complex square roots, no conjugation, no interchanges).  Both
 * operands of every trailing update come from a 64-row strip of the row-major matrix itself, so the factorisation works in place
 * on the UPPER triangle: only the upper triangle and the diagonal 64 x 64 tiles of A are read; on return they hold U, the
 * augmented columns the solutions.  Same workspace size, d_info codes (rejected multiplier: -(first row of the 64-row panel + 1);
 * growth: -(Npad + 1)) and acceptance tests as biem_ldlt_factor_solve. */
int biem_sym_factor_solve(int nb, int n_pad, int nrhs, double* d_A, long long lda, long long sys_stride, int* d_info /*[nb]*/,
                          void* d_work, size_t work_bytes, void* stream);
/* biem_sym_factor_solve for systems of n_active <= n_pad unknowns (1 <= n_active): rows and columns n_active .. n_pad-1 of every
 * system are identity padding (the caller's promise) and the right-hand sides' padding rows are zero.  Where the whole system fits
 * the one-launch LDS-resident path (n_active <= 128, nrhs <= 8, n_active + nrhs <= 128; what biem_solve_ldlt runs for small
 * systems) the padding rows and columns are neither read nor written; otherwise the blocked factorisation runs over all n_pad
 * rows as biem_sym_factor_solve does.  Arguments, workspace and d_info as biem_sym_factor_solve. */
int biem_sym_factor_solve_n(int nb, int n_pad, int n_active, int nrhs, double* d_A, long long lda, long long sys_stride,
                            int* d_info /*[nb]*/, void* d_work, size_t work_bytes, void* stream);
/* Form of the bulk update biem_sym_factor_solve runs for a call of this shape (host only, no GPU work): 1 = left-looking (the rows of
 * a four-panel group take all pending updates of the finished rows in one K-long pass before the group is factored; every tile of the
 * matrix is read and written once by the bulk update), 0 = right-looking (a K = 256 update of everything below after every group).
 * Left runs when even its smallest launch, the last group's band, has a tile for every CU over the nb systems: 256 tiles, half the
 * update kernel's persistent grid of 512 workgroups.  BIEM_SYM_UPDATE=left|right in the environment forces a form; read per call. */
int biem_sym_update_form(int nb, int n_pad, int nrhs);
/* The whole form biem_sym_factor_solve_n takes for a call of this shape, and the layout of its workspace (host only, no GPU work;
 * either array may be null).  n_pad a multiple of 64, 1 <= n_active <= n_pad.
 *   form[BIEM_SYM_FORM_LEN] = one-launch small path (0 / 1), KR and TWO of its k_small_utu<KR, TWO> (0 off that path), bulk update
 *     left-looking, stacked group pass, right-hand sides in the compact copy, back substitution (0 rows, 1 column blocks, 2 block
 *     steps with the kept inverses), kept inverses (1 exactly with form 2), diagonal kernel with four pivots per barrier.
 *     Off the small path the fields behind KR and TWO are what the blocked path runs; on it they are not used.
 *   work[BIEM_SYM_WORK_LEN] = byte offsets of the regions of the biem_lu_workspace_bytes(nb, n_pad, nrhs) bytes, in order: the four
 *     panels, the 64 x 64 block per system, the tile map, the growth slots, 64 unused complex per system, the slab of the stacked pass;
 *     then the total; then what this form keeps in the panel region: offset and bytes of the kept inverses, offset and bytes of the
 *     compact copy of the right-hand sides (0 bytes: not used).
 * The environment switches BIEM_SYM_UPDATE, BIEM_SYM_GROUP, BIEM_BACK_FORM, BIEM_DIAG_FORM and BIEM_NO_SMALL_PATH enter as in a call. */
#define BIEM_SYM_FORM_LEN 9
#define BIEM_SYM_WORK_LEN 11
int biem_sym_form(int nb, int n_pad, int n_active, int nrhs, int* form, size_t* work);
/* The left-looking bulk update of the band at row J (a multiple of 256, 0 < J < n_pad) and the identity padding (host only, no GPU
 * work).  The last tile column of an n_pad system holds n_pad - n_active padding columns, where U is zero off the diagonal; of its
 * four 16-column groups only NF = ceil((64 - padding) / 16) need multiplying.  Returns NF in 1 .. 3 where the band's launch splits
 * that tile column off into a narrow launch (min(h, w) tiles per system: h = min(4, w) tile rows, w = n_pad / 64 - J / 64 tile
 * columns), and 4 where the launch stays whole: padding below 16 columns, or fewer than 512 narrow tiles over the nb systems unless
 * the last tile column is the whole band (w = 1).  It describes calls whose right-hand sides are not tile columns of the update
 * (nrhs <= 8); others stay whole.  BIEM_GEMM_NARROW=0 in the environment turns the split off, =1 drops the size rule only; read
 * per call. */
int biem_gemm_narrow_frags(int nb, int n_pad, int n_active, int J);
/* How the last biem_solve_ldlt / biem_solve_ldlt_n call of this thread ran: npE = npO = 0 unsplit, otherwise the padded orders of the
 * two blocks it factored one after the other (biem_plan_split_order).  The split form runs for shared geometry (geom_batched = 0) of a
 * chain tree whose centres all have the same last coordinate (compared bit for bit on the host, -0.0 as 0.0: one small copy and one
 * stream synchronisation, only for calls that pass every other condition), filled by the default fill form, N = B H >= 1024 and not on
 * the one-launch small path.  BIEM_SYM_SPLIT=0 in the environment disables it, =1 drops the size rule only; read per call.
 * Rejection codes are in the split layout's row numbers (O's rows shifted by npE), growth -(npE + npO + 1), unscalable -(npE + npO + 2).
 * biem_solve_workspace_bytes covers either form. */
int biem_last_solve_split(int* npE, int* npO);

/* density[s][r][b][h] = x / (gh * blc): the reference's `density` from the equilibrated unknowns (also the
 * single-ball shortcut _biem.py:648-691 with x = f).  x element (s, r, i) at d_x[s*sys_stride + i*elem_stride + r*rhs_stride]. */
int biem_density(const biem_plan* plan, int nb, int B, int nrhs, const double* d_x, long long sys_stride, long long elem_stride,
                 long long rhs_stride, const double* d_tab, double* d_density /*[nb][nrhs][B][H] c128*/, void* stream);

/* ---- field evaluation (biem_u, _biem.py:822-977) ----
 * d_points[d][P] (or [d][P][nb] with BIEM_USCAT_POINTS_BATCHED); out[P][nb] or [P][nb][B] (per ball), complex128.
 * Workspace: biem_uscat_workspace_bytes (holds density * blc). */
size_t biem_uscat_workspace_bytes(const biem_plan* plan, int nb, int B);
int biem_uscat(const biem_plan* plan, int nb, int B, int P, const double* d_k /*c128*/, const double* d_eta,
               const double* d_centers, const double* d_radii, int geom_batched, const double* d_density,
               const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* Cartesian gradient of the near field at the same points: out[d][P][nb] or [d][P][nb][B] (per ball), complex128, component i
 * along axis i of the plan's tree; NaN in every component where biem_uscat gives NaN.  Arguments, flags and workspace
 * (biem_uscat_workspace_bytes) as biem_uscat.  BIEM_USCAT_FAR_FIELD is BIEM_ERR_ARG (the far-field pattern is no field in
 * space).  Covered: trees a, ba, bba, caa up to the per-lane orders (n_end <= 320, 48, 14, 12; kind inner on tree a further while
 * a workgroup's 64 rows of n_end + 3 radial values fit the LDS); chain trees and larger orders are BIEM_ERR_UNSUPPORTED. */
int biem_uscat_grad(const biem_plan* plan, int nb, int B, int P, const double* d_k /*c128*/, const double* d_eta,
                    const double* d_centers, const double* d_radii, int geom_batched, const double* d_density,
                    const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* Hessian of the near field at the same points by a coefficient ladder: out[d (d + 1) / 2][P][nb] or [..][P][nb][B]
 * (per ball), complex128, the component pairs i <= j in row-major order along the axes of the plan's tree (the Hessian is symmetric:
 * the caller copies the lower triangle); NaN in every pair where biem_uscat gives NaN.  Arguments and flags as biem_uscat, with
 * one difference: `plan` is the plan of order n_end + 2, where n_end is the order of the density, and d_density[nb][B][H] is in THAT
 * plan's harmonic layout.  Only its degrees < n_end(plan) - 2 are read; the two top degrees are left free for the result (a
 * derivative of a multipole expansion is one degree longer) and may hold anything.  The plan is not const: the first call builds and
 * uploads its force coupling table (as biem_force does); no other table is added.
 * Workspace: biem_uscat_hess_workspace_bytes (d + 2 coefficient sets).  BIEM_USCAT_FAR_FIELD is BIEM_ERR_ARG (a pattern has no
 * Hessian in space), a plan of n_end < 3 too.  Covered: every tree and order biem_uscat covers at that plan - the chain trees and
 * orders above the per-lane ceilings included; what biem_uscat refuses there is BIEM_ERR_UNSUPPORTED with the order in the message. */
size_t biem_uscat_hess_workspace_bytes(const biem_plan* plan, int nb, int B);
int biem_uscat_hess(biem_plan* plan, int nb, int B, int P, const double* d_k /*c128*/, const double* d_eta,
                    const double* d_centers, const double* d_radii, int geom_batched, const double* d_density,
                    const double* d_points, int flags, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* ---- total field inside penetrable fluid balls ----
 * Ball b holds a fluid of wavenumber d_kint[b] and density d_delta[b] times the exterior's (what fluid_inclusion_bc takes; both
 * complex128, [nb][B] when fluid_batched != 0, else [B] shared by all systems).  With s = density blc_n the interior field is
 *   u_b(y) = sum_h a[b][h] j_n(k_b |y - c_b|) Y_h,   a = -s delta k W / gj_n,   W = i / (k rho)^{d-1},
 *   gj_n = alpha_n j_n(k rho) + beta_n k j_n'(k rho),   alpha_n = -k_b j_n'(k_b rho),   beta_n = delta j_n(k_b rho):
 * algebra on the solved density, no second solve.  biem_interior_coef writes the coefficients alone.  An entry that is not finite
 * (k_b NaN: an impenetrable ball; gj_n = 0 to rounding: a degree the ball does not scatter) is written as NaN.
 * biem_uinterior: d_points as biem_uscat; out[P][nb] complex128 = u_b where |y - c_b| < rho_b (the points biem_uscat masks), NaN at
 * every other point and inside a ball with a NaN coefficient.  flags: BIEM_USCAT_POINTS_BATCHED only, any other is BIEM_ERR_ARG.
 * Workspace: biem_uinterior_workspace_bytes (holds a).  Covered: trees a, ba, bba, caa up to the per-lane orders (n_end <= 320, 48,
 * 14, 12) while a workgroup's 64 rows of n_end + 2 radial values fit the LDS beside the kernel's own (tree a: n_end <= 152); chain trees, larger orders
 * and more than 65535 systems are BIEM_ERR_UNSUPPORTED with a message. */
int biem_interior_coef(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_kint /*[nb or 1][B] c128*/, const double* d_delta /*c128*/,
                       int fluid_batched, const double* d_density, double* d_a /*[nb][B][H] c128*/, void* stream);
size_t biem_uinterior_workspace_bytes(const biem_plan* plan, int nb, int B);
int biem_uinterior(const biem_plan* plan, int nb, int B, int P, const double* d_k /*c128*/, const double* d_eta,
                   const double* d_centers, const double* d_radii, int geom_batched, const double* d_kint /*[nb or 1][B] c128*/,
                   const double* d_delta /*c128*/, int fluid_batched, const double* d_density, const double* d_points, int flags,
                   double* d_out /*[P][nb]*/, void* d_work, size_t work_bytes, void* stream);

/* Cartesian gradient of that field at the same points: out[d][P][nb] complex128, component i along axis i of the plan's tree; NaN
 * in every component exactly where biem_uinterior gives NaN (a NaN coefficient poisons all components of its ball).  The centre of
 * a ball and points on the axes of the tree are ordinary points.  Arguments, flags, errors and workspace
 * (biem_uinterior_workspace_bytes) as biem_uinterior.  Covered as biem_uinterior, with per-lane rows of n_end + 3 radial values
 * (tree a: n_end <= 152). */
int biem_uinterior_grad(const biem_plan* plan, int nb, int B, int P, const double* d_k /*c128*/, const double* d_eta,
                        const double* d_centers, const double* d_radii, int geom_batched, const double* d_kint /*[nb or 1][B] c128*/,
                        const double* d_delta /*c128*/, int fluid_batched, const double* d_density, const double* d_points, int flags,
                        double* d_out /*[d][P][nb]*/, void* d_work, size_t work_bytes, void* stream);

/* ---- one call for the whole path: ball tables + fill (equilibrated) + LU + density, systems processed in
 *      chunks of `chunk` resident matrices (0 = choose); every system is factored once for its nrhs right-hand sides.
 *      d_g [nb][nrhs][B][Q] as in biem_rhs_project, d_density [nb][nrhs][B][H]. ---- */
size_t biem_solve_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int chunk);
int biem_solve(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
               const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched,
               const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream);

/* The same through the complex-symmetric form of the system: with W the unitary map to real harmonics and
 * R = diag(1/sqrt(gj gh)), R W^H M W R^-1 is complex symmetric (the reference solves the general system with LU,
 * _biem.py:797; the symmetry is a property of (S|R), tests/test_oracle_golden.py).  Symmetric fill (upper triangle), U^T U
 * factorisation without interchanges (biem_sym_factor_solve), back-transform, density.  d_info[s] < 0: a diagonal pivot was rejected (see biem_ldlt_factor_solve) - the caller
 * re-solves those systems with biem_solve.  Same arguments and workspace as biem_solve.
 * With geom_batched = 0 and ab_batched = 0 the fill contracts the block of ball pairs that share their displacement vector and
 * their (radius, alpha, beta) on either side once and stores it to each of them (identical blocks by translation invariance;
 * displacements are matched to the rounding of the subtraction, so on an exactly representable lattice the densities are bit for bit
 * those of the pair-by-pair fill, otherwise equal to rounding); systems of at most 128 unknowns (N + nrhs <= 128) are factorised and
 * solved by one launch. */
int biem_solve_ldlt(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                    const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                    int ab_batched, const double* d_g, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                    void* stream);

/* ---- factor now, solve later: the symmetric path split at its factorisation (the reference factors again on every call,
 *      _biem.py:797).  A factor is kept and solved against any number of times; the solve reads it and never writes it. ----
 * biem_sym_factor: biem_sym_factor_solve with no right-hand side (lda >= n_pad suffices): on return the upper triangle of every
 * system holds U with A = U^T U, for every n_pad (the one-launch path of n_pad <= 128 stores the whole U too); d_info and workspace
 * as biem_sym_factor_solve (biem_lu_workspace_bytes(nb, n_pad, 0)).
 * biem_sym_solve: U^T U x = b with such a factor (only its upper triangle is read): B row-major [n_pad][ldb] per system (nrhs <= ldb
 * columns, system s at d_B + 2*s*b_stride doubles; rows of an identity-padded system past its size must hold zeros), overwritten by
 * the solutions.  Forward solve U^T y = b by 64-row blocks (diagonal step, then an update of the rows below from the 64-row strip of U
 * right of the block, each U element read once for all right-hand sides), back solve by the column form of biem_sym_factor_solve.
 * No workspace; n_pad a multiple of 64, lda >= n_pad, ldb >= nrhs, at most 65535 systems and right-hand sides. */
int biem_sym_factor(int nb, int n_pad, double* d_A, long long lda, long long sys_stride, int* d_info /*[nb]*/, void* d_work,
                    size_t work_bytes, void* stream);
int biem_sym_solve(int nb, int n_pad, int nrhs, const double* d_U, long long lda, long long sys_stride, double* d_B, long long ldb,
                   long long b_stride, void* stream);
/* biem_factor_ldlt: ball tables (into d_tab [nb][B][3][n_end], which the solve needs), symmetric fill and U^T U factorisation of the
 * systems of biem_solve_ldlt, without right-hand sides, into the caller's factor buffer d_F (n_pad = biem_lu_npad(B H) rows, lda >=
 * n_pad, system s at d_F + 2*s*sys_stride doubles, sys_stride >= n_pad lda; identity padding written).  Same chunking of the fill and
 * factorisation workspace (`chunk` systems at a time, 0 = choose; the factors of ALL nb systems stay in d_F), pair-block dedupe and
 * d_info codes as biem_solve_ldlt: a system with d_info[s] < 0 is to be factored by the pivoted LU instead (biem_fill with
 * BIEM_FILL_EQUILIBRATED into the same slot, biem_lu_factor; solved by biem_lu_solve).  Workspace: biem_factor_workspace_bytes.
 * biem_solve_factored: densities [nb][nrhs][B][H] of the right-hand sides d_g [nb][nrhs][B][Q] (as biem_solve_ldlt) against such
 * factors: biem_rhs_project in slot order, f~ = R W^H f, biem_sym_solve, x = W R^-1 x~, biem_density.  Systems in LU form are not
 * told apart: their densities are the caller's to replace.  Workspace: biem_solve_factored_workspace_bytes (the right-hand sides). */
size_t biem_factor_workspace_bytes(const biem_plan* plan, int nb, int B, int chunk);
int biem_factor_ldlt(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                     const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_F,
                     long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work, size_t work_bytes,
                     void* stream);
size_t biem_solve_factored_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs);
int biem_solve_factored(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                        const double* d_tab, const double* d_g, double* d_density, void* d_work, size_t work_bytes, void* stream);

/* ---- boundary coefficients that depend on the harmonic degree:  alpha_{b,n} u + beta_{b,n} d_n u = 0 on ball b (a sphere the wave
 *      enters acts on the exterior field through one scalar per degree).  Every entry below mirrors its namesake
 *      without _n; only what differs is described.  d_alpha_n / d_beta_n are [nb][B][n_end] complex128 when ab_batched != 0, else
 *      [B][n_end] shared by all systems.  The tables have biem_ball_tables' layout, so biem_fill, biem_density, biem_lu_*,
 *      biem_sym_*, biem_uscat and biem_uscat_grad take them and their results as they are. ----
 * biem_ball_tables_n: [0] gj_n = alpha_n j_n + beta_n k j_n', [1] gh_n = alpha_n h_n + beta_n k h_n', [2] blc_n; per degree the
 * arithmetic of biem_ball_tables, so coefficients that do not vary with n give its table.  Same trees and orders. */
int biem_ball_tables_n(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_alpha_n /*c128*/, const double* d_beta_n /*c128*/, int ab_batched,
                       double* d_tab, void* stream);
/* biem_rhs_project_n: the degree of a harmonic is known only after the projection, so the two parts of the boundary data cross the
 * ABI apart and unweighted: d_gu[s][r][b][q] = u_in(c_b + rho_b y_q), d_gdn[s][r][b][q] = (y_q . grad u_in)(c_b + rho_b y_q), each
 * [nb][nrhs][B][Q] complex128; a null pointer is a set of zeros (and costs nothing).  Writes
 *   f(s, r, b, h) = -( alpha_{b,n(h)} sum_q W[q][h] gu[s][r][b][q] + beta_{b,n(h)} sum_q W[q][h] gdn[s][r][b][q] )
 * to d_f[s*sys_stride + (b*H + h)*elem_stride + r*rhs_stride] as biem_rhs_project does (one read of W serves both sums). */
int biem_rhs_project_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_gu, const double* d_gdn,
                       const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_f, long long sys_stride,
                       long long elem_stride, long long rhs_stride, void* stream);
/* biem_solve_n / biem_solve_ldlt_n: biem_solve / biem_solve_ldlt with (d_alpha_n, d_beta_n) for (d_alpha, d_beta) and (d_gu, d_gdn)
 * for d_g; workspace biem_solve_workspace_bytes.  The symmetric fill takes every ball pair on its own (no pair classes: they are keyed
 * on one (alpha, beta) per ball).  One more d_info code of biem_solve_ldlt_n: -(Npad+2) marks a system with a (ball, degree) whose
 * gj_n gh_n is zero or whose scaling 1/sqrt(gj_n gh_n) is not finite - a degree the ball does not scatter, e.g. a transparent sphere
 * (k_b = k, density ratio 1) - for which the symmetric form does not exist; like every d_info < 0 the caller re-solves it with
 * biem_solve_n, whose equilibrated form divides by gh only. */
int biem_solve_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                 const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                 const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                 void* stream);
int biem_solve_ldlt_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                      const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n,
                      int ab_batched, const double* d_gu, const double* d_gdn, double* d_density, int* d_info, int chunk, void* d_work,
                      size_t work_bytes, void* stream);
/* biem_factor_ldlt_n: biem_factor_ldlt with the tables of biem_ball_tables_n (workspace biem_factor_workspace_bytes; no pair classes;
 * d_info as biem_solve_ldlt_n).  biem_solve_factored_n: biem_solve_factored with the right-hand sides of biem_rhs_project_n - the
 * coefficients are passed again because the stored tables hold only their combinations gj, gh (workspace
 * biem_solve_factored_workspace_bytes). */
/* the check behind that d_info code, on its own (tests): d_info[s] = code for every system s of d_tab [nb][B][3][n_end] with a
 * (ball, degree) whose 1/sqrt(gj gh) or gj/sqrt(gj gh) is not finite; the entries of the other systems are left as they are. */
int biem_flag_unscalable(const biem_plan* plan, int nb, int B, const double* d_tab, int* d_info, int code, void* stream);
int biem_factor_ldlt_n(const biem_plan* plan, int nb, int B, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                       const double* d_radii, int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched,
                       double* d_F, long long lda, long long sys_stride, double* d_tab, int* d_info, int chunk, void* d_work,
                       size_t work_bytes, void* stream);
int biem_solve_factored_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                          const double* d_tab, const double* d_alpha_n, const double* d_beta_n, int ab_batched, const double* d_gu,
                          const double* d_gdn, double* d_density, void* d_work, size_t work_bytes, void* stream);

/* ---- plane-wave incidence in closed form: exact right-hand sides without samples.  With orthonormal harmonics and the
 *      radial normalisation of biem_radial, u_in = e^{i k p^.x} has on the surface of ball b the projections
 *        U_h = C_d i^n j_n(k rho) conj(Y_h(p^)) e^{i k p^.c_b},  V_h = C_d i^n k j_n'(k rho) conj(Y_h(p^)) e^{i k p^.c_b},
 *        C_d = 2^{(d+1)/2} pi^{(d-1)/2}, so f(s, r, b, h) = -C_d i^{n(h)} gj_{n(h)}(s, b) conj(Y_h(p^_r)) e^{i k_s p^_r.c_b}
 *      with gj row 0 of d_tab (biem_ball_tables or biem_ball_tables_n: degree-dependent coefficients need no form of their own); real
 *      and complex k, every tree, the chains included.  d_dirs: UNIT vectors in the plan's axes, [nrhs][d] shared by all systems or
 *      [nb][nrhs][d] with dirs_batched != 0 (a zero direction is the caller's error).  Every element is written by one lane, no
 *      atomics: two calls give the same bits.  At most 65535 systems and right-hand sides per call (BIEM_ERR_ARG).
 * biem_rhs_plane_wave writes f where biem_rhs_project does, d_f[s*sys_stride + (b*H + h)*elem_stride + r*rhs_stride].  Workspace:
 * biem_rhs_plane_wave_workspace_bytes (the harmonics of the directions, twice).
 * biem_solve_pw / biem_solve_ldlt_pw / biem_solve_factored_pw: biem_solve / biem_solve_ldlt / biem_solve_factored with that source in
 * place of the samples.  per_degree != 0: d_alpha / d_beta are the [nb or 1][B][n_end] pair of the _n entries, which then run
 * (biem_ball_tables_n, the pair-by-pair fill, the -(Npad+2) code).  biem_solve_factored_pw reads the stored tables (its coefficient
 * arguments are not read and may be null) and takes the wavenumbers and centres the factored solve otherwise does not need.
 * Workspace: the bytes of biem_solve_workspace_bytes (biem_solve_factored_workspace_bytes) PLUS biem_rhs_plane_wave_workspace_bytes,
 * the harmonics at the tail. ---- */
size_t biem_rhs_plane_wave_workspace_bytes(const biem_plan* plan, int nb, int nrhs, int dirs_batched);
int biem_rhs_plane_wave(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_centers,
                        int geom_batched, const double* d_tab, const double* d_dirs, int dirs_batched, double* d_f, long long sys_stride,
                        long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream);
int biem_solve_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_dirs, int dirs_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream);
int biem_solve_ldlt_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                       const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                       int ab_batched, int per_degree, const double* d_dirs, int dirs_batched, double* d_density, int* d_info, int chunk,
                       void* d_work, size_t work_bytes, void* stream);
int biem_solve_factored_pw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                           const double* d_alpha, const double* d_beta, int ab_batched, int per_degree, const double* d_dirs,
                           int dirs_batched, double* d_density, void* d_work, size_t work_bytes, void* stream);

/* ---- point-source incidence in closed form: exact right-hand sides without samples.  The monopole
 *      u_in(x) = h_0(k |x - s|) (point_source with n = 0) has on the surface of ball b, with t = s - c_b and |t| > rho_b, the projections
 *        U_h = C_d j_n(k rho) h_n(k |t|) conj(Y_h(t^)),  V_h = C_d k j_n'(k rho) h_n(k |t|) conj(Y_h(t^)),
 *      so f(s, r, b, h) = -C_d gj_{n(h)}(s, b) h_{n(h)}(k_s |t_{r,b}|) conj(Y_h(t^_{r,b})) with gj row 0 of d_tab (biem_ball_tables or
 *      biem_ball_tables_n); real and complex k, every tree, the chains included, kind inner and outer alike.  d_src: source positions
 *      in the plan's axes, [nrhs][d] shared by all systems or [nb][nrhs][d] with src_batched != 0.  NOT TESTED HERE: every source
 *      must lie strictly outside every ball.  A source on or inside a sphere gives finite values that mean nothing, a source at a
 *      centre (t = 0) non-finite ones.  Every element is written by one lane, no atomics: two calls give the same bits.  At most
 *      65535 systems and right-hand sides per call (BIEM_ERR_ARG); n_end above 320 (2-D only) is BIEM_ERR_UNSUPPORTED, nothing launched.
 * biem_rhs_point_source writes f where biem_rhs_project does, d_f[s*sys_stride + (b*H + h)*elem_stride + r*rhs_stride].  Workspace:
 * biem_rhs_point_source_workspace_bytes (unit vectors and distances, their harmonics twice, the radial table nb x nrhs x B x n_end).
 * biem_solve_ps / biem_solve_ldlt_ps / biem_solve_factored_ps: the _pw entries with d_src, src_batched in place of d_dirs,
 * dirs_batched.  Workspace: the bytes of biem_solve_workspace_bytes (biem_solve_factored_workspace_bytes) PLUS
 * biem_rhs_point_source_workspace_bytes, at the tail. ---- */
size_t biem_rhs_point_source_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int src_batched, int geom_batched);
int biem_rhs_point_source(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_centers,
                          int geom_batched, const double* d_tab, const double* d_src, int src_batched, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream);
int biem_solve_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_src, int src_batched, double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes,
                  void* stream);
int biem_solve_ldlt_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                       const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                       int ab_batched, int per_degree, const double* d_src, int src_batched, double* d_density, int* d_info, int chunk,
                       void* d_work, size_t work_bytes, void* stream);
int biem_solve_factored_ps(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                           const double* d_alpha, const double* d_beta, int ab_batched, int per_degree, const double* d_src,
                           int src_batched, double* d_density, void* d_work, size_t work_bytes, void* stream);

/* ---- multipole incidence in closed form: exact right-hand sides for any degree, without samples.  The outgoing
 *      multipole u_in(x) = h_n'(k |x - s|) Y_h'((x - s)^) at s (orthonormal harmonics, the radial functions of this header), expanded about
 *      the centre of ball b with t = c_b - s and |t| > rho_b, is a column of the translation operator of the fill:
 *        u_in(c_b + r) = sum_h (S|R)_{h'->h}(t) j_n(k |r|) Y_h(r^),   f(s, r, b, h) = -gj_{n(h)}(s, b) (S|R)_{h'_r->h}(c_b - s_r),
 *      gj row 0 of d_tab; (S|R) from the plan's term lists and a table row C_d h_n''(k |t|) Y_l(t^) per (system, source, ball), in 2-D
 *      from Graf's one term per entry.  d_src as biem_rhs_point_source's; d_idx: the harmonic h' of every source, an index into the
 *      plan's harmonic axis (biem_plan_labels), int [nrhs] or [nb][nrhs] with src_batched != 0.  h' of degree 0 gives Y_0 times the
 *      point-source problem.  NOT TESTED HERE: every source strictly outside every ball, 0 <= h' < H (an index outside gives NaN).
 *      Every element is written by one lane, no atomics: two calls give the same bits.  At most 65535 systems and right-hand sides
 *      per call (BIEM_ERR_ARG); BIEM_ERR_UNSUPPORTED, nothing launched: n_end above 320 in 2-D, above 160 elsewhere, a plan without
 *      term lists that is not 2-D.
 * Workspace: biem_rhs_multipole_workspace_bytes, the table rows of one slice of (systems x right-hand sides): the launcher walks slices
 * whose table stays under 512 MiB (BIEM_RHS_TABLE_BYTES=n in the environment lowers that, read per call; the result does not depend on
 * it).  biem_solve_ms / biem_solve_ldlt_ms / biem_solve_factored_ms: the _ps entries with d_idx after src_batched; workspace: the
 * bytes of biem_solve_workspace_bytes (biem_solve_factored_workspace_bytes) PLUS biem_rhs_multipole_workspace_bytes, at the tail. ---- */
size_t biem_rhs_multipole_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int src_batched, int geom_batched);
int biem_rhs_multipole(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_centers,
                       int geom_batched, const double* d_tab, const double* d_src, int src_batched, const int* d_idx, double* d_f,
                       long long sys_stride, long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream);
int biem_solve_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_src, int src_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work,
                  size_t work_bytes, void* stream);
int biem_solve_ldlt_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                       const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                       int ab_batched, int per_degree, const double* d_src, int src_batched, const int* d_idx, double* d_density,
                       int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream);
int biem_solve_factored_ms(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                           const double* d_alpha, const double* d_beta, int ab_batched, int per_degree, const double* d_src,
                           int src_batched, const int* d_idx, double* d_density, void* d_work, size_t work_bytes, void* stream);
/* The field of such a source itself, u(x) = h_n'(k_s |x - s_s|) Y_h'((x - s_s)^), one source per system: d_src [nb][d], d_idx [nb] (an
 * index into the harmonic axis of `plan`), points and flags as biem_uscat (BIEM_USCAT_POINTS_BATCHED, BIEM_USCAT_KIND_INNER); out [P][nb]
 * complex128.  grad != 0: the Cartesian gradient in the plan's axes, out [d][P][nb]; `plan` is then a plan of order n' + 2 or more (its
 * force coupling table is built on the first such call).  Every tree the value kernels of biem_uscat cover, the chains included.
 * BIEM_USCAT_KIND_INNER: the regular wave j_n'(k_s |x - o_s|) Y_h'((x - o_s)^) about o = d_src instead (the incident field of
 * biem_rhs_regular_wave); x = o is an ordinary point. */
size_t biem_multipole_field_workspace_bytes(const biem_plan* plan, int nb);
int biem_multipole_field(biem_plan* plan, int nb, int P, const double* d_k /*c128*/, const double* d_src, const int* d_idx,
                         const double* d_points, int flags, int grad, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* ---- regular-wave incidence in closed form: the basis of every source-free incident field.  u_in(x) =
 *      j_n'(k |x - o|) Y_h'((x - o)^) about an origin o, expanded about the centre of ball b with t = c_b - o, is the same column with
 *      the regular radial function in the table row:
 *        u_in(c_b + r) = sum_h (R|R)_{h'->h}(t) j_n(k |r|) Y_h(r^),   f(s, r, b, h) = -gj_{n(h)}(s, b) (R|R)_{h'_r->h}(c_b - o_r).
 *      Arguments, layouts, limits, workspace and slicing (BIEM_RHS_TABLE_BYTES) are those of biem_rhs_multipole with d_origin for d_src.
 *      The origin is unrestricted - outside the balls, inside one, or exactly on a centre, where (R|R)(0) is the identity: that ball's
 *      block is -gj_n delta_{h h'} with exact zeros off the diagonal.  Nothing is non-finite for any origin.  biem_solve_rw /
 *      biem_solve_ldlt_rw / biem_solve_factored_rw: the _ms entries. ---- */
size_t biem_rhs_regular_wave_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs, int origin_batched, int geom_batched);
int biem_rhs_regular_wave(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_centers,
                          int geom_batched, const double* d_tab, const double* d_origin, int origin_batched, const int* d_idx, double* d_f,
                          long long sys_stride, long long elem_stride, long long rhs_stride, void* d_work, size_t work_bytes, void* stream);
int biem_solve_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_origin, int origin_batched, const int* d_idx, double* d_density, int* d_info, int chunk, void* d_work,
                  size_t work_bytes, void* stream);
int biem_solve_ldlt_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                       const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                       int ab_batched, int per_degree, const double* d_origin, int origin_batched, const int* d_idx, double* d_density,
                       int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream);
int biem_solve_factored_rw(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                           const double* d_alpha, const double* d_beta, int ab_batched, int per_degree, const double* d_origin,
                           int origin_batched, const int* d_idx, double* d_density, void* d_work, size_t work_bytes, void* stream);

/* ---- incident fields by their expansion coefficients: beams, standing waves, the near field of a neighbouring cluster
 *      as ONE right-hand side.  u_in(x) = sum_h' p_h' z_n'(k |x - o|) Y_h'((x - o)^) with z = j (regular != 0; any origin) or z = h (the
 *      origin strictly outside every ball: NOT TESTED HERE), and
 *        f(s, r, b, h) = -gj_{n(h)}(s, b) sum_{h' : n(h') < n_in} p[s, r, h'] (X|R)_{h'->h}(c_b - o),   X = R or S:
 *      the columns biem_rhs_regular_wave / biem_rhs_multipole take one at a time, contracted with whole coefficient vectors.  The order
 *      n_in of the coefficients is independent of the order of `plan`: `list_plan` is a plan of the same tree of order max(n_in, n_end)
 *      (`plan` itself where n_in <= n_end) whose term lists, table labels and harmonic axis are read; d_coef [nrhs][H(list_plan)] complex128,
 *      or [nb][nrhs][H(list_plan)] with coef_batched != 0, lies along that axis (biem_plan_labels; entries of degree >= n_in are not read),
 *      and d_map [H(plan)] holds the position of every harmonic of `plan` on it, matched by label (may be null with list_plan == plan).
 *      d_origin [n_origin][d], or [nb][n_origin][d] with origin_batched != 0; n_origin is 1 - one origin for all right-hand sides of a
 *      system: the table rows are formed once per (system, ball) and a lane applies each translation entry to 8 right-hand sides - or
 *      nrhs.  f is written where biem_rhs_project writes it for `plan`.  d >= 3: the table row and the coefficient vectors of a workgroup
 *      sit in LDS while they fit 152 KiB (BIEM_RHS_EX_LDS_BYTES=n in the environment lowers that, read per call), else they are read
 *      from memory, by the same statements.  Every element is written by one lane in a fixed order of summation (h' ascending, then
 *      the list's order), no atomics: two calls, any table slicing (BIEM_RHS_TABLE_BYTES), either LDS branch and any nrhs give the
 *      same bits per right-hand side (within n_origin == 1 and within n_origin == nrhs).  stage: 0; 1 / 2 run the table rows / the
 *      contraction alone (timing).  Stage 1 then stage 2 is stage 0 only for a call of ONE table slice: the workspace holds one slice,
 *      so with several stage 1 leaves the last one's rows and stage 2 contracts every slice against those.  Limits and errors as biem_rhs_multipole, applied to list_plan (n_end above 320 in 2-D, above 160
 *      elsewhere: BIEM_ERR_UNSUPPORTED); BIEM_ERR_ARG for a list plan of another tree or a lower order, n_in outside [1, n_end(list_plan)],
 *      n_origin neither 1 nor nrhs.
 * Workspace: biem_rhs_expansion_workspace_bytes, the table rows of one slice of (systems x origins) of list_plan (2-D: none).
 * biem_solve_ex / biem_solve_ldlt_ex / biem_solve_factored_ex: the _rw entries with (n_origin, d_coef, coef_batched, list_plan, d_map, n_in,
 * regular) in place of d_idx; workspace: the bytes of biem_solve_workspace_bytes (biem_solve_factored_workspace_bytes) PLUS
 * biem_rhs_expansion_workspace_bytes, at the tail. ---- */
size_t biem_rhs_expansion_workspace_bytes(const biem_plan* list_plan, int nb, int B, int n_origin);
int biem_rhs_expansion(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                       const double* d_tab, const double* d_origin, int origin_batched, int n_origin, const double* d_coef /*c128*/,
                       int coef_batched, const biem_plan* list_plan, const int* d_map, int n_in, int regular, double* d_f,
                       long long sys_stride, long long elem_stride, long long rhs_stride, int stage, void* d_work, size_t work_bytes,
                       void* stream);
int biem_solve_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_centers,
                  const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, int per_degree,
                  const double* d_origin, int origin_batched, int n_origin, const double* d_coef /*c128*/, int coef_batched,
                  const biem_plan* list_plan, const int* d_map, int n_in, int regular, double* d_density, int* d_info, int chunk,
                  void* d_work, size_t work_bytes, void* stream);
int biem_solve_ldlt_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta,
                       const double* d_centers, const double* d_radii, int geom_batched, const double* d_alpha, const double* d_beta,
                       int ab_batched, int per_degree, const double* d_origin, int origin_batched, int n_origin,
                       const double* d_coef /*c128*/, int coef_batched, const biem_plan* list_plan, const int* d_map, int n_in, int regular,
                       double* d_density, int* d_info, int chunk, void* d_work, size_t work_bytes, void* stream);
int biem_solve_factored_ex(const biem_plan* plan, int nb, int B, int nrhs, const double* d_F, long long lda, long long sys_stride,
                           const double* d_tab, const double* d_k /*c128*/, const double* d_centers, int geom_batched,
                           const double* d_alpha, const double* d_beta, int ab_batched, int per_degree, const double* d_origin,
                           int origin_batched, int n_origin, const double* d_coef /*c128*/, int coef_batched, const biem_plan* list_plan,
                           const int* d_map, int n_in, int regular, double* d_density, void* d_work, size_t work_bytes, void* stream);
/* The field of such an expansion itself, one per system: biem_multipole_field with a coefficient vector d_coef [nb][H] complex128 along
 * the harmonic axis of `plan` in place of the index (one body serves both; workspace: biem_multipole_field_workspace_bytes).  Flags as
 * there: BIEM_USCAT_KIND_INNER is the regular expansion, where x = o is an ordinary point.  grad != 0: `plan` is a plan of order
 * n_in + 1 or more, the vector placed on its axis by label; coefficients of degree >= n_end(plan) - 1 are not read. */
int biem_expansion_field(biem_plan* plan, int nb, int P, const double* d_k /*c128*/, const double* d_origin, const double* d_coef /*c128*/,
                         const double* d_points, int flags, int grad, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* ---- the cluster's outgoing coefficients about an origin: the scattered field of all balls as one expansion,
 *        u_scat(x) = sum_h'' A_h'' h_n''(k |x - o|) Y_h''((x - o)^)  for |x - o| > max_b (|c_b - o| + rho_b),
 *        A[s][r][h''] = sum_b sum_h (R|R)_{h->h''}(o_s - c_b) c[s][r][b][h],   c = density * blc (biem_uscat's coefficients).
 *      kind outer.  d_density [nb][nrhs][B][H] on the harmonic axis of `plan`; entries of degree >= n_src (1 <= n_src <= n_end) are not
 *      read: a density of order n_src placed by label on the axis of a plan of larger order gives the expansion up to that order.
 *      d_origin [d], or [nb][d] with origin_batched != 0, in the plan's axes; d_out [nb][nrhs][H] complex128.  Every element is written
 *      by one lane in a fixed order of summation: two calls, any table slicing (BIEM_RHS_TABLE_BYTES) and any nrhs give the same bits
 *      per right-hand side.  stage: 0; 1 / 2 run the table rows / the contraction alone (timing).  Limits and errors as
 *      biem_rhs_multipole (n_end above 320 in 2-D, above 160 elsewhere: BIEM_ERR_UNSUPPORTED). ---- */
size_t biem_cluster_coefficients_workspace_bytes(const biem_plan* plan, int nb, int B, int nrhs);
int biem_cluster_coefficients(const biem_plan* plan, int nb, int B, int nrhs, int n_src, const double* d_k /*c128*/, const double* d_eta,
                              const double* d_centers, const double* d_radii, int geom_batched, const double* d_origin, int origin_batched,
                              const double* d_density, double* d_out, int stage, void* d_work, size_t work_bytes, void* stream);

/* ---- cross sections: extinction and absorbed power per ball from what the solve already has (no second solve, no
 *      matrix, no workspace).  Real k only, in the far-field normalisation u_scat ~ F(x^) e^{ikr} / r^{(d-1)/2}: "power" is
 *      (1/k) Im oint conj(u) d_n u dS, for a unit plane wave the cross section.  With c_h = density_h blc_n(rho_b), U_h / V_h the
 *      projections of u_in / d_n u_in on the surface of ball b onto Y_h - biem_rhs_project of the unweighted samples d_gu / d_gdn of
 *      biem_rhs_project_n, natural order, d_pu / d_pv [nb][nrhs][B][H] complex128 like d_density -
 *        P_ext = -(rho^{d-1} / k) sum_h Im[ conj(U_h) k c_h h_n'(k rho) + conj(c_h h_n(k rho)) V_h ]      (any incident field)
 *        P_abs = rho^{d-1} k (k rho)^{2-2d} sum_h Im(alpha_n conj beta_n) |c_h|^2 / |gj_n|^2
 *      and d_out[s][r][b][0..1] = (P_ext, P_abs), doubles.  A degree with Im(alpha_n conj beta_n) == 0 adds exactly 0 and divides by
 *      nothing (gj_n = 0 of a lossless ball is harmless); a lossy degree whose gj_n is zero or not finite makes P_abs of that ball NaN.
 *      The scattered power is sum_b P_ext - sum_b P_abs, the caller's subtraction.  d_tab: the tables of biem_ball_tables (biem_power)
 *      or biem_ball_tables_n (biem_power_n) for the same coefficients; d_alpha / d_beta [nb or 1][B], d_alpha_n / d_beta_n
 *      [nb or 1][B][n_end], as there.  d_eta is not read (blc comes with the tables); it keeps the operands of biem_ball_tables in
 *      their order.  Sums run in a fixed order: two calls give the same bits.  Every tree, the chains included, n_end <= 320.
 *      BIEM_ERR_ARG for a system with Im k != 0 (the wavenumbers are copied to the host for this test: the one entry of the field
 *      group that waits for the stream) and for nb or nrhs above 65535. ---- */
int biem_power(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
               int geom_batched, const double* d_alpha /*c128*/, const double* d_beta /*c128*/, int ab_batched, const double* d_tab,
               const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream);
int biem_power_n(const biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
                 int geom_batched, const double* d_alpha_n /*c128*/, const double* d_beta_n /*c128*/, int ab_batched, const double* d_tab,
                 const double* d_density, const double* d_pu, const double* d_pv, double* d_out, void* stream);

/* ---- radiation force: the time-averaged force on each ball from what the solve already has (no second solve, no
 *      matrix, no workspace, no incident field).  Real k, exterior problems, in the normalisation of biem_power: with u the total field,
 *        Phi_b = -(1 / (2 k^2)) oint_{S_b} [ (k^2 |u|^2 - |grad u|^2) n + 2 Re(grad u conj(d_n u)) ] dS
 *      over any closed surface in the fluid around ball b alone (for a unit plane wave an area; the physical force on a ball in a
 *      fluid of density rho_0 at angular frequency omega is Phi k^2 / (2 rho_0 omega^2) for pressure amplitude u).  Evaluated on the
 *      ball's own surface, where the boundary condition gives both traces from c_h = density_h blc_n: s_h = c_h k Wr / gj_n,
 *      Wr = i (k rho)^{1-d}, u_h = -beta_n s_h, v_h = alpha_n s_h, contracted with the plan's coupling table (biem_plan_force_terms,
 *      built by the first call).  d_out[s][r][b][0..d-1] doubles, component i along axis i of the plan's tree.  A degree with a nonzero
 *      coefficient whose gj_n is zero (to the rounding of its two terms) or not finite makes every component of that ball NaN.
 *      Operands as biem_power: d_tab the tables of biem_ball_tables (biem_force) or biem_ball_tables_n (biem_force_n) for the same
 *      coefficients, d_eta not read.  Sums run in a fixed order: two calls give the same bits.  Every tree, the chains included,
 *      n_end <= 320 (beyond: BIEM_ERR_UNSUPPORTED).  BIEM_ERR_ARG for a system with Im k != 0 (one copy of the wavenumbers to the host,
 *      one wait for the stream) and for nb or nrhs above 65535. ---- */
int biem_force(biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
               int geom_batched, const double* d_alpha /*c128*/, const double* d_beta /*c128*/, int ab_batched, const double* d_tab,
               const double* d_density, double* d_out, void* stream);
int biem_force_n(biem_plan* plan, int nb, int B, int nrhs, const double* d_k /*c128*/, const double* d_eta, const double* d_radii,
                 int geom_batched, const double* d_alpha_n /*c128*/, const double* d_beta_n /*c128*/, int ab_batched, const double* d_tab,
                 const double* d_density, double* d_out, void* stream);

/* ---- per-kernel-class timing with HIP events on the launch stream (thread-local; used by bench.py for the
 *      live `roofline` figures).  Between begin and end every launch of the calling thread is bracketed by two
 *      events; end synchronises on them and returns, per class, elapsed ms, algorithmic work and launch count.
 *      Classes: 0 tables, 1 fill (work = bytes written), 2 rhs, 3 panel, 4 swap (LU row interchanges; symmetrising transform of the LDL^T path), 5 trsm, 6 gemm = the K=256 trailing
 *      updates of the four-panel groups (work = real flops, 8 per complex multiply-add), 7 back substitution, 8 the K=64 and
 *      K=128 updates inside a group. */
#define BIEM_PROFILE_CLASSES 9
int biem_profile_begin(void);
int biem_profile_end(double* ms /*[9]*/, double* work /*[9]*/, long long* launches /*[9]*/);

/* ---- microbenchmarks used by bench.py / DESIGN.md (peak checks, not part of the path) ---- */
/* issues `iters` dependent-free v_mfma_f64_16x16x4_f64 per wave on every SIMD; returns achieved FLOP/s */
int biem_bench_mfma_f64(int iters, double* tflops, void* stream);
/* the same with a choice of instruction: variant 0 v_mfma_f64_16x16x4_f64, variant 1 v_mfma_f64_4x4x4_4b_f64 (the one the trailing
 * update uses).  What a pure MFMA stream SUSTAINS on the box it runs on (1 MI355X, 2 waves per SIMD, 2-second runs: 47.3 and
 * 75.3 TFLOP/s) - bench.py reports variant 1 beside the 78.6 TFLOP/s the roofline is priced against */
int biem_bench_mfma_f64_ex(int iters, int variant, double* tflops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BIEM_MI355_H */
