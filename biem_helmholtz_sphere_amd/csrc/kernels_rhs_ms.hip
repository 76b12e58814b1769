// kernels_rhs_ms.hip -- right-hand sides of multipole incidence in closed form (gfx950): no samples, no projection.
//
// The outgoing multipole u_in(x) = h_n'(k |x - s|) Y_h'((x - s)^) at s, expanded about the centre of ball b (t = c_b - s, |t| > rho_b), is a
// column of the translation operator the fill contracts for every ball pair - the source is a ball pair's partner without a radius:
//   u_in(c_b + r) = sum_h (S|R)_{h'->h}(t) j_n(k |r|) Y_h(r^),      f(s, r, b, h) = -gj_{n(h)}(s, b) (S|R)_{h'_r->h}(c_b - s_r)
// with gj = alpha j_n + beta k j_n' row 0 of the ball tables (degree-dependent coefficients included).  Written where
// launch_rhs_project writes: s sys_stride + split.rhs_off(b, H, slot of h, elem_stride) + r rhs_stride.
//
// d >= 3: (S|R)_{h'->h}(t) = sum_p coef[p] T[tidx[p]] over the plan's term list of entry e = h H + h', T[l] = C_d h_n''(k |t|) Y_l(t^)
// over the labels of degree < 2 n_end - 1 - a row of the fill's pair tables in their plain layout, with the arithmetic of k_pair_tables'
// label-by-label branch.  Stages: table rows T[(s, r, b)][H2] (geometry, radial recurrence by one lane into LDS, one label per lane)
// into the workspace -> contraction, one lane per (s, r, b, h), the row read where it lies (L2).  The table of a whole call can be
// large (256 systems x 64 sources x 16 balls x 1521 labels: 6 GB), so the launcher walks slices of the flattened (system, right-hand
// side) axis whose table stays under kRhsTableBytes; the slices are independent, so their number does not change a bit of the result.
// Tree a: Graf's theorem leaves one term per entry (kernels_fill.hip, "2-D fills without term lists"),
//   (S|R)_{m'->m}(t) = i^{|m| + |mu| - |m'|} C_2 h_{|mu|}(k |t|) e^{i mu phi} / (2 pi),   mu = m' - m,
// so a workgroup keeps the radial row of its (s, r, b) in LDS and needs no table, no lists and no workspace, up to n_end = kMaxRad.
//
// Nothing here tests |t| > rho: a source on or inside a sphere gives finite values that mean nothing, t = 0 gives non-finite ones.  An
// index outside [0, H) gives NaN in its column and reads nothing.  Every element of f is written by one lane, without atomics.
//
// Regular waves: u_in(x) = j_n'(k |x - o|) Y_h'((x - o)^) about an origin o is the same column with the regular radial row,
//   f(s, r, b, h) = -gj_{n(h)}(s, b) (R|R)_{h'_r->h}(c_b - o_r),   (R|R) = (S|R) with j_n'' for h_n'' in T (tree a: J for H in Graf's term):
// the same kernels with REG = true.  The origin is unrestricted: at t = 0 (o on a centre, the common case) the row is formed from
// j_l(0) = delta_{l0} j_0(0) and a fixed unit vector, so (R|R)(0) is the identity with exact zeros off the diagonal.
// launch_regular_tables hands the table stage to the cluster coefficients (kernels_cluster.hip), which take t from the other end (flip).
#include "common.hpp"
#include "rhs_translate.hpp"
#include <climits>
#include <cstdlib>

namespace biem {
namespace {
constexpr size_t kRhsTableBytes = (size_t)512 << 20;   // table rows of one slice of (systems x right-hand sides)
constexpr long long kGridMax = 1 << 20;                // workgroups of a strided launch
inline unsigned strided_grid(long long groups) { return (unsigned)(groups < kGridMax ? groups : kGridMax); }

// plain table rows T[row][H2] = C_d h_n''(k_s |t|) Y_l(t^) of the rows [0, rows) of a slice: one workgroup per row (strided), lane 0 runs the
// radial recurrence into LDS, then one label per lane, every label from scratch (k_pair_tables' generic branch; chain trees: chain_harmonic).
// REG: j_n'' for h_n'' (regular waves; the cluster coefficients, which take the displacement from the other end: flip)
template <bool REG>
__global__ void __launch_bounds__(256) k_ms_tables(int tree, int d, int n2, int H2, double Cd, const int* __restrict__ labels2,
                                                    const int* __restrict__ deg2, int B, int nrhs, long long sr0, long long rows,
                                                    const cplx* __restrict__ k, const double* __restrict__ centers, int geom_batched,
                                                    const double* __restrict__ src, int src_batched, int flip, cplx* __restrict__ T) {
  __shared__ cplx sJ[kMaxRad * 2 + 6], sH[REG ? 1 : kMaxRad * 2 + 6];
  __shared__ double sC[kChainDimMax], sS[kChainDimMax], sPhi;
  const cplx* sR = REG ? sJ : sH;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const MsRow w = ms_row(row, sr0, B, nrhs);
    double t[kChainDimMax], dist;
    ms_displacement(w, d, B, nrhs, centers, geom_batched, src, src_batched, t, &dist, flip != 0);
    if (REG) ms_unit_if_zero(d, dist, t);
    __syncthreads();                                      // the previous row's tables are no longer read
    if (threadIdx.x == 0) {
      ms_radial_row<REG>(d, n2 - 1, k[w.s], dist, sJ, sH);
      if (tree == TREE_CHAIN) { double phi; chain_angles(d, t, sC, sS, &phi); sPhi = phi; }
    }
    __syncthreads();
    cplx* out = T + row * H2;
    if (tree == TREE_CHAIN) {
      for (int l = threadIdx.x; l < H2; l += 256) {
        double re, im;
        chain_harmonic(d, labels2 + (size_t)l * (d - 1), sC, sS, sPhi, &re, &im);
        out[l] = cmul(cscale(sR[deg2[l]], Cd), make_double2(re, im));
      }
    } else {
      const Dir dir = make_dir(tree, t);
      for (int l = threadIdx.x; l < H2; l += 256) {
        double re, im;
        harmonic_single(tree, labels2[3 * l], labels2[3 * l + 1], labels2[3 * l + 2], dir, &re, &im);
        out[l] = cmul(cscale(sR[deg2[l]], Cd), make_double2(re, im));
      }
    }
  }
}

// f = -gj_n sum_p coef[p] T[tidx[p]] over the list of entry e = h H + h'_r, in the list's order: one lane per (row, h), h fastest
__global__ void __launch_bounds__(256) k_rhs_ms(int H, int H2, int n_end, int B, int nrhs, long long sr0, long long count,
                                                 const int* __restrict__ idx, int src_batched, const uint32_t* __restrict__ ptr,
                                                 const double* __restrict__ coef, const uint16_t* __restrict__ tidx, const int* __restrict__ deg,
                                                 const cplx* __restrict__ T, const cplx* __restrict__ tab, cplx* __restrict__ f,
                                                 long long sys_stride, long long elem_stride, long long rhs_stride, const int* __restrict__ hpos,
                                                 SplitMap sm) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const int h = (int)(i % H);
    const long long row = i / H;
    const MsRow w = ms_row(row, sr0, B, nrhs);
    const int hp = idx[(src_batched ? w.s * nrhs : 0) + w.r];
    double ar = nan(""), ai = ar;
    if (hp >= 0 && hp < H) {
      const cplx* Tr = T + row * H2;
      const size_t e = (size_t)h * H + hp;
      ar = ai = 0.0;
      for (uint32_t p = ptr[e]; p < ptr[e + 1]; ++p) {
        const double c = coef[p];
        const cplx v = Tr[tidx[p]];
        ar = fma(c, v.x, ar); ai = fma(c, v.y, ai);
      }
    }
    const cplx gj = tab[(w.s * B + w.b) * 3 * n_end + deg[h]];
    f[w.s * sys_stride + sm.rhs_off(w.b, H, hpos ? hpos[h] : h, elem_stride) + w.r * rhs_stride] = cscale(cmul(gj, make_double2(ar, ai)), -1.0);
  }
}

// tree a: one workgroup per (s, r, b) (strided), the radial row h_j(k_s |t|) (REG: j_j), j < 2 n_end - 1, in LDS, one harmonic per lane
template <bool REG>
__global__ void __launch_bounds__(256) k_rhs_ms_2d(int n_end, int H, double Cd, const int* __restrict__ labels, int B, int nrhs, long long rows,
                                                    const cplx* __restrict__ k, const double* __restrict__ centers, int geom_batched,
                                                    const double* __restrict__ src, int src_batched, const int* __restrict__ idx,
                                                    const cplx* __restrict__ tab, cplx* __restrict__ f, long long sys_stride,
                                                    long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  __shared__ cplx sJ[kMaxRad * 2 + 6], sH[REG ? 1 : kMaxRad * 2 + 6];
  const cplx* sR = REG ? sJ : sH;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const MsRow w = ms_row(row, 0, B, nrhs);
    double t[2], dist;
    ms_displacement(w, 2, B, nrhs, centers, geom_batched, src, src_batched, t, &dist);
    if (REG) ms_unit_if_zero(2, dist, t);
    __syncthreads();
    if (threadIdx.x == 0) ms_radial_row<REG>(2, 2 * n_end - 2, k[w.s], dist, sJ, sH);
    __syncthreads();
    const double phi = atan2(t[1], t[0]);
    const int hp = idx[(src_batched ? w.s * nrhs : 0) + w.r];
    const bool ok = hp >= 0 && hp < H;
    const int mp = ok ? labels[3 * hp] : 0, amp = mp < 0 ? -mp : mp;
    const cplx* gj = tab + (w.s * B + w.b) * 3 * n_end;
    cplx* fs = f + w.s * sys_stride + w.r * rhs_stride;
    for (int h = threadIdx.x; h < H; h += 256) {
      const int m = labels[3 * h], am = m < 0 ? -m : m, mu = mp - m, j = mu < 0 ? -mu : mu;
      double sn, cs;
      sincos((double)mu * phi, &sn, &cs);
      // T'[j] = C_2 h_j / sqrt(2 pi) times the phase, times i^{|m| + |mu| - |m'|} / sqrt(2 pi): k_fill2d's entry
      const cplx raw = cscale(cmul(cscale(sR[j], Cd * kInvSqrt2Pi), make_double2(cs, sn)), ms_sign_even(am + j - amp) * kInvSqrt2Pi);
      const cplx v = ok ? cscale(cmul(gj[am], raw), -1.0) : make_double2(nan(""), nan(""));
      fs[sm.rhs_off(w.b, H, hpos ? hpos[h] : h, elem_stride)] = v;
    }
  }
}

// (system, right-hand side) pairs per slice: as many as keep B H2 complex per pair under the cap; BIEM_RHS_TABLE_BYTES lowers the cap
// (tests: read per call).  At least one pair, at most all of them
long long ms_slice_pairs(const biem_plan* p, int nb, int B, int nrhs) {
  size_t cap = kRhsTableBytes;
  if (const char* e = getenv("BIEM_RHS_TABLE_BYTES")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0 && v < cap) cap = (size_t)v;
  }
  const size_t per = (size_t)B * p->H2 * sizeof(cplx);
  const long long all = (long long)nb * nrhs, fit = (long long)(cap / per);
  return fit < 1 ? 1 : (fit < all ? fit : all);
}
}  // namespace

long long rhs_table_slice_pairs(const biem_plan* p, int nb, int B, int nrhs) { return ms_slice_pairs(p, nb, B, nrhs); }

int launch_translation_tables(const biem_plan* p, bool regular, int B, int nrhs, long long sr0, long long rows, const double* d_k,
                              const double* d_centers, int geom_batched, const double* d_src, int src_batched, int flip, double* d_T,
                              hipStream_t st) {
  hipLaunchKernelGGL(regular ? k_ms_tables<true> : k_ms_tables<false>, dim3(strided_grid(rows)), dim3(256), 0, st, p->tree, p->d, p->n2, p->H2, p->Cd,
                     p->d_labels2, p->d_deg2, B, nrhs, sr0, rows, (const cplx*)d_k, d_centers, geom_batched, d_src, src_batched, flip, (cplx*)d_T);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_regular_tables(const biem_plan* p, int B, int nrhs, long long sr0, long long rows, const double* d_k, const double* d_centers,
                          int geom_batched, const double* d_src, int src_batched, int flip, double* d_T, hipStream_t st) {
  return launch_translation_tables(p, true, B, nrhs, sr0, rows, d_k, d_centers, geom_batched, d_src, src_batched, flip, d_T, st);
}

size_t rhs_multipole_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int src_batched, int geom_batched) {
  (void)src_batched; (void)geom_batched;                 // (the wavenumber differs between the systems: a table row per system always)
  if (nb <= 0 || B <= 0 || nrhs <= 0 || p->tree == TREE_A) return 0;
  return align256((size_t)ms_slice_pairs(p, nb, B, nrhs) * B * p->H2 * sizeof(cplx));
}

int launch_rhs_multipole(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                         const double* d_tab, const double* d_src, int src_batched, const int* d_idx, double* d_f, long long sys_stride,
                         long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work,
                         bool regular) {
  const char* who = regular ? "biem_rhs_regular_wave" : "biem_rhs_multipole";
  if (nrhs < 1) { set_error("%s: nrhs < 1", who); return BIEM_ERR_ARG; }
  // (nb, nrhs <= 65535, the order limits and the term lists: RhsSource::check has refused the rest)
  if (nb <= 0 || B <= 0) return BIEM_OK;
  const int H = p->H;
  const long long pairs = (long long)nb * nrhs;
  if (pairs * B > INT_MAX) { set_error("%s: %lld (source, ball) pairs in one call, at most %d", who, pairs * B, INT_MAX); return BIEM_ERR_ARG; }
  ProfScope ps(PK_RHS, st, 0.0);
  const int* hpos = slot_order ? p->d_hpos : nullptr;
  if (p->tree == TREE_A) {
    hipLaunchKernelGGL(regular ? k_rhs_ms_2d<true> : k_rhs_ms_2d<false>, dim3(strided_grid(pairs * B)), dim3(256), 0, st, p->n_end, H, p->Cd, p->d_labels, B, nrhs, pairs * B,
                       (const cplx*)d_k, d_centers, geom_batched, d_src, src_batched, d_idx, (const cplx*)d_tab, (cplx*)d_f, sys_stride,
                       elem_stride, rhs_stride, hpos, split);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  const long long slice = ms_slice_pairs(p, nb, B, nrhs);
  cplx* T = (cplx*)d_work;
  for (long long sr0 = 0; sr0 < pairs; sr0 += slice) {
    const long long rows = (pairs - sr0 < slice ? pairs - sr0 : slice) * B;
    hipLaunchKernelGGL(regular ? k_ms_tables<true> : k_ms_tables<false>, dim3(strided_grid(rows)), dim3(256), 0, st, p->tree, p->d, p->n2, p->H2,
                       p->Cd, p->d_labels2, p->d_deg2, B, nrhs, sr0, rows, (const cplx*)d_k, d_centers, geom_batched, d_src, src_batched, 0, T);
    BIEM_LAUNCHCHK();
    hipLaunchKernelGGL(k_rhs_ms, dim3(strided_grid((rows * H + 255) / 256)), dim3(256), 0, st, H, p->H2, p->n_end, B, nrhs, sr0, rows * H, d_idx,
                       src_batched, p->d_ptr, p->d_coef, p->d_tidx16, p->d_deg, T, (const cplx*)d_tab, (cplx*)d_f, sys_stride, elem_stride,
                       rhs_stride, hpos, split);
    BIEM_LAUNCHCHK();
  }
  return BIEM_OK;
}

}  // namespace biem
