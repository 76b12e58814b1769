// kernels_rhs_ex.hip -- right-hand sides of an incident field given by its expansion coefficients (gfx950): beams,
// standing waves, the near field of a neighbouring cluster - one solve instead of one per basis function.
//
//   u_in(x) = sum_h' p_h' z_n'(k |x - o|) Y_h'((x - o)^),   z = j (regular, any origin o) or z = h (outgoing, o outside every ball),
//   f(s, r, b, h) = -gj_{n(h)}(s, b) sum_{h' : n(h') < n_in} p[s, r, h'] (X|R)_{h'->h}(c_b - o),   X = R or S:
// the columns of the translation operator the single-harmonic right-hand sides take one at a time (kernels_rhs_ms.hip), contracted with
// a whole coefficient vector.  The order n_in of the coefficients is independent of the order n_end of the system: the term lists and the
// table labels are those of the LIST plan, of order n_list = max(n_in, n_end); `map` takes harmonic h of the solve plan to its position
// on the list plan's axis (matched by label by the caller), and the coefficient vectors lie along the list plan's axis, entries of
// degree >= n_in not read.  f is written where launch_rhs_project writes it for the SOLVE plan (strides, slot order, SplitMap).
//
// d >= 3: table rows T[row][H2] of the list plan by k_ms_tables (launch_translation_tables), one per (system, origin, ball) - with one
// origin for all right-hand sides of a system they are formed once per (system, ball) -, in slices under the byte cap of the
// single-harmonic right-hand sides (BIEM_RHS_TABLE_BYTES).  Contraction: one workgroup per table row; the row and the coefficient
// vectors of the workgroup's right-hand sides go to LDS; lanes run over h, and each lane walks the contiguous run of lists
// e = map[h] H_list + h', h' = 0 .. H_list - 1, forms each translation entry ONCE and applies it to a register tile of right-hand
// sides: 8 (16 accumulators) when the origin is shared, blockIdx.y the tile, 1 when every right-hand side has its own origin.  Where
// row and vectors exceed the LDS budget (kLdsBudget; BIEM_RHS_EX_LDS_BYTES lowers it per call) both are read where they lie (L2), by
// the same statements in the same order: the two branches give the same bits.
// Tree a: list-free (Graf's one term per entry, k_rhs_ms_2d): the row E[mu] = C_2 z_|mu|(k |t|) e^{i mu phi} / (2 pi), |mu| < 2 n_list - 1,
// in LDS per (system, origin, ball), the sum over m' in the lane; no table, no workspace, n_list up to kMaxRad.
//
// One writer per element of f, a fixed order of summation (h' ascending, then the list's order), no atomics: two calls, any slicing,
// either LDS branch and any number of right-hand sides give the same bits per right-hand side (within the shared-origin form and
// within the per-origin form).  Every product that is added to something is an explicit fma (cfma), so the instantiations of a kernel
// cannot differ by the compiler's choice of contraction.  Nothing tests |c_b - o| > rho_b of an outgoing expansion: the caller's to ensure.
#include "common.hpp"
#include "rhs_translate.hpp"
#include <climits>
#include <cstdlib>

namespace biem {
namespace {
constexpr int kTile = 8;                               // right-hand sides per lane with a shared origin (16 accumulator registers)
constexpr size_t kLdsBudget = (size_t)152 << 10;       // of the 160 KB of a CU: the row and the coefficient tile of one workgroup
constexpr long long kGridMax = 1 << 20;                // workgroups of a strided launch
inline unsigned strided_grid(long long groups) { return (unsigned)(groups < 1 ? 1 : groups < kGridMax ? groups : kGridMax); }

// what both kernels know of a call.  Rows are (pair - sr0) B + b over the pairs (system, origin) = s n_origin + o
struct ExCall {
  int H, H_list, n_end, n_in, B, nrhs, n_origin;
  long long sr0;
  const int* map;                                      // [H] solve-plan harmonic -> list-plan position (null: the same axis)
  const int* deg;                                      // [H] of the solve plan
  const int* hpos;                                     // slot order of the solve plan, or null
  const cplx* tab;                                     // ball tables of the solve plan's order
  const cplx* P; int p_batched;                        // [nb or 1][nrhs][H_list]
  cplx* f; long long sys_stride, elem_stride, rhs_stride;
  SplitMap sm;
};

// the right-hand sides r0 .. r0 + nr of the workgroup at table row `row`
template <int TILE>
__device__ inline void ex_tile(const ExCall& a, long long row, long long* s, int* b, int* r0, int* nr) {
  const MsRow w = ms_row(row, a.sr0, a.B, a.n_origin);
  *s = w.s; *b = w.b;
  *r0 = TILE == 1 ? w.r : (int)blockIdx.y * TILE;
  *nr = TILE == 1 ? 1 : (a.nrhs - *r0 < TILE ? a.nrhs - *r0 : TILE);
}

// the coefficient vectors of a tile into LDS as sP[h'][q] (missing right-hand sides: zero); reads coalesced along h'
template <int TILE>
__device__ inline void ex_stage_coef(const ExCall& a, const cplx* __restrict__ Ps, int nr, cplx* sP) {
  for (int i = threadIdx.x; i < TILE * a.H_list; i += 256) {
    const int q = i / a.H_list, hp = i - q * a.H_list;
    sP[hp * TILE + q] = q < nr ? Ps[(size_t)q * a.H_list + hp] : make_double2(0.0, 0.0);
  }
}

template <int TILE>
__device__ inline void ex_store(const ExCall& a, long long s, int b, int r0, int nr, int h, cplx gj, const cplx* acc) {
  cplx* out = a.f + s * a.sys_stride + a.sm.rhs_off(b, a.H, a.hpos ? a.hpos[h] : h, a.elem_stride) + (long long)r0 * a.rhs_stride;
#pragma unroll
  for (int q = 0; q < TILE; ++q)
    if (q < nr) out[q * a.rhs_stride] = cscale(cfma(gj, acc[q], make_double2(0.0, 0.0)), -1.0);
}

// d >= 3.  T: the table rows [row][H2] of the slice.  LDS: sx = the row [H2], then the coefficient tile [H_list][TILE]
template <int TILE, bool LDS>
__global__ void __launch_bounds__(256) k_rhs_ex(ExCall a, int H2, long long rows, const uint32_t* __restrict__ ptr, const double* __restrict__ coef,
                                                 const uint16_t* __restrict__ tidx, const int* __restrict__ deg_list, const cplx* __restrict__ T) {
  extern __shared__ cplx sx[];
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    long long s; int b, r0, nr;
    ex_tile<TILE>(a, row, &s, &b, &r0, &nr);
    const cplx* __restrict__ Tr = T + row * H2;
    const cplx* __restrict__ Ps = a.P + ((a.p_batched ? s * a.nrhs : 0) + r0) * (long long)a.H_list;
    cplx* sP = sx + H2;
    if (LDS) {
      __syncthreads();                                  // the previous row is no longer read
      for (int i = threadIdx.x; i < H2; i += 256) sx[i] = Tr[i];
      ex_stage_coef<TILE>(a, Ps, nr, sP);
      __syncthreads();
    }
    const cplx* gj = a.tab + (s * a.B + b) * 3 * a.n_end;
    for (int h = threadIdx.x; h < a.H; h += 256) {
      const uint32_t* __restrict__ pe = ptr + (size_t)(a.map ? a.map[h] : h) * a.H_list;
      cplx acc[TILE];
#pragma unroll
      for (int q = 0; q < TILE; ++q) acc[q] = make_double2(0.0, 0.0);
      uint32_t p = pe[0];
      for (int hp = 0; hp < a.H_list; ++hp) {
        const uint32_t p1 = pe[hp + 1];
        if (deg_list[hp] >= a.n_in || p == p1) { p = p1; continue; }
        double er = 0.0, ei = 0.0;
        for (; p < p1; ++p) {
          const double c = coef[p];
          const cplx v = LDS ? sx[tidx[p]] : Tr[tidx[p]];
          er = fma(c, v.x, er); ei = fma(c, v.y, ei);
        }
        const cplx ent = make_double2(er, ei);
#pragma unroll
        for (int q = 0; q < TILE; ++q)
          if (q < nr) acc[q] = cfma(ent, LDS ? sP[hp * TILE + q] : Ps[(size_t)q * a.H_list + hp], acc[q]);
      }
      ex_store<TILE>(a, s, b, r0, nr, h, gj[a.deg[h]], acc);
    }
  }
}

// tree a.  labels / labels_list: (m, -, -) of the solve and of the list plan; n2 = 2 n_list - 1.  LDS: sx = the coefficient tile
template <bool REG, int TILE, bool LDS>
__global__ void __launch_bounds__(256) k_rhs_ex_2d(ExCall a, int n2, double Cd, long long rows, const int* __restrict__ labels,
                                                    const int* __restrict__ labels_list, const cplx* __restrict__ k,
                                                    const double* __restrict__ centers, int geom_batched, const double* __restrict__ org,
                                                    int org_batched) {
  __shared__ cplx sJ[kMaxRad * 2 + 6], sH[REG ? 1 : kMaxRad * 2 + 6], sE[kMaxRad * 4];
  extern __shared__ cplx sx[];
  const cplx* sR = REG ? sJ : sH;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    long long s; int b, r0, nr;
    ex_tile<TILE>(a, row, &s, &b, &r0, &nr);
    const MsRow w = ms_row(row, a.sr0, a.B, a.n_origin);
    double t[2], dist;
    ms_displacement(w, 2, a.B, a.n_origin, centers, geom_batched, org, org_batched, t, &dist);
    if (REG) ms_unit_if_zero(2, dist, t);
    __syncthreads();                                    // the previous row's tables are no longer read
    if (threadIdx.x == 0) ms_radial_row<REG>(2, n2 - 1, k[s], dist, sJ, sH);
    __syncthreads();
    const double phi = atan2(t[1], t[0]);
    for (int q = threadIdx.x; q < 2 * n2 - 1; q += 256) {
      const int mu = q - (n2 - 1);
      double sn, cs;
      sincos((double)mu * phi, &sn, &cs);
      sE[q] = cscale(cfma(cscale(sR[mu < 0 ? -mu : mu], Cd * kInvSqrt2Pi), make_double2(cs, sn), make_double2(0.0, 0.0)), kInvSqrt2Pi);    // k_rhs_ms_2d's entry
    }
    const cplx* __restrict__ Ps = a.P + ((a.p_batched ? s * a.nrhs : 0) + r0) * (long long)a.H_list;
    if (LDS) ex_stage_coef<TILE>(a, Ps, nr, sx);
    __syncthreads();
    const cplx* gj = a.tab + (s * a.B + b) * 3 * a.n_end;
    for (int h = threadIdx.x; h < a.H; h += 256) {
      const int m = labels[3 * h], am = m < 0 ? -m : m;
      cplx acc[TILE];
#pragma unroll
      for (int q = 0; q < TILE; ++q) acc[q] = make_double2(0.0, 0.0);
      for (int hp = 0; hp < a.H_list; ++hp) {
        const int mp = labels_list[3 * hp], amp = mp < 0 ? -mp : mp;
        if (amp >= a.n_in) continue;
        const int mu = mp - m, j = mu < 0 ? -mu : mu;
        const cplx ent = cscale(sE[mu + n2 - 1], ms_sign_even(am + j - amp));
#pragma unroll
        for (int q = 0; q < TILE; ++q)
          if (q < nr) acc[q] = cfma(ent, LDS ? sx[hp * TILE + q] : Ps[(size_t)q * a.H_list + hp], acc[q]);
      }
      ex_store<TILE>(a, s, b, r0, nr, h, gj[am], acc);
    }
  }
}

size_t lds_budget() {
  size_t cap = kLdsBudget;
  if (const char* e = getenv("BIEM_RHS_EX_LDS_BYTES")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v < cap) cap = (size_t)v;
  }
  return cap;
}

// more dynamic LDS than the default ceiling; per call, not per slice (the attribute is per device: no process-wide memo)
template <class K>
int allow_lds(K kernel, size_t shm) {
  if (shm > ((size_t)48 << 10)) BIEM_HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  return BIEM_OK;
}
}  // namespace

size_t rhs_expansion_workspace_bytes(const biem_plan* lp, int nb, int B, int n_origin) {
  if (nb <= 0 || B <= 0 || n_origin <= 0 || lp->tree == TREE_A) return 0;
  return align256((size_t)rhs_table_slice_pairs(lp, nb, B, n_origin) * B * lp->H2 * sizeof(cplx));
}

int launch_rhs_expansion(const biem_plan* p, const biem_plan* lp, const int* d_map, int n_in, bool regular, int nb, int B, int nrhs,
                         const double* d_k, const double* d_centers, int geom_batched, const double* d_tab, const double* d_origin,
                         int origin_batched, int n_origin, const double* d_coef, int coef_batched, double* d_f, long long sys_stride,
                         long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, int stage,
                         void* d_work) {
  const char* who = "biem_rhs_expansion";
  if (nrhs < 1) { set_error("%s: nrhs < 1", who); return BIEM_ERR_ARG; }
  if (n_origin != 1 && n_origin != nrhs) { set_error("%s: n_origin=%d is neither 1 nor nrhs=%d", who, n_origin, nrhs); return BIEM_ERR_ARG; }
  if (lp->tree != p->tree || lp->d != p->d || lp->n_end < p->n_end) {
    set_error("%s: the list plan (tree %d, d=%d, n_end=%d) is not a plan of the solve plan's tree (tree %d, d=%d) of order n_end=%d or more", who,
              lp->tree, lp->d, lp->n_end, p->tree, p->d, p->n_end);
    return BIEM_ERR_ARG;
  }
  if (n_in < 1 || n_in > lp->n_end) { set_error("%s: n_in=%d outside [1, n_end=%d of the list plan]", who, n_in, lp->n_end); return BIEM_ERR_ARG; }
  if (lp != p && !d_map) { set_error("%s: null d_map with a list plan of its own", who); return BIEM_ERR_ARG; }
  if (stage < 0 || stage > 2) { set_error("%s: stage=%d outside 0 .. 2", who, stage); return BIEM_ERR_ARG; }
  // (nb, nrhs <= 65535, the order limits and the term lists of the list plan: RhsSource::check has refused the rest)
  if (nb <= 0 || B <= 0) return BIEM_OK;
  const long long pairs = (long long)nb * n_origin;
  if (pairs * B > INT_MAX) { set_error("%s: %lld (origin, ball) pairs in one call, at most %d", who, pairs * B, INT_MAX); return BIEM_ERR_ARG; }
  ProfScope ps(PK_RHS, st, 0.0);
  const bool shared = n_origin == 1;
  const unsigned tiles = shared ? (unsigned)((nrhs + kTile - 1) / kTile) : 1u;
  ExCall a = {p->H, lp->H, p->n_end, n_in, B, nrhs, n_origin, 0, d_map, p->d_deg, slot_order ? p->d_hpos : nullptr, (const cplx*)d_tab,
              (const cplx*)d_coef, coef_batched, (cplx*)d_f, sys_stride, elem_stride, rhs_stride, split};
  const size_t coef_lds = (size_t)(shared ? kTile : 1) * lp->H * sizeof(cplx);
  if (p->tree == TREE_A) {
    if (stage == 1) return BIEM_OK;
    const size_t fixed = (size_t)((regular ? 1 : 2) * (kMaxRad * 2 + 6) + (regular ? 1 : 0) + kMaxRad * 4) * sizeof(cplx);
    const bool lds = fixed + coef_lds <= lds_budget();
    const size_t shm = lds ? coef_lds : 0;
    const dim3 grid(strided_grid(pairs * B), tiles);
#define BIEM_EX_2D(REG, TILE, LDS)                                                                                                         \
  {                                                                                                                                      \
    if (const int rc = allow_lds(k_rhs_ex_2d<REG, TILE, LDS>, shm)) return rc;                                                            \
    hipLaunchKernelGGL((k_rhs_ex_2d<REG, TILE, LDS>), grid, dim3(256), shm, st, a, lp->n2, p->Cd, pairs * B, p->d_labels, lp->d_labels,   \
                       (const cplx*)d_k, d_centers, geom_batched, d_origin, origin_batched);                                              \
  }
#define BIEM_EX_2D_REG(REG)                                                                                                                \
  {                                                                                                                                      \
    if (shared) { if (lds) BIEM_EX_2D(REG, kTile, true) else BIEM_EX_2D(REG, kTile, false) }                                              \
    else { if (lds) BIEM_EX_2D(REG, 1, true) else BIEM_EX_2D(REG, 1, false) }                                                             \
  }
    if (regular) BIEM_EX_2D_REG(true) else BIEM_EX_2D_REG(false)
#undef BIEM_EX_2D_REG
#undef BIEM_EX_2D
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  const size_t both = (size_t)lp->H2 * sizeof(cplx) + coef_lds;
  const bool lds = both <= lds_budget();
  const size_t shm = lds ? both : 0;
  const long long slice = rhs_table_slice_pairs(lp, nb, B, n_origin);
  cplx* T = (cplx*)d_work;
  for (long long sr0 = 0; sr0 < pairs; sr0 += slice) {
    const long long rows = (pairs - sr0 < slice ? pairs - sr0 : slice) * B;
    if (stage != 2) {
      if (const int rc = launch_translation_tables(lp, regular, B, n_origin, sr0, rows, d_k, d_centers, geom_batched, d_origin, origin_batched, 0,
                                                   (double*)T, st))
        return rc;
    }
    if (stage == 1) continue;
    a.sr0 = sr0;
    const dim3 grid(strided_grid(rows), tiles);
#define BIEM_EX(TILE, LDS)                                                                                                                 \
  {                                                                                                                                      \
    if (sr0 == 0) { if (const int rc = allow_lds(k_rhs_ex<TILE, LDS>, shm)) return rc; }                                                  \
    hipLaunchKernelGGL((k_rhs_ex<TILE, LDS>), grid, dim3(256), shm, st, a, lp->H2, rows, lp->d_ptr, lp->d_coef, lp->d_tidx16, lp->d_deg, T); \
  }
    if (shared) { if (lds) BIEM_EX(kTile, true) else BIEM_EX(kTile, false) }
    else { if (lds) BIEM_EX(1, true) else BIEM_EX(1, false) }
#undef BIEM_EX
    BIEM_LAUNCHCHK();
  }
  return BIEM_OK;
}

}  // namespace biem
