// kernels_cluster.hip -- the scattered field of the whole cluster as ONE outgoing expansion about an origin (gfx950).
//
// Ball b radiates sum_h c_{b,h} h_n(k |x - c_b|) Y_h((x - c_b)^), c = density * blc (kernels_uscat.hip).  Outside the sphere about o that
// holds every ball, |x - o| > max_b (|c_b - o| + rho_b), each of these is an outgoing expansion about o, translated by (S|S) = (R|R):
//   u_scat(x) = sum_h'' A_h'' h_n''(k |x - o|) Y_h''((x - o)^),     A[s][r][h''] = sum_b sum_h (R|R)_{h->h''}(o_s - c_b) c[s][r][b][h].
// d >= 3: (R|R)_{h->h''}(t) = sum_p coef[p] T[tidx[p]] over the plan's term list of entry e = h'' H + h, T[l] = C_d j_n(k |t|) Y_l(t^): the
// regular table rows of the regular-wave right-hand side (kernels_rhs_ms.hip, launch_regular_tables) with t taken from the other end.
// They do not depend on the right-hand side: one row per (system, ball).  Stages: c (one pass over the density) -> table rows of a
// slice of systems (the byte cap of the right-hand sides, BIEM_RHS_TABLE_BYTES) -> contraction, one lane per (system, h'') with a
// register tile of kTile right-hand sides: the lane walks the balls in index order and the entries e = h'' H + h, one contiguous run of
// ptr / coef / tidx16 per ball, forms each translation entry ONCE and applies it to the whole tile.  Every element of A is written by
// one lane, without atomics, in an order of summation (b, then h, then the list) that depends on neither the slices nor the tiles: the
// result is bit-reproducible.  Tree a: Graf's one term per entry (kernels_rhs_ms.hip), one workgroup per (system, tile of m''), the
// row J_j(k |t_b|) e^{i mu phi} in LDS ball by ball: no table, no lists, up to n_end = kMaxRad.
// t = 0 (the origin on a centre) is an ordinary displacement: the regular rows are formed without a division there.
#include "common.hpp"

namespace biem {
namespace {
constexpr int kTile = 8;                               // right-hand sides per lane (16 accumulator registers)
constexpr long long kGridMax = 1 << 20;
inline unsigned strided_grid(long long groups) { return (unsigned)(groups < 1 ? 1 : groups < kGridMax ? groups : kGridMax); }

__global__ void __launch_bounds__(256) k_cluster_ones(long long count, cplx* __restrict__ x) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) x[i] = make_double2(1.0, 0.0);
}

// c[s][r][b][h] = density[s][r][b][h] blc[s][b][h]
__global__ void __launch_bounds__(256) k_cluster_coef(int H, int B, int nrhs, long long count, const cplx* __restrict__ blc,
                                                       const cplx* __restrict__ density, cplx* __restrict__ c) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const int h = (int)(i % H);
    const long long srb = i / H;
    const int b = (int)(srb % B);
    const long long s = srb / B / nrhs;
    c[i] = cmul(density[i], blc[(s * B + b) * H + h]);
  }
}

// d >= 3: one lane per (system of the slice, h''), blockIdx.y = tile of right-hand sides.  T: the rows [sl B + b][H2] of the slice
__global__ void __launch_bounds__(256) k_cluster(int H, int H2, int B, int nrhs, int n_src, long long s0, long long count,
                                                  const uint32_t* __restrict__ ptr, const double* __restrict__ coef,
                                                  const uint16_t* __restrict__ tidx, const int* __restrict__ deg, const cplx* __restrict__ T,
                                                  const cplx* __restrict__ c, cplx* __restrict__ out) {
  const int r0 = blockIdx.y * kTile, nr = nrhs - r0 < kTile ? nrhs - r0 : kTile;
  const size_t rs = (size_t)B * H;                     // from one right-hand side of a system to the next
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const int hpp = (int)(i % H);
    const long long sl = i / H, s = s0 + sl;
    cplx acc[kTile];
#pragma unroll
    for (int q = 0; q < kTile; ++q) acc[q] = make_double2(0.0, 0.0);
    for (int b = 0; b < B; ++b) {
      const cplx* Tr = T + (sl * B + b) * H2;
      const cplx* cb = c + ((size_t)(s * nrhs + r0) * B + b) * H;
      const uint32_t* pe = ptr + (size_t)hpp * H;
      for (int h = 0; h < H; ++h) {
        const uint32_t p0 = pe[h], p1 = pe[h + 1];
        if (p0 == p1 || deg[h] >= n_src) continue;
        double er = 0.0, ei = 0.0;
        for (uint32_t p = p0; p < p1; ++p) {
          const double w = coef[p];
          const cplx v = Tr[tidx[p]];
          er = fma(w, v.x, er); ei = fma(w, v.y, ei);
        }
        const cplx ent = make_double2(er, ei);
#pragma unroll
        for (int q = 0; q < kTile; ++q)
          if (q < nr) acc[q] = cfma(ent, cb[q * rs + h], acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kTile; ++q)
      if (q < nr) out[(size_t)(s * nrhs + r0 + q) * H + hpp] = acc[q];
  }
}

__device__ inline double sign_even(int e) { return ((e / 2) & 1) ? -1.0 : 1.0; }      // i^e for even e (either sign)

// tree a: workgroup (tile of m'', system, tile of right-hand sides).  Per ball the row E[mu + n2 - 1] = C_2 J_|mu|(k |t|) e^{i mu phi} / (2 pi),
// |mu| < n2 = 2 n_end - 1, t = o - c_b, goes to LDS; (R|R)_{m->m''}(t) = i^{|m''| + |mu| - |m|} E[mu], mu = m - m''
__global__ void __launch_bounds__(256) k_cluster_2d(int n_end, int H, double Cd, const int* __restrict__ labels, int B, int nrhs, int n_src,
                                                     const cplx* __restrict__ k, const double* __restrict__ centers, int geom_batched,
                                                     const double* __restrict__ origin, int origin_batched, const cplx* __restrict__ c,
                                                     cplx* __restrict__ out) {
  __shared__ cplx sJ[kMaxRad * 2 + 6], sE[kMaxRad * 4];
  const int hpp = blockIdx.x * 256 + threadIdx.x;
  const long long s = blockIdx.y;
  const int r0 = blockIdx.z * kTile, nr = nrhs - r0 < kTile ? nrhs - r0 : kTile;
  const size_t rs = (size_t)B * H;
  const int n2 = 2 * n_end - 1;
  const bool live = hpp < H;
  const int mt = live ? labels[3 * hpp] : 0, amt = mt < 0 ? -mt : mt;
  const double* o = origin + (origin_batched ? s * 2 : 0);
  cplx acc[kTile];
#pragma unroll
  for (int q = 0; q < kTile; ++q) acc[q] = make_double2(0.0, 0.0);
  for (int b = 0; b < B; ++b) {
    const double* cc = centers + ((geom_batched ? s * B : 0) + b) * 2;
    const double tx = o[0] - cc[0], ty = o[1] - cc[1], dist = sqrt(tx * tx + ty * ty);
    __syncthreads();                                    // the previous ball's row is no longer read
    if (threadIdx.x == 0) {
      if (dist == 0.0) for (int j = 0; j < n2; ++j) sJ[j] = make_double2(j == 0 ? radial_z0_at_zero(2) : 0.0, 0.0);
      else radial_jh(2, n2 - 1, cscale(k[s], dist), sJ, nullptr);
    }
    __syncthreads();
    const double phi = dist == 0.0 ? 0.0 : atan2(ty, tx);
    for (int q = threadIdx.x; q < 2 * n2 - 1; q += 256) {
      const int mu = q - (n2 - 1);
      double sn, cs;
      sincos((double)mu * phi, &sn, &cs);
      sE[q] = cscale(cmul(cscale(sJ[mu < 0 ? -mu : mu], Cd * kInvSqrt2Pi), make_double2(cs, sn)), kInvSqrt2Pi);
    }
    __syncthreads();
    if (!live) continue;
    const cplx* cb = c + ((size_t)(s * nrhs + r0) * B + b) * H;
    for (int h = 0; h < H; ++h) {
      const int m = labels[3 * h], am = m < 0 ? -m : m;
      if (am >= n_src) continue;
      const int mu = m - mt, j = mu < 0 ? -mu : mu;
      const cplx ent = cscale(sE[mu + n2 - 1], sign_even(amt + j - am));
#pragma unroll
      for (int q = 0; q < kTile; ++q)
        if (q < nr) acc[q] = cfma(ent, cb[q * rs + h], acc[q]);
    }
  }
  if (!live) return;
#pragma unroll
  for (int q = 0; q < kTile; ++q)
    if (q < nr) out[(size_t)(s * nrhs + r0 + q) * H + hpp] = acc[q];
}

struct ClusterWork { size_t blc, c, table, total; long long slice; };
// blc [nb][B][H] | c [nb][nrhs][B][H] (first the ones blc is formed from) | the table rows of one slice of systems (tree a: none)
ClusterWork cluster_work(const biem_plan* p, int nb, int B, int nrhs) {
  ClusterWork w = {};
  if (nb <= 0 || B <= 0 || nrhs <= 0) return w;
  w.slice = p->tree == TREE_A ? nb : rhs_table_slice_pairs(p, nb, B, 1);
  w.blc = 0;
  w.c = align256((size_t)nb * B * p->H * sizeof(cplx));
  w.table = w.c + align256((size_t)nb * nrhs * B * p->H * sizeof(cplx));
  w.total = w.table + (p->tree == TREE_A ? 0 : align256((size_t)w.slice * B * p->H2 * sizeof(cplx)));
  return w;
}
}  // namespace

size_t cluster_coefficients_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs) { return cluster_work(p, nb, B, nrhs).total; }

int launch_cluster_coefficients(const biem_plan* p, int nb, int B, int nrhs, int n_src, const double* d_k, const double* d_eta,
                                const double* d_centers, const double* d_radii, int geom_batched, const double* d_origin, int origin_batched,
                                const double* d_density, double* d_out, int stage, void* d_work, size_t work_bytes, hipStream_t st) {
  const char* who = "biem_cluster_coefficients";
  if (const int rc = check_counts(who, nb, nrhs, B)) return rc;
  if (nrhs < 1) { set_error("%s: nrhs < 1", who); return BIEM_ERR_ARG; }
  if (n_src < 1 || n_src > p->n_end) { set_error("%s: n_src=%d outside [1, n_end=%d]", who, n_src, p->n_end); return BIEM_ERR_ARG; }
  if (stage < 0 || stage > 2) { set_error("%s: stage=%d outside 0 .. 2", who, stage); return BIEM_ERR_ARG; }
  // the order limits and the term lists are those of the translated right-hand sides: refused in their words
  if (const int rc = RhsSource::multipole_sources(nullptr, nullptr, 0, nullptr, nullptr, 0).check(who, p, nb, nrhs)) return rc;
  if (nb <= 0 || B <= 0) return BIEM_OK;
  const int H = p->H;
  const ClusterWork w = cluster_work(p, nb, B, nrhs);
  if (work_bytes < w.total) { set_error("%s: workspace too small (%zu < %zu)", who, work_bytes, w.total); return BIEM_ERR_ARG; }
  cplx* blc = (cplx*)((char*)d_work + w.blc);
  cplx* c = (cplx*)((char*)d_work + w.c);
  cplx* T = (cplx*)((char*)d_work + w.table);
  const int tiles = (nrhs + kTile - 1) / kTile;
  if (stage != 1) {
    const long long one = (long long)nb * B * H, all = one * nrhs;
    hipLaunchKernelGGL(k_cluster_ones, dim3(strided_grid((one + 255) / 256)), dim3(256), 0, st, one, c);
    BIEM_LAUNCHCHK();
    if (const int rc = uscat_form_coef(p, nb, B, d_k, d_eta, d_radii, geom_batched, (const double*)c, 0, blc, st)) return rc;
    hipLaunchKernelGGL(k_cluster_coef, dim3(strided_grid((all + 255) / 256)), dim3(256), 0, st, H, B, nrhs, all, blc, (const cplx*)d_density, c);
    BIEM_LAUNCHCHK();
  }
  if (p->tree == TREE_A) {
    if (stage == 1) return BIEM_OK;
    hipLaunchKernelGGL(k_cluster_2d, dim3((H + 255) / 256, nb, tiles), dim3(256), 0, st, p->n_end, H, p->Cd, p->d_labels, B, nrhs, n_src,
                       (const cplx*)d_k, d_centers, geom_batched, d_origin, origin_batched, c, (cplx*)d_out);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  for (long long s0 = 0; s0 < nb; s0 += w.slice) {
    const long long n = nb - s0 < w.slice ? nb - s0 : w.slice;
    // rows (system, ball): the "sources" are the origins, one per system, the displacement o - c_b
    if (stage != 2) {
      if (const int rc = launch_regular_tables(p, B, 1, s0, n * B, d_k, d_centers, geom_batched, d_origin, origin_batched, 1, (double*)T, st)) return rc;
    }
    if (stage != 1) {
      hipLaunchKernelGGL(k_cluster, dim3(strided_grid((n * H + 255) / 256), tiles), dim3(256), 0, st, H, p->H2, B, nrhs, n_src, s0, n * H, p->d_ptr,
                         p->d_coef, p->d_tidx16, p->d_deg, T, c, (cplx*)d_out);
      BIEM_LAUNCHCHK();
    }
  }
  return BIEM_OK;
}

}  // namespace biem
