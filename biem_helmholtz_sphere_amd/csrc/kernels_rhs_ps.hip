// kernels_rhs_ps.hip -- right-hand sides of point-source incidence in closed form (gfx950): no samples, no projection.
//
// With the radial normalisation of special.hpp and orthonormal harmonics, the monopole u_in = h_0(k |x - s|) projects on the surface of
// ball b, t = s - c_b and |t| > rho_b, to
//   U_h = C_d j_n(k rho) h_n(k |t|) conj(Y_h(t^)),   V_h = C_d k j_n'(k rho) h_n(k |t|) conj(Y_h(t^))
// (C_d = 2^{(d+1)/2} pi^{(d-1)/2}, the plan's Cd), so
//   f(s, r, b, h) = -(alpha U_h + beta V_h) = -C_d gj_{n(h)}(s, b) h_{n(h)}(k_s |t_{r,b}|) conj(Y_h(t^_{r,b}))
// with gj = alpha j_n + beta k j_n' row 0 of the ball tables (degree-dependent coefficients included).  Written where
// launch_rhs_project writes: s sys_stride + split.rhs_off(b, H, slot of h, elem_stride) + r rhs_stride.
//
// Nothing here tests |t| > rho: a source on or inside a sphere gives finite values that mean nothing, t = 0 gives non-finite ones.
//
// Stages: geometry (t, |t|, t^ per direction system, source, ball) -> launch_harmonics at the t^ -> radial table
// G = -C_d gj_n h_n(k_s |t|) per (system, source, ball) by radial_jh -> combine f = G conj(Y).  Direction systems: nb when the geometry
// or the sources differ between the systems, else 1; the wavenumber differs always, so G is per system.  Every grid is flat and
// strided, every index 64-bit: nb nrhs B exceeds a grid dimension at production shapes.
#include "common.hpp"
#include <climits>

namespace biem {
namespace {
constexpr long long kGridMax = 1 << 20;      // workgroups of a strided launch (256 CUs: thousands per CU are plenty)
inline unsigned strided_grid(long long groups) { return (unsigned)(groups < kGridMax ? groups : kGridMax); }

struct PsWork { double* unit; double* dist; cplx* Y; cplx* Yt; cplx* G; size_t total; };
PsWork ps_layout(const biem_plan* p, int nb, int B, int nrhs, int dsys, void* base) {
  const size_t pts = (size_t)dsys * nrhs * B;
  char* w = (char*)base;
  size_t o = 0;
  PsWork L;
  L.unit = (double*)(w + o); o = align256(o + pts * p->d * sizeof(double));
  L.dist = (double*)(w + o); o = align256(o + pts * sizeof(double));
  L.Y = (cplx*)(w + o); o = align256(o + pts * p->H * sizeof(cplx));
  L.Yt = (cplx*)(w + o); o = align256(o + pts * p->H * sizeof(cplx));
  L.G = (cplx*)(w + o); o = align256(o + (size_t)nb * nrhs * B * p->n_end * sizeof(cplx));
  L.total = o;
  return L;
}

// t = s - c, |t| and t^ of every (direction system ds, source r, ball b), point index (ds nrhs + r) B + b; one lane each
__global__ void __launch_bounds__(256) k_ps_geometry(int d, int B, int nrhs, long long count, const double* __restrict__ centers,
                                                      int geom_batched, const double* __restrict__ src, int src_batched,
                                                      double* __restrict__ unit, double* __restrict__ dist) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const int b = (int)(i % B);
    const long long sr = i / B;
    const int r = (int)(sr % nrhs);
    const long long ds = sr / nrhs;
    const double* c = centers + ((geom_batched ? ds * B : 0) + b) * d;
    const double* s = src + ((src_batched ? ds * nrhs : 0) + r) * d;
    double t[kChainDimMax], m = 0.0, r2 = 0.0;
    for (int j = 0; j < d; ++j) { t[j] = s[j] - c[j]; m = fmax(m, fabs(t[j])); }
    for (int j = 0; j < d; ++j) { t[j] /= m; r2 += t[j] * t[j]; }       // (scaled: no overflow or underflow of the squares)
    const double n = sqrt(r2);
    for (int j = 0; j < d; ++j) unit[i * d + j] = t[j] / n;
    dist[i] = m * n;
  }
}

// G = -C_d gj_n(s, b) h_n(k_s |t|), n < n_end, of every (s, r, b): one lane per triple, thread-local radial arrays as k_radial_c.
// r_major == 0: lane index (s nrhs + r) B + b, G[(s nrhs + r) B + b][n] (the form with h along the lanes);
// r_major != 0: lane index (s B + b) nrhs + r, G[s B + b][n][r] (the form with r along the lanes reads and this writes r contiguous)
__global__ void __launch_bounds__(64) k_ps_radial(int d, int n_end, int B, int nrhs, long long count, int dsys_batched, double Cd,
                                                   const cplx* __restrict__ k, const cplx* __restrict__ tab,
                                                   const double* __restrict__ dist, int r_major, cplx* __restrict__ G) {
  cplx lj[kMaxRad + 3 + kRadShiftMax], lh[kMaxRad + 3 + kRadShiftMax];
  for (long long i = (long long)blockIdx.x * 64 + threadIdx.x; i < count; i += (long long)gridDim.x * 64) {
    int b, r;
    long long s;
    if (r_major) { r = (int)(i % nrhs); b = (int)(i / nrhs % B); s = i / nrhs / B; }
    else { b = (int)(i % B); r = (int)(i / B % nrhs); s = i / B / nrhs; }
    const double rt = dist[((dsys_batched ? s * nrhs : 0) + r) * B + b];
    radial_jh(d, n_end - 1, cscale(k[s], rt), lj, lh);
    const cplx* gj = tab + (s * B + b) * 3 * n_end;
    if (r_major) {
      cplx* g = G + (s * B + b) * n_end * nrhs + r;
      for (int n = 0; n < n_end; ++n) g[(long long)n * nrhs] = cscale(cmul(gj[n], lh[n]), -Cd);
    } else {
      cplx* g = G + i * n_end;
      for (int n = 0; n < n_end; ++n) g[n] = cscale(cmul(gj[n], lh[n]), -Cd);
    }
  }
}

// h along the lanes: a workgroup takes 256 harmonics of one (s, r, b); work items (s, r, b, block of h), strided
__global__ void __launch_bounds__(256) k_rhs_ps_h(int H, int n_end, int B, int nrhs, long long items, int dsys_batched,
                                                   const cplx* __restrict__ G, const cplx* __restrict__ Y, const int* __restrict__ deg,
                                                   cplx* __restrict__ f, long long sys_stride, long long elem_stride, long long rhs_stride,
                                                   const int* __restrict__ hpos, SplitMap sm) {
  const int hb = (H + 255) / 256;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int h = (int)(w % hb) * 256 + threadIdx.x;
    if (h >= H) continue;
    const long long srb = w / hb;
    const int b = (int)(srb % B), r = (int)(srb / B % nrhs);
    const long long s = srb / B / nrhs;
    const cplx y = Y[(((dsys_batched ? s * nrhs : 0) + r) * B + b) * H + h];
    f[s * sys_stride + sm.rhs_off(b, H, hpos ? hpos[h] : h, elem_stride) + r * rhs_stride] = cmulc(G[srb * n_end + deg[h]], y);
  }
}

// r along the lanes (rhs_stride == 1): a workgroup takes 64 right-hand sides of one (s, b), its four waves every fourth harmonic;
// G[s B + b][n][r] and Yt[ds][b H + h][r] read, rows of f written, 64 consecutive complex at a time; work items (s, b, block of r), strided
__global__ void __launch_bounds__(256) k_rhs_ps_r(int H, int n_end, int B, int nrhs, long long items, int dsys_batched,
                                                   const cplx* __restrict__ G, const cplx* __restrict__ Yt, const int* __restrict__ deg,
                                                   cplx* __restrict__ f, long long sys_stride, long long elem_stride,
                                                   const int* __restrict__ hpos, SplitMap sm) {
  const int rb = (nrhs + 63) / 64;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int r = (int)(w % rb) * 64 + (threadIdx.x & 63);
    if (r >= nrhs) continue;
    const long long sb = w / rb;
    const int b = (int)(sb % B);
    const long long s = sb / B;
    const cplx* g = G + sb * n_end * nrhs + r;
    const cplx* yt = Yt + ((dsys_batched ? s * B : 0) + b) * H * nrhs + r;
    cplx* fs = f + s * sys_stride + r;
    for (int h = threadIdx.x >> 6; h < H; h += 4)
      fs[sm.rhs_off(b, H, hpos ? hpos[h] : h, elem_stride)] = cmulc(g[(long long)deg[h] * nrhs], yt[(long long)h * nrhs]);
  }
}
}  // namespace

size_t rhs_point_source_workspace_bytes(const biem_plan* p, int nb, int B, int nrhs, int src_batched, int geom_batched) {
  if (nb <= 0 || B <= 0 || nrhs <= 0) return 0;
  return ps_layout(p, nb, B, nrhs, (src_batched || geom_batched) ? nb : 1, nullptr).total;
}

int launch_rhs_point_source(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                            const double* d_tab, const double* d_src, int src_batched, double* d_f, long long sys_stride,
                            long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work) {
  if (nrhs < 1) { set_error("biem_rhs_point_source: nrhs < 1"); return BIEM_ERR_ARG; }
  // (nb, nrhs <= 65535: grid dimensions, n_end <= kMaxRad: the arrays of k_ps_radial - RhsSource::check has refused the rest)
  if (nb <= 0 || B <= 0) return BIEM_OK;
  const int H = p->H, n_end = p->n_end, batched = (src_batched || geom_batched) ? 1 : 0, dsys = batched ? nb : 1;
  const long long pts = (long long)dsys * nrhs * B, triples = (long long)nb * nrhs * B;
  if (pts > INT_MAX) { set_error("biem_rhs_point_source: %lld (source, ball) pairs in one call, at most %d", pts, INT_MAX); return BIEM_ERR_ARG; }
  ProfScope ps(PK_RHS, st, 0.0);
  const PsWork W = ps_layout(p, nb, B, nrhs, dsys, d_work);
  hipLaunchKernelGGL(k_ps_geometry, dim3(strided_grid((pts + 255) / 256)), dim3(256), 0, st, p->d, B, nrhs, pts, d_centers, geom_batched,
                     d_src, src_batched, W.unit, W.dist);
  BIEM_LAUNCHCHK();
  if (const int rc = launch_harmonics(p, (int)pts, W.unit, (double*)W.Y, st)) return rc;
  const int* hpos = slot_order ? p->d_hpos : nullptr;
  // consecutive right-hand sides of a row contiguous and at least a wave of them: r along the lanes; else h along the lanes
  const int r_major = (rhs_stride == 1 && nrhs >= 64) ? 1 : 0;
  hipLaunchKernelGGL(k_ps_radial, dim3(strided_grid((triples + 63) / 64)), dim3(64), 0, st, p->d, n_end, B, nrhs, triples, batched, p->Cd,
                     (const cplx*)d_k, (const cplx*)d_tab, W.dist, r_major, W.G);
  BIEM_LAUNCHCHK();
  if (r_major) {
    // per direction system [r][b H + h] -> [b H + h][r]
    if (const int rc = launch_transpose_rows(B * H, nrhs, dsys, (const double*)W.Y, (double*)W.Yt, st)) return rc;
    const long long items = (long long)nb * B * ((nrhs + 63) / 64);
    hipLaunchKernelGGL(k_rhs_ps_r, dim3(strided_grid(items)), dim3(256), 0, st, H, n_end, B, nrhs, items, batched, W.G, W.Yt, p->d_deg,
                       (cplx*)d_f, sys_stride, elem_stride, hpos, split);
  } else {
    const long long items = triples * ((H + 255) / 256);
    hipLaunchKernelGGL(k_rhs_ps_h, dim3(strided_grid(items)), dim3(256), 0, st, H, n_end, B, nrhs, items, batched, W.G, W.Y, p->d_deg,
                       (cplx*)d_f, sys_stride, elem_stride, rhs_stride, hpos, split);
  }
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
