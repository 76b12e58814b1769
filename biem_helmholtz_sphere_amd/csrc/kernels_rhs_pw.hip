// kernels_rhs_pw.hip -- right-hand sides of plane-wave incidence in closed form (gfx950): no samples, no projection.
//
// With the radial normalisation of special.hpp and orthonormal harmonics, u_in = e^{i k p^.x} projects on the surface of ball b to
//   U_h = C_d i^n j_n(k rho) conj(Y_h(p^)) e^{i k p^.c_b},   V_h = C_d i^n k j_n'(k rho) conj(Y_h(p^)) e^{i k p^.c_b}
// (C_d = 2^{(d+1)/2} pi^{(d-1)/2}, the plan's Cd), so
//   f(s, r, b, h) = -(alpha U_h + beta V_h) = -C_d i^{n(h)} gj_{n(h)}(s, b) conj(Y_h(p^_r)) e^{i k_s p^_r.c_b}
// with gj = alpha j_n + beta k j_n' row 0 of the ball tables (degree-dependent coefficients included).  Written where
// launch_rhs_project writes: s sys_stride + split.rhs_off(b, H, slot of h, elem_stride) + r rhs_stride.
#include "common.hpp"

namespace biem {
namespace {
// e^{i k t} for complex k: exp(-Im k t) (cos(Re k t) + i sin(Re k t)); scaled by -C_d once per (s, r, b)
__device__ inline cplx pw_phase(cplx k, const double* __restrict__ p, const double* __restrict__ c, int d, double scale) {
  double t = 0.0;
  for (int i = 0; i < d; ++i) t += p[i] * c[i];
  double sn, cs;
  sincos(k.x * t, &sn, &cs);
  const double a = (k.y != 0.0 ? exp(-k.y * t) : 1.0) * scale;
  return make_double2(a * cs, a * sn);
}

// i^n z by swapping and negating components
__device__ inline cplx mul_i_pow(cplx z, int n) {
  switch (n & 3) {
    case 0: return z;
    case 1: return make_double2(-z.y, z.x);
    case 2: return make_double2(-z.x, -z.y);
    default: return make_double2(z.y, -z.x);
  }
}

// harmonics [dir][h] -> [sys][h][r] (r contiguous), 32 x 32 tiles through LDS; grid (H / 32, nrhs / 32, systems of directions)
__global__ void __launch_bounds__(256) k_pw_transpose(int H, int nrhs, const cplx* __restrict__ Y, cplx* __restrict__ Yt) {
  __shared__ cplx tile[32][33];
  const int h0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const cplx* src = Y + (size_t)blockIdx.z * nrhs * H;
  cplx* dst = Yt + (size_t)blockIdx.z * nrhs * H;
  for (int j = ty; j < 32; j += 8)
    if (r0 + j < nrhs && h0 + tx < H) tile[j][tx] = src[(size_t)(r0 + j) * H + h0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (h0 + j < H && r0 + tx < nrhs) dst[(size_t)(h0 + j) * nrhs + r0 + tx] = tile[tx][j];
}

// h along the lanes: a workgroup takes 256 harmonics of one (s, r, b); grid (H / 256 x B, nrhs, nb)
__global__ void __launch_bounds__(256) k_rhs_pw_h(int d, int H, int n_end, int B, int nrhs, double Cd, const cplx* __restrict__ k,
                                                   const double* __restrict__ centers, int geom_batched, const cplx* __restrict__ tab,
                                                   const double* __restrict__ dirs, int dirs_batched, const cplx* __restrict__ Y,
                                                   const int* __restrict__ deg, cplx* __restrict__ f, long long sys_stride,
                                                   long long elem_stride, long long rhs_stride, const int* __restrict__ hpos, SplitMap sm) {
  __shared__ cplx sph;
  const int hb = (H + 255) / 256;
  const int b = blockIdx.x / hb, h = (blockIdx.x - b * hb) * 256 + threadIdx.x, r = blockIdx.y, s = blockIdx.z;
  const size_t dir = (dirs_batched ? (size_t)s * nrhs : 0) + r;
  if (threadIdx.x == 0)
    sph = pw_phase(k[s], dirs + dir * d, centers + ((geom_batched ? (size_t)s * B : 0) + b) * d, d, -Cd);
  __syncthreads();
  if (h >= H) return;
  const int n = deg[h];
  const cplx y = Y[dir * H + h];
  const cplx v = cmul(cmul(tab[((size_t)s * B + b) * 3 * n_end + n], sph), make_double2(y.x, -y.y));
  f[(long long)s * sys_stride + sm.rhs_off(b, H, hpos ? hpos[h] : h, elem_stride) + (long long)r * rhs_stride] = mul_i_pow(v, n);
}

// r along the lanes (rhs_stride == 1): a workgroup takes 64 right-hand sides of one (s, b), its four waves every fourth harmonic;
// harmonics read as Yt[h][r], rows of f written 64 consecutive complex at a time; grid (nrhs / 64 x B, nb)
__global__ void __launch_bounds__(256) k_rhs_pw_r(int d, int H, int n_end, int B, int nrhs, double Cd, const cplx* __restrict__ k,
                                                   const double* __restrict__ centers, int geom_batched, const cplx* __restrict__ tab,
                                                   const double* __restrict__ dirs, int dirs_batched, const cplx* __restrict__ Yt,
                                                   const int* __restrict__ deg, cplx* __restrict__ f, long long sys_stride,
                                                   long long elem_stride, const int* __restrict__ hpos, SplitMap sm) {
  __shared__ cplx sph[64];
  const int rb = (nrhs + 63) / 64;
  const int b = blockIdx.x / rb, r = (blockIdx.x - b * rb) * 64 + (threadIdx.x & 63), s = blockIdx.y;
  const size_t dsys = dirs_batched ? (size_t)s : 0;
  if (threadIdx.x < 64 && r < nrhs)
    sph[threadIdx.x] = pw_phase(k[s], dirs + (dsys * nrhs + r) * d, centers + ((geom_batched ? (size_t)s * B : 0) + b) * d, d, -Cd);
  __syncthreads();
  if (r >= nrhs) return;
  const cplx ph = sph[threadIdx.x & 63];
  const cplx* tb = tab + ((size_t)s * B + b) * 3 * n_end;
  const cplx* yt = Yt + dsys * nrhs * H + r;
  cplx* fs = f + (long long)s * sys_stride + r;
  for (int h = threadIdx.x >> 6; h < H; h += 4) {
    const int n = deg[h];
    const cplx y = yt[(size_t)h * nrhs];
    const cplx v = cmul(cmul(tb[n], ph), make_double2(y.x, -y.y));
    fs[sm.rhs_off(b, H, hpos ? hpos[h] : h, elem_stride)] = mul_i_pow(v, n);
  }
}
}  // namespace

int launch_transpose_rows(int cols, int rows, int batches, const double* d_in, double* d_out, hipStream_t st) {
  hipLaunchKernelGGL(k_pw_transpose, dim3((cols + 31) / 32, (rows + 31) / 32, batches), dim3(256), 0, st, cols, rows, (const cplx*)d_in, (cplx*)d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

size_t rhs_plane_wave_workspace_bytes(const biem_plan* p, int nb, int nrhs, int dirs_batched) {
  if (nb <= 0 || nrhs <= 0) return 0;
  // the harmonics of the directions [dir][H], and their copy [h][r] per system of directions for the form with r along the lanes
  return 2 * align256((size_t)(dirs_batched ? nb : 1) * nrhs * p->H * sizeof(cplx));
}

int launch_rhs_plane_wave(const biem_plan* p, int nb, int B, int nrhs, const double* d_k, const double* d_centers, int geom_batched,
                          const double* d_tab, const double* d_dirs, int dirs_batched, double* d_f, long long sys_stride,
                          long long elem_stride, long long rhs_stride, hipStream_t st, bool slot_order, const SplitMap& split, void* d_work) {
  if (nrhs < 1) { set_error("biem_rhs_plane_wave: nrhs < 1"); return BIEM_ERR_ARG; }
  // (nb, nrhs <= 65535: grid dimensions - RhsSource::check has refused the rest)
  if (nb <= 0 || B <= 0) return BIEM_OK;
  const int H = p->H, dsys = dirs_batched ? nb : 1;
  ProfScope ps(PK_RHS, st, 0.0);
  cplx* Y = (cplx*)d_work;
  cplx* Yt = (cplx*)((char*)d_work + align256((size_t)dsys * nrhs * H * sizeof(cplx)));
  if (const int rc = launch_harmonics(p, dsys * nrhs, d_dirs, (double*)Y, st)) return rc;
  const int* hpos = slot_order ? p->d_hpos : nullptr;
  // consecutive right-hand sides of a row contiguous and at least a wave of them: r along the lanes; else h along the lanes
  if (rhs_stride == 1 && nrhs >= 64) {
    if (const int rc = launch_transpose_rows(H, nrhs, dsys, (const double*)Y, (double*)Yt, st)) return rc;
    hipLaunchKernelGGL(k_rhs_pw_r, dim3((nrhs + 63) / 64 * B, nb), dim3(256), 0, st, p->d, H, p->n_end, B, nrhs, p->Cd, (const cplx*)d_k,
                       d_centers, geom_batched, (const cplx*)d_tab, d_dirs, dirs_batched, Yt, p->d_deg, (cplx*)d_f, sys_stride,
                       elem_stride, hpos, split);
  } else {
    hipLaunchKernelGGL(k_rhs_pw_h, dim3((H + 255) / 256 * B, nrhs, nb), dim3(256), 0, st, p->d, H, p->n_end, B, nrhs, p->Cd, (const cplx*)d_k,
                       d_centers, geom_batched, (const cplx*)d_tab, d_dirs, dirs_batched, Y, p->d_deg, (cplx*)d_f, sys_stride,
                       elem_stride, rhs_stride, hpos, split);
  }
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
