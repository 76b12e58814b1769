// kernels_tables.hip -- what a fill reads: radial functions, harmonics, per-ball tables, per-pair translation tables in their four layouts and
// the pair classes of the symmetric fill, each with its launcher (gfx950).  The fills themselves: kernels_fill.hip, kernels_fill_sym.hip.
#include "fill.hpp"
#include <cstdlib>

namespace biem {

// ---------------------------------------------------------------------------------------------
// test entry: radial functions at arbitrary arguments
// ---------------------------------------------------------------------------------------------
__global__ void k_radial(int d, int nmax, int count, const double* __restrict__ x, double* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double* J = out + (size_t)i * 2 * (nmax + 1);
  double* Y = J + (nmax + 1);
  if (d == 4) {
    // needs one more order: compute integer orders 0..nmax+1 in place with a shifted write
    double xi = x[i];
    // order nmax+1 does not fit the output slot: run the recurrence with the last slot as scratch
    // (output layout leaves no spare element) -> compute J/Y of integer order via local arrays
    double lj[kMaxRad + 2], ly[kMaxRad + 2];
    bessel_jy_int(nmax + 1, xi, lj, ly);
    double f = kSqrtHalfPi / xi;
    for (int n = 0; n <= nmax; ++n) { J[n] = lj[n + 1] * f; Y[n] = ly[n + 1] * f; }
  } else if (d >= 5) {
    double lj[kMaxRad + 2 + kRadShiftMax], ly[kMaxRad + 2 + kRadShiftMax];
    radial_d(d, nmax, x[i], lj, ly);
    for (int n = 0; n <= nmax; ++n) { J[n] = lj[n]; Y[n] = ly[n]; }
  } else {
    radial_d(d, nmax, x[i], J, Y);
  }
}

// complex arguments: out[i][0][n] = z_n (regular), out[i][1][n] = h_n (outgoing), complex128
__global__ void k_radial_c(int d, int nmax, int count, const cplx* __restrict__ z, cplx* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  cplx lj[kMaxRad + 3 + kRadShiftMax], lh[kMaxRad + 3 + kRadShiftMax];
  radial_jh(d, nmax, z[i], lj, lh);
  cplx* J = out + (size_t)i * 2 * (nmax + 1);
  cplx* Hh = J + (nmax + 1);
  for (int n = 0; n <= nmax; ++n) { J[n] = lj[n]; Hh[n] = lh[n]; }
}

int launch_radial_c(int d, int nmax, int count, const double* d_z, double* d_out, hipStream_t st) {
  if (nmax < 0 || nmax > kMaxRad || d < 2 || d > kChainDimMax) { set_error("biem_radial_complex: bad d/nmax"); return BIEM_ERR_ARG; }
  if (count <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_radial_c, dim3((count + 63) / 64), dim3(64), 0, st, d, nmax, count, (const cplx*)d_z, (cplx*)d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_radial(int d, int nmax, int count, const double* d_x, double* d_out, hipStream_t st) {
  if (nmax < 0 || nmax > kMaxRad || d < 2 || d > kChainDimMax) { set_error("biem_radial: bad d/nmax"); return BIEM_ERR_ARG; }
  if (count <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_radial, dim3((count + 63) / 64), dim3(64), 0, st, d, nmax, count, d_x, d_out);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// test entry + building block: all harmonics of degree < n_end at given directions
// ---------------------------------------------------------------------------------------------
__global__ void k_harmonics(int tree, int d, int H, const int* __restrict__ labels, int count,
                            const double* __restrict__ u, cplx* __restrict__ Y) {
  int p = blockIdx.x;
  if (p >= count) return;
  double v[4];
  for (int i = 0; i < d; ++i) v[i] = u[(size_t)p * d + i];
  Dir dir = make_dir(tree, v);
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    double re, im;
    harmonic_single(tree, labels[3 * h], labels[3 * h + 1], labels[3 * h + 2], dir, &re, &im);
    Y[(size_t)p * H + h] = make_double2(re, im);
  }
}

// chain trees: every label from scratch (test entry; the fill and the field evaluation use node tables)
__global__ void k_harmonics_chain(int d, int H, const int* __restrict__ labels, int count, const double* __restrict__ u, cplx* __restrict__ Y) {
  int p = blockIdx.x;
  if (p >= count) return;
  double c[kChainDimMax], s[kChainDimMax], phi;
  chain_angles(d, u + (size_t)p * d, c, s, &phi);
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    double re, im;
    chain_harmonic(d, labels + (size_t)h * (d - 1), c, s, phi, &re, &im);
    Y[(size_t)p * H + h] = make_double2(re, im);
  }
}

int launch_harmonics(const biem_plan* p, int count, const double* d_u, double* d_Y, hipStream_t st) {
  if (count <= 0) return BIEM_OK;
  if (p->tree == TREE_CHAIN) {
    hipLaunchKernelGGL(k_harmonics_chain, dim3(count), dim3(128), 0, st, p->d, p->H, p->d_labels, count, d_u, (cplx*)d_Y);
    BIEM_LAUNCHCHK();
    return BIEM_OK;
  }
  hipLaunchKernelGGL(k_harmonics, dim3(count), dim3(128), 0, st, p->tree, p->d, p->H, p->d_labels, count, d_u, (cplx*)d_Y);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
// K0a: per-ball tables  gj_n = alpha j_n + beta k j_n',  gh_n = alpha h_n + beta k h_n',  blc = dlc - i eta slc
//   (ush.harmonics_regular_singular_component x4 + potential_coef S/D, _biem.py:723-789)
// one thread per (system, ball); outputs tab[s][b][3][n_end] complex.
// PER_DEGREE: alpha / beta [nb or 1][B][n_end], one pair per degree, else [nb or 1][B].  The arithmetic per degree is
// the same text, so degree-constant coefficients give the scalar table.
// ---------------------------------------------------------------------------------------------
template <bool PER_DEGREE>
__global__ void k_ball_tables(int d, int n_end, int nb, int B, const cplx* __restrict__ k, const double* __restrict__ eta,
                              const double* __restrict__ radii, int geom_batched, const cplx* __restrict__ alpha,
                              const cplx* __restrict__ beta, int ab_batched, cplx* __restrict__ tab, cplx* __restrict__ scratch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * B) return;
  int s = i / B, b = i % B;
  const cplx kk = k[s];
  const double et = eta[s];
  double rho = radii[(geom_batched ? (size_t)s * B : 0) + b];
  const cplx* al = alpha + ((ab_batched ? (size_t)s * B : 0) + b) * (PER_DEGREE ? n_end : 1);
  const cplx* be = beta + ((ab_batched ? (size_t)s * B : 0) + b) * (PER_DEGREE ? n_end : 1);
  cplx a0 = make_double2(0.0, 0.0), b0 = a0;       // one pair per ball: read here, in front of the radial functions, as it always was
  if (!PER_DEGREE) { a0 = al[0]; b0 = be[0]; }
  // orders up to kMaxRad: thread-local arrays; beyond (2-D only): 2 (n_end + 3) complex of global scratch per (system, ball)
  cplx Jl[kMaxRad + 3], Hl[kMaxRad + 3];
  cplx* J = scratch ? scratch + (size_t)i * 2 * (n_end + 3) : Jl;
  cplx* Hh = scratch ? J + (n_end + 3) : Hl;
  const cplx x = cscale(kk, rho);
  radial_jh(d, n_end, x, J, Hh);   // orders 0..n_end (one extra for the derivative); Im k = 0 takes the real routines
  const cplx ix = crecip(x);
  cplx* out = tab + (size_t)i * 3 * n_end;
  double rp = 1.0;               // rho^{d-1}
  for (int q = 0; q < d - 1; ++q) rp *= rho;
  cplx kd2 = make_double2(1.0, 0.0);   // k^{d-2}
  for (int q = 0; q < d - 2; ++q) kd2 = cmul(kd2, kk);
  for (int n = 0; n < n_end; ++n) {
    const cplx j = J[n], h = Hh[n];
    const cplx jp = csub(cscale(cmul(ix, j), (double)n), J[n + 1]);
    const cplx hp = csub(cscale(cmul(ix, h), (double)n), Hh[n + 1]);
    const cplx kjp = cmul(kk, jp), khp = cmul(kk, hp);
    // gj = alpha j + beta k j',  gh = alpha h + beta k h'
    const cplx a = PER_DEGREE ? al[n] : a0, bt = PER_DEGREE ? be[n] : b0;
    cplx gj = cadd(cmul(a, j), cmul(bt, kjp));
    cplx gh = cadd(cmul(a, h), cmul(bt, khp));
    // blc = i k^{d-1} rho^{d-1} j' - i eta * i k^{d-2} rho^{d-1} j = k^{d-2} rho^{d-1} (eta j + i k j')
    cplx blc = cscale(cmul(kd2, make_double2(et * j.x - kjp.y, et * j.y + kjp.x)), rp);
    out[n] = gj;
    out[n_end + n] = gh;
    out[2 * n_end + n] = blc;
  }
}

template <bool PER_DEGREE>
static int launch_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii, int geom_batched,
                         const double* d_alpha, const double* d_beta, int ab_batched, double* d_tab, hipStream_t st) {
  if (p->n_end > kMaxRad && p->tree != TREE_A) { set_error("n_end=%d exceeds the built table size %d", p->n_end, kMaxRad); return BIEM_ERR_UNSUPPORTED; }
  int total = nb * B;
  if (total <= 0) return BIEM_OK;
  ProfScope ps(PK_TABLES, st);
  cplx* scratch = nullptr;
  if (p->n_end > kMaxRad) BIEM_HIPCHK(hipMallocAsync((void**)&scratch, (size_t)total * 2 * (p->n_end + 3) * sizeof(cplx), st));   // (2-D, large orders: stream-ordered)
  hipLaunchKernelGGL(k_ball_tables<PER_DEGREE>, dim3((total + 63) / 64), dim3(64), 0, st, p->d, p->n_end, nb, B, (const cplx*)d_k, d_eta, d_radii,
                     geom_batched, (const cplx*)d_alpha, (const cplx*)d_beta, ab_batched, (cplx*)d_tab, scratch);
  BIEM_LAUNCHCHK();
  if (scratch) BIEM_HIPCHK(hipFreeAsync(scratch, st));
  return BIEM_OK;
}

int launch_ball_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                       int geom_batched, const double* d_alpha, const double* d_beta, int ab_batched, double* d_tab, hipStream_t st) {
  return launch_tables<false>(p, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha, d_beta, ab_batched, d_tab, st);
}

int launch_ball_tables_n(const biem_plan* p, int nb, int B, const double* d_k, const double* d_eta, const double* d_radii,
                         int geom_batched, const double* d_alpha_n, const double* d_beta_n, int ab_batched, double* d_tab, hipStream_t st) {
  return launch_tables<true>(p, nb, B, d_k, d_eta, d_radii, geom_batched, d_alpha_n, d_beta_n, ab_batched, d_tab, st);
}

// ---------------------------------------------------------------------------------------------
// K0b: per-pair translation tables  T[s][b][b'][l] = C_d h_{n''}(k |t|) Y_l(t^),  t = c_b - c_b'
//   (argument order of _biem.py:694-699), l over labels of degree < 2 n_end - 1.
// One wave per (system, ordered pair): lane 0 runs the radial recurrences into LDS, then all lanes
// evaluate harmonics.  Diagonal pairs are skipped (the reference evaluates them at t = 0 and masks
// the inf/nan afterwards, _biem.py:745-746).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_pair_tables(int tree, int d, int n2, int H2, double Cd, const int* __restrict__ labels2,
                                                     const int* __restrict__ deg2, int B, const cplx* __restrict__ k,
                                                     const double* __restrict__ centers, int geom_batched, cplx* __restrict__ T,
                                                     int lower, int nbp, const int* __restrict__ lin2, int H2lin,
                                                     const int* __restrict__ red_of = nullptr, const int* __restrict__ red_first = nullptr,
                                                     const int* __restrict__ ph_mu = nullptr, int E = 0, int NP = 0,
                                                     const cplx* __restrict__ tab = nullptr, int n_end = 0, cplx* __restrict__ rad_scratch = nullptr,
                                                     const int* __restrict__ rep_flag = nullptr) {
  __shared__ cplx sJl[kMaxRad * 2 + 6];
  __shared__ cplx sHl[kMaxRad * 2 + 6];
  int pair = blockIdx.x, s = blockIdx.y;
  // radial functions of the pair: LDS up to order 2 kMaxRad; beyond (2-D only) 2 (n2 + 6) complex of global scratch per block (written by
  // thread 0, read by the block after the barrier: same CU, fresh addresses)
  cplx* sJ = rad_scratch ? rad_scratch + ((size_t)s * gridDim.x + pair) * 2 * (n2 + 6) : sJl;
  cplx* sH = rad_scratch ? sJ + (n2 + 6) : sHl;
  int b = pair / B, bp = pair % B;
  // both fills contract the blocks b < bp (the general fill derives block (bp, b) from (b, bp) by the parity sign, the symmetric
  // fill writes the upper triangle only); lower = 1 (tables of the pairs b > bp instead) is kept for tests
  if (lower ? b <= bp : b >= bp) return;
  if (rep_flag != nullptr && !rep_flag[b * B + bp]) return;      // pair classes: only a class's first pair is read by the fill
  const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
  const double* cp = centers + ((geom_batched ? (size_t)s * B : 0) + bp) * d;
  double t[4];
  double r2 = 0.0;
  for (int i = 0; i < d; ++i) { t[i] = cb[i] - cp[i]; r2 += t[i] * t[i]; }
  double r = sqrt(r2);
  if (threadIdx.x == 0) radial_jh(d, n2 - 1, cscale(k[s], r), sJ, sH);
  __syncthreads();
  Dir dir = make_dir(tree, t);
  if (red_of != nullptr) {
    // reduced table of the entry-per-lane symmetric fill (plan.hpp): T'[e] = C_d h_{n''} x (real angular factor of the unit's first
    // member: the harmonic at zero azimuth), then the NP phases e^{i mu . phi}
    // ... and the per-degree factors q = gj / sqrt(gj gh) of the row ball b and of the column ball bp (the kernel multiplies the block by
    // q_b[n] q_bp[n']): a table row is everything a (pair, system) combination of the fill needs, E + NP + 2 n_end complex numbers
    cplx* o = T + ((size_t)s * B * B + pair) * (size_t)(E + NP + 2 * n_end);
    for (int i = threadIdx.x; i < 2 * n_end; i += 64) {
      const int which = i >= n_end, n = i - which * n_end;
      const cplx* tb = tab + ((size_t)s * B + (which ? bp : b)) * 3 * n_end;
      o[E + NP + i] = cmul(tb[n], crecip(zsqrt(cmul(tb[n], tb[n_end + n]))));
    }
    if (tree == TREE_BA) {
      for (int m = threadIdx.x; m < n2; m += 64) {          // one lane per |mu|: the degree recurrence of Pbar_n^m once
        double pmm = 0.70710678118654752440;
        for (int i = 1; i <= m; ++i) pmm *= sqrt((double)(2 * i + 1) / (double)(2 * i)) * dir.s0;
        double p0 = 0.0, p1 = pmm;
        for (int n = m; n < n2; ++n) {
          if (n > m) {
            double p2;
            if (n == m + 1) p2 = sqrt((double)(2 * m + 3)) * dir.c0 * pmm;
            else {
              const double a = sqrt((double)(4 * n * n - 1) / (double)(n * n - m * m));
              const double bq = sqrt((double)((n - 1) * (n - 1) - m * m) / (double)(4 * (n - 1) * (n - 1) - 1));
              p2 = a * (dir.c0 * p1 - bq * p0);
            }
            p0 = p1; p1 = p2;
          }
          o[red_of[n * n + n - m]] = cscale(sH[n], Cd * p1 * kInvSqrt2Pi);       // label (n, -m) is the first member of its unit
        }
      }
    } else {
      Dir d0 = dir; d0.phi = 0.0; d0.phi2 = 0.0;
      for (int l = threadIdx.x; l < H2; l += 64) {
        if (!red_first[l]) continue;
        double re, im;
        harmonic_single(tree, labels2[3 * l], labels2[3 * l + 1], labels2[3 * l + 2], d0, &re, &im);
        o[red_of[l]] = cscale(sH[deg2[l]], Cd * re);
      }
    }
    for (int i = threadIdx.x; i < NP; i += 64) {
      double sn, cs;
      sincos((double)ph_mu[2 * i] * dir.phi + (double)ph_mu[2 * i + 1] * dir.phi2, &sn, &cs);
      o[E + i] = make_double2(cs, sn);
    }
    return;
  }
  // nbp > 0: systems-in-lanes layout Tt[group of 64 systems][pair index of (b < bp)][l][system in group]: a group's table rows are
  // contiguous 1-KiB lines (with the systems of ALL groups in one row, the rows one group reads lie 4 KiB apart and every
  // workgroup of a fill - they all work on the same group at a time - hits the same quarter of the L2 channels)
  cplx* out = nbp > 0 ? T + (((size_t)(s >> 6) * (B * (B - 1) / 2) + (bp * (bp - 1) / 2 + b)) * H2) * 64 + (s & 63) : T + ((size_t)s * B * B + pair) * H2;
  const size_t ostride = nbp > 0 ? 64 : 1;
  auto emit = [&](int l, cplx val, bool self_conjugate) {
    if (lin2 == nullptr) { out[(size_t)l * ostride] = val; return; }
    // paired layout of the entry-per-lane symmetric fill: conjugate partners adjacent, a self-conjugate label in both places
    cplx* o2 = T + ((size_t)s * B * B + pair) * H2lin;
    const int i = lin2[l];
    o2[i] = val;
    if (self_conjugate) o2[i + 1] = val;
  };
  if (tree == TREE_BA) {
    // d = 3: one lane per order |m| runs the degree recurrence of Pbar_n^m ONCE (n = m .. n2-1) and writes both signs; evaluating
    // every label from scratch (generic branch below) repeats that recurrence, square roots and divisions included, per label:
    // 10 ms per 256 systems of cfg 3 against the fill's 47
    for (int m = threadIdx.x; m < n2; m += 64) {
      double sn, cs;
      sincos((double)m * dir.phi, &sn, &cs);
      double pmm = 0.70710678118654752440;
      for (int i = 1; i <= m; ++i) pmm *= sqrt((double)(2 * i + 1) / (double)(2 * i)) * dir.s0;
      double p0 = 0.0, p1 = pmm;
      for (int n = m; n < n2; ++n) {
        if (n > m) {
          double p2;
          if (n == m + 1) p2 = sqrt((double)(2 * m + 3)) * dir.c0 * pmm;
          else {
            const double a = sqrt((double)(4 * n * n - 1) / (double)(n * n - m * m));
            const double bq = sqrt((double)((n - 1) * (n - 1) - m * m) / (double)(4 * (n - 1) * (n - 1) - 1));
            p2 = a * (dir.c0 * p1 - bq * p0);
          }
          p0 = p1; p1 = p2;
        }
        const double amp = p1 * kInvSqrt2Pi;
        const cplx h = cscale(sH[n], Cd);
        const int l0 = n * n + n;
        emit(l0 + m, cmul(h, make_double2(amp * cs, amp * sn)), m == 0);
        if (m > 0) emit(l0 - m, cmul(h, make_double2(amp * cs, -amp * sn)), false);
      }
    }
    return;
  }
  for (int l = threadIdx.x; l < H2; l += 64) {
    double re, im;
    harmonic_single(tree, labels2[3 * l], labels2[3 * l + 1], labels2[3 * l + 2], dir, &re, &im);
    int n = deg2[l];
    const cplx val = cmul(cscale(sH[n], Cd), make_double2(re, im));
    emit(l, val, labels2[3 * l + (tree == TREE_A ? 0 : 2)] == 0 && (tree != TREE_CAA || labels2[3 * l + 1] == 0));
  }
}

// Pair tables of the chain trees (same outputs and arguments as k_pair_tables).  Every label is a product of d - 2 polar node
// factors F_j[l_j][l_{j+1}] = sin^{l_{j+1}} t_j Gbar_{l_j - l_{j+1}}^{(l_{j+1} + (d-j-2)/2)}(cos t_j) (l_{d-2} = |m|) and one phase: one
// lane per (node j, l_{j+1}) runs the Gegenbauer degree recurrence once per (pair, system) into LDS, then every label is d - 2
// lookups - the pattern of the ba branch above, one table per node.
__global__ void __launch_bounds__(64) k_pair_tables_chain(int tree, int d, int n2, int H2, double Cd, const int* __restrict__ labels2,
                                                           const int* __restrict__ deg2, int B, const cplx* __restrict__ k,
                                                           const double* __restrict__ centers, int geom_batched, cplx* __restrict__ T,
                                                           int lower, int nbp, const int* __restrict__ lin2, int H2lin,
                                                           const int* __restrict__ red_of, const int* __restrict__ red_first,
                                                           const int* __restrict__ ph_mu, int E, int NP,
                                                           const cplx* __restrict__ tab, int n_end, cplx* __restrict__ rad_scratch,
                                                           const int* __restrict__ rep_flag) {
  __shared__ cplx sJ[kMaxRad * 2 + 6], sH[kMaxRad * 2 + 6];
  __shared__ double sF[kChainNodeTab];                 // [j][L][L1], n2 x n2 per node
  __shared__ double sC[kChainDimMax], sS[kChainDimMax], sPhi;
  (void)tree; (void)rad_scratch;
  int pair = blockIdx.x, s = blockIdx.y;
  int b = pair / B, bp = pair % B;
  if (lower ? b <= bp : b >= bp) return;
  if (rep_flag != nullptr && !rep_flag[b * B + bp]) return;
  const double* cb = centers + ((geom_batched ? (size_t)s * B : 0) + b) * d;
  const double* cp = centers + ((geom_batched ? (size_t)s * B : 0) + bp) * d;
  const int np = d - 2, lw = d - 1;
  if (threadIdx.x == 0) {
    double t[kChainDimMax];
    double r2 = 0.0;
    for (int i = 0; i < d; ++i) { t[i] = cb[i] - cp[i]; r2 += t[i] * t[i]; }
    radial_jh(d, n2 - 1, cscale(k[s], sqrt(r2)), sJ, sH);
    double phi;
    chain_angles(d, t, sC, sS, &phi);
    sPhi = phi;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np * n2; i += 64) {
    const int j = i / n2, L1 = i - j * n2;
    const double lam = (double)L1 + 0.5 * (d - j - 2), c = sC[j], sn = sS[j];
    double sl = 1.0;
    for (int q = 0; q < L1; ++q) sl *= sn;
    // orthonormal Gegenbauer recurrence of gbar_lam in the degree k = L - L1
    double p0 = sl / sqrt(sqrt(kPi) * exp(lgamma(lam + 0.5) - lgamma(lam + 1.0))), p1 = 0.0, aprev = 0.0;
    double* F = sF + ((size_t)j * n2) * n2 + L1;
    for (int L = L1; L < n2; ++L) {
      const int kq = L - L1;
      if (kq > 0) {
        const double aq = 0.5 * sqrt((double)kq * ((double)kq + 2.0 * lam - 1.0) / (((double)kq + lam - 1.0) * ((double)kq + lam)));
        const double p2 = (c * p0 - aprev * p1) / aq;
        p1 = p0; p0 = p2; aprev = aq;
      }
      F[(size_t)L * n2] = p0;
    }
  }
  __syncthreads();
  auto amp_of = [&](int l) {
    const int* lb = labels2 + (size_t)l * lw;
    double a = Cd * kInvSqrt2Pi;
    for (int j = 0; j < np; ++j) {
      const int L1 = j + 1 < np ? lb[j + 1] : (lb[lw - 1] < 0 ? -lb[lw - 1] : lb[lw - 1]);
      a *= sF[((size_t)j * n2 + lb[j]) * n2 + L1];
    }
    return a;
  };
  if (red_of != nullptr) {
    cplx* o = T + ((size_t)s * B * B + pair) * (size_t)(E + NP + 2 * n_end);
    for (int i = threadIdx.x; i < 2 * n_end; i += 64) {
      const int which = i >= n_end, n = i - which * n_end;
      const cplx* tb = tab + ((size_t)s * B + (which ? bp : b)) * 3 * n_end;
      o[E + NP + i] = cmul(tb[n], crecip(zsqrt(cmul(tb[n], tb[n_end + n]))));
    }
    for (int l = threadIdx.x; l < H2; l += 64) {
      if (!red_first[l]) continue;
      o[red_of[l]] = cscale(sH[deg2[l]], amp_of(l));
    }
    for (int i = threadIdx.x; i < NP; i += 64) {
      double sn, cs;
      sincos((double)ph_mu[2 * i] * sPhi, &sn, &cs);
      o[E + i] = make_double2(cs, sn);
    }
    return;
  }
  cplx* out = nbp > 0 ? T + (((size_t)(s >> 6) * (B * (B - 1) / 2) + (bp * (bp - 1) / 2 + b)) * H2) * 64 + (s & 63) : T + ((size_t)s * B * B + pair) * H2;
  const size_t ostride = nbp > 0 ? 64 : 1;
  for (int l = threadIdx.x; l < H2; l += 64) {
    const int m = labels2[(size_t)l * lw + lw - 1];
    double sn, cs;
    sincos((double)m * sPhi, &sn, &cs);
    const cplx val = cmul(cscale(sH[deg2[l]], amp_of(l)), make_double2(cs, sn));
    if (lin2 == nullptr) { out[(size_t)l * ostride] = val; continue; }
    cplx* o2 = T + ((size_t)s * B * B + pair) * H2lin;
    const int i = lin2[l];
    o2[i] = val;
    if (m == 0) o2[i + 1] = val;
  }
}

typedef decltype(&k_pair_tables) PairTablesKernel;
// the pair-table kernel of a plan: the chain trees have their own (node tables), every other tree k_pair_tables
static PairTablesKernel pair_tables_kernel(const biem_plan* p) { return p->tree == TREE_CHAIN ? &k_pair_tables_chain : &k_pair_tables; }

// The one place that writes the pair-table kernels' argument list.  Radial functions of a pair: LDS up to order 2 kMaxRad; the reduced
// rows of a 2-D order beyond that take stream-ordered global scratch (only the list-free 2-D fills get there: the list forms stop at fill_lists_order_ok)
int launch_pair_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched, const double* d_tab,
                       PairTableMode mode, const int* rep_flag, cplx* T, hipStream_t st) {
  if (B <= 1) return BIEM_OK;
  const bool red = mode == PT_REDUCED, paired = mode == PT_PAIRED;
  cplx* scratch = nullptr;
  if (red && p->n2 + 6 > kMaxRad * 2 + 6) {
    if (p->tree != TREE_A) { set_error("n_end=%d exceeds the built table size", p->n_end); return BIEM_ERR_UNSUPPORTED; }
    BIEM_HIPCHK(hipMallocAsync((void**)&scratch, (size_t)nb * B * B * 2 * (p->n2 + 6) * sizeof(cplx), st));
  }
  hipLaunchKernelGGL(pair_tables_kernel(p), dim3(B * B, nb), dim3(64), 0, st, p->tree, p->d, p->n2, p->H2, p->Cd, p->d_labels2, p->d_deg2, B,
                     (const cplx*)d_k, d_centers, geom_batched, T, 0, mode == PT_SYS_LANES ? (nb + 63) / 64 * 64 : 0,
                     paired ? p->d_lin2 : nullptr, paired ? p->H2lin : 0, red ? p->d_red_of : nullptr, red ? p->d_red_first : nullptr,
                     red ? p->d_ph_mu : nullptr, red ? p->E : 0, red ? p->NP : 0, red ? (const cplx*)d_tab : nullptr, red ? p->n_end : 0,
                     scratch, rep_flag);
  BIEM_LAUNCHCHK();
  if (scratch) BIEM_HIPCHK(hipFreeAsync(scratch, st));
  return BIEM_OK;
}

// ---------------------------------------------------------------------------------------------
constexpr int kDedupeMaxPairs = 2048;       // (the class search is quadratic in the pairs, in one workgroup)
// Pair classes (FillDedupe, common.hpp).  Upper pairs are numbered pr = bp (bp - 1) / 2 + b, b < bp.  out: [0] = number of classes,
// [4 ..] rep_list[class] = its first pair, then dup_ptr[class .. class + 1] into dup_bb[] = (b << 16 | bp) of the class's pairs
// (the representative first).  enable = 0: every pair its own class.  One workgroup; quadratic search, npairs <= kDedupeMaxPairs.
__global__ void __launch_bounds__(256) k_pair_dedupe(int B, int d, int npairs, const double* __restrict__ centers, const double* __restrict__ radii,
                                                      const double* __restrict__ alpha, const double* __restrict__ beta, int enable,
                                                      int* __restrict__ out) {
  extern __shared__ int sd_int[];
  int* cls = sd_int;                 // [B] first ball with the same (radius, alpha, beta)
  int* rep = cls + B;                // [npairs] first pair of the same class
  int* cnt = rep + npairs;           // [npairs] members per representative, then write cursors
  int* rep_list = out + 4;
  int* dup_ptr = rep_list + npairs;
  int* dup_bb = dup_ptr + npairs + 1;
  int* rep_flag = dup_bb + npairs;            // [B * B]
  const int tid = threadIdx.x;
  for (int e = tid; e < B * B; e += 256) rep_flag[e] = enable ? 0 : 1;
  auto pair_of = [&](int pr, int& b, int& bp) {
    int bb = (int)((sqrtf(8.0f * (float)pr + 1.0f) + 1.0f) * 0.5f);
    while (bb * (bb - 1) / 2 > pr) --bb;
    while ((bb + 1) * bb / 2 <= pr) ++bb;
    bp = bb; b = pr - bb * (bb - 1) / 2;
  };
  if (!enable) {
    for (int p = tid; p < npairs; p += 256) { int b, bp; pair_of(p, b, bp); rep_list[p] = p; dup_ptr[p] = p; dup_bb[p] = b << 16 | bp; }
    if (tid == 0) { out[0] = npairs; dup_ptr[npairs] = npairs; }
    return;
  }
  for (int b = tid; b < B; b += 256) {
    int c = b;
    for (int b2 = 0; b2 < b; ++b2)
      if (radii[b2] == radii[b] && alpha[2 * b2] == alpha[2 * b] && alpha[2 * b2 + 1] == alpha[2 * b + 1] && beta[2 * b2] == beta[2 * b] &&
          beta[2 * b2 + 1] == beta[2 * b + 1]) { c = b2; break; }
    cls[b] = c;
  }
  __syncthreads();
  // per pair: its ball classes (packed) and its displacement, once - the quadratic search below then only compares
  int* key = cnt + npairs;                                   // [npairs] cls[b] << 16 | cls[bp]
  double* disp = (double*)(key + npairs + ((B + 3 * npairs) & 1));    // [npairs][d], 8-byte aligned
  for (int p = tid; p < npairs; p += 256) {
    int b, bp; pair_of(p, b, bp);
    key[p] = cls[b] << 16 | cls[bp];
    for (int i = 0; i < d; ++i) disp[p * d + i] = centers[bp * d + i] - centers[b * d + i];
  }
  __syncthreads();
  // displacements equal up to the rounding of the subtraction (a lattice with a pitch that is no binary fraction: 2.1 - 1.4 and
  // 1.4 - 0.7 differ in the last place): 32 ulp of the largest coordinate; an exact lattice matches bit for bit either way
  double cmax = 0.0;
  for (int e = 0; e < B * d; ++e) cmax = fmax(cmax, fabs(centers[e]));
  const double tol = 32.0 * 2.220446049250313e-16 * cmax;
  for (int p = tid; p < npairs; p += 256) {
    int r = p;
    const int kp = key[p];
    for (int q = 0; q < p; ++q) {
      if (key[q] != kp) continue;
      bool same = true;
      for (int i = 0; i < d; ++i) same = same && (fabs(disp[q * d + i] - disp[p * d + i]) <= tol);
      if (same) { r = q; break; }
    }
    rep[p] = r; cnt[p] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    for (int p = 0; p < npairs; ++p) if (rep[p] != p) rep[p] = rep[rep[p]];     // (near-equality need not be transitive: resolve chains; rep[q], q < p, is final)
    for (int p = 0; p < npairs; ++p) cnt[rep[p]]++;
    int nrep = 0, pos = 0;
    for (int p = 0; p < npairs; ++p)
      if (rep[p] == p) { rep_list[nrep] = p; dup_ptr[nrep] = pos; pos += cnt[p]; cnt[p] = dup_ptr[nrep]; rep[p] = -nrep - 1; ++nrep;   // rep[p] < 0: class index
                         int b, bp; pair_of(p, b, bp); rep_flag[b * B + bp] = 1; }
    dup_ptr[nrep] = pos;
    out[0] = nrep;
    for (int p = 0; p < npairs; ++p) {           // pairs in ascending order: the representative is the first of its class
      const int r = rep[p] < 0 ? p : rep[p];
      int b, bp; pair_of(p, b, bp);
      dup_bb[cnt[r]++] = b << 16 | bp;
    }
  }
}


// Classes are on for a call with shared geometry and coefficients of at least 8 systems (a handful of systems: fewer, longer combinations
// would leave most of the chip without a workgroup - one N = 4064 system filled in 0.49 instead of 0.17 ms with classes - so every pair
// stays on its own below 8 systems); BIEM_FILL_DEDUPE_MIN (tests: classes for small batches too), BIEM_FILL_NO_DEDUPE
int launch_pair_classes(const biem_plan* p, int nb, int B, const double* d_centers, int geom_batched, const FillDedupe* dedupe,
                        const PairClasses& pc, hipStream_t st) {
  const int npairs = B * (B - 1) / 2;
  const char* mn = getenv("BIEM_FILL_DEDUPE_MIN");
  const bool on = dedupe && !geom_batched && nb >= (mn ? atoi(mn) : 8) && npairs <= kDedupeMaxPairs && B <= 65535 && !getenv("BIEM_FILL_NO_DEDUPE");
  const size_t shm_dd = on ? (size_t)(B + 3 * npairs + 2) * sizeof(int) + (size_t)npairs * p->d * sizeof(double) : 0;
  if (shm_dd > 48 * 1024) BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_pair_dedupe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_dd));
  hipLaunchKernelGGL(k_pair_dedupe, dim3(1), dim3(256), shm_dd, st, B, p->d, npairs, d_centers,
                     on ? dedupe->radii : nullptr, on ? dedupe->alpha : nullptr, on ? dedupe->beta : nullptr, on ? 1 : 0, pc.classes);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_classes_and_tables(const SymFill& c, PairTableMode mode) {
  const int rc = launch_pair_classes(c.p, c.nb, c.B, c.d_centers, c.geom_batched, c.dedupe, c.pc, c.st);
  return rc ? rc : launch_pair_tables(c.p, c.nb, c.B, c.d_k, c.d_centers, c.geom_batched, c.d_tab, mode, c.pc.rep_flag, c.T, c.st);
}

}  // namespace biem
