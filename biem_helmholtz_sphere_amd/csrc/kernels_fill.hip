// kernels_fill.hip -- the general matrix fill (reference / equilibrated scaling), the form decision of the symmetric fill and the fill
// workspace (gfx950).  Tables: kernels_tables.hip; the symmetric fill: kernels_fill_sym.hip; right-hand sides: kernels_rhs.hip.
//
// Replaces the span _biem.py:694-792 (matrix) of the reference, which there is ~40 array-API ops and 3-5 full-size temporaries; here
// every matrix element is written exactly once.
#include "fill.hpp"
#include <cstdlib>

namespace biem {

// ---------------------------------------------------------------------------------------------
// K1-K3: generic fill.  For every ordered pair block (b, b') and every entry (h, h'):
//   off-diagonal:  A = R_b[n(h)] * Cc_{b'}[n(h')] * sum_p coef[p] T_{bb'}[tidx[p]]        ((S|R)^T, _biem.py:769)
//   diagonal    :  A = delta_{hh'} * Dg_b[n(h)]
// with (R, Cc, Dg) = (gj, blc, gh*blc) for the reference scaling (_biem.py:745-789) and (gj, 1/gh, 1) for the
// equilibrated system the LU factors.
// One 1024-thread workgroup per (entry chunk, ball b, system).  The chunk's slice of the term list (8-byte coefficient +
// 2-byte table index per term) and its row pointers are loaded into LDS ONCE and reused for all partner balls b'; per
// partner only its pair table T (H2 complex) and column factors are staged.  Every thread keeps two independent entries
// in flight (the per-term chain idx -> T -> fma is LDS-latency bound).  The first version (256 threads, term list from
// L2 for every pair) ran at 487 GB/s (profiles/r01_bench_cfg3_32sys.json).  Consecutive lanes own consecutive columns
// h': 16-byte coalesced stores, every matrix element written exactly once.
// ---------------------------------------------------------------------------------------------
constexpr int FILL_THREADS = 1024;

__global__ void __launch_bounds__(FILL_THREADS) k_fill(int H, int H2, int n_end, int B, const int* __restrict__ deg,
                                                        const int* __restrict__ chunk_ent, int chunk_terms_max, int chunk_ents_max,
                                                        const uint32_t* __restrict__ ptr, const double* __restrict__ coef,
                                                        const uint16_t* __restrict__ tidx, const cplx* __restrict__ T,
                                                        const cplx* __restrict__ tab, int scaling, cplx* __restrict__ A,
                                                        long long lda, long long sys_stride, int table_global) {
  extern __shared__ char smem[];
  // table_global: the pair table is read where it lies (global memory, served by L2) - orders whose table does not fit LDS; the
  // generic pointer sT then addresses global memory and nothing is staged
  cplx* const sTl = (cplx*)smem;                        // [H2] pair table T_{b,bp}
  cplx* sC = table_global ? sTl : sTl + H2;             // [H] column factors of the partner ball bp
  cplx* sC2 = sC + H;                                   // [H] column factors of the owner ball b (mirrored block)
  double* sCoef = (double*)(sC2 + H);                   // [chunk_terms_max]
  uint32_t* sPtr = (uint32_t*)(sCoef + chunk_terms_max);   // [chunk_ents_max + 1], relative to the chunk's first term
  uint16_t* sIdx = (uint16_t*)(sPtr + chunk_ents_max + 1);
  const int chunk = blockIdx.x, s = blockIdx.z, tid = threadIdx.x;
  const int e0 = chunk_ent[chunk], e1 = chunk_ent[chunk + 1], nent = e1 - e0;
  const uint32_t t0 = ptr[e0], t1 = ptr[e1];
  for (uint32_t q = t0 + tid; q < t1; q += FILL_THREADS) { sCoef[q - t0] = coef[q]; sIdx[q - t0] = tidx[q]; }
  for (int e = tid; e <= nent; e += FILL_THREADS) sPtr[e] = ptr[e0 + e] - t0;
  cplx* As = A + (size_t)s * sys_stride;
  auto colfac = [&](const cplx* tball, int hp) {        // column factor of a ball for harmonic hp
    const int n = deg[hp];
    return scaling == BIEM_FILL_REFERENCE ? tball[2 * n_end + n] : crecip(tball[n_end + n]);
  };
  // the raw sum of an entry is shared by the two blocks of an unordered pair: T_{bp,b}[l] = (-1)^{n''} T_{b,bp}[l] (harmonics of
  // degree n'' at -t) and every term of entry (h, h') has n'' = n + n' (mod 2), so S_{bp,b}[h,h'] = (-1)^{n+n'} S_{b,bp}[h,h'].
  // A workgroup owns balls b1 = blockIdx.y and b2 = B-1-b1 and contracts each with its partners bp > b: B-1 contractions per
  // workgroup whatever b1 is, half the contractions of the one-block-per-contraction form.
  const int b1 = blockIdx.y, b2 = B - 1 - b1;
  for (int own = 0; own < 2; ++own) {
    const int b = own == 0 ? b1 : b2;
    if (own == 1 && b2 == b1) break;
    const cplx* tb = tab + ((size_t)s * B + b) * 3 * n_end;
    {  // diagonal block of b
      cplx* Ab = As + ((size_t)b * H) * lda + (size_t)b * H;
      for (int e = tid; e < nent; e += FILL_THREADS) {
        int h = (e0 + e) / H, hp = (e0 + e) - h * H;
        cplx v = make_double2(0.0, 0.0);
        if (hp == h) {
          int n = deg[h];
          v = scaling == BIEM_FILL_REFERENCE ? cmul(tb[n_end + n], tb[2 * n_end + n]) : make_double2(1.0, 0.0);
        }
        Ab[(size_t)h * lda + hp] = v;
      }
    }
    if (b + 1 >= B) continue;
    __syncthreads();                                     // previous owner's sC2 no longer in use (also orders the chunk loads)
    for (int hp = tid; hp < H; hp += FILL_THREADS) sC2[hp] = colfac(tb, hp);
    for (int bp = b + 1; bp < B; ++bp) {
      const cplx* tbp = tab + ((size_t)s * B + bp) * 3 * n_end;
      const cplx* Tp = T + ((size_t)s * B * B + (size_t)b * B + bp) * H2;
      cplx* Ab = As + ((size_t)b * H) * lda + (size_t)bp * H;     // block (b, bp)
      cplx* Am = As + ((size_t)bp * H) * lda + (size_t)b * H;     // block (bp, b)
      __syncthreads();                                   // previous partner's table no longer in use
      const cplx* sT = table_global ? Tp : sTl;
      if (!table_global) for (int l = tid; l < H2; l += FILL_THREADS) sTl[l] = Tp[l];
      for (int hp = tid; hp < H; hp += FILL_THREADS) sC[hp] = colfac(tbp, hp);
      __syncthreads();
      auto put = [&](int e, double sr, double si) {
        const int h = (e0 + e) / H, hp = (e0 + e) - h * H;
        const int nh = deg[h];
        const cplx raw = make_double2(sr, si);
#ifdef BIEM_ABL_FILL_NOSTORE       // timing ablation: results computed, not stored
        const cplx v1 = cmul(cmul(raw, tb[nh]), sC[hp]);
        const cplx m = cmul(cmul(raw, tbp[nh]), sC2[hp]);
        asm volatile("" ::"v"(v1.x), "v"(v1.y), "v"(m.x), "v"(m.y));
        (void)Ab; (void)Am;
#else
        Ab[(size_t)h * lda + hp] = cmul(cmul(raw, tb[nh]), sC[hp]);
        const cplx m = cmul(cmul(raw, tbp[nh]), sC2[hp]);
        Am[(size_t)h * lda + hp] = ((nh + deg[hp]) & 1) ? make_double2(-m.x, -m.y) : m;
#endif
      };
      for (int e = tid; e < nent; e += 2 * FILL_THREADS) {
        const int eb = e + FILL_THREADS;
        const bool two = eb < nent;
        uint32_t p0 = sPtr[e], p1 = sPtr[e + 1];
        uint32_t q0 = two ? sPtr[eb] : 0, q1 = two ? sPtr[eb + 1] : 0;
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
        while (p0 < p1 && q0 < q1) {                     // two independent chains
          double c = sCoef[p0], d = sCoef[q0];
          cplx t = sT[sIdx[p0]], u = sT[sIdx[q0]];
          ar = fma(c, t.x, ar); ai = fma(c, t.y, ai);
          br = fma(d, u.x, br); bi = fma(d, u.y, bi);
          ++p0; ++q0;
        }
        for (; p0 < p1; ++p0) { double c = sCoef[p0]; cplx t = sT[sIdx[p0]]; ar = fma(c, t.x, ar); ai = fma(c, t.y, ai); }
        for (; q0 < q1; ++q0) { double d = sCoef[q0]; cplx u = sT[sIdx[q0]]; br = fma(d, u.x, br); bi = fma(d, u.y, bi); }
        put(e, ar, ai);
        if (two) put(eb, br, bi);
      }
    }
  }
}

__global__ void k_fill_pad(int N, int n_pad, cplx* __restrict__ A, long long lda, long long sys_stride) {
  int s = blockIdx.y;
  cplx* As = A + (size_t)s * sys_stride;
  int npadrows = n_pad - N;
  // region 1: rows [N, n_pad) x cols [0, n_pad);  region 2: rows [0, N) x cols [N, n_pad)
  long long total1 = (long long)npadrows * n_pad, total2 = (long long)N * npadrows;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total1 + total2; i += (long long)gridDim.x * blockDim.x) {
    int r, c;
    if (i < total1) { r = N + (int)(i / n_pad); c = (int)(i % n_pad); }
    else { long long q = i - total1; r = (int)(q / npadrows); c = N + (int)(q % npadrows); }
    As[(size_t)r * lda + c] = (r == c) ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0);
  }
}

// ---------------------------------------------------------------------------------------------
// 2-D fills without term lists (tree a, any order).  Graf's theorem leaves ONE term per entry,
//     S(m, m') = i^{|m| + |mu| - |m'|} T[mu] / sqrt(2 pi),   mu = m' - m,   T[mu] = T'[|mu|] e^{i mu phi},   T'[j] = C_2 H_j(k|t|) / sqrt(2 pi)
// (the 1 / sqrt(2 pi) in front is the triple integral of three circular harmonics - the coefficient of the plan's one-term lists),
// so a block is a Toeplitz matrix in (m, m') up to signs: every thread evaluates its entries from the table row of the pair
// (k_pair_tables in reduced mode: T'[0 .. 2 n_end - 2], the phases e^{i j phi}, j >= 0, and the q factors of the two balls) read
// straight from global memory - consecutive lanes read consecutive entries, the row (at most 6 n_end complex numbers) stays in L1 /
// L2 - and stores them.  No LDS, no term lists: the plan of a 2-D order beyond kLists2dMax holds none (they would be H^2 = 47 M
// one-term entries at the reference's n_end = 3444, accuracy/accuracy_k_a.csv), and the kernels are bound by their stores.
// ---------------------------------------------------------------------------------------------
__device__ inline double sign_even(int e) { return ((e / 2) & 1) ? -1.0 : 1.0; }      // i^e for even e (either sign)

// general form (reference / equilibrated scaling, natural order of the harmonics: m = 0 .. n-1, -(n-1) .. -1): one thread per entry
// (h, h') of the pair (b, bp), b < bp, writes block (b, bp) and - through T(-t) = (-1)^{n''} T(t) - block (bp, b); blockIdx.y >=
// npairs: the diagonal block of ball blockIdx.y - npairs.
__global__ void __launch_bounds__(256) k_fill2d(int n_end, int H, int B, int npairs, const cplx* __restrict__ T, const cplx* __restrict__ tab,
                                                 int scaling, cplx* __restrict__ A, long long lda, long long sys_stride) {
  const int E = 2 * n_end - 1, HR = 2 * E + 2 * n_end;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)H * H) return;
  const int h = (int)(e / H), hp = (int)(e - (long long)h * H);
  const int s = blockIdx.z;
  cplx* As = A + (size_t)s * sys_stride;
  if ((int)blockIdx.y >= npairs) {
    const int b = blockIdx.y - npairs;
    const int n = h < n_end ? h : H - h;
    const cplx* tb = tab + ((size_t)s * B + b) * 3 * n_end;
    cplx v = make_double2(0.0, 0.0);
    if (h == hp) v = scaling == BIEM_FILL_REFERENCE ? cmul(tb[n_end + n], tb[2 * n_end + n]) : make_double2(1.0, 0.0);
    As[((size_t)b * H + h) * lda + (size_t)b * H + hp] = v;
    return;
  }
  int bp = (int)((sqrtf(8.0f * (float)blockIdx.y + 1.0f) + 1.0f) * 0.5f);
  while (bp * (bp - 1) / 2 > (int)blockIdx.y) --bp;
  while ((bp + 1) * bp / 2 <= (int)blockIdx.y) ++bp;
  const int b = blockIdx.y - bp * (bp - 1) / 2;
  const int m = h < n_end ? h : h - H, mp = hp < n_end ? hp : hp - H;          // signed orders
  const int am = m < 0 ? -m : m, amp = mp < 0 ? -mp : mp, mu = mp - m, j = mu < 0 ? -mu : mu;
  const cplx* row = T + ((size_t)s * B * B + (size_t)b * B + bp) * HR;
  cplx ph = row[E + j];
  if (mu < 0) ph.y = -ph.y;
  const cplx raw = cscale(cmul(row[j], ph), sign_even(am + j - amp) * kInvSqrt2Pi);
  const cplx* tb = tab + ((size_t)s * B + b) * 3 * n_end;
  const cplx* tbp = tab + ((size_t)s * B + bp) * 3 * n_end;
  auto colfac = [&](const cplx* tball, int n) { return scaling == BIEM_FILL_REFERENCE ? tball[2 * n_end + n] : crecip(tball[n_end + n]); };
  As[((size_t)b * H + h) * lda + (size_t)bp * H + hp] = cmul(cmul(raw, tb[am]), colfac(tbp, amp));
  const cplx mm = cmul(cmul(raw, tbp[am]), colfac(tb, amp));
  As[((size_t)bp * H + h) * lda + (size_t)b * H + hp] = ((am + amp) & 1) ? make_double2(-mm.x, -mm.y) : mm;
}

// symmetric form: one thread per unit pair (m, m'), 0 <= m, m' < n_end, of the block (b, bp), b < bp; grid (unit pairs / 256, combinations)
__global__ void __launch_bounds__(256) k_fill2d_sym(int n_end, int H, int B, int nb, int npairs, const cplx* __restrict__ T, cplx* __restrict__ A,
                                                     long long lda, long long sys_stride, const int* __restrict__ classes) {
  const int E = 2 * n_end - 1, HR = 2 * E + 2 * n_end, U = n_end;
  const int pi = blockIdx.x * 256 + threadIdx.x;
  if (pi >= U * U) return;
  const int m = pi / U, mp = pi - m * U;
  const bool r2 = m > 0, c2 = mp > 0;
  // slots of a ball's unknowns: cosine combination of unit m at m, its sine combination at U + m - 1
  const int row_c = m, row_s = U + m - 1, col_c = mp, col_s = U + mp - 1;
  const long long o00 = (long long)row_c * lda + col_c, o01 = (long long)row_c * lda + col_s, o10 = (long long)row_s * lda + col_c,
                  o11 = (long long)row_s * lda + col_s;
  const int muA = mp - m, jA = muA < 0 ? -muA : muA, jB = m + mp;
  const double sA = (muA >= 0 ? 1.0 : ((jA & 1) ? -1.0 : 1.0)) * kInvSqrt2Pi;     // i^{m + |mu| - m'} / sqrt(2 pi): sign 1 for m' >= m, (-1)^{m - m'} otherwise
  const double sB = ((m & 1) ? -1.0 : 1.0) * kInvSqrt2Pi;                          // (h, p'): mu = -(m + m'), i^{2 m}
  const double q2 = 0.70710678118654752440;
  const int nrep = classes[0];
  const int* dup_ptr = classes + 4 + npairs;
  const int* dup_bb = dup_ptr + npairs + 1;
  const int ncomb = nrep * nb;
  for (int comb = blockIdx.y; comb < ncomb; comb += gridDim.y) {
    const int s = comb / nrep, ci = comb - s * nrep;
    const int e0 = dup_ptr[ci], e1 = dup_ptr[ci + 1], bb0 = dup_bb[e0];
    const cplx* row = T + ((size_t)s * B * B + (size_t)(bb0 >> 16) * B + (bb0 & 0xffff)) * HR;
    const cplx tA = row[jA], tB = row[jB];
    cplx phA = row[E + jA], phB = row[E + jB];
    const cplx scale = cmul(row[2 * E + m], row[2 * E + n_end + mp]);
    if (muA < 0) phA.y = -phA.y;                          // T[mu] = T'[|mu|] e^{i mu phi}
    const cplx RA = cscale(tA, sA), RB = cscale(tB, sB);
    // raw 2 x 2 block of the units (m, -m) x (m', -m'): (h,h') = R_A e^{i mu_A phi}, (p,p') its conjugate-phase partner,
    // (h,p') = R_B e^{-i (m + m') phi}, (p,h') = R_B e^{+i (m + m') phi}
    const cplx mA = cmul(RA, make_double2(phA.x, -phA.y));
    cplx x00 = cmul(RA, phA), x01 = (r2 && c2) ? cmul(RB, make_double2(phB.x, -phB.y)) : mA, x10 = (r2 && c2) ? cmul(RB, phB) : mA, x11 = mA;
    if (r2) {
      const cplx a0c = make_double2((x00.x + x10.x) * q2, (x00.y + x10.y) * q2), a1c = make_double2((x01.x + x11.x) * q2, (x01.y + x11.y) * q2);
      const cplx d0 = make_double2((x00.x - x10.x) * q2, (x00.y - x10.y) * q2), d1 = make_double2((x01.x - x11.x) * q2, (x01.y - x11.y) * q2);
      x00 = a0c; x01 = a1c; x10 = make_double2(-d0.y, d0.x); x11 = make_double2(-d1.y, d1.x);
    }
    if (c2) {
      const cplx a0c = make_double2((x00.x + x01.x) * q2, (x00.y + x01.y) * q2), d0 = make_double2((x01.x - x00.x) * q2, (x01.y - x00.y) * q2);
      const cplx a1c = make_double2((x10.x + x11.x) * q2, (x10.y + x11.y) * q2), d1 = make_double2((x11.x - x10.x) * q2, (x11.y - x10.y) * q2);
      x00 = a0c; x01 = make_double2(-d0.y, d0.x); x10 = a1c; x11 = make_double2(-d1.y, d1.x);
    }
    x00 = cmul(x00, scale); x01 = cmul(x01, scale); x10 = cmul(x10, scale); x11 = cmul(x11, scale);
    cplx* As = A + (size_t)s * sys_stride;
    for (int e = e0; e < e1; ++e) {                          // every pair of the class (the representative first)
      const int bb = dup_bb[e];
      const int rb0 = (bb >> 16) * H, cb0 = (bb & 0xffff) * H;
      cplx* Ab = As + (size_t)rb0 * lda + cb0;
      Ab[o00] = x00;
      if (c2) Ab[o01] = x01;
      if (r2) { Ab[o10] = x10; if (c2) Ab[o11] = x11; }
      if (cb0 - rb0 - H < NB_TILE) {                         // entries inside a diagonal 64 x 64 tile are mirrored (read whole)
        auto mirror = [&](int rslot, int cslot, cplx w) {
          const int rr = rb0 + rslot, cc = cb0 + cslot;
          if ((rr >> 6) == (cc >> 6)) As[(size_t)cc * lda + rr] = w;
        };
        mirror(row_c, col_c, x00);
        if (c2) mirror(row_c, col_s, x01);
        if (r2) { mirror(row_s, col_c, x10); if (c2) mirror(row_s, col_s, x11); }
      }
    }
  }
}

// does the one-unit-pair-per-lane form of the symmetric fill fit this plan's tables into LDS?
static bool fill_sym_entry_fits(const biem_plan* p, size_t& shm) {
  shm = (size_t)(p->H2lin + 2 * p->n_end) * sizeof(cplx) + (size_t)(p->qchunk_terms_max + 1) * 10 + (size_t)(2 * p->qchunk_pairs_max + 1) * 4 + 16;
  return p->pair_lists_ok && (int)p->qchunk.size() > 1 && shm <= 160 * 1024 && p->H2lin <= 8 * 1024;
}

// the reduced-table form (k_fill_red): reduced pair table + phases, q factors and the chunk's transposed lists in LDS
static bool fill_red_fits(const biem_plan* p, size_t& shm) {
  shm = (size_t)p->red_nc * (p->E + p->NP + 2 * p->n_end) * sizeof(cplx) + (size_t)p->rchunk_rows_max * 64 * 10 + 33 * 4 + 64;
  return p->red_lists_ok && shm <= (size_t)(p->red_waves == 16 ? 158 : 79) * 1024 && p->E + p->NP + 2 * p->n_end <= 8 * 64 * p->red_waves;
}

// the list-free 2-D kernels index the table row directly: T'[j] at j, phase e^{i j phi} at E + j (phase ids in order of the orders)
bool plan_2d_direct(const biem_plan* p) {
  if (p->tree != TREE_A || p->E != p->n2 || p->NP != p->n2 || (int)p->ph_mu.size() != 2 * p->n2) return false;
  for (int i = 0; i < p->n2; ++i) if (p->ph_mu[2 * i] != i || p->red_label[i] != i) return false;
  return true;
}

// BIEM_FILL_FORM (A / B runs; read per call, by first letter): "sys" = systems in lanes, "entry" = the gather form k_fill_sym, any other
// word ("red") = the reduced-table form k_fill_red where it fits, which is also the default.  On a 2-D plan with term lists ANY value
// selects the list kernels of both fills instead of the list-free 2-D kernels
enum FillFormEnv { FORM_UNSET, FORM_RED, FORM_ENTRY, FORM_SYS };
static FillFormEnv fill_form_env() {
  const char* form = getenv("BIEM_FILL_FORM");
  return !form ? FORM_UNSET : form[0] == 's' ? FORM_SYS : form[0] == 'e' ? FORM_ENTRY : FORM_RED;
}

// Two kinds of list forms.  "entry" (one unit pair per lane, pair table in LDS: RED / ENTRY) is the fast one wherever its tables fit LDS;
// "sys" (one system per lane, pair tables from L2 / Infinity Cache: bound by the ~35-70 GB/s a CU gets from there, 150 vs 92 ms per 256
// systems at cfg 3) has no ceiling on the order and takes over where the entry form does not fit.  DIRECT2D also tells launch_fill to
// run its list-free kernel
FillSymForm fill_sym_form(const biem_plan* p) {
  const FillFormEnv env = fill_form_env();
  size_t shm_red = 0, shm_entry = 0;
  const bool red_fits = fill_red_fits(p, shm_red), entry_fits = fill_sym_entry_fits(p, shm_entry);
  const bool sys_ws = env == FORM_SYS || !(entry_fits || red_fits);
  if (p->tree == TREE_A && (!p->lists_built || env == FORM_UNSET)) return {FillSymForm::DIRECT2D, 0, sys_ws};
  if (red_fits && env != FORM_SYS && env != FORM_ENTRY) return {FillSymForm::RED, shm_red, sys_ws};
  if (env == FORM_UNSET ? !entry_fits : env == FORM_SYS)
    return {FillSymForm::SYS, (size_t)(p->schunk_terms_max + 1) * 12 + (size_t)(4 * p->schunk_pairs_max + 1) * 4 + (size_t)p->schunk_pairs_max * 12 + 16, sys_ws};
  if (entry_fits) return {FillSymForm::ENTRY, shm_entry, sys_ws};
  return {FillSymForm::UNFIT, 0, sys_ws};
}

size_t fill_workspace_bytes(const biem_plan* p, int nb, int B) {
  // pair tables of the general / entry forms: [nb][B][B][H2 or H2lin]; of the systems-in-lanes form (needed where the entry form
  // does not fit, or when BIEM_FILL_FORM=sys forces it): [nb rounded up to 64][pairs][H2] + q factors
  size_t row = (size_t)(p->H2lin > p->H2 ? p->H2lin : p->H2);            // general / gather forms; reduced form: T', phases, q factors
  if ((size_t)(p->E + p->NP + 2 * p->n_end) > row) row = (size_t)(p->E + p->NP + 2 * p->n_end);
  const size_t a = (size_t)nb * B * B * row, nbp = (size_t)(nb + 63) / 64 * 64;
  const size_t b = ((size_t)(B * (B - 1) / 2) * p->H2 + (size_t)B * p->n_end) * nbp;
  return (fill_sym_form(p).sys_workspace && b > a ? b : a) * sizeof(cplx) + fill_dedupe_bytes(B);
}

// the symmetric fill of a 2-D plan without lists (any order); pair classes as in the list forms
int launch_fill2d_sym(const SymFill& c) {
  const biem_plan* p = c.p;
  if (!plan_2d_direct(p)) { set_error("biem_fill (symmetric): internal: 2-D table order"); return BIEM_ERR_ARG; }
  const int U = (int)(p->units.size() / 2), npairs = c.B * (c.B - 1) / 2;
  { const int rc = launch_classes_and_tables(c, PT_REDUCED); if (rc) return rc; }
  const long long ncomb = (long long)npairs * c.nb;
  const unsigned gx = (unsigned)(((long long)U * U + 255) / 256);
  hipLaunchKernelGGL(k_fill2d_sym, dim3(gx, (unsigned)(ncomb < 65535 ? ncomb : 65535)), dim3(256), 0, c.st, p->n_end, p->H, c.B, c.nb, npairs, c.T,
                     c.A, c.lda, c.sys_stride, c.pc.classes);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

static int launch_fill_pad(int nb, int N, int n_pad, double* d_A, long long lda, long long sys_stride, hipStream_t st) {
  if (n_pad <= N) return BIEM_OK;
  hipLaunchKernelGGL(k_fill_pad, dim3(64, nb), dim3(256), 0, st, N, n_pad, (cplx*)d_A, lda, sys_stride);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_fill(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched,
                const double* d_tab, int scaling, double* d_A, long long lda, long long sys_stride, int n_pad,
                void* d_work, size_t work_bytes, hipStream_t st) {
  const int H = p->H, N = B * H;
  if (nb <= 0 || B <= 0) return BIEM_OK;
  if (lda < (n_pad > N ? n_pad : N) || n_pad < N) { set_error("biem_fill: lda/n_pad too small"); return BIEM_ERR_ARG; }
  if (work_bytes < fill_workspace_bytes(p, nb, B)) { set_error("biem_fill: workspace too small"); return BIEM_ERR_ARG; }
  if (scaling != BIEM_FILL_REFERENCE && scaling != BIEM_FILL_EQUILIBRATED) { set_error("biem_fill: bad scaling"); return BIEM_ERR_ARG; }
  cplx* T = (cplx*)d_work;
  ProfScope ps(PK_FILL, st, 16.0 * (double)nb * N * (double)N);
  if (fill_sym_form(p).kind == FillSymForm::DIRECT2D) {
    // 2-D: no term lists, any order (BIEM_FILL_FORM set: the generic list kernel below, for A / B tests)
    if (!plan_2d_direct(p)) { set_error("biem_fill: internal: 2-D table order"); return BIEM_ERR_ARG; }
    if (nb > 65535) { set_error("biem_fill: at most 65535 systems per call"); return BIEM_ERR_ARG; }
    const int npairs = B * (B - 1) / 2;
    if (npairs + B > 65535) { set_error("biem_fill (2-D): too many balls for one launch (%d)", B); return BIEM_ERR_UNSUPPORTED; }
    { const int rc = launch_pair_tables(p, nb, B, d_k, d_centers, geom_batched, d_tab, PT_REDUCED, nullptr, T, st); if (rc) return rc; }
    hipLaunchKernelGGL(k_fill2d, dim3((unsigned)(((long long)H * H + 255) / 256), npairs + B, nb), dim3(256), 0, st, p->n_end, H, B, npairs, T,
                       (const cplx*)d_tab, scaling, (cplx*)d_A, lda, sys_stride);
    BIEM_LAUNCHCHK();
    return launch_fill_pad(nb, N, n_pad, d_A, lda, sys_stride, st);
  }
  if (!fill_lists_order_ok(p)) { set_error("n_end=%d exceeds the built table size", p->n_end); return BIEM_ERR_UNSUPPORTED; }
  { const int rc = launch_pair_tables(p, nb, B, d_k, d_centers, geom_batched, d_tab, PT_PLAIN, nullptr, T, st); if (rc) return rc; }
  size_t shm = (size_t)((p->fill_table_global ? 0 : p->H2) + 2 * H) * sizeof(cplx) + (size_t)p->chunk_terms_max * 10 + (size_t)(p->chunk_ents_max + 1) * 4 + 16;
  if (shm > 160 * 1024 || (p->chunk_terms_max == 0 && p->coef.size() > 0)) {
    set_error("biem_fill: tables do not fit LDS (H=%d, H2=%d, chunk terms=%d)", H, p->H2, p->chunk_terms_max);
    return BIEM_ERR_UNSUPPORTED;
  }
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  const int nchunks = (int)p->chunk_ent.size() - 1;
  hipLaunchKernelGGL(k_fill, dim3(nchunks, (B + 1) / 2, nb), dim3(FILL_THREADS), shm, st, H, p->H2, p->n_end, B, p->d_deg, p->d_chunk_ent,
                     p->chunk_terms_max, p->chunk_ents_max, p->d_ptr, p->d_coef, p->d_tidx16, T, (const cplx*)d_tab, scaling,
                     (cplx*)d_A, lda, sys_stride, p->fill_table_global ? 1 : 0);
  BIEM_LAUNCHCHK();
  return launch_fill_pad(nb, N, n_pad, d_A, lda, sys_stride, st);
}

}  // namespace biem
