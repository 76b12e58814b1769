// kernels_fill_sym.hip -- the symmetric fill (default path) in its four forms: reduced table, gather, systems in lanes, list-free 2-D; the
// unit diagonal and padding; launch_fill_sym (gfx950).  Tables and pair classes: kernels_tables.hip; the form decision: kernels_fill.hip.
#include "fill.hpp"
#include <cstdlib>

namespace biem {

// ---------------------------------------------------------------------------------------------
// Symmetric fill (default path): the complex-symmetric form A~ = R W^H M W R^-1 of the equilibrated system, written ONCE and
// only where the symmetric factorisation reads it (UPPER triangle + the diagonal 64 x 64 tiles) - the general fill followed by
// the in-place symmetrising transform moved 4x the bytes.
//   W: unitary map to real harmonics (units (h, p), conj Y_h = Y_p: "cosine" (e_h + e_p)/sqrt2, "sine" i (e_p - e_h)/sqrt2),
//   R = diag(1/sqrt(gj gh)) per (ball, degree).  With q_b[n] = gj / sqrt(gj gh) the block (b, b'), b != b', is
//        A~[(b,x), (b',x')] = q_b[n] q_b'[n'] (W^H S_{bb'} W)[x, x'],      S = (S|R)^T raw sums,  diagonal blocks = identity.
// Internal order of a ball's unknowns: slot u = cosine combination of unit u, slot U + spos[u] = its sine combination
// (plan.hpp); consecutive lanes own consecutive u', so every store instruction covers contiguous runs of a matrix row.
// One 512-thread workgroup owns a chunk of unit pairs (its four term lists per pair stay in LDS) and loops over
// (upper ball pair b < b', system) combinations: per combination only the pair table T (H2 complex) is staged - fetched into
// registers during the previous combination's contraction - so the term lists are read from L2 once per workgroup.
// Each thread runs the four independent chains of its 2 x 2 block (the per-term chain idx -> T -> fma is LDS-latency bound).
// ---------------------------------------------------------------------------------------------
constexpr int FILL_SYM_THREADS = 1024;
constexpr int FILL_SYM_MAXT = 8;           // pair-table elements prefetched per thread: H2lin <= 8 * 1024

// KT = pair-table elements each thread carries in registers from one combination to the next (KT * 512 >= H2); the loads are
// unconditional with a clamped index (a conditionally assigned register array was kept in scratch by hipcc)
template <int KT>
__global__ void __launch_bounds__(FILL_SYM_THREADS) k_fill_sym(int H, int U, int H2, int n_end, int B, int nb, int npairs,
                                                                const int* __restrict__ deg, const int* __restrict__ units,
                                                                const int* __restrict__ spos, const int* __restrict__ qchunk,
                                                                int terms_max, int pairs_max, const uint32_t* __restrict__ qptr,
                                                                const double* __restrict__ qcoef, const uint16_t* __restrict__ qidx,
                                                                const cplx* __restrict__ T, const cplx* __restrict__ tab,
                                                                cplx* __restrict__ A, long long lda, long long sys_stride,
                                                                const int* __restrict__ classes) {
  extern __shared__ char smem[];
  cplx* sT = (cplx*)smem;                                  // [H2] pair table of the current combination
  cplx* sQ = sT + H2;                                      // [2][n_end]: q of the row ball, q of the column ball
  double* sCoef = (double*)(sQ + 2 * n_end);               // [terms_max + 1]: the chunk's terms, then a dummy (0.0, index 0)
  uint32_t* sPtr = (uint32_t*)(sCoef + terms_max + 1);     // [2 pairs_max + 1], relative to the chunk's first term
  uint16_t* sIdx = (uint16_t*)(sPtr + 2 * pairs_max + 1);  // [terms_max + 1]
  const int tid = threadIdx.x;
  const int p0 = qchunk[blockIdx.x], p1 = qchunk[blockIdx.x + 1], npr = p1 - p0;
  const uint32_t t0 = qptr[2 * (size_t)p0], t1 = qptr[2 * (size_t)p1];
  for (uint32_t q = t0 + tid; q < t1; q += FILL_SYM_THREADS) { sCoef[q - t0] = qcoef[q]; sIdx[q - t0] = qidx[q]; }
  for (int e = tid; e <= 2 * npr; e += FILL_SYM_THREADS) sPtr[e] = qptr[2 * (size_t)p0 + e] - t0;
  if (tid == 0) { sCoef[t1 - t0] = 0.0; sIdx[t1 - t0] = 0; }
  // this thread's unit pair (fixed for the whole kernel)
  const bool active = tid < npr;
  const int pi = p0 + (active ? tid : 0);
  const int u = pi / U, v = pi - u * U;
  const int rh = units[2 * u], rp = units[2 * u + 1], ch = units[2 * v], cp = units[2 * v + 1];
  const bool r2 = rp != rh, c2 = cp != ch;                 // two rows / two columns in this block
  const int row_c = u, row_s = r2 ? U + spos[u] : 0, col_c = v, col_s = c2 ? U + spos[v] : 0;
  const int nrow = deg[rh], ncol = deg[ch];
  const double q2 = 0.70710678118654752440;
  // pair classes (k_pair_dedupe): a combination is (system, class); its block is contracted once from the representative pair's
  // table and stored to every pair of the class
  const int nrep = classes[0];
  const int* rep_list = classes + 4;
  const int* dup_ptr = rep_list + npairs;
  const int* dup_bb = dup_ptr + npairs + 1;
  const int ncomb = nrep * nb;
  // eight named registers instead of an array: hipcc kept every array form (plain, unrolled, compile-time indexed through
  // lambdas) in scratch memory
#define BIEM_TN_LIST(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define BIEM_TN_DECL(k) cplx tn##k = make_double2(0.0, 0.0);
  BIEM_TN_LIST(BIEM_TN_DECL)
#define BIEM_TN_LOAD(k) if (k < KT) { const int l = k * FILL_SYM_THREADS + tid; tn##k = Tp_[l < H2 ? l : H2 - 1]; }
#define BIEM_TN_PUT(k) if (k < KT) { const int l = k * FILL_SYM_THREADS + tid; if (l < H2) sT[l] = tn##k; }
  auto pair_of = [&](int pr, int& b, int& bp) {           // pr-th upper pair (row ball b < column ball bp)
    int bb = (int)((sqrtf(8.0f * (float)pr + 1.0f) + 1.0f) * 0.5f);
    while (bb * (bb - 1) / 2 > pr) --bb;
    while ((bb + 1) * bb / 2 <= pr) ++bb;
    bp = bb; b = pr - bb * (bb - 1) / 2;
  };
  auto table_of = [&](int cb) -> const cplx* {
    const int s = cb / nrep, pr = rep_list[cb - s * nrep];
    int b, bp; pair_of(pr, b, bp);
    return T + ((size_t)s * B * B + (size_t)b * B + bp) * H2;
  };
  int comb = blockIdx.y;
  if (comb < ncomb) { const cplx* Tp_ = table_of(comb); BIEM_TN_LIST(BIEM_TN_LOAD) }
  for (; comb < ncomb; comb += gridDim.y) {
    const int s = comb / nrep, ci = comb - s * nrep, pr = rep_list[ci];
    int b, bp; pair_of(pr, b, bp);
    __syncthreads();                                       // the previous combination's readers are done (also orders the chunk loads)
    BIEM_TN_LIST(BIEM_TN_PUT)
    if (tid < 2 * n_end) {
      const int which = tid >= n_end, n = tid - which * n_end;
      const cplx* tb = tab + ((size_t)s * B + (which ? bp : b)) * 3 * n_end;
      sQ[tid] = cmul(tb[n], crecip(zsqrt(cmul(tb[n], tb[n_end + n]))));     // gj / sqrt(gj gh)
    }
    __syncthreads();
    if (comb + (int)gridDim.y < ncomb) { const cplx* Tp_ = table_of(comb + (int)gridDim.y); BIEM_TN_LIST(BIEM_TN_LOAD) }   // lands while this combination is contracted
    if (!active) continue;
    // Two term lists per unit pair (plan.hpp): A = (h,h'), B = (h,p'); the conjugate entries (p,p') and (p,h') have the same
    // coefficients with every table index replaced by its partner's, which the paired table layout keeps at index ^ 1.  So one
    // coefficient and one index read feed two chains; per step all reads of both lists are issued, then the four table reads,
    // then the FMAs.  A list that has run out reads the chunk's dummy term (coefficient 0, index 0).
    const uint32_t dummy = sPtr[2 * npr];                 // = number of terms of the chunk: the slot behind them
    uint32_t qa = sPtr[2 * tid], qb = sPtr[2 * tid + 1];
    const uint32_t ea = qb, eb = sPtr[2 * tid + 2];
    const uint32_t lm = (ea - qa) > (eb - qb) ? (ea - qa) : (eb - qb);
    double s0r = 0, s0i = 0, s1r = 0, s1i = 0, s2r = 0, s2i = 0, s3r = 0, s3i = 0;      // A, mirror of A, B, mirror of B
    for (uint32_t i = 0; i < lm; ++i) {
      const uint32_t ga = qa < ea ? qa : dummy, gb = qb < eb ? qb : dummy;
      const double ca = sCoef[ga], cb = sCoef[gb];
      const unsigned ia = sIdx[ga], ib = sIdx[gb];
      const cplx za = sT[ia], zam = sT[ia ^ 1u], zb = sT[ib], zbm = sT[ib ^ 1u];
      s0r = fma(ca, za.x, s0r); s0i = fma(ca, za.y, s0i);
      s1r = fma(ca, zam.x, s1r); s1i = fma(ca, zam.y, s1i);
      s2r = fma(cb, zb.x, s2r); s2i = fma(cb, zb.y, s2i);
      s3r = fma(cb, zbm.x, s3r); s3i = fma(cb, zbm.y, s3i);
      ++qa; ++qb;
    }
    // W^H S W on the 2 x 2 block: rows (h + p)/sqrt2, i (h - p)/sqrt2; columns (h' + p')/sqrt2, i (p' - h')/sqrt2
    // raw entries: (h,h') = A; (p,p') = mirror A and (h,p') = B, (p,h') = mirror B when both units are doubles; with a single
    // row unit the mirror of A is (h,p'), with a single column unit it is (p,h')
    const cplx mA = make_double2(s1r, s1i);
    cplx x00 = make_double2(s0r, s0i), x01 = (r2 && c2) ? make_double2(s2r, s2i) : mA, x10 = (r2 && c2) ? make_double2(s3r, s3i) : mA, x11 = mA;
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
    const cplx scale = cmul(sQ[nrow], sQ[n_end + ncol]);
    cplx* As = A + (size_t)s * sys_stride;
    const int e0 = dup_ptr[ci], e1 = dup_ptr[ci + 1];
    auto put = [&](int rslot, int cslot, cplx val) {
      const cplx w = cmul(val, scale);
      for (int e = e0; e < e1; ++e) {                        // every pair of the class (the representative first)
        const int bb = dup_bb[e];
        const int row = (bb >> 16) * H + rslot, col = (bb & 0xffff) * H + cslot;   // b < bp: strictly above the diagonal
        As[(size_t)row * lda + col] = w;
        if ((row >> 6) == (col >> 6)) As[(size_t)col * lda + row] = w;   // a diagonal 64 x 64 tile is read whole: mirror (A~ = A~^T)
      }
    };
    put(row_c, col_c, x00);
    if (c2) put(row_c, col_s, x01);
    if (r2) { put(row_s, col_c, x10); if (c2) put(row_s, col_s, x11); }
  }
#undef BIEM_TN_LIST
#undef BIEM_TN_DECL
#undef BIEM_TN_LOAD
#undef BIEM_TN_PUT
}

// ---------------------------------------------------------------------------------------------
// Symmetric fill, reduced-table form (default where its tables fit LDS).  Same work split as k_fill_sym above - a workgroup owns a
// chunk of unit pairs, one per thread, and loops over (class, system) combinations, the next combination's table prefetched into
// registers - but the contraction reads LDS without bank conflicts and half as much of it:
//   * the phase e^{i mu . phi} is common to all terms of an entry and leaves the sum (plan.hpp): ONE chain per list over the
//     reduced table T'[e] (a label and its conjugate partner share an entry), the conjugate entry is conj(phase) x the same sum;
//   * the term lists of the 64 unit pairs of a wave are stored transposed and padded to the wave's longest list: per step the wave
//     reads 64 consecutive coefficients and 64 consecutive 16-bit indices, all trip counts are wave-uniform (no divergence, no
//     clamped dummy terms);
//   * consecutive lanes are consecutive column units (n', m' = -n' .. 0) and T' is laid out degree-major, so the 64 table reads of a
//     step fall on (nearly) consecutive entries.
// The gather form above measured 51 % of its LDS cycles as bank conflicts and 42 bytes of LDS per term and lane (profiles/r02_pmc_summary.txt).
// ---------------------------------------------------------------------------------------------
// workgroup barrier that orders LDS traffic only (see k_fill_red)
__device__ inline void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
#ifdef BIEM_FILL_TRACE
__device__ unsigned long long g_fill_trace[8];
#define BIEM_FT(i) { if (tid == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ft_acc[i] += now_ - ft_t; ft_t = now_; } }
#else
#define BIEM_FT(i)
#endif
// SPLIT (flat layouts, SplitMap in common.hpp): the cosine-cosine entry goes to the E block (ball origins b U, bp U), the sine-sine
// entry to the O block (origins npE + b (H - U), npE + bp (H - U)); the two mixed entries are structural zeros and are not stored.
template <int KT, int NC, bool SPLIT = false>
__global__ void __launch_bounds__(FILL_SYM_THREADS) k_fill_red(int H, int U, int HR, int E, int NP, int n_end, int B, int nb, int npairs,
                                                                const int* __restrict__ deg, const int* __restrict__ units,
                                                                const int* __restrict__ spos, const int* __restrict__ rchunk,
                                                                const int* __restrict__ rcrow, const int* __restrict__ rwrow, int rows_max,
                                                                const double* __restrict__ rcoef, const uint16_t* __restrict__ ridx,
                                                                const uint16_t* __restrict__ rphsel,
                                                                const cplx* __restrict__ T,
                                                                cplx* __restrict__ A, long long lda, long long sys_stride,
                                                                const int* __restrict__ classes, int npE) {
  extern __shared__ char smem[];
  // NC = 2: TWO combinations per iteration - the coefficient and index reads of a group of rows feed both tables (a fifth less LDS
  // traffic per term: 21 instead of 26 bytes) and the barriers, the loop head and the list walk are paid once for two blocks
  cplx* sT = (cplx*)smem;                                  // [NC][HR = E + NP + 2 n_end] table rows of the current combinations: T', phases, q factors
  double* sCoef = (double*)(sT + (size_t)NC * HR);         // [rows_max][64]
  uint16_t* sIdx = (uint16_t*)(sCoef + (size_t)rows_max * 64);   // [rows_max / 4][64][4]
  // (no static __shared__ here: statics precede the dynamic region unpadded, 33 ints would leave every ds_read_b64 / b128 below
  // misaligned - replayed at 64 cycles per wave-instruction; measured: 143 instead of 46 ms per 256 systems of cfg 3)
  int* sW = (int*)(sIdx + (size_t)rows_max * 64);          // [33] row offsets of the waves' lists
  const int tid = threadIdx.x, lane = tid & 63, TH = blockDim.x;          // 1024 threads (one workgroup per CU) or 512 (two)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p0 = rchunk[blockIdx.x], p1 = rchunk[blockIdx.x + 1], npr = p1 - p0;
  const int r0 = rcrow[blockIdx.x], nrows = rcrow[blockIdx.x + 1] - r0;
  {
    const double* gc = rcoef + (size_t)r0 * 64;
    const uint16_t* gi = ridx + (size_t)r0 * 64;
    for (int q = tid; q < nrows * 64; q += TH) { sCoef[q] = gc[q]; sIdx[q] = gi[q]; }
    if (tid < 33) sW[tid] = rwrow[blockIdx.x * 33 + tid];
  }
  // this thread's unit pair (fixed for the whole kernel): slots, degrees, phase selectors and the offsets of its (up to) four
  // entries inside a block, so that a combination's stores need no 64-bit multiplications
  const bool active = tid < npr;
  const int pi = p0 + (active ? tid : 0);
  const int u = pi / U, v = pi - u * U;
  const int rh = units[2 * u], rp = units[2 * u + 1], ch = units[2 * v], cp = units[2 * v + 1];
  const bool r2 = rp != rh, c2 = cp != ch;                 // two rows / two columns in this block
  const int row_c = u, row_s = r2 ? U + spos[u] : 0, col_c = v, col_s = c2 ? U + spos[v] : 0;
  const int nrow = deg[rh], ncol = deg[ch];
  const unsigned selA = rphsel[2 * (size_t)pi], selB = rphsel[2 * (size_t)pi + 1];
  const long long o00 = (long long)row_c * lda + col_c, o01 = (long long)row_c * lda + col_s, o10 = (long long)row_s * lda + col_c,
                  o11 = SPLIT ? (long long)(row_s - U) * lda + (col_s - U) : (long long)row_s * lda + col_s;   // (SPLIT: inside the O block)
  const double q2 = 0.70710678118654752440;
  const int nrep = classes[0];
  const int* dup_ptr = classes + 4 + npairs;
  const int* dup_bb = dup_ptr + npairs + 1;
  const int ncomb = nrep * nb;
#define BIEM_TN_LIST(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
  typedef double v2d_t __attribute__((ext_vector_type(2)));   // (a native vector: a struct cannot be a tied asm operand)
#define BIEM_TN_DECL(k) v2d_t tn##k = {0.0, 0.0};
  BIEM_TN_LIST(BIEM_TN_DECL)
#define BIEM_TM_DECL(k) v2d_t tm##k = {0.0, 0.0};
  BIEM_TN_LIST(BIEM_TM_DECL)                                 // (second combination of an iteration, NC = 2)
  // The prefetch loads are inline asm and their wait is the explicit one of BIEM_TN_CLAIM: hipcc's own wait for a VGPR load is a
  // vmcnt(0) wherever control flow joins, i.e. at the top of the loop, AFTER this combination's stores - every iteration would then
  // wait for the acknowledgement of its own stores (microseconds under a full HBM write queue, with the CU to itself).
#define BIEM_TN_LOAD(k) if (k < KT) { const int l = k * TH + tid; const cplx* a_ = Tp_ + (l < HR ? l : HR - 1); \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tn##k) : "v"(a_) : "memory"); }
#define BIEM_TN_CLAIM(k) if (k < KT) asm volatile("s_waitcnt vmcnt(0)" : "+v"(tn##k) : : "memory");
#define BIEM_TN_PUT(k) if (k < KT) { const int l = k * TH + tid; if (l < HR) sT[l] = make_double2(tn##k.x, tn##k.y); }
#define BIEM_TM_LOAD(k) if (NC > 1 && k < KT) { const int l = k * TH + tid; const cplx* a_ = Tp_ + (l < HR ? l : HR - 1); \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tm##k) : "v"(a_) : "memory"); }
#define BIEM_TM_CLAIM(k) if (NC > 1 && k < KT) asm volatile("s_waitcnt vmcnt(0)" : "+v"(tm##k) : : "memory");
#define BIEM_TM_PUT(k) if (NC > 1 && k < KT) { const int l = k * TH + tid; if (l < HR) sT[HR + l] = make_double2(tm##k.x, tm##k.y); }
  // a combination is (system s, class ci); its table is the one of the class's first pair (dup_bb: b << 16 | bp, the representative first)
  auto table_of = [&](int cb) -> const cplx* {
    const int s = cb / nrep, bb = dup_bb[dup_ptr[cb - s * nrep]];
    return T + ((size_t)s * B * B + (size_t)(bb >> 16) * B + (bb & 0xffff)) * HR;
  };
  // iteration i of this workgroup takes the combinations comb and (NC = 2) comb + G, G = gridDim.y; the next one comb + NC G
  const int G = gridDim.y;
  int comb = blockIdx.y;
  if (comb < ncomb) { const cplx* Tp_ = table_of(comb); BIEM_TN_LIST(BIEM_TN_LOAD) }
  if (NC > 1 && comb + G < ncomb) { const cplx* Tp_ = table_of(comb + G); BIEM_TN_LIST(BIEM_TM_LOAD) }
  BIEM_TN_LIST(BIEM_TN_CLAIM)
  BIEM_TN_LIST(BIEM_TM_CLAIM)
#ifdef BIEM_FILL_TRACE
  unsigned long long ft_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ft_t = __builtin_amdgcn_s_memtime();
#endif
  for (; comb < ncomb; comb += NC * G) {
    const bool two = NC > 1 && comb + G < ncomb;           // (wave-uniform) a second combination in this iteration
    BIEM_FT(0)
    // Raw barriers with an LDS-only wait: __syncthreads() carries a workgroup-scope fence, which hipcc lowers to s_waitcnt vmcnt(0) -
    // every barrier would wait for the acknowledgement of the previous combination's global stores (nobody in the workgroup reads
    // them).  Only LDS traffic has to be ordered here: this wave's LDS reads / writes are complete at lgkmcnt(0).
    lds_barrier();                                         // the previous combination's readers are done (also orders the chunk loads)
    BIEM_FT(1)
    BIEM_TN_LIST(BIEM_TN_PUT)
    BIEM_TN_LIST(BIEM_TM_PUT)
    BIEM_FT(2)
    lds_barrier();
    BIEM_FT(4)
    if (comb + NC * G < ncomb) { const cplx* Tp_ = table_of(comb + NC * G); BIEM_TN_LIST(BIEM_TN_LOAD) }   // lands while this iteration is contracted
    if (NC > 1 && comb + (NC + 1) * G < ncomb) { const cplx* Tp_ = table_of(comb + (NC + 1) * G); BIEM_TN_LIST(BIEM_TM_LOAD) }
    // (a wave without unit pairs runs zero groups and joins the others at the claim of the prefetched registers below: every path
    // through the loop body must pass that point, or the compiler drains the memory queue again where the paths meet)
    const bool wave_on = wave * 64 < npr;
    // rows of list A: [ra, rb), of list B: [rb, re), all multiples of 4.  One loop over the groups of four rows, software
    // pipelined: the coefficient / index reads of group g + 1 are in flight while the four table reads of group g are waited for
    // (the chain index -> table entry -> fma is two dependent LDS round trips otherwise); at the A | B boundary (wave-uniform)
    // the accumulators are handed over.
    const int ga = wave_on ? sW[2 * wave] >> 2 : 0, gb = wave_on ? sW[2 * wave + 1] >> 2 : 0, ge = wave_on ? sW[2 * wave + 2] >> 2 : 0;
    double ar = 0.0, ai = 0.0, xr = 0.0, xi = 0.0;        // running sums; (xr, xi) keeps list A's once list B has started
    double br = 0.0, bi = 0.0, yr = 0.0, yi = 0.0;        // the same for the second combination
    if (ga < ge) {
      const double* cc = sCoef + lane;
      const uint2* ii = (const uint2*)sIdx + lane;
      uint2 pk = ii[(size_t)ga * 64];
      double c0 = cc[(size_t)(4 * ga) * 64], c1 = cc[(size_t)(4 * ga + 1) * 64], c2v = cc[(size_t)(4 * ga + 2) * 64], c3 = cc[(size_t)(4 * ga + 3) * 64];
      for (int g = ga; g < ge; ++g) {
        const int gn = g + 1 < ge ? g + 1 : g;             // (the last trip re-reads its own group: harmless)
        const cplx z0 = sT[pk.x & 0xffffu], z1 = sT[pk.x >> 16], z2 = sT[pk.y & 0xffffu], z3 = sT[pk.y >> 16];
        cplx w0, w1, w2, w3;
        if (NC > 1) { w0 = sT[HR + (pk.x & 0xffffu)]; w1 = sT[HR + (pk.x >> 16)]; w2 = sT[HR + (pk.y & 0xffffu)]; w3 = sT[HR + (pk.y >> 16)]; }
        const uint2 pkn = ii[(size_t)gn * 64];
        const double n0 = cc[(size_t)(4 * gn) * 64], n1 = cc[(size_t)(4 * gn + 1) * 64], n2 = cc[(size_t)(4 * gn + 2) * 64], n3 = cc[(size_t)(4 * gn + 3) * 64];
        if (g == gb) { xr = ar; xi = ai; ar = 0.0; ai = 0.0; yr = br; yi = bi; br = 0.0; bi = 0.0; }
        ar = fma(c0, z0.x, ar); ai = fma(c0, z0.y, ai);
        ar = fma(c1, z1.x, ar); ai = fma(c1, z1.y, ai);
        ar = fma(c2v, z2.x, ar); ai = fma(c2v, z2.y, ai);
        ar = fma(c3, z3.x, ar); ai = fma(c3, z3.y, ai);
        if (NC > 1) {
          br = fma(c0, w0.x, br); bi = fma(c0, w0.y, bi);
          br = fma(c1, w1.x, br); bi = fma(c1, w1.y, bi);
          br = fma(c2v, w2.x, br); bi = fma(c2v, w2.y, bi);
          br = fma(c3, w3.x, br); bi = fma(c3, w3.y, bi);
        }
        pk = pkn; c0 = n0; c1 = n1; c2v = n2; c3 = n3;
      }
    }
    BIEM_FT(5)
    // The prefetched table row is claimed HERE, before this combination's stores are issued: the wait then sees only the loads (issued
    // before the contraction) and the PREVIOUS combination's stores, which have had a whole iteration to drain.
    BIEM_TN_LIST(BIEM_TN_CLAIM)
    BIEM_TN_LIST(BIEM_TM_CLAIM)
    if (!active) continue;
    // the block of one combination from its two sums: phases, the 2 x 2 transform to real harmonics, q factors, stores
    auto finish = [&](const cplx* sTc, int cb, cplx RA, cplx RB) {
    const int s = cb / nrep, ci = cb - s * nrep;
    // entries of the 2 x 2 raw block: (h,h') = phase_A R_A, its conjugate entry conj(phase_A) R_A; (h,p') = phase_B R_B, (p,h') = conj(phase_B) R_B
    cplx phA = sTc[E + (selA >> 1)], phB = sTc[E + (selB >> 1)];
    if (selA & 1u) phA.y = -phA.y;
    if (selB & 1u) phB.y = -phB.y;
    const cplx mA = cmul(RA, make_double2(phA.x, -phA.y));
    cplx x00 = cmul(RA, phA), x01 = (r2 && c2) ? cmul(RB, phB) : mA, x10 = (r2 && c2) ? cmul(RB, make_double2(phB.x, -phB.y)) : mA, x11 = mA;
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
    const cplx scale = cmul(sTc[E + NP + nrow], sTc[E + NP + n_end + ncol]);
    x00 = cmul(x00, scale); x01 = cmul(x01, scale); x10 = cmul(x10, scale); x11 = cmul(x11, scale);
    cplx* As = A + (size_t)s * sys_stride;
    const int e0 = dup_ptr[ci], e1 = dup_ptr[ci + 1];
    for (int e = e0; e < e1; ++e) {                          // every pair of the class (the representative first)
      const int bb = dup_bb[e];
      if (SPLIT) {
        // the same mirror rule per block: tiles are counted from the block's own origin (npE is a multiple of 64)
        const int S = H - U, re0 = (bb >> 16) * U, ce0 = (bb & 0xffff) * U;            // (wave-uniform: scalar arithmetic)
        (As + (size_t)re0 * lda + ce0)[o00] = x00;
        if (ce0 - re0 - U < NB_TILE) {
          const int row = re0 + row_c, col = ce0 + col_c;
          if ((row >> 6) == (col >> 6)) As[(size_t)col * lda + row] = x00;
        }
        if (r2 && c2) {
          const int ro0 = npE + (bb >> 16) * S, co0 = npE + (bb & 0xffff) * S;
          (As + (size_t)ro0 * lda + co0)[o11] = x11;
          if (co0 - ro0 - S < NB_TILE) {
            const int row = ro0 + row_s - U, col = co0 + col_s - U;
            if ((row >> 6) == (col >> 6)) As[(size_t)col * lda + row] = x11;
          }
        }
        continue;
      }
      const int rb0 = (bb >> 16) * H, cb0 = (bb & 0xffff) * H;     // b < bp: the block lies strictly above the diagonal
      cplx* Ab = As + (size_t)rb0 * lda + cb0;               // (wave-uniform: scalar arithmetic)
      Ab[o00] = x00;
      if (c2) Ab[o01] = x01;
      if (r2) { Ab[o10] = x10; if (c2) Ab[o11] = x11; }
      if (cb0 - rb0 - H < NB_TILE) {
        // a diagonal 64 x 64 tile is read whole by the factorisation: entries of this block that fall into one are mirrored (A~ = A~^T);
        // only blocks whose first column lies within 64 of their last row can reach one
        auto mirror = [&](int rslot, int cslot, cplx w) {
          const int row = rb0 + rslot, col = cb0 + cslot;
          if ((row >> 6) == (col >> 6)) As[(size_t)col * lda + row] = w;
        };
        mirror(row_c, col_c, x00);
        if (c2) mirror(row_c, col_s, x01);
        if (r2) { mirror(row_s, col_c, x10); if (c2) mirror(row_s, col_s, x11); }
      }
    }
    };
    if (gb < ge) finish(sT, comb, make_double2(xr, xi), make_double2(ar, ai));
    else finish(sT, comb, make_double2(ar, ai), make_double2(0.0, 0.0));
    if (two) {
      if (gb < ge) finish(sT + HR, comb + G, make_double2(yr, yi), make_double2(br, bi));
      else finish(sT + HR, comb + G, make_double2(br, bi), make_double2(0.0, 0.0));
    }
    BIEM_FT(6)
  }
#ifdef BIEM_FILL_TRACE
  if (tid == 0) for (int i = 0; i < 8; ++i) atomicAdd(&g_fill_trace[i], ft_acc[i]);
#endif
#undef BIEM_TN_LIST
#undef BIEM_TN_DECL
#undef BIEM_TN_LOAD
#undef BIEM_TN_PUT
#undef BIEM_TN_CLAIM
#undef BIEM_TM_DECL
#undef BIEM_TM_LOAD
#undef BIEM_TM_CLAIM
#undef BIEM_TM_PUT
}
#ifdef BIEM_FILL_TRACE
extern "C" int biem_debug_fill_trace(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fill_trace), sizeof(unsigned long long) * 8) != hipSuccess) return 1;
  if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_fill_trace), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif

// ---------------------------------------------------------------------------------------------
// Symmetric fill, systems in lanes (batches of >= 32 systems): lane = system, the wave walks the unit pairs of its chunk one
// after the other.  Every lane of a wave then runs the SAME term list: the coefficient and the table index of a term are
// wave-uniform (broadcast LDS reads), the pair-table row T[l][0..63] of the 64 systems is one contiguous 1-KiB load (tables
// stored Tt[pair][l][system]), all lanes have the same trip counts (the entry-per-lane form above runs each wave to its longest
// list: 59 % lane efficiency at n_end = 20) and no LDS gather, so no bank conflicts (58 % of its LDS cycles).  The pair tables
// are not staged in LDS at all (they are served by L1 / L2), which also removes the H2 ceiling of the LDS budget.
// A lane writes its 2 x 2 block into its own system's matrix: 16-byte stores 64 systems apart; consecutive unit pairs of a
// chunk are consecutive columns, so a 128-byte line of every system fills up within a few hundred cycles and merges in L2.
// q factors per (ball, degree, system) come transposed as well (Qt[b][n][system], k_qfactors_t).
// ---------------------------------------------------------------------------------------------
constexpr int FILL_SYS_THREADS = 256;

__global__ void k_qfactors_t(int n_end, int B, int nb, int nbp, const cplx* __restrict__ tab, cplx* __restrict__ Qt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;            // (b, n, system), system fastest
  if (i >= B * n_end * nbp) return;
  // i = ((g * B + b) * n_end + n) * 64 + lane
  const int lane = i & 63, r = i >> 6, n = r % n_end, gb = r / n_end, b = gb % B, g = gb / B;
  const int s = g * 64 + lane, sc = s < nb ? s : nb - 1;
  const cplx* tb = tab + ((size_t)sc * B + b) * 3 * n_end;
  Qt[i] = cmul(tb[n], crecip(zsqrt(cmul(tb[n], tb[n_end + n]))));    // gj / sqrt(gj gh)
}

__global__ void __launch_bounds__(FILL_SYS_THREADS) k_fill_sys(int H, int U, int H2, int n_end, int B, int nb, int nbp, int npairs,
                                                                const int* __restrict__ deg, const int* __restrict__ units,
                                                                const int* __restrict__ spos, const int* __restrict__ schunk,
                                                                int terms_max, int pairs_max, const uint32_t* __restrict__ qptr,
                                                                const double* __restrict__ qcoef, const uint16_t* __restrict__ qidx,
                                                                const cplx* __restrict__ Tt, const cplx* __restrict__ Qt,
                                                                cplx* __restrict__ A, long long lda, long long sys_stride, int abl_nostore) {
  extern __shared__ char smem[];
  double* sCoef = (double*)smem;                                    // [terms_max + 1]: the chunk's terms, then a dummy (0.0, row 0)
  uint32_t* sOff = (uint32_t*)(sCoef + terms_max + 1);              // [terms_max + 1]: row offset of the term's table entry, in elements
  uint32_t* sPtr = sOff + terms_max + 1;                            // [4 pairs_max + 1]
  int* sMeta = (int*)(sPtr + 4 * pairs_max + 1);                    // [3 pairs_max]: slots and degrees of the pair's units
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = schunk[blockIdx.x], p1 = schunk[blockIdx.x + 1], npr = p1 - p0;
  const uint32_t t0 = qptr[4 * (size_t)p0], t1 = qptr[4 * (size_t)p1];
  for (uint32_t q = t0 + tid; q < t1; q += FILL_SYS_THREADS) { sCoef[q - t0] = qcoef[q]; sOff[q - t0] = (uint32_t)qidx[q] * 64u; }
  for (int e = tid; e <= 4 * npr; e += FILL_SYS_THREADS) sPtr[e] = qptr[4 * (size_t)p0 + e] - t0;
  if (tid == 0) { sCoef[t1 - t0] = 0.0; sOff[t1 - t0] = 0; }
  for (int e = tid; e < npr; e += FILL_SYS_THREADS) {
    const int pi = p0 + e, u = pi / U, v = pi - u * U;
    const int rh = units[2 * u], rp = units[2 * u + 1], ch = units[2 * v], cp = units[2 * v + 1];
    sMeta[3 * e] = u | ((rp != rh ? U + spos[u] : 0xffff) << 16);          // row slots: cosine, sine (0xffff: none)
    sMeta[3 * e + 1] = v | ((cp != ch ? U + spos[v] : 0xffff) << 16);      // column slots
    sMeta[3 * e + 2] = deg[rh] | (deg[ch] << 16);
  }
  __syncthreads();
  const double q2 = 0.70710678118654752440;
  const int ng = nbp >> 6;
  const int ncomb = npairs * ng;
  for (int comb = blockIdx.y; comb < ncomb; comb += gridDim.y) {
    const int g = comb / npairs, pr = comb - g * npairs;
    int bp = (int)((sqrtf(8.0f * (float)pr + 1.0f) + 1.0f) * 0.5f);
    while (bp * (bp - 1) / 2 > pr) --bp;
    while ((bp + 1) * bp / 2 <= pr) ++bp;
    const int b = pr - bp * (bp - 1) / 2;                              // row ball b < column ball bp
    const int sys = g * 64 + lane;
    const bool live = sys < nb;
    const cplx* __restrict__ Tl = Tt + ((size_t)g * npairs + pr) * H2 * 64 + lane;    // + row offset of a term
    const cplx* __restrict__ Qr = Qt + ((size_t)g * B + b) * n_end * 64 + lane;
    const cplx* __restrict__ Qc = Qt + ((size_t)g * B + bp) * n_end * 64 + lane;
    cplx* As = A + (size_t)(live ? sys : 0) * sys_stride;
    for (int e = wave; e < npr; e += FILL_SYS_THREADS / 64) {
      const uint32_t a0 = sPtr[4 * e], a1 = sPtr[4 * e + 1], a2 = sPtr[4 * e + 2], a3 = sPtr[4 * e + 3], a4 = sPtr[4 * e + 4];
      const uint32_t l0 = a1 - a0, l1 = a2 - a1, l2 = a3 - a2, l3 = a4 - a3;
      uint32_t lm = l0 > l1 ? l0 : l1; lm = lm > l2 ? lm : l2; lm = lm > l3 ? lm : l3;
      double s0r = 0, s0i = 0, s1r = 0, s1i = 0, s2r = 0, s2i = 0, s3r = 0, s3i = 0;
      // all bounds are wave-uniform.  Per step the four chains' coefficient / offset reads are issued, then the four table loads,
      // then the FMAs (one `if (i < len)` block per chain made hipcc wait for each load in turn: 175 ms per 256 systems);
      // a chain that has run out takes the chunk's dummy term (coefficient 0, row 0).  Two steps per trip: eight loads in flight.
      const uint32_t dummy = sPtr[4 * npr];
      uint32_t q0 = a0, q1 = a1, q2p = a2, q3 = a3;
      for (uint32_t i = 0; i < lm; i += 2) {
        const uint32_t g0 = q0 < a1 ? q0 : dummy, g1 = q1 < a2 ? q1 : dummy, g2 = q2p < a3 ? q2p : dummy, g3 = q3 < a4 ? q3 : dummy;
        const uint32_t h0 = q0 + 1 < a1 ? q0 + 1 : dummy, h1 = q1 + 1 < a2 ? q1 + 1 : dummy, h2 = q2p + 1 < a3 ? q2p + 1 : dummy, h3 = q3 + 1 < a4 ? q3 + 1 : dummy;
        const double c0 = sCoef[g0], c1 = sCoef[g1], c2v = sCoef[g2], c3 = sCoef[g3];
        const double d0 = sCoef[h0], d1 = sCoef[h1], d2v = sCoef[h2], d3 = sCoef[h3];
        const uint32_t o0 = sOff[g0], o1 = sOff[g1], o2 = sOff[g2], o3 = sOff[g3];
        const uint32_t r0 = sOff[h0], r1 = sOff[h1], r2o = sOff[h2], r3 = sOff[h3];
        const cplx z0 = Tl[o0], z1 = Tl[o1], z2 = Tl[o2], z3 = Tl[o3];
        const cplx w0 = Tl[r0], w1 = Tl[r1], w2 = Tl[r2o], w3 = Tl[r3];
        s0r = fma(c0, z0.x, s0r); s0i = fma(c0, z0.y, s0i);
        s1r = fma(c1, z1.x, s1r); s1i = fma(c1, z1.y, s1i);
        s2r = fma(c2v, z2.x, s2r); s2i = fma(c2v, z2.y, s2i);
        s3r = fma(c3, z3.x, s3r); s3i = fma(c3, z3.y, s3i);
        s0r = fma(d0, w0.x, s0r); s0i = fma(d0, w0.y, s0i);
        s1r = fma(d1, w1.x, s1r); s1i = fma(d1, w1.y, s1i);
        s2r = fma(d2v, w2.x, s2r); s2i = fma(d2v, w2.y, s2i);
        s3r = fma(d3, w3.x, s3r); s3i = fma(d3, w3.y, s3i);
        q0 += 2; q1 += 2; q2p += 2; q3 += 2;
      }
      const int mr = sMeta[3 * e], mc = sMeta[3 * e + 1], md = sMeta[3 * e + 2];
      const int row_c = mr & 0xffff, row_s = (mr >> 16) & 0xffff, col_c = mc & 0xffff, col_s = (mc >> 16) & 0xffff;
      const bool r2 = row_s != 0xffff, c2 = col_s != 0xffff;
      cplx x00 = make_double2(s0r, s0i), x01 = make_double2(s1r, s1i), x10 = make_double2(s2r, s2i), x11 = make_double2(s3r, s3i);
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
      const cplx scale = cmul(Qr[(md & 0xffff) * 64], Qc[(md >> 16) * 64]);
      if (live && !abl_nostore) {
        auto put = [&](int rslot, int cslot, cplx val) {
          const int row = b * H + rslot, col = bp * H + cslot;        // b < bp: strictly above the diagonal
          const cplx w = cmul(val, scale);
          As[(size_t)row * lda + col] = w;
          if ((row >> 6) == (col >> 6)) As[(size_t)col * lda + row] = w;
        };
        put(row_c, col_c, x00);
        if (c2) put(row_c, col_s, x01);
        if (r2) { put(row_s, col_c, x10); if (c2) put(row_s, col_s, x11); }
      }
    }
  }
}

// what k_fill_sym leaves: the identity diagonal blocks and the padding, again only where the factorisation reads
// (columns c >= 64 (r / 64) of row r); one workgroup per row
__global__ void __launch_bounds__(64) k_fill_sym_diag(int H, int N, int n_pad, cplx* __restrict__ A, long long lda, long long sys_stride, int no_pad) {
  const int r = blockIdx.x, s = blockIdx.y;
  cplx* row = A + (size_t)s * sys_stride + (size_t)r * lda;
  const int c0 = (r / 64) * 64;
  auto put = [&](int c) { row[c] = (r == c) ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0); };
  if (r >= N) { for (int c = c0 + threadIdx.x; c < n_pad; c += 64) put(c); return; }
  const int br = r / H, bend = (br + 1) * H;              // this row's own ball: columns [br H, bend)
  for (int c = (c0 > br * H ? c0 : br * H) + threadIdx.x; c < bend; c += 64) put(c);
  if (!no_pad) for (int c = N + threadIdx.x; c < n_pad; c += 64) put(c);
}

// split form: the same for the E block (rows [0, npE): nE active, ball runs of U) and the O block (rows [npE, npE + npO): nO active,
// runs of H - U), each with its own unit diagonal and identity padding, columns counted from the block's origin
__global__ void __launch_bounds__(64) k_fill_sym_diag_split(int H, int U, int B, int npE, int npO, cplx* __restrict__ A, long long lda,
                                                            long long sys_stride) {
  const int r = blockIdx.x, s = blockIdx.y;
  const bool odd = r >= npE;
  const int base = odd ? npE : 0, lr = r - base, run = odd ? H - U : U, nact = B * run, np = odd ? npO : npE;
  cplx* row = A + (size_t)s * sys_stride + (size_t)r * lda + base;
  const int c0 = (lr / 64) * 64;
  auto put = [&](int c) { row[c] = (lr == c) ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0); };
  if (lr >= nact) { for (int c = c0 + threadIdx.x; c < np; c += 64) put(c); return; }
  const int br = lr / run, bend = (br + 1) * run;
  for (int c = (c0 > br * run ? c0 : br * run) + threadIdx.x; c < bend; c += 64) put(c);
  for (int c = nact + threadIdx.x; c < np; c += 64) put(c);
}

__global__ void k_split_info_merge(int nb, int npE, int npO, int* __restrict__ info, const int* __restrict__ info_O) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  const int e = info[s], o = info_O[s], grow = -(npE + npO + 1);
  if (e != 0) info[s] = e == -(npE + 1) ? grow : e;
  else if (o != 0) info[s] = o == -(npO + 1) ? grow : o < 0 ? o - npE : o;
}

int launch_split_info_merge(int nb, int npE, int npO, int* d_info, const int* d_info_O, hipStream_t st) {
  if (nb <= 0) return BIEM_OK;
  hipLaunchKernelGGL(k_split_info_merge, dim3((nb + 255) / 256), dim3(256), 0, st, nb, npE, npO, d_info, d_info_O);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// bytes of one system the symmetric path writes and the factorisation reads: sum over rows of 16 * 64 (r / 64 + 1)
double fill_sym_bytes(int n_pad) {
  const double t = n_pad / 64;
  return 16.0 * 64.0 * 64.0 * t * (t + 1.0) * 0.5;
}

// whether launch_fill_sym runs k_fill_red (the one form with a split mode)
bool fill_sym_red_form(const biem_plan* p, int B) { return B > 1 && fill_sym_form(p).kind == FillSymForm::RED && fill_lists_order_ok(p); }

// ---- grid-y of the list forms: workgroups per chunk, each looping over its share of the ncomb combinations
static unsigned fill_gy_clamp(long long gy, long long ncomb) {
  if (gy < 1) gy = 1;
  if (gy > ncomb) gy = ncomb;
  if (gy > 65535) gy = 65535;
  return (unsigned)gy;
}
// systems in lanes: about 16 workgroups per CU in all; BIEM_FILL_GY (this form only) overrides
static unsigned fill_sys_gy(int nchunks, long long ncomb) {
  long long gy = (16 * 256 + nchunks - 1) / nchunks;
  { const char* e = getenv("BIEM_FILL_GY"); if (e && atoi(e) > 0) gy = atoi(e); }
  return fill_gy_clamp(gy, ncomb);
}
// one unit pair per lane: enough workgroups to fill the chip a few times over, each with a long loop over combinations
static unsigned fill_lane_gy(const biem_plan* p, bool use_red, int nchunks, long long ncomb) {
  long long gy = (8 * 256 + nchunks - 1) / nchunks;
  if (use_red && p->red_waves == 16) {
    // one workgroup per CU at a time (its lists take the CU's LDS): the grid runs in rounds of 256 workgroups of about equal work, so a
    // grid of 8.1 rounds costs 9.  Among 6 .. 10 rounds' worth of workgroups take the count that wastes least of its last round
    // (cfg 3: 77 chunks x 27 = 8.12 rounds -> x 26 = 7.82: -10 % fill time)
    static int ncu_of[64] = {0};               // CUs per device, queried once
    int devid = 0, ncu = 256;
    if (hipGetDevice(&devid) == hipSuccess && devid >= 0 && devid < 64) {
      if (ncu_of[devid] == 0) { int v = 0; ncu_of[devid] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, devid) == hipSuccess && v > 0) ? v : 256; }
      ncu = ncu_of[devid];
    }
    double best = 1e30;
    for (long long g = (6LL * ncu + nchunks - 1) / nchunks; g <= (10LL * ncu) / nchunks + 1; ++g) {
      if (g < 1) continue;
      const double wgs = (double)nchunks * g, rounds = ceil(wgs / ncu);
      const double waste = rounds * ncu / wgs;
      if (waste < best - 1e-9 || (waste < best + 1e-9 && g > gy)) { best = waste; gy = g; }
    }
  }
  return fill_gy_clamp(gy, ncomb);
}

// ---- the forms (SymFill, fill.hpp: the operands of one call)
// systems in lanes.  Workspace: Tt[groups][npairs][H2][64] then Qt[groups][B][n_end][64] (fill_workspace_bytes covers it)
static int fill_sym_sys(const SymFill& c, size_t shm, size_t work_bytes) {
  const biem_plan* p = c.p;
  const int nb = c.nb, B = c.B, U = (int)(p->units.size() / 2);
  const int nbp = (nb + 63) / 64 * 64, npairs = B * (B - 1) / 2;
  const size_t need = ((size_t)npairs * p->H2 + (size_t)B * p->n_end) * nbp * sizeof(cplx);
  if (need > work_bytes) { set_error("biem_fill (symmetric, systems in lanes): workspace too small for %d systems", nb); return BIEM_ERR_ARG; }
  cplx* Qt = c.T + (size_t)npairs * p->H2 * nbp;
  if (p->H2 > 65536) { set_error("biem_fill (symmetric, systems in lanes): n_end=%d has %d table labels, the 16-bit term indices hold 65536", p->n_end, p->H2); return BIEM_ERR_UNSUPPORTED; }
  if (shm > 64 * 1024 || (size_t)p->H2 * 64 >= (1ull << 32)) { set_error("biem_fill (symmetric, systems in lanes): a unit pair of n_end=%d has %d terms", p->n_end, p->schunk_terms_max); return BIEM_ERR_UNSUPPORTED; }
  { const int rc = launch_pair_tables(p, nb, B, c.d_k, c.d_centers, c.geom_batched, c.d_tab, PT_SYS_LANES, nullptr, c.T, c.st); if (rc) return rc; }
  const int nq = B * p->n_end * nbp;
  hipLaunchKernelGGL(k_qfactors_t, dim3((nq + 255) / 256), dim3(256), 0, c.st, p->n_end, B, nb, nbp, (const cplx*)c.d_tab, Qt);
  BIEM_LAUNCHCHK();
  const int nchunks = (int)p->schunk.size() - 1;
  const unsigned gy = fill_sys_gy(nchunks, (long long)npairs * (nbp / 64));
  BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_fill_sys, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  hipLaunchKernelGGL(k_fill_sys, dim3(nchunks, gy), dim3(FILL_SYS_THREADS), shm, c.st, p->H, U, p->H2, p->n_end, B, nb, nbp, npairs, p->d_deg,
                     p->d_units, p->d_spos, p->d_schunk, p->schunk_terms_max, p->schunk_pairs_max, p->d_qptr, p->d_qcoef, p->d_qidx16,
                     (const cplx*)c.T, (const cplx*)Qt, c.A, c.lda, c.sys_stride, getenv("BIEM_ABL_FILL_NOSTORE") ? 1 : 0);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

// one unit pair per lane: k_fill_red (reduced table; with the split layout of flat sphere configurations) or the gather form k_fill_sym
static int fill_sym_lanes(const SymFill& c, bool use_red, size_t shm, const SplitMap& split) {
  const biem_plan* p = c.p;
  const int nb = c.nb, B = c.B, H = p->H, U = (int)(p->units.size() / 2), npairs = B * (B - 1) / 2;
  const int nchunks = use_red ? (int)p->rchunk.size() - 1 : (int)p->qchunk.size() - 1;
  { const int rc = launch_classes_and_tables(c, use_red ? PT_REDUCED : PT_PAIRED); if (rc) return rc; }
  const unsigned gy = fill_lane_gy(p, use_red, nchunks, (long long)npairs * nb);
  const int HR = p->E + p->NP + 2 * p->n_end;
  const int red_threads = 64 * p->red_waves;
  const int kt_need = use_red ? (HR + red_threads - 1) / red_threads : (p->H2lin + FILL_SYM_THREADS - 1) / FILL_SYM_THREADS;
#define BIEM_LAUNCH_FILL_RED_AS(KT, NC, SP)                                                                                               \
  {                                                                                                                                       \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_fill_red<KT, NC, SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));          \
    hipLaunchKernelGGL((k_fill_red<KT, NC, SP>), dim3(nchunks, gy), dim3(red_threads), shm, c.st, H, U, HR, p->E, p->NP, p->n_end, B, nb, npairs, \
                       p->d_deg, p->d_units, p->d_spos, p->d_rchunk, p->d_rcrow, p->d_rwrow, p->rchunk_rows_max, p->d_rcoef, p->d_ridx,   \
                       p->d_rphsel, c.T, c.A, c.lda, c.sys_stride, c.pc.classes, split.npE);                                              \
  }
  // two combinations per iteration (the plan reserves LDS for two table rows) unless BIEM_FILL_NC=1 at plan build (A / B runs).
  // KT = 8 runs one combination per iteration whatever the plan says: with two, 16 prefetch registers of four VGPRs each are live under
  // the 128-VGPR bound of a 1024-thread workgroup, and the register allocator spilled outputs of the inline-asm loads right behind the
  // asm statement - BEFORE their wait in BIEM_TN_CLAIM - and reused the registers as the next load's address (k_fill_red<8, 2, false>:
  // 101 spilled VGPRs; caa n_end 14 was the first plan the tests ran through it, and it ended in an illegal memory access).  The
  // instantiation is not built any more; _build.check_isa refuses a library in which any k_fill_red reads a prefetch register before
  // the wait.  (The kernel's LDS layout follows its own NC, so the second table row the plan reserved stays unused.)
#define BIEM_LAUNCH_FILL_RED(KT)                                                                                                          \
  {                                                                                                                                       \
    if (p->red_nc == 2) { if (split.on()) BIEM_LAUNCH_FILL_RED_AS(KT, 2, true) else BIEM_LAUNCH_FILL_RED_AS(KT, 2, false) }               \
    else { if (split.on()) BIEM_LAUNCH_FILL_RED_AS(KT, 1, true) else BIEM_LAUNCH_FILL_RED_AS(KT, 1, false) }                              \
  }
#define BIEM_LAUNCH_FILL_RED_ONE(KT) { if (split.on()) BIEM_LAUNCH_FILL_RED_AS(KT, 1, true) else BIEM_LAUNCH_FILL_RED_AS(KT, 1, false) }
#define BIEM_LAUNCH_FILL_SYM(KT)                                                                                                          \
  {                                                                                                                                       \
    BIEM_HIPCHK(hipFuncSetAttribute((const void*)k_fill_sym<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));                  \
    hipLaunchKernelGGL(k_fill_sym<KT>, dim3(nchunks, gy), dim3(FILL_SYM_THREADS), shm, c.st, H, U, p->H2lin, p->n_end, B, nb, npairs,     \
                       p->d_deg, p->d_units, p->d_spos, p->d_qchunk, p->qchunk_terms_max, p->qchunk_pairs_max, p->d_q2ptr, p->d_q2coef,   \
                       p->d_q2idx16, c.T, (const cplx*)c.d_tab, c.A, c.lda, c.sys_stride, c.pc.classes);                                  \
  }
  if (use_red) {
    if (kt_need <= 1) BIEM_LAUNCH_FILL_RED(1)
    else if (kt_need <= 2) BIEM_LAUNCH_FILL_RED(2)
    else if (kt_need <= 4) BIEM_LAUNCH_FILL_RED(4)
    else BIEM_LAUNCH_FILL_RED_ONE(8)
  }
  else if (kt_need <= 1) BIEM_LAUNCH_FILL_SYM(1)
  else if (kt_need <= 2) BIEM_LAUNCH_FILL_SYM(2)
  else if (kt_need <= 3) BIEM_LAUNCH_FILL_SYM(3)
  else if (kt_need <= 4) BIEM_LAUNCH_FILL_SYM(4)
  else if (kt_need <= 6) BIEM_LAUNCH_FILL_SYM(6)
  else BIEM_LAUNCH_FILL_SYM(8)
#undef BIEM_LAUNCH_FILL_SYM
#undef BIEM_LAUNCH_FILL_RED
#undef BIEM_LAUNCH_FILL_RED_ONE
#undef BIEM_LAUNCH_FILL_RED_AS
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

int launch_fill_sym(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched, const double* d_tab,
                    double* d_A, long long lda, long long sys_stride, int n_pad, void* d_work, size_t work_bytes, hipStream_t st, bool no_padding,
                    const FillDedupe* dedupe, const SplitMap& split) {
  const int H = p->H, N = B * H, U = (int)(p->units.size() / 2);
  if (nb <= 0 || B <= 0) return BIEM_OK;
  if (lda < n_pad || n_pad < N || n_pad % 64) { set_error("biem_fill (symmetric): lda / n_pad too small or n_pad not a multiple of 64"); return BIEM_ERR_ARG; }
  const size_t ws = fill_workspace_bytes(p, nb, B);
  if (work_bytes < ws) { set_error("biem_fill: workspace too small"); return BIEM_ERR_ARG; }
  if (nb > 65535) { set_error("biem_fill (symmetric): at most 65535 systems per call"); return BIEM_ERR_ARG; }
  if (split.on() && (split.U != U || n_pad != split.npE + split.npO || !fill_sym_red_form(p, B) || no_padding)) {
    set_error("biem_fill (symmetric, split): internal: layout or fill form"); return BIEM_ERR_ARG;
  }
  ProfScope ps(PK_FILL, st, (double)nb * (split.on() ? fill_sym_bytes(split.npE) + fill_sym_bytes(split.npO) : fill_sym_bytes(n_pad)));
  const FillSymForm form = fill_sym_form(p);
  if (form.kind != FillSymForm::DIRECT2D && !fill_lists_order_ok(p)) { set_error("n_end=%d exceeds the built table size", p->n_end); return BIEM_ERR_UNSUPPORTED; }
  const SymFill c = {p, nb, B, d_k, d_centers, geom_batched, d_tab, (cplx*)d_A, lda, sys_stride, (cplx*)d_work,
                     pair_classes_at((char*)d_work + ws - fill_dedupe_bytes(B), B), dedupe, st};
  int rc = BIEM_OK;
  if (B > 1) switch (form.kind) {
    case FillSymForm::DIRECT2D: rc = launch_fill2d_sym(c); break;
    case FillSymForm::SYS: rc = fill_sym_sys(c, form.shm, work_bytes); break;
    case FillSymForm::RED: rc = fill_sym_lanes(c, true, form.shm, split); break;
    case FillSymForm::ENTRY: rc = fill_sym_lanes(c, false, form.shm, split); break;
    case FillSymForm::UNFIT:
      set_error("biem_fill (symmetric, one unit pair per lane): tables do not fit LDS (n_end=%d: H2=%d, chunk terms=%d)", p->n_end, p->H2, p->qchunk_terms_max);
      return BIEM_ERR_UNSUPPORTED;
  }
  if (rc) return rc;
  // the diagonal behind the form kernel (no_padding: the caller's solver never reads the identity padding - the LDS-resident path of small systems)
  if (split.on()) hipLaunchKernelGGL(k_fill_sym_diag_split, dim3(n_pad, nb), dim3(64), 0, st, H, U, B, split.npE, split.npO, (cplx*)d_A, lda, sys_stride);
  else hipLaunchKernelGGL(k_fill_sym_diag, dim3(no_padding ? N : n_pad, nb), dim3(64), 0, st, H, N, n_pad, (cplx*)d_A, lda, sys_stride, no_padding ? 1 : 0);
  BIEM_LAUNCHCHK();
  return BIEM_OK;
}

}  // namespace biem
