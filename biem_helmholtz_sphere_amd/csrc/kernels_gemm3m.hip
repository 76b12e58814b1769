// kernels_gemm3m.hip -- trailing update of the dense factorisations: persistent 3M zgemm on v_mfma_f64_4x4x4_4b_f64.  One body,
// gemm3m_body, for four kernels: k_gemm3m_pipe<KD> (K = 64 / 128 / 192 / 256, and KD = 0, the K-long form of the left-looking update),
// k_gemm3m_narrow<NF> (its last tile column), and the pure products k_gemm3m_strip (K = 64) and k_gemm3m_stack<KD> (K = 128 / 192 /
// 256).  The asm statement of the chunk loop is composed from one set of pieces (BIEM_FRAG_READS16 ... BIEM_DMA_INS, above the body),
// where the timing ablations that cut into it are defined too.  Also here: the tile grids and launchers, the MFMA micro-benchmark and
// the BIEM_GEMM_TRACE debug entries.
//
// MFMA form.  Measured on MI355X (tools/mfma_probe*.hip, profiles/r01_mfma_f64_*probe*.txt): the 16x16x4 f64 MFMA
// saturates at ~47-49 TFLOP/s (one per ~100 cycles per SIMD) at any occupancy, the 4-block 4x4x4 form issues every
// 16.3 cycles = 75-78 TFLOP/s with >= 48 independent accumulators.  The 4-block form multiplies A_blk (4x4) by B_blk (4x4)
// for blk = 0..3 (lane l: i|j = l&3, blk = (l>>2)&3, k = l>>4; D: j = l&3, blk, i = l>>4; CBSZ/ABID are not honoured
// for f64: profiles/r01_mfma_f64_4x4x4_layout.txt), so a 16x16 tile is built from 4 instructions whose A fragment holds
// the SAME 4-row block in all four slots (an LDS broadcast read): accumulator g = rows 4g..4g+3 x 16 columns, i.e.
// register g of the 16x16x4 result layout.  The f64 NEG bits (blgp bit 0 negates A) give acc = C - A*B directly.
//
// Memory schedule.  With K = NB the update is only 16 flop per byte of C traffic; a read-modify-write epilogue leaves
// every wave ~60 % of its cycles in s_waitcnt (profiles/r01_gemm_pmc.txt) because all workgroups hit HBM together and
// the MFMAs then idle.  Each workgroup is persistent and streams: the C tile is loaded in slices during the K-chunks,
// the final stores stay in flight while the next tile starts, and the operand stream runs ahead across tile boundaries.
//
// Tile order.  Tiles are numbered system-major, then bands of 8 tile-rows, then column-major inside a band, so 64
// consecutive tiles form an 8 x 8 block sharing 8 A- and 8 B-panels.  The workgroups that share blockIdx % 8 (one XCD
// under the observed round-robin placement; speed only) sweep one block together.
// (Superseded variants - 16x16x4 MFMA with RMW epilogue, 2-stage 4M and 3M kernels - are described with their numbers
// in DESIGN.md section 5; their sources are in the git history.)
#include "dense.hpp"

namespace biem {

// (every member has its "off" value as default: a launcher sets what its launch uses)
struct TileGrid {
  int ty_n = 0, tx_n = 0, per_sys = 0, full_bands = 0, ntiles = 0;
  int row_begin = 0, row_end = 0, col_begin = 0, col_end = 0;   // C region updated by this launch
  int brow = 0;                                 // first row of the B operand (U12 rows brow .. brow + K)
  // tiles of tile column `pcol_tx` deliver their result transposed into the panel workspace (the next panel to factor:
  // column-major P[c][row]) instead of the matrix, which saves that panel's transposing load; pout == nullptr: off
  cplx* pout = nullptr; long long pout_ld = 0, pout_stride = 0; int pcol_tx = 0;
  int tri = 0;                                  // 1: only tiles with tx <= ty (square region, symmetric update); 2: only tx >= ty
  // (ty << 16 | tx) of the first tri_full tiles of that order (the full bands); the K-long launch (k_gemm3m_pipe<0>, band order
  // below, no tile map) keeps its K-chunks per tile, kd / 8, in the same word: the argument layout of the other launches is unchanged
  const int* tri_map = nullptr; union { int tri_full = 0; int nch; };
  int blk_sh = 0;                               // log2 of the tiles per XCD block of the workgroup -> tile map: 6, or 3 for small launches
  unsigned long long per_sys_magic = 0;         // ceil(2^40 / per_sys): t / per_sys = (t * magic) >> 40 for t < 2^25 (scalar multiply, no VALU division)
};
// nch shares tri_full's word: only k_gemm3m_pipe<0> reads nch, and it never calls tile_decode (the one reader of tri_full); its
// launch (launch_gemm_left) sets tri = 0 and no tile map.  The layout the fixed-K instances were compiled against is pinned:
static_assert(sizeof(TileGrid) == 96 && offsetof(TileGrid, nch) == offsetof(TileGrid, tri_full) && offsetof(TileGrid, tri_full) == 80 &&
              offsetof(TileGrid, per_sys_magic) == 88, "TileGrid: the kernel-argument layout of k_gemm3m_pipe changed");

// the triangular order: lower triangle incl. the diagonal tiles in bands of 8 tile rows; band b (tile rows 8b .. 8b+hb-1) holds
// the columns 0 .. 8b+hb-1, column-major; column tx <= 8b has hb tiles, column 8b+q has hb-q.  A full band holds 64 b + 36
// tiles, 32 b^2 + 4 b tiles precede it - independent of the matrix size, so ONE table serves every launch of a factorisation.
__device__ __host__ inline void tri_decode_band(int r, int b, int hb, int& ty, int& tx) {
  int rr = r - (32 * b * b + 4 * b);
  if (rr < 8 * b * hb) { tx = rr / hb; ty = 8 * b + rr - tx * hb; }
  else {
    int rem = rr - 8 * b * hb, q = 0;
    while (rem >= hb - q) { rem -= hb - q; ++q; }
    tx = 8 * b + q; ty = 8 * b + q + rem;
  }
}
__global__ void k_tri_map(int* map, int n) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int b = (int)((sqrtf(16.0f + 128.0f * (float)r) - 4.0f) * (1.0f / 64.0f));
  while (b > 0 && 32 * b * b + 4 * b > r) --b;
  while (32 * (b + 1) * (b + 1) + 4 * (b + 1) <= r) ++b;
  int ty, tx;
  tri_decode_band(r, b, 8, ty, tx);
  map[r] = ty << 16 | tx;
}

__device__ inline void tile_decode(const TileGrid& tg, int t, int& s, int& ty, int& tx) {
  s = (int)(((unsigned long long)(unsigned)t * tg.per_sys_magic) >> 40);
  int r = t - s * tg.per_sys;
  if (r >= tg.per_sys) { r -= tg.per_sys; ++s; }      // (never taken for t < 2^25; kept as a guard)
  if (tg.tri) {
    if (r < tg.tri_full) { const int v = tg.tri_map[r]; ty = v >> 16; tx = v & 0xffff; }
    else tri_decode_band(r, tg.full_bands, tg.ty_n - 8 * tg.full_bands, ty, tx);      // the partial last band
    if (tg.tri == 2) { const int t2 = ty; ty = tx; tx = t2; }                          // upper triangle: the mirror tile
    return;
  }
  int fb = tg.full_bands * 8 * tg.tx_n;
  if (r < fb) {
    int band = r / (8 * tg.tx_n), rr = r - band * 8 * tg.tx_n;
    tx = rr >> 3; ty = band * 8 + (rr & 7);
  } else {
    int rem = r - fb, h = tg.ty_n - tg.full_bands * 8;
    tx = rem / h; ty = tg.full_bands * 8 + rem - tx * h;
  }
}

// the band order of a left-looking launch: a band of h = ty_n <= 4 tile rows, the tiles with tx >= ty, column-major (four-tall):
// column q < h holds q + 1 tiles (q (q + 1) / 2 precede it), every later column h; h (h + 1) / 2 + (tx_n - h) h tiles per system.
// 64 consecutive tiles right of the diagonal block are 4 A panels x 16 B panels.
__device__ __host__ inline int band_tiles(int h, int tx_n) { return tx_n >= h ? h * (h + 1) / 2 + (tx_n - h) * h : tx_n * (tx_n + 1) / 2; }
__device__ __host__ inline void band_decode(int r, int h, int& ty, int& tx) {
  const int head = h * (h + 1) / 2;
  if (r < head) {
    int q = 0;
    while (r >= q + 1) { r -= q + 1; ++q; }
    tx = q; ty = r;
  } else {
    const int rem = r - head;
    if (h == 4) { tx = 4 + (rem >> 2); ty = rem & 3; }
    else { const int c = rem / h; tx = h + c; ty = rem - c * h; }
  }
}
// ROW1: a launch of ONE tile row without a tile map (the stacked pass): tile r of a system is tile column r
// COL1: a launch of ONE tile column without a tile map (the narrow launch of the left-looking update): tile r of a system is tile row r
template <int KD, bool ROW1 = false, bool COL1 = false>
__device__ inline void tile_decode_of(const TileGrid& tg, int t, int& s, int& ty, int& tx) {
  if constexpr (COL1) {
    s = (int)(((unsigned long long)(unsigned)t * tg.per_sys_magic) >> 40);
    ty = t - s * tg.per_sys;
    if (ty >= tg.per_sys) { ty -= tg.per_sys; ++s; }
    tx = 0;
  } else if constexpr (ROW1) {
    s = (int)(((unsigned long long)(unsigned)t * tg.per_sys_magic) >> 40);
    tx = t - s * tg.per_sys;
    if (tx >= tg.per_sys) { tx -= tg.per_sys; ++s; }
    ty = 0;
  } else if constexpr (KD == 0) {
    s = (int)(((unsigned long long)(unsigned)t * tg.per_sys_magic) >> 40);
    int r = t - s * tg.per_sys;
    if (r >= tg.per_sys) { r -= tg.per_sys; ++s; }
    band_decode(r, tg.ty_n, ty, tx);
  } else tile_decode(tg, t, s, ty, tx);
}

constexpr int BM3 = 64, BN3 = 64;   // workgroup tile of the trailing update
constexpr int GEMM_GRID_CAP = 512;  // the persistent grid of the update kernels: 2 workgroups per CU
constexpr int KC = 8;               // K rows per LDS stage (chunk)

// ---------------------------------------------------------------------------------------------
// trailing update, 3M form with a 3-stage LDS-DMA ring (product kernel).
// Evidence for the structure: the 2-stage kernels above run the 3M and the 4M arithmetic in the SAME time
// (444.7 vs 447.7 ms per 32-system step) - the update is bound by the latency of loads issued one chunk ahead, not by the
// MFMA pipe: hipcc drains vmcnt(0) at every __syncthreads() while an LDS-DMA is in flight and before any use of a
// VGPR-destination load.  Here every byte (A chunk, B chunk and the C slice of the chunk) arrives by LDS-DMA, each wave
// issues exactly NDMA instructions per chunk (addresses are clamped instead of masked, so the count is uniform), the
// barrier is a raw s_barrier and the waits are hand-counted: s_waitcnt vmcnt(NDMA) retires the group of the chunk about
// to be multiplied and leaves the next chunk's group in flight.  A full tile's 16 result stores also sit in the VM
// queue; the first two chunks after them wait vmcnt(NDMA + 16).
// Stage = A[8][64] + B[8][64] + C slice (UPC x 256 lanes) = 20 (K=128) or 24 KiB (K=64); 3 stages; 2 workgroups per CU.
// ---------------------------------------------------------------------------------------------
template <int N> __device__ inline void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// acc += a*b / acc -= a*b on the 4-block f64 MFMA (the f64 NEG bit, blgp bit 0, negates A).
// (An inline-asm form with the accumulator tied "+v" was tried to stop hipcc from rotating accumulators through the
// register file; it produced wrong results on gfx950 even with hazard padding, and the rolled chunk loop made it
// unnecessary - the builtin is the only form used.)
__device__ inline void mfma_acc(double& acc, double a, double b) { acc = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc, 0, 0, 0); }
__device__ inline void mfma_acc_neg(double& acc, double a, double b) { acc = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc, 0, 0, 1); }
// keeps hipcc from moving VALU work into the MFMA block (and the MFMAs out of it)
__device__ inline void mfma_fence() { __builtin_amdgcn_sched_barrier(0); }

// What the ISA of earlier attempts taught (all measured):
//  * hipcc puts s_waitcnt vmcnt(0) in front of every ds_read it can see while an LDS-DMA is pending (even with one
//    __shared__ array per stage) -> fragment reads are inline asm with an explicit lgkmcnt wait;
//  * unrolling the chunk loop (3 stage copies) made hipcc rotate the 48 accumulators through the register file and copy
//    them back with ~100-200 v_mov_b64 per chunk (they share the SIMD's vector issue port with the MFMAs) -> one rolled
//    chunk loop with a run-time stage offset;
//  * per-lane 64-bit address arithmetic for 5 DMAs per chunk cost ~250 VALU instructions -> wave-uniform scalar bases plus
//    per-lane 32-bit offsets that are constant for the whole kernel.
#define BIEM_PRIO_M() __builtin_amdgcn_s_setprio(1)
#define BIEM_PRIO_O() __builtin_amdgcn_s_setprio(3)
#ifdef BIEM_GEMM_TRACE
// diagnostic build only (tools/gemm_trace.cpp): wave 0 of the first 4 workgroups stamps (all 4 waves) s_memtime at 7 points of each of its
// first 64 chunks into LDS and dumps them at exit (no VM traffic inside the loop, the hand-counted vmcnt waits stay valid)
__device__ unsigned long long g_gemm_trace[16][64][8];
#ifdef BIEM_TR_STAMPS
#define BIEM_TR(i) { if (lane == 0 && tr_n < 64) s_tr[(wave * 64 + tr_n) * 8 + (i)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define BIEM_TR_NEXT() { ++tr_n; }
#else
#define BIEM_TR(i)
#define BIEM_TR_NEXT()
#endif
#else
#define BIEM_TR(i)
#define BIEM_TR_NEXT()
#endif
// The pieces of the chunk statement.  All seven asm statements of the chunk loop of gemm3m_body - fused (with the next DMA group
// between the fragment reads and their wait) and unfused, product form, one C unit, none, two - are composed from them, so every
// instruction's text and every slot offset stands here once; the vmcnt counts rest on this text.  A fused statement reads
//   reads [C reads] | M0 save | operand DMAs [C DMAs] | M0 restore | lgkmcnt wait
// (M0 is compiler-reserved, hence save and restore; the C DMAs sit in front of the restore), an unfused one the reads and the wait.
// Byte offsets inside a stage: k4 * 4352 + g * 64 (A fragments, from aA), k4 * 4096 + n * 256 (B, from aB), u * 4096 (C units, from
// aC); DMA slots: mA and mA + 4352 (A rows w, w + 4), mB and mB + 4096 (B rows), mB + 8192 / 12288 (C units 0 / 1).
//
// The timing ablations that cut into this text (tools/build_trace.sh; results wrong by construction) are alternative definitions of
// the piece they remove or redirect, beside the count they imply - so they hold for EVERY instance that uses the piece:
//   BIEM_ABL_NOLDS    no fragment and no C reads                BIEM_ABL_NOCDMA  no C-unit DMA (BIEM_NDMA_PER_CUNIT = 0)
//   BIEM_ABL_ONLYCDMA no operand DMAs (BIEM_NDMA_OPERAND = 0)   BIEM_ABL_CHOT    the C units come from an L2-resident address
// NDMA in gemm3m_body is BIEM_NDMA_OPERAND + C units x BIEM_NDMA_PER_CUNIT: it follows the text.  (The groups that issue_dma builds
// from builtins - prologue and edge tiles - keep their full count under these flags.)
#ifdef BIEM_ABL_NOLDS
#define BIEM_FRAG_READS16 ""
#define BIEM_C_READ1 ""
#define BIEM_C_READ2 ""
#else
#define BIEM_FRAG_READS16                                                                                                                  \
  "ds_read_b128 %[b0], %[aB]\n\tds_read_b128 %[b1], %[aB] offset:256\n\tds_read_b128 %[b2], %[aB] offset:512\n\tds_read_b128 %[b3], %[aB] offset:768\n\t" \
  "ds_read_b128 %[b4], %[aB] offset:4096\n\tds_read_b128 %[b5], %[aB] offset:4352\n\tds_read_b128 %[b6], %[aB] offset:4608\n\tds_read_b128 %[b7], %[aB] offset:4864\n\t" \
  "ds_read_b128 %[a0], %[aA]\n\tds_read_b128 %[a1], %[aA] offset:64\n\tds_read_b128 %[a2], %[aA] offset:128\n\tds_read_b128 %[a3], %[aA] offset:192\n\t" \
  "ds_read_b128 %[a4], %[aA] offset:4352\n\tds_read_b128 %[a5], %[aA] offset:4416\n\tds_read_b128 %[a6], %[aA] offset:4480\n\tds_read_b128 %[a7], %[aA] offset:4544\n\t"
#define BIEM_C_READ1 "ds_read_b128 %[c0], %[aC]\n\t"
#define BIEM_C_READ2 BIEM_C_READ1 "ds_read_b128 %[c1], %[aC] offset:4096\n\t"
#endif
#define BIEM_M0_SAVE "s_mov_b32 %[keep], m0\n\t"
#define BIEM_M0_RESTORE "s_mov_b32 m0, %[keep]\n\t"
#ifdef BIEM_ABL_ONLYCDMA
#define BIEM_OPERAND_DMA4 ""
#define BIEM_NDMA_OPERAND 0
#else
#define BIEM_OPERAND_DMA4                                                                     \
  "s_mov_b32 m0, %[mA]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[oA0], %[pA]\n\t"               \
  "s_add_u32 m0, %[mA], 4352\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[oA1], %[pA]\n\t"         \
  "s_mov_b32 m0, %[mB]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[oB0], %[pB]\n\t"               \
  "s_add_u32 m0, %[mB], 4096\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[oB1], %[pB]\n\t"
#define BIEM_NDMA_OPERAND 4
#endif
#ifdef BIEM_ABL_NOCDMA
#define BIEM_C_DMA(slot, ptr) ""
#define BIEM_NDMA_PER_CUNIT 0
#else
#define BIEM_C_DMA(slot, ptr) "s_add_u32 m0, %[mB], " #slot "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[oC], %[" #ptr "]\n\t"
#define BIEM_NDMA_PER_CUNIT 1
#endif
#ifdef BIEM_ABL_CHOT
#define BIEM_C_SRC(d) ((const char*)Pw + ((d) & 0xfffff))   // (the panel workspace)
#else
#define BIEM_C_SRC(d) (pC + (d))                            // source of the C unit at byte offset d of the producer's tile
#endif
#define BIEM_LGKM_WAIT "s_waitcnt lgkmcnt(0)"
// operand lists: outputs (a fused statement puts [keep] in front), inputs (a statement with C DMAs adds [oC] and its C pointers)
#define BIEM_FRAG_OUTS                                                                                                                     \
  [a0] "=&v"(fa[0][0]), [a1] "=&v"(fa[0][1]), [a2] "=&v"(fa[0][2]), [a3] "=&v"(fa[0][3]), [a4] "=&v"(fa[1][0]), [a5] "=&v"(fa[1][1]),       \
  [a6] "=&v"(fa[1][2]), [a7] "=&v"(fa[1][3]), [b0] "=&v"(fb[0][0]), [b1] "=&v"(fb[0][1]), [b2] "=&v"(fb[0][2]), [b3] "=&v"(fb[0][3]),       \
  [b4] "=&v"(fb[1][0]), [b5] "=&v"(fb[1][1]), [b6] "=&v"(fb[1][2]), [b7] "=&v"(fb[1][3])
#define BIEM_C_OUTS1 [c0] "=&v"(cv[0])
#define BIEM_C_OUTS2 BIEM_C_OUTS1, [c1] "=&v"(cv[UPC - 1])
#define BIEM_FRAG_INS [aA] "v"(aA), [aB] "v"(aB)
#define BIEM_C_IN [aC] "v"(aC)
#define BIEM_DMA_INS [mA] "s"(mA), [mB] "s"(mB), [oA0] "v"(offA0), [oA1] "v"(offA1), [oB0] "v"(offB0), [oB1] "v"(offB1), [pA] "s"(pA), [pB] "s"(pB)

// One text of the tile loop for three kernels (as fast_layout.hpp does for the field kernels): k_gemm3m_pipe<KD> is the body with
// PROD = false.  PROD = true is the pure product of the symmetric strip pass (k_gemm3m_strip, K = 64) and of the stacked pass of a
// later panel of a group (k_gemm3m_stack<KD>, K = 128 / 192 / 256): no C slots in the stage, four DMAs and 16 fragment reads per
// chunk, no C additions; the accumulators start at zero, so the tile stored is -A^T B.
//
// The product form also carries the forward substitution of up to 8 right-hand sides (StripRhs, Y[s][q][row] compact): the strip of
// panel j holds the finished rows U[j .. j+63, :], and y[c] -= sum_r U[j + r, c] z_j[r] for the 64 columns c of a tile is taken from the
// tile in registers - in a fixed order: in-lane over the four row quads, across lane >> 4, then across the four waves through LDS.
// Exactly one workgroup per (panel, tile column, system) touches those 64 entries: no atomics, two solves agree bit for bit.  Its
// loads and stores are unknown to the ring's vmcnt counts: such a tile ends with stores_pending = 2 (vmcnt(0) at the next first chunk).
struct StripRhs { cplx* Y; int nrhs; int ld; };   // Y == nullptr: none; ld = rows per right-hand side (n_pad)
//
// NF < 4 is the narrow K-long form (k_gemm3m_narrow<NF>): the tiles of the LAST tile column of a left-looking band whose column groups
// n >= NF lie in the identity padding, where U is zero off the diagonal and the update a sum of exact zeros.  Only the 3M operand sums
// and the MFMA nests run over n < NF (24 NF MFMAs per chunk); ring, fragment reads, C units, stores and every vmcnt count are those of
// k_gemm3m_pipe<0>: the accumulators n >= NF carry their C unit and store it back.  Its launch is one tile column (COL1 decode).
template <int KD, bool PROD, bool ROW1 = false, int NF = 4>
__device__ __forceinline__ void gemm3m_body(cplx* __restrict__ A, long long lda, long long sys_stride, const cplx* __restrict__ Pw,
                                            long long ldp, long long p_stride, const TileGrid& tg, const StripRhs& yr) {
  static_assert(NF == 4 || (NF >= 1 && NF < 4 && KD == 0 && !PROD && !ROW1), "the narrow form exists for the K-long update only");
  constexpr bool COL1 = NF < 4;
  static_assert(!PROD || KD == 64 || KD == 128 || KD == 192 || KD == 256, "the product form exists for K = 64 (strip) and K = 128 / 192 / 256 (stacked pass)");
  const int n_pad = tg.row_end, n_cols = tg.col_end;
  // KD = 0 is the K-long form of the left-looking update: the chunk count is a run-time value (TileGrid.nch = kd / 8 >= 16), the
  // accumulators stay in registers over the whole K, C is read in the first 16 chunks and stored once
  constexpr int NCHC = KD / KC;              // 8, 16, 24 or 32 K-chunks per tile (0: run-time)
  const int NCH = KD != 0 ? NCHC : tg.nch;
  constexpr int UPC = KD == 0 || NCHC >= 16 ? 1 : 16 / NCHC;   // C units (one complex per lane) per chunk that carries C: 1 or 2
  constexpr int NCC = 16 / UPC;              // chunks that carry C units: the first NCC of a tile (all of them for K <= 128)
  constexpr bool ALLC = KD != 0 && NCC == NCHC;   // every chunk of a tile carries C units
  constexpr int NCD = UPC * BIEM_NDMA_PER_CUNIT;                           // C-unit DMAs of a group that carries C: UPC
  constexpr int NDMA = PROD ? BIEM_NDMA_OPERAND : BIEM_NDMA_OPERAND + NCD;   // LDS-DMA instructions per wave per chunk: 4, or 4 + UPC
  constexpr int AST = 68;                    // A row stride in LDS: +4 elements (64 B) so the broadcast A-fragment reads of
                                             // two k-rows in one ds_read_b128 lane group hit different banks
  constexpr int BOF = KC * AST;              // B block offset inside a stage
  constexpr int COF = BOF + KC * 64;         // C-slice offset
  constexpr int STG = COF + (PROD ? 0 : UPC * 256);   // complex elements per stage
  // (A fused group of its own for the K-long steady state - consumer and producer both past the NCC chunks that carry C, so 16 reads
  // and no read of the C slot - was built and measured against this text in one A/B: the bulk update ran 11 ms per cfg 3 step SLOWER
  // with it, 972.2 against 961.0 ms.  Not kept)
  __shared__ cplx ring[3 * STG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: LDS-DMA bases (M0) and tile offsets stay on the SALU
  const int l3 = lane & 3, l15 = lane & 15, l4 = lane >> 4;
  const int w = blockIdx.x, nblk = gridDim.x >> 3, xl = w & 7;
  int q = (w >> 3) - nblk;
  auto next_tile = [&]() -> int {
    for (;;) {
      q += nblk;
      int base = ((q >> tg.blk_sh) * 8 + xl) << tg.blk_sh;
      if (base >= tg.ntiles) return -1;
      int t = base + (q & ((1 << tg.blk_sh) - 1));
      if (t < tg.ntiles) return t;
    }
  };
  int t = next_tile();
  if (t < 0) return;

  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* glb_ptr_t;
  int cs, cty, ctx;
  tile_decode_of<KD, ROW1, COL1>(tg, t, cs, cty, ctx);

  const unsigned offA0 = (unsigned)(((size_t)(wave) * ldp + lane) * sizeof(cplx));
  const unsigned offA1 = (unsigned)(((size_t)(wave + 4) * ldp + lane) * sizeof(cplx));
  const unsigned offB0 = (unsigned)(((size_t)(wave) * lda + lane) * sizeof(cplx));
  const unsigned offB1 = (unsigned)(((size_t)(wave + 4) * lda + lane) * sizeof(cplx));
  // wave w owns rows 16w .. 16w+15 of the 64 x 64 tile and all 64 columns: 4 broadcast A fragments (row quads g) and 4 B
  // fragments (column groups n) per k4-step instead of the 8 + 2 of a 32 x 32 wave tile: 16 instead of 20 fragment reads
  // and 3M operand sums per chunk.  C unit u = 4 n + g: rows 16w + 4g + (lane >> 4), columns 16n + (lane & 15).
  const unsigned offC = (unsigned)(((size_t)(wave * 16 + l4) * lda + l15) * sizeof(cplx));
  // Producer state: the DMA stream runs two chunks ahead of the multiplication and crosses tile boundaries on its own.
  // Interior tiles use running scalar bases (pA, pB advance by a constant per chunk; pC = tile origin + a 16-entry
  // pattern); edge tiles recompute clamped per-lane addresses (rare).
  const long long strideA = (long long)KC * ldp * (long long)sizeof(cplx);
  const long long strideB = (long long)KC * lda * (long long)sizeof(cplx);
  int p_s = cs, p_ty = cty, p_tx = ctx, p_ch = 0;       // tile / chunk the next DMA group belongs to
  bool p_interior = false, p_valid = true;
  int p_tiles = 0, c_tiles = 0;                          // tiles started by the producer / finished by the consumer
  const char *pA = nullptr, *pB = nullptr, *pC = nullptr;
  int n_new = NDMA;                                      // size of the newest DMA group in flight (K = 256: 5 with a C unit, 4 without)
  auto producer_tile = [&]() {                             // (re)compute the bases for chunk 0 of tile (p_s, p_ty, p_tx)
    const int r0 = tg.row_begin + p_ty * BM3, c0 = tg.col_begin + p_tx * BN3;
    p_interior = r0 + BM3 <= n_pad && c0 + BN3 <= n_cols;
    pA = (const char*)(Pw + ((size_t)p_s * p_stride + r0));
    pB = (const char*)(A + ((size_t)p_s * sys_stride + (size_t)tg.brow * lda + c0));
    pC = (const char*)(A + ((size_t)p_s * sys_stride + (size_t)r0 * lda + c0));
    p_ch = 0;
    ++p_tiles;
  };
  producer_tile();
  // issue the DMA group of the producer's current chunk into stage st (exactly NDMA instructions, all lanes active), advance
  auto issue_dma = [&](int st) {
    cplx* S = ring + st * STG;
    if (p_interior) {
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(pA + offA0), (lds_ptr_t)(S + wave * AST), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(pA + offA1), (lds_ptr_t)(S + (wave + 4) * AST), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(pB + offB0), (lds_ptr_t)(S + BOF + wave * 64), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(pB + offB1), (lds_ptr_t)(S + BOF + (wave + 4) * 64), 16, 0, 0);
      if (!PROD && (ALLC || p_ch < NCC)) {
#pragma unroll
        for (int i = 0; i < UPC; ++i) {
          const int u = p_ch * UPC + i;
          const long long dC = ((long long)(4 * (u & 3)) * lda + (u >> 2) * 16) * (long long)sizeof(cplx);
          __builtin_amdgcn_global_load_lds((glb_ptr_t)(pC + dC + offC), (lds_ptr_t)(S + COF + i * 256 + wave * 64), 16, 0, 0);
        }
      }
    } else {
      // edge tile: clamp instead of masking (the instruction count must stay uniform)
      const cplx* Ps = Pw + (size_t)p_s * p_stride;
      const cplx* As = A + (size_t)p_s * sys_stride;
      const int r0 = tg.row_begin + p_ty * BM3, c0 = tg.col_begin + p_tx * BN3;
      const int ar = min(r0 + lane, n_pad - 1), bc = min(c0 + lane, n_cols - 1);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(Ps + (size_t)(p_ch * KC + wave + 4 * r) * ldp + ar),
                                         (lds_ptr_t)(S + (wave + 4 * r) * AST), 16, 0, 0);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(As + (size_t)(tg.brow + p_ch * KC + wave + 4 * r) * lda + bc),
                                         (lds_ptr_t)(S + BOF + (wave + 4 * r) * 64), 16, 0, 0);
      if (!PROD && (ALLC || p_ch < NCC)) {
#pragma unroll
        for (int i = 0; i < UPC; ++i) {
          const int u = p_ch * UPC + i;
          const int row = min(r0 + wave * 16 + 4 * (u & 3) + l4, n_pad - 1);
          const int col = min(c0 + (u >> 2) * 16 + l15, n_cols - 1);
          __builtin_amdgcn_global_load_lds((glb_ptr_t)(As + (size_t)row * lda + col),
                                           (lds_ptr_t)(S + COF + i * 256 + wave * 64), 16, 0, 0);
        }
      }
    }
    n_new = (PROD || ALLC || p_ch < NCC) ? NDMA : NDMA - NCD;      // VM instructions of the group just issued
  };
  auto advance = [&]() {
    pA += strideA; pB += strideB;
    if (++p_ch == NCH) {                                   // producer moves on to the next tile of this workgroup
      int tn = next_tile();
      if (tn >= 0) { tile_decode_of<KD, ROW1, COL1>(tg, tn, p_s, p_ty, p_tx); producer_tile(); }
      else p_valid = false;
    }
  };

  double N1[4][4], P2[4][4], N3[4][4];       // [column group n][row quad g]; flat index = C unit u = 4 n + g
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) { N1[n][g] = 0.0; P2[n][g] = 0.0; N3[n][g] = 0.0; }

#ifdef BIEM_TR_STAMPS
  __shared__ unsigned long long s_tr[4 * 64 * 8];
  int tr_n = 0;
  for (int i = tid; i < 4 * 64 * 8; i += 256) s_tr[i] = 0;
  __syncthreads();
#endif
  auto issue = [&](int st) { issue_dma(st); advance(); };
  issue(0);
  issue(1);
  int st = 0;                 // stage of the chunk about to be multiplied
  int stores_pending = 0;     // 0: none, 1: 16 stores of a full tile were issued after the groups in flight, 2: unknown count
  // per-lane LDS offsets of the fragments inside a stage (elements)
  const int fbo = BOF + l4 * 64 + l15;                    // + k4*4*64 + n*16
  const int fao = l4 * AST + wave * 16 + l3;              // + k4*4*AST + 4g
  // A VALU instruction issued while the SIMD partner (the other workgroup's wave) streams MFMAs costs ~28 cycles even at
  // priority 3 (tools/mfma_valu_mix: 8 alone, 101 at equal priority; SALU and LDS instructions are unaffected).  So the
  // phase between two MFMA blocks holds no VALU work at all: the fragment addresses of the NEXT chunk, the 3M operand sums
  // and the C-slice additions are all issued inside this wave's own MFMA block, in the shadow of its MFMAs.
  typedef const __attribute__((address_space(3))) cplx* lds_cptr_t;
  unsigned aA = (unsigned)(size_t)(lds_cptr_t)(ring + fao), aB = (unsigned)(size_t)(lds_cptr_t)(ring + fbo),
           aC = (unsigned)(size_t)(lds_cptr_t)(ring + COF + tid);                      // stage 0
  // the producer is exactly one tile ahead whenever the consumer finishes a tile (it switches at the consumer's chunk
  // NCH-3 and not again before chunk NCH-3 of the next tile): its current coordinates are the consumer's next tile
  for (;;) {
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
      // retire this chunk's DMA group (mine), then meet the other waves: their groups have landed too and nobody still
      // reads the stage the next group is about to overwrite
      BIEM_TR(0)
      // (the newest group holds n_new instructions: NDMA, or NDMA - NCD for the chunks of a K = 256 tile without a C unit)
      const bool small_grp = !ALLC && n_new != NDMA;
      if (__builtin_expect(stores_pending == 0 && p_valid, 1)) {
        if (small_grp) wait_vmcnt<NDMA - NCD>(); else wait_vmcnt<NDMA>();
      } else if (!p_valid) {
        wait_vmcnt<0>();                                   // tail of this workgroup's work: no further groups are issued
      } else if (stores_pending == 2 && c == 0) {
        wait_vmcnt<0>();
      } else if (stores_pending == 1 && c < 2) {
        if (small_grp) wait_vmcnt<NDMA - NCD + 16>(); else wait_vmcnt<NDMA + 16>();
      } else {
        if (small_grp) wait_vmcnt<NDMA - NCD>(); else wait_vmcnt<NDMA>();
      }
      BIEM_TR(1)
#ifndef BIEM_ABL_NOBARRIER
      __builtin_amdgcn_s_barrier();
#endif
      __builtin_amdgcn_sched_barrier(0);
      BIEM_TR(2)
      const int st2 = st >= 1 ? st - 1 : 2;            // (st + 2) % 3
      // interior chunks put their DMA group between the fragment reads and the lgkmcnt wait (below):
      // the VMEM issue (~100 cycles per instruction with 8 waves' groups in flight) then runs under the LDS latency
#ifdef BIEM_ABL_NODMA      // timing ablation: no DMA at all (compute-only period)
      const bool fused = false;
      if (p_valid) advance();
#else
      const bool fused = p_valid && p_interior;
      if (p_valid && !fused) issue(st2);
#endif
      __builtin_amdgcn_sched_barrier(0);
      BIEM_TR(3)
      // fragments of both k4-steps and the C units of this chunk: 16 + UPC ds_read_b128 and their lgkmcnt wait in ONE asm
      // statement - hipcc may copy an asm output right after the statement, i.e. before a separate wait (that was the
      // cause of percent-level errors in an earlier build).  Seven statements, one per group form, all from the pieces above
      cplx fb[2][4], fa[2][4], cv[UPC];   // [k4][column group of 16], [k4][row quad]
      unsigned m0_keep;                    // M0 is compiler-reserved: the fused statements save and restore it
      {
        if (PROD && fused) {
          // the product form: 16 fragment reads, the four operand DMAs
          typedef __attribute__((address_space(3))) cplx* lds_cplx_t;
          cplx* S2 = ring + st2 * STG;
          const unsigned mA = (unsigned)(size_t)(lds_cplx_t)(S2 + wave * AST), mB = (unsigned)(size_t)(lds_cplx_t)(S2 + BOF + wave * 64);
          asm volatile(BIEM_FRAG_READS16 BIEM_M0_SAVE BIEM_OPERAND_DMA4 BIEM_M0_RESTORE BIEM_LGKM_WAIT
                       : [keep] "=&s"(m0_keep), BIEM_FRAG_OUTS
                       : BIEM_FRAG_INS, BIEM_DMA_INS
                       : "memory", "scc");
          __builtin_amdgcn_sched_barrier(0);
          n_new = NDMA;
          advance();
        } else if constexpr (PROD) {
          asm volatile(BIEM_FRAG_READS16 BIEM_LGKM_WAIT : BIEM_FRAG_OUTS : BIEM_FRAG_INS : "memory");
        } else if (UPC == 1 && fused && (ALLC || p_ch < NCC)) {
          typedef __attribute__((address_space(3))) cplx* lds_cplx_t;
          cplx* S2 = ring + st2 * STG;
          const unsigned mA = (unsigned)(size_t)(lds_cplx_t)(S2 + wave * AST), mB = (unsigned)(size_t)(lds_cplx_t)(S2 + BOF + wave * 64);
          const long long dC = ((long long)(4 * (p_ch & 3)) * lda + (p_ch >> 2) * 16) * (long long)sizeof(cplx);
          const char* pCc = BIEM_C_SRC(dC);
          asm volatile(BIEM_FRAG_READS16 BIEM_C_READ1 BIEM_M0_SAVE BIEM_OPERAND_DMA4 BIEM_C_DMA(8192, pC) BIEM_M0_RESTORE BIEM_LGKM_WAIT
                       : [keep] "=&s"(m0_keep), BIEM_FRAG_OUTS, BIEM_C_OUTS1
                       : BIEM_FRAG_INS, BIEM_C_IN, BIEM_DMA_INS, [oC] "v"(offC), [pC] "s"(pCc)
                       : "memory", "scc");
          __builtin_amdgcn_sched_barrier(0);
          n_new = NDMA;
          advance();
        } else if (UPC == 1 && fused) {     // K = 256, producer chunk >= 16: no C unit in this group
          typedef __attribute__((address_space(3))) cplx* lds_cplx_t;
          cplx* S2 = ring + st2 * STG;
          const unsigned mA = (unsigned)(size_t)(lds_cplx_t)(S2 + wave * AST), mB = (unsigned)(size_t)(lds_cplx_t)(S2 + BOF + wave * 64);
          // (the consumer may still be inside the NCC chunks that carry C: the C read stays)
          asm volatile(BIEM_FRAG_READS16 BIEM_C_READ1 BIEM_M0_SAVE BIEM_OPERAND_DMA4 BIEM_M0_RESTORE BIEM_LGKM_WAIT
                       : [keep] "=&s"(m0_keep), BIEM_FRAG_OUTS, BIEM_C_OUTS1
                       : BIEM_FRAG_INS, BIEM_C_IN, BIEM_DMA_INS
                       : "memory", "scc");
          __builtin_amdgcn_sched_barrier(0);
          n_new = NDMA - NCD;
          advance();
        } else if (UPC == 2 && fused) {
          // the K = 64 form: two C units per chunk (slots mB + 8192 and mB + 12288)
          typedef __attribute__((address_space(3))) cplx* lds_cplx_t;
          cplx* S2 = ring + st2 * STG;
          const unsigned mA = (unsigned)(size_t)(lds_cplx_t)(S2 + wave * AST), mB = (unsigned)(size_t)(lds_cplx_t)(S2 + BOF + wave * 64);
          const int u0 = p_ch * 2, u1 = u0 + 1;
          const char* pC0 = BIEM_C_SRC(((long long)(4 * (u0 & 3)) * lda + (u0 >> 2) * 16) * (long long)sizeof(cplx));
          const char* pC1 = BIEM_C_SRC(((long long)(4 * (u1 & 3)) * lda + (u1 >> 2) * 16) * (long long)sizeof(cplx));
          asm volatile(BIEM_FRAG_READS16 BIEM_C_READ2 BIEM_M0_SAVE BIEM_OPERAND_DMA4 BIEM_C_DMA(8192, pC0) BIEM_C_DMA(12288, pC1)
                       BIEM_M0_RESTORE BIEM_LGKM_WAIT
                       : [keep] "=&s"(m0_keep), BIEM_FRAG_OUTS, BIEM_C_OUTS2
                       : BIEM_FRAG_INS, BIEM_C_IN, BIEM_DMA_INS, [oC] "v"(offC), [pC0] "s"(pC0), [pC1] "s"(pC1)
                       : "memory", "scc");
          __builtin_amdgcn_sched_barrier(0);
          n_new = NDMA;
          advance();
        } else if constexpr (UPC == 1) {
          asm volatile(BIEM_FRAG_READS16 BIEM_C_READ1 BIEM_LGKM_WAIT : BIEM_FRAG_OUTS, BIEM_C_OUTS1 : BIEM_FRAG_INS, BIEM_C_IN : "memory");
        } else {
          asm volatile(BIEM_FRAG_READS16 BIEM_C_READ2 BIEM_LGKM_WAIT : BIEM_FRAG_OUTS, BIEM_C_OUTS2 : BIEM_FRAG_INS, BIEM_C_IN : "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      BIEM_TR(4)
      // 3M operand sums and the C-slice additions BEFORE the MFMA block (measured: issued inside the block, in the shadow of
      // this wave's own MFMAs, the FP64 adds cost more - they share the FP64 pipe with the MFMAs and the C additions then
      // wait for accumulators in flight: 57.6 vs 63.1 TFLOP/s; only the integer address work below is free in there).
      double fbs[2][4], fas[2][4];
#pragma unroll
      for (int k4 = 0; k4 < 2; ++k4) {
#ifdef BIEM_ABL_NOSUMS
#pragma unroll
        for (int n = 0; n < 4; ++n) fbs[k4][n] = fb[k4][n].x;
#pragma unroll
        for (int g = 0; g < 4; ++g) fas[k4][g] = fa[k4][g].x;
#else
#pragma unroll
        for (int n = 0; n < NF; ++n) fbs[k4][n] = fb[k4][n].x + fb[k4][n].y;
#pragma unroll
        for (int g = 0; g < 4; ++g) fas[k4][g] = fa[k4][g].x + fa[k4][g].y;
#endif
      }
      // this chunk's C units (u = c*UPC + i -> column group u>>2, row quad u&3) join their accumulators.  Which
      // accumulator that is depends on c: a switch over c made hipcc merge all 32 accumulators through v_mov_b64 copies
      // behind the MFMA block (~1300 stalled cycles per chunk, found with tools/gemm_trace), an fma(value, sel_u, acc_u) over
      // all units cost 32 FP64 VALU instructions that compete with the MFMAs for the FP64 pipe.  A dynamically indexed
      // register array compiles to s_set_gpr_idx + v_mov (indirect VGPR addressing): 3 FP64 adds per unit.
#ifndef BIEM_ABL_NOCADD
      if (!PROD && (ALLC || c < NCC)) {
#pragma unroll
        for (int i = 0; i < UPC; ++i) {
          (&N1[0][0])[c * UPC + i] += cv[i].x;
          (&N3[0][0])[c * UPC + i] += cv[i].x + cv[i].y;
        }
      }
#endif
      // the MFMA block runs at low priority, everything else at high (the partner's SALU / LDS / VMEM phase slips between
      // this wave's MFMAs); the next chunk's fragment addresses are computed in its shadow
      mfma_fence();
      BIEM_PRIO_M();
      mfma_fence();
      BIEM_TR(5)
      {
        const int stn = st == 2 ? 0 : st + 1;
        const unsigned sbase = (unsigned)(size_t)(lds_cptr_t)(ring + stn * STG);     // wave-uniform
        aA = sbase + (unsigned)(fao * (int)sizeof(cplx));
        aB = sbase + (unsigned)(fbo * (int)sizeof(cplx));
        aC = sbase + (unsigned)((COF + tid) * (int)sizeof(cplx));
      }
#ifdef BIEM_ABL_NOMFMA     // timing ablation: data movement only
#pragma unroll
      for (int k4 = 0; k4 < 2; ++k4) {
#pragma unroll
        for (int n = 0; n < 4; ++n) asm volatile("" ::"v"(fb[k4][n].x), "v"(fb[k4][n].y), "v"(fbs[k4][n]));
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("" ::"v"(fa[k4][g].x), "v"(fa[k4][g].y), "v"(fas[k4][g]));
      }
#else
#pragma unroll
      for (int k4 = 0; k4 < 2; ++k4) {
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g) mfma_acc_neg(N1[n][g], fa[k4][g].x, fb[k4][n].x);
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g) mfma_acc(P2[n][g], fa[k4][g].y, fb[k4][n].y);
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g) mfma_acc_neg(N3[n][g], fas[k4][g], fbs[k4][n]);
      }
#endif
      mfma_fence();
      BIEM_PRIO_O();
      BIEM_TR(6)
      __builtin_amdgcn_sched_barrier(0);
      BIEM_TR(7)
      BIEM_TR_NEXT()
      st = st == 2 ? 0 : st + 1;
      if (c == 1) stores_pending = 0;
    }
    // tile finished: Cr' = N1 + P2, Ci' = N3 - N1 + P2; plain stores stay in flight while the next tile starts.
    // Full tiles address their 16 stores as (scalar tile origin + scalar unit offset) + the constant per-lane 32-bit offset
    // the C-slice DMA uses: no VALU address arithmetic (the generic form cost ~10 VALU instructions per store, three of them
    // integer multiplies, in the phase where the SIMD partner streams MFMAs: 10 % of the kernel, tools/gemm_trace ablation)
    cplx* Cs = A + (size_t)cs * sys_stride;
    const int row0 = tg.row_begin + cty * BM3, col0 = tg.col_begin + ctx * BN3;
    const bool full = row0 + BM3 <= n_pad && col0 + BN3 <= n_cols;
    if (full && tg.pout != nullptr && ctx == tg.pcol_tx) {
      // P[(16 n + l15)][row0 + 16 w + 4 g + l4]: 64-byte runs (4 rows) per lane quad; the 64-column panel tiles are always full
      cplx* Po = tg.pout + (size_t)cs * tg.pout_stride + (size_t)l15 * tg.pout_ld + (row0 + wave * 16 + l4);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const cplx v = make_double2(N1[n][g] + P2[n][g], N3[n][g] - N1[n][g] + P2[n][g]);
          Po[(size_t)(16 * n) * tg.pout_ld + 4 * g] = v;
          N1[n][g] = 0.0; P2[n][g] = 0.0; N3[n][g] = 0.0;
        }
      }
    } else if (full) {
      if constexpr (PROD) {
        // (only full tiles carry right-hand sides: launch_gemm_strip refuses Y with a partial tile column, so no tile of a launch
        // with Y takes the clamped branch below, which would skip its term)
        if (yr.Y != nullptr) {
          __shared__ cplx red[2][4][64];                   // [q & 1][wave][column]: one barrier per right-hand side
          // the tile's values take the accumulators' place (N1: real, N3: imaginary part); the stores below read them there
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const double re = N1[n][g] + P2[n][g], im = N3[n][g] - N1[n][g] + P2[n][g];
              N1[n][g] = re; N3[n][g] = im; P2[n][g] = 0.0;
            }
          cplx* Yq = yr.Y + (size_t)cs * yr.nrhs * yr.ld;
#pragma unroll 1
          for (int q = 0; q < yr.nrhs; ++q, Yq += yr.ld) {
            const cplx* zq = Yq + row0 + wave * 16 + l4;   // z_j of this lane's four rows 16 w + 4 g + (lane >> 4)
            cplx z[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) z[g] = zq[4 * g];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
              cplx a = make_double2(0.0, 0.0);
#pragma unroll
              for (int g = 0; g < 4; ++g) a = cfma(make_double2(N1[n][g], N3[n][g]), z[g], a);
              a.x += __shfl_xor(a.x, 16, 64); a.y += __shfl_xor(a.y, 16, 64);
              a.x += __shfl_xor(a.x, 32, 64); a.y += __shfl_xor(a.y, 32, 64);
              if (l4 == 0) red[q & 1][wave][16 * n + l15] = a;
            }
            __syncthreads();
            if (wave == 0) {
              const cplx r0 = red[q & 1][0][lane], r1 = red[q & 1][1][lane], r2 = red[q & 1][2][lane], r3 = red[q & 1][3][lane];
              cplx* yp = Yq + col0 + lane;
              cplx y = *yp;
              y.x -= (r0.x + r1.x) + (r2.x + r3.x);
              y.y -= (r0.y + r1.y) + (r2.y + r3.y);
              *yp = y;
            }
          }
          char* tb = (char*)(Cs + (size_t)row0 * lda + col0);
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const long long du = ((long long)(4 * g) * lda + n * 16) * (long long)sizeof(cplx);
              *(cplx*)(tb + du + offC) = make_double2(N1[n][g], N3[n][g]);
              N1[n][g] = 0.0; N3[n][g] = 0.0;
            }
          if (++c_tiles == p_tiles) break;
          stores_pending = 2;
          cs = p_s; cty = p_ty; ctx = p_tx;
          continue;
        }
      }
      char* tb = (char*)(Cs + (size_t)row0 * lda + col0);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const long long du = ((long long)(4 * g) * lda + n * 16) * (long long)sizeof(cplx);
#ifdef BIEM_ABL_NOEPI
          asm volatile("" ::"v"(N1[n][g]), "v"(P2[n][g]), "v"(N3[n][g]));   // keep the MFMAs alive
#elif defined(BIEM_ABL_ONESTORE)
          { const cplx v = make_double2(N1[n][g] + P2[n][g], N3[n][g] - N1[n][g] + P2[n][g]);
            if (n == 3 && g == 3) *(cplx*)(tb + du + offC) = v; else asm volatile("" ::"v"(v.x), "v"(v.y)); }
#elif defined(BIEM_ABL_NOSTORE)
          { const cplx v = make_double2(N1[n][g] + P2[n][g], N3[n][g] - N1[n][g] + P2[n][g]);
            asm volatile("" ::"v"(v.x), "v"(v.y)); }
#else
          const cplx v = make_double2(N1[n][g] + P2[n][g], N3[n][g] - N1[n][g] + P2[n][g]);
          *(cplx*)(tb + du + offC) = v;
#endif
          N1[n][g] = 0.0; P2[n][g] = 0.0; N3[n][g] = 0.0;
        }
      }
    } else {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = col0 + n * 16 + l15;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = row0 + wave * 16 + 4 * g + l4;
          const cplx v = make_double2(N1[n][g] + P2[n][g], N3[n][g] - N1[n][g] + P2[n][g]);
          if (col < n_cols && row < n_pad) Cs[(size_t)row * lda + col] = v;
          N1[n][g] = 0.0; P2[n][g] = 0.0; N3[n][g] = 0.0;
        }
      }
    }
    if (++c_tiles == p_tiles) break;                     // the producer started no further tile: done
    stores_pending = full ? 1 : 2;
    cs = p_s; cty = p_ty; ctx = p_tx;
  }
#ifdef BIEM_TR_STAMPS
  __syncthreads();
  if (blockIdx.x < 4) {     // 4 workgroups x 4 waves
    if (lane == 0) s_tr[wave * 512 + 7] = __builtin_amdgcn_s_getreg((16 - 1) << 11 | 0 << 6 | 4);     // HW_ID[15:0]
    __syncthreads();
    for (int i = tid; i < 4 * 64 * 8; i += 256) g_gemm_trace[blockIdx.x * 4 + (i >> 9)][(i >> 3) & 63][i & 7] = s_tr[i];
  }
#endif
}

template <int KD>
__global__ void __launch_bounds__(256, 2) k_gemm3m_pipe(cplx* __restrict__ A, long long lda, long long sys_stride,
                                                         const cplx* __restrict__ Pw, long long ldp, long long p_stride,
                                                         TileGrid tg) {
  gemm3m_body<KD, false>(A, lda, sys_stride, Pw, ldp, p_stride, tg, StripRhs{nullptr, 0, 0});
}
// the narrow K-long form: the last tile column of a left-looking band, column groups n < NF only (gemm3m_body; launch_gemm_left)
template <int NF>
__global__ void __launch_bounds__(256, 2) k_gemm3m_narrow(cplx* __restrict__ A, long long lda, long long sys_stride,
                                                           const cplx* __restrict__ Pw, long long ldp, long long p_stride,
                                                           TileGrid tg) {
  gemm3m_body<0, false, false, NF>(A, lda, sys_stride, Pw, ldp, p_stride, tg, StripRhs{nullptr, 0, 0});
}
// the strip pass of the symmetric factorisation, U12 = U11^{-T} C as the pure product -V^T C with V = -U11^{-T} (64 x 64 per system, K = 64)
__global__ void __launch_bounds__(256, 2) k_gemm3m_strip(cplx* __restrict__ A, long long lda, long long sys_stride,
                                                          const cplx* __restrict__ Pw, long long ldp, long long p_stride,
                                                          TileGrid tg, StripRhs yr) {
  gemm3m_body<64, true>(A, lda, sys_stride, Pw, ldp, p_stride, tg, yr);
}

// the stacked pass of panel p = J + 64 q (q = 1 .. 3) of a group that starts at row J: the pending updates of the group and the solve
// with the panel's diagonal block as ONE pure product over K = 64 (q + 1), -[S_J ; .. ; S_{p-64} ; V_p]^T A[J : p+64, tile column]
// (launch_gemm_stack); the tile is stored over the panel's own rows, epilogue and right-hand sides as in k_gemm3m_strip
template <int KD>
__global__ void __launch_bounds__(256, 2) k_gemm3m_stack(cplx* __restrict__ A, long long lda, long long sys_stride,
                                                          const cplx* __restrict__ Pw, long long ldp, long long p_stride,
                                                          TileGrid tg, StripRhs yr) {
  gemm3m_body<KD, true, true>(A, lda, sys_stride, Pw, ldp, p_stride, tg, yr);
}

void launch_tri_map(hipStream_t st, int* tri_map, int n_pad) {
  const int T = n_pad / NB, fb = T / 8, n_map = 32 * fb * fb + 4 * fb;
  if (n_map > 0) hipLaunchKernelGGL(k_tri_map, dim3((n_map + 255) / 256), dim3(256), 0, st, tri_map, n_map);
}

// What both launchers finish alike in a TileGrid: the tiles of all systems, the blocks the workgroups sweep them in and the division
// by per_sys.  Returns the size of the persistent grid, or 0 with the error set.
static int finish_tile_grid(TileGrid& tg, int per_sys, int nb) {
  tg.per_sys = per_sys; tg.ntiles = per_sys * nb;
  // Workgroups with the same blockIdx % 8 (one XCD) sweep blocks of 64 consecutive tiles together (shared operand panels in that
  // XCD's L2).  A small launch - one system, or the last groups of a factorisation - would leave most workgroups without a
  // tile that way (63 tiles: all in block 0, i.e. on the 8 workgroups of one label, 8 tiles each in sequence: 204 us for a
  // K = 192 tile row of one N = 4064 system): blocks of 8 tiles then.
  // Up to 512 tiles every tile has its own workgroup: tile = blockIdx (a block of ONE tile per label and round) - with blocks of 8 a
  // 33-tile launch (the strip of one system half-way through its factorisation) ran on the workgroups of 5 labels, several of them
  // taking two tiles in sequence while three quarters of the grid had none: 29.5 us per K = 64 strip launch instead of 13.
  tg.blk_sh = tg.ntiles <= GEMM_GRID_CAP ? 0 : tg.ntiles < 2048 ? 3 : 6;
  tg.per_sys_magic = ((1ULL << 40) + (unsigned long long)tg.per_sys - 1) / (unsigned long long)tg.per_sys;
  if (tg.ntiles >= (1 << 25)) { set_error("biem_lu: more than 2^25 tiles in one update launch"); return 0; }   // unreachable: 2^25 tiles are 2 TB of matrix
  const int want = (tg.ntiles + 7) / 8 * 8;          // one workgroup per tile up to the cap, multiple of 8
  return want < GEMM_GRID_CAP ? want : GEMM_GRID_CAP;   // persistent grid: 2 workgroups per CU
}

// C[row_begin:row_end, col_begin:col_end] -= P[0:kd]^T (rows of the region) * M[brow:brow+kd, cols of the region]
int launch_gemm_stream(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* Pw, long long ldp,
                       long long p_stride, int row_begin, int row_end, int col_begin, int col_end, int brow, int kd, int prof_class,
                       double prof_work, cplx* pout, long long pout_ld, long long pout_stride, int pcol_tx, const int* tri_map, bool upper) {
  const int tri = tri_map != nullptr ? (upper ? 2 : 1) : 0;
  const int rrows = row_end - row_begin, rcols = col_end - col_begin;
  if (rrows <= 0 || rcols <= 0) return BIEM_OK;
  TileGrid tg;
  tg.pout = pout; tg.pout_ld = pout_ld; tg.pout_stride = pout_stride; tg.pcol_tx = pcol_tx; tg.tri = tri;
  tg.ty_n = (rrows + BM3 - 1) / BM3; tg.tx_n = (rcols + BN3 - 1) / BN3;
  tg.full_bands = tg.ty_n / 8;
  tg.tri_map = tri_map; tg.tri_full = 32 * tg.full_bands * tg.full_bands + 4 * tg.full_bands;
  tg.row_begin = row_begin; tg.row_end = row_end; tg.col_begin = col_begin; tg.col_end = col_end; tg.brow = brow;
  const int grid = finish_tile_grid(tg, tri ? tg.ty_n * (tg.ty_n + 1) / 2 : tg.ty_n * tg.tx_n, nb);
  if (grid == 0) return BIEM_ERR_ARG;
  ProfScope ps(prof_class, st, prof_work >= 0.0 ? prof_work : 8.0 * (double)nb * (tri ? (double)tg.per_sys * BM3 * BN3 : rrows * (double)rcols) * kd);
  if (kd == 64)
    hipLaunchKernelGGL(k_gemm3m_pipe<64>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, Pw, ldp, p_stride, tg);
  else if (kd == 256)
    hipLaunchKernelGGL(k_gemm3m_pipe<256>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, Pw, ldp, p_stride, tg);
  else if (kd == 192)
    hipLaunchKernelGGL(k_gemm3m_pipe<192>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, Pw, ldp, p_stride, tg);
  else
    hipLaunchKernelGGL(k_gemm3m_pipe<128>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, Pw, ldp, p_stride, tg);
  return BIEM_OK;
}

// The strip of panel j of the symmetric factorisation: rows j .. j+63, columns j+64 .. col_end become -V^T times themselves (V: 64 x 64
// per system, addressed by absolute row like the panels: pass V - j) - the product kernel, C is neither read nor added.  With Y (compact
// right-hand sides Y[s][q][row], y_ld rows each, nrhs <= 8) every tile also takes its 64 columns' term of the forward substitution,
// Y[.., c] -= U[j : j+64, c]^T Y[.., j : j+64]; col_end is then a multiple of 64 past j (full tiles only).
int launch_gemm_strip(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* V, long long v_stride, int j, int col_end,
                      cplx* Y, int nrhs, int y_ld) {
  if (col_end <= j + NB) return BIEM_OK;
  if (Y != nullptr && ((col_end - j) % BN3 != 0 || nrhs < 1 || nrhs > 8)) { set_error("biem_sym: strip with right-hand sides over a partial tile column"); return BIEM_ERR_ARG; }
  TileGrid tg;
  tg.ty_n = 1; tg.tx_n = (col_end - j - NB + BN3 - 1) / BN3;
  tg.row_begin = j; tg.row_end = j + NB; tg.col_begin = j + NB; tg.col_end = col_end; tg.brow = j;
  const int grid = finish_tile_grid(tg, tg.tx_n, nb);
  if (grid == 0) return BIEM_ERR_ARG;
  ProfScope ps(PK_PANEL, st, 8.0 * (double)nb * (col_end - j - NB) * NB * NB);
  hipLaunchKernelGGL(k_gemm3m_strip, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, V, (long long)NB, v_stride, tg, StripRhs{Y, Y != nullptr ? nrhs : 0, y_ld});
  return BIEM_OK;
}

// The stacked pass of panel p (J < p <= J + 192, a multiple of 64 past J): rows p .. p+63, columns p+64 .. col_end become
//   -slab^T A[J : p+64, same columns],   slab = [S_J ; .. ; S_{p-64} ; V_p]  ((p - J + 64) x 64 per system, slab_stride apart)
// i.e. the B operand is the rows J .. p+63 of the matrix itself - the group's finished U rows, then the panel's own rows as the bulk
// update left them - and a tile overwrites rows that it alone reads at its columns.  Y as in launch_gemm_strip.
int launch_gemm_stack(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, const cplx* slab, long long slab_stride, int J, int p,
                      int col_end, cplx* Y, int nrhs, int y_ld) {
  if (col_end <= p + NB) return BIEM_OK;
  const int kd = p - J + NB;
  if (p <= J || (p - J) % NB != 0 || kd > 4 * NB) { set_error("biem_sym: stacked pass outside its group"); return BIEM_ERR_ARG; }
  if (Y != nullptr && ((col_end - p) % BN3 != 0 || nrhs < 1 || nrhs > 8)) { set_error("biem_sym: stacked pass with right-hand sides over a partial tile column"); return BIEM_ERR_ARG; }
  TileGrid tg;
  tg.ty_n = 1; tg.tx_n = (col_end - p - NB + BN3 - 1) / BN3;
  tg.row_begin = p; tg.row_end = p + NB; tg.col_begin = p + NB; tg.col_end = col_end; tg.brow = J;
  const int grid = finish_tile_grid(tg, tg.tx_n, nb);
  if (grid == 0) return BIEM_ERR_ARG;
  ProfScope ps(PK_PANEL, st, 8.0 * (double)nb * (col_end - p - NB) * NB * (double)kd);
  const StripRhs yr{Y, Y != nullptr ? nrhs : 0, y_ld};
  // (the A operand is addressed by absolute row like the panels: slab - p)
  if (kd == 128) hipLaunchKernelGGL(k_gemm3m_stack<128>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, slab - p, (long long)NB, slab_stride, tg, yr);
  else if (kd == 192) hipLaunchKernelGGL(k_gemm3m_stack<192>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, slab - p, (long long)NB, slab_stride, tg, yr);
  else hipLaunchKernelGGL(k_gemm3m_stack<256>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, slab - p, (long long)NB, slab_stride, tg, yr);
  return BIEM_OK;
}

// Left-looking update of the row form A = U^T U: the band of rows J .. row_end (up to four tile rows) takes every pending update
// of the finished rows 0 .. J-1 in one K-long pass,
//   A[J:row_end, J:col_end] -= U[0:J, J:row_end]^T U[0:J, J:col_end]      (tiles with tx >= ty only)
// Both operands are rows of the matrix itself (Pw = A, brow = 0, kd = J); every tile reads and writes its C once.
//
// nf < 4 (gemm_narrow_frags below): col_end is the end of the last matrix tile column, whose column groups nf .. 3 are identity padding.
// The launch then splits in two that write disjoint tiles and read finished rows only: the band without its last tile column
// (k_gemm3m_pipe<0>; nothing where that column is the whole band), and the last column's min(h, w) tiles per system, which multiply
// nf of their four column groups (k_gemm3m_narrow<nf>, one tile column starting at col_begin).  Both count in PK_GEMM; the narrow
// launch's work is that of its active column groups, so the class's flops stay executed flops.
static int launch_gemm_narrow_col(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, int J, int row_end, int col_end,
                                  int h_last, int nf);
int launch_gemm_left(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, int J, int row_end, int col_end, int nf) {
  if (J <= 0 || row_end <= J || col_end < row_end) return BIEM_OK;
  if (nf < 1 || nf > 4 || (nf < 4 && (col_end - J) % BN3 != 0)) { set_error("biem_sym: narrow bulk update over a partial tile column"); return BIEM_ERR_ARG; }
  TileGrid tg;
  tg.ty_n = (row_end - J) / BM3; tg.tx_n = (col_end - J + BN3 - 1) / BN3 - (nf < 4 ? 1 : 0);
  tg.row_begin = J; tg.row_end = row_end; tg.col_begin = J; tg.col_end = col_end - (nf < 4 ? BN3 : 0); tg.brow = 0;
  if (tg.tx_n > 0) {
    const int grid = finish_tile_grid(tg, band_tiles(tg.ty_n, tg.tx_n), nb);
    if (grid == 0) return BIEM_ERR_ARG;
    tg.nch = J / KC;                                  // (shares tri_full's word: set after the tile map's fields)
    ProfScope ps(PK_GEMM, st, 8.0 * (double)nb * (double)tg.per_sys * BM3 * BN3 * (double)J);
    hipLaunchKernelGGL(k_gemm3m_pipe<0>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, A, lda, sys_stride, tg);
  }
  if (nf == 4) return BIEM_OK;
  return launch_gemm_narrow_col(st, nb, A, lda, sys_stride, J, row_end, col_end, tg.ty_n < tg.tx_n + 1 ? tg.ty_n : tg.tx_n + 1, nf);
}
// the narrow launch: the tile rows 0 .. h_last-1 of the band at row J in the tile column that ends at col_end - tile row r of a system
// at tile column 0 of a region that starts at that column
static int launch_gemm_narrow_col(hipStream_t st, int nb, cplx* A, long long lda, long long sys_stride, int J, int row_end, int col_end,
                                  int h_last, int nf) {
  TileGrid tg;
  tg.ty_n = (row_end - J) / BM3; tg.tx_n = 1;
  tg.row_begin = J; tg.row_end = row_end; tg.col_begin = col_end - BN3; tg.col_end = col_end; tg.brow = 0;
  const int grid = finish_tile_grid(tg, h_last, nb);
  if (grid == 0) return BIEM_ERR_ARG;
  tg.nch = J / KC;
  ProfScope ps(PK_GEMM, st, 8.0 * (double)nb * (double)tg.per_sys * BM3 * 16.0 * nf * (double)J);
  if (nf == 1) hipLaunchKernelGGL(k_gemm3m_narrow<1>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, A, lda, sys_stride, tg);
  else if (nf == 2) hipLaunchKernelGGL(k_gemm3m_narrow<2>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, A, lda, sys_stride, tg);
  else hipLaunchKernelGGL(k_gemm3m_narrow<3>, dim3(grid), dim3(256), 0, st, A, lda, sys_stride, A, lda, sys_stride, tg);
  return BIEM_OK;
}

// Whether launch_gemm_left splits the last tile column off the band at row J of an n_pad system with n_active active rows and columns
// (the factorisation ending at column n_pad): the column groups of that tile column to multiply, NF = ceil((64 - padding) / 16), or 4
// where the launch stays whole - padding below 16 columns, or too few narrow tiles.  The narrow launch holds min(h, w) tiles per system
// (h = min(4, w) tile rows, w = T - J / 64 tile columns): below GEMM_GRID_CAP tiles a few K = J tiles would run on part of the chip
// while the rest of the band has finished, so the launch splits only from one tile per workgroup of the persistent grid - or where the
// last column is the whole band and nothing is split at all.  (512 is reasoned, not measured: DESIGN.md section 5.)
// mode: BIEM_GEMM_NARROW - 0 never, 1 without the size rule, anything else the rule.
int gemm_narrow_frags(int nb, int n_pad, int n_active, int J, int mode) {
  if (mode == 0 || J <= 0 || J >= n_pad || n_active > n_pad || n_active <= n_pad - BN3) return 4;
  const int nf = (BN3 - (n_pad - n_active) + 15) / 16;
  if (nf >= 4) return 4;
  const int w = (n_pad - J) / NB, h = w < 4 ? w : 4;      // (h <= w: the narrow launch has h tiles per system)
  const bool whole_band = w == 1;
  if (mode != 1 && !whole_band && (long long)h * nb < GEMM_GRID_CAP) return 4;
  return nf;
}

// Which form of the bulk update launch_sym_factor_solve runs by default (sym_form, kernels_sym.hip: SymForm.left): left-looking
// (launch_gemm_left before every group) or right-looking (the K = 256 update after every group).  Left-looking tiles of late groups are
// long and few: a launch with fewer tiles than the chip has CUs leaves CUs idle for a whole K = J tile, where the right-looking form
// spreads the same work over every tile below the group.  So the left form runs when even the SMALLEST of its launches - the last
// group's band - has a tile for every CU, i.e. half the persistent grid of two workgroups per CU (one workgroup per CU runs at 75-80 %
// of the two-workgroup rate).  Measured at N = 6400: 8 systems per call (80 tiles) right by 4 %, 32 systems
// (320 tiles) left by 3 %, more systems left by 3-6 %.
bool gemm_left_fills_grid(int nb, int n_pad, int nrhs) {
  const int T = n_pad / NB, h_last = T % 4 ? T % 4 : 4;
  const int cols_last = h_last + (nrhs > 8 ? (nrhs + BN3 - 1) / BN3 : 0);
  const long long smallest = (long long)band_tiles(h_last, cols_last) * nb;
  return 2 * smallest >= GEMM_GRID_CAP;
}

// ---------------------------------------------------------------------------------------------
// microbenchmark: issue rate of v_mfma_f64_16x16x4_f64 (confirms the FP64 matrix peak the roofline is priced against)
// ---------------------------------------------------------------------------------------------
// V = 0: v_mfma_f64_16x16x4_f64 (2048 flops, 32 cycles);  V = 1: v_mfma_f64_4x4x4_4b_f64, the instruction of k_gemm3m_pipe (512 flops,
// 16 cycles).  Both price at 32 flops per cycle and SIMD.
template <int V>
__global__ void __launch_bounds__(256) k_bench_mfma(int iters, double* sink) {
  v4d acc[8];
  double acc1[16];
  for (int i = 0; i < 8; ++i) acc[i] = (v4d){0, 0, 0, 0};
  for (int i = 0; i < 16; ++i) acc1[i] = 0.0;
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  for (int it = 0; it < iters; ++it) {
    if (V == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc1[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc1[i], 0, 0, 0);
    }
  }
  double sacc = 0.0;
  for (int i = 0; i < 8; ++i) sacc += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  for (int i = 0; i < 16; ++i) sacc += acc1[i];
  if (sacc == 123.456) sink[0] = sacc;
}

int bench_mfma_f64(int iters, double* tflops, hipStream_t st, int variant) {
  double* sink = nullptr;
  BIEM_HIPCHK(hipMalloc((void**)&sink, 16));
  hipEvent_t e0, e1;
  BIEM_HIPCHK(hipEventCreate(&e0));
  BIEM_HIPCHK(hipEventCreate(&e1));
  const int blocks = 256 * 2;   // 2 workgroups of 4 waves per CU -> 2 waves per SIMD
  auto launch = [&](int n) {
    if (variant == 1) hipLaunchKernelGGL(k_bench_mfma<1>, dim3(blocks), dim3(256), 0, st, n, sink);
    else hipLaunchKernelGGL(k_bench_mfma<0>, dim3(blocks), dim3(256), 0, st, n, sink);
  };
  launch(16);   // warm-up
  BIEM_HIPCHK(hipEventRecord(e0, st));
  launch(iters);
  BIEM_HIPCHK(hipEventRecord(e1, st));
  BIEM_HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  BIEM_HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  const double per_iter = variant == 1 ? 16.0 * (2.0 * 4 * 4 * 4 * 4) : 8.0 * (2.0 * 16 * 16 * 4);
  double flops = (double)blocks * 4.0 * (double)iters * per_iter;
  *tflops = flops / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(sink);
  return BIEM_OK;
}

#ifdef BIEM_GEMM_TRACE
__global__ void k_trace_fill(double* p, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = 1e-3 * (double)((i * 2654435761ull >> 7) & 1023) / 1024.0 - 5e-4;
}
// one trailing update of an (n x n, K = kd) region of nb systems on synthetic data; returns the stamps and the launch time
extern "C" int biem_debug_gemm(int nb, int n, int kd, int reps, unsigned long long* trace_out, float* ms_out) {
  const long long lda = n + 8, ldp = n + 256;   // the panel workspace is indexed by absolute row
  cplx *A = nullptr, *P = nullptr;
  const size_t na = (size_t)nb * (n + 256) * lda, np = (size_t)nb * 256 * ldp;
  if (hipMalloc((void**)&A, na * sizeof(cplx)) != hipSuccess) return 1;
  if (hipMalloc((void**)&P, np * sizeof(cplx)) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)A, na * 2);
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)P, np * 2);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  launch_gemm_stream(0, nb, A, lda, (long long)(n + 256) * lda, P, ldp, 256 * ldp, 256, 256 + n, 0, n, 0, kd);
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  for (int r = 0; r < reps; ++r)
    launch_gemm_stream(0, nb, A, lda, (long long)(n + 256) * lda, P, ldp, 256 * ldp, 256, 256 + n, 0, n, 0, kd);
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_out = ms / reps;
  hipMemcpyFromSymbol(trace_out, HIP_SYMBOL(g_gemm_trace), sizeof(unsigned long long) * 16 * 64 * 8);
  hipFree(A); hipFree(P);
  return 0;
}
// the K-long launch of the left-looking update alone: a band of four tile rows J = kd .. kd + 256 over n columns right of J
extern "C" int biem_debug_gemm_left(int nb, int n, int kd, int reps, float* ms_out, int* tiles_out) {
  const long long lda = kd + n + 8, rows = kd + 256;
  cplx* A = nullptr;
  const size_t na = (size_t)nb * rows * lda;
  if (hipMalloc((void**)&A, na * sizeof(cplx)) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)A, na * 2);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  launch_gemm_left(0, nb, A, lda, rows * lda, kd, kd + 256, kd + n);
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  for (int r = 0; r < reps; ++r) launch_gemm_left(0, nb, A, lda, rows * lda, kd, kd + 256, kd + n);
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_out = ms / reps;
  *tiles_out = nb * band_tiles(4, n / 64);
  hipFree(A);
  return hipGetLastError() != hipSuccess;
}
// the narrow launch alone: the four tiles per system of the last tile column of a four-row band at J = kd (k_gemm3m_narrow<nf>); nf = 4:
// four full K-long tiles per system for comparison (k_gemm3m_pipe<0> on a one-row band of four tile columns).  Either way nb * 4
// tiles of K = kd; up to 128 systems every tile has a workgroup of its own, from 64 systems every CU holds two
extern "C" int biem_debug_gemm_narrow(int nb, int kd, int nf, int reps, float* ms_out, int* tiles_out) {
  const long long lda = kd + 256 + 8, rows = kd + 256;
  cplx* A = nullptr;
  const size_t na = (size_t)nb * rows * lda;
  if (nf < 1 || nf > 4 || kd < 128 || kd % 8 || hipMalloc((void**)&A, na * sizeof(cplx)) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)A, na * 2);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  auto launch = [&]() {
    return nf == 4 ? launch_gemm_left(0, nb, A, lda, rows * lda, kd, kd + 64, kd + 256)
                   : launch_gemm_narrow_col(0, nb, A, lda, rows * lda, kd, kd + 256, kd + 256, 4, nf);
  };
  int rc = launch();
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  for (int r = 0; r < reps && rc == 0; ++r) rc = launch();
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_out = ms / reps;
  *tiles_out = nb * 4;
  hipFree(A);
  return rc != 0 || hipGetLastError() != hipSuccess;
}
// one small update launch, as a single system sees it: C[r0 : r0 + rows, 0 : n] -= P^T M[brow ..], `reps` launches back to back; cold = 1:
// every launch takes another row strip (the matrix is far larger than the caches), cold = 0: the same one
extern "C" int biem_debug_gemm_strip(int n, int kd, int rows, int reps, int cold, float* us_out, int extra_cols, int col0) {
  const long long lda = n + 8, ldp = n + 256;
  cplx *A = nullptr, *P = nullptr;
  const size_t na = (size_t)(n + 256) * lda, np = (size_t)256 * ldp;
  if (hipMalloc((void**)&A, na * sizeof(cplx)) != hipSuccess) return 1;
  if (hipMalloc((void**)&P, np * sizeof(cplx)) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)A, na * 2);
  hipLaunchKernelGGL(k_trace_fill, dim3(2048), dim3(256), 0, 0, (double*)P, np * 2);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const int nstrips = (n - rows) / 64;
  for (int r = 0; r < 3; ++r) launch_gemm_stream(0, 1, A, lda, 0, P, ldp, 0, 256, 256 + rows, col0, n + extra_cols, 0, kd);
  hipDeviceSynchronize();
  hipEventRecord(e0, 0);
  for (int r = 0; r < reps; ++r) {
    const int r0 = 256 + (cold ? 64 * ((r * 7) % nstrips) : 0);
    launch_gemm_stream(0, 1, A, lda, 0, P, ldp, 0, r0, r0 + rows, col0, n + extra_cols, cold ? r0 : 0, kd);
  }
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float ms = 0; hipEventElapsedTime(&ms, e0, e1); *us_out = ms * 1e3f / reps;
  hipFree(A); hipFree(P);
  return 0;
}
#endif

}  // namespace biem
