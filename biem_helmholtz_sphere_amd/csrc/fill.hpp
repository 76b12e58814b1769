// fill.hpp -- private to the units of the matrix fill: kernels_tables.hip (radial, harmonic, ball and pair tables, pair classes),
// kernels_fill.hip (the general fill, the form decision and the workspace size) and kernels_fill_sym.hip (the symmetric fill in its four
// forms); kernels_rhs.hip (right-hand sides, density) needs nothing from the others.  The small types the units pass to each other and the
// host functions through which a unit reaches another unit's kernels - a kernel is launched only by the unit that defines it.
#pragma once
#include "common.hpp"
#include <cstdlib>

namespace biem {

// the form launch_fill_sym takes for B > 1 balls: the list-free 2-D kernel, systems in lanes, one unit pair per lane with the reduced
// table (RED) or the gather form it replaced (ENTRY); UNFIT: BIEM_FILL_FORM asks for a lane form whose tables do not fit LDS.
// shm: dynamic LDS of the form's kernel; sys_workspace: fill_workspace_bytes has to cover the systems-in-lanes layout
struct FillSymForm {
  enum Kind { DIRECT2D, SYS, RED, ENTRY, UNFIT } kind;
  size_t shm;
  bool sys_workspace;
};

// the four layouts of a pair table T: [s][b][b'][H2]; systems in lanes Tt[group of 64 systems][pair][l][system] (nb rounded up to 64);
// conjugate partners adjacent, [s][b][b'][H2lin] (plan's lin2); reduced rows T' | phases | q factors of E + NP + 2 n_end
enum PairTableMode { PT_PLAIN, PT_SYS_LANES, PT_PAIRED, PT_REDUCED };

// Pair classes of the symmetric fill (k_pair_dedupe), the last fill_dedupe_bytes of the fill workspace:
//   nrep (+3 pad), rep_list[np], dup_ptr[np + 1], dup_bb[np], rep_flag[B * B]         (np = B (B - 1) / 2 upper pairs)
// rep_flag: 1 where the pair (b, bp) is the first of its class - only those pairs' tables are read by the fill
inline size_t fill_dedupe_bytes(int B) { const size_t np = (size_t)B * (B - 1) / 2; return ((3 * np + 5 + (size_t)B * B) * sizeof(int) + 15) / 16 * 16; }
struct PairClasses { int* classes; const int* rep_flag; };
inline PairClasses pair_classes_at(void* block, int B) { int* c = (int*)block; return {c, c + 4 + 3 * (B * (B - 1) / 2) + 1}; }

constexpr int NB_TILE = 64;             // the factorisation's tile: diagonal 64 x 64 tiles are read whole

// the list forms of both fills (every form but the list-free 2-D kernels) stop at half the built table order
inline bool fill_lists_order_ok(const biem_plan* p) { return 2 * p->n_end <= kMaxRad; }

// the operands of one symmetric fill its forms share (T: pair tables at the front of the workspace, pc: the class block at its end)
struct SymFill {
  const biem_plan* p; int nb, B; const double *d_k, *d_centers; int geom_batched; const double* d_tab;
  cplx* A; long long lda, sys_stride; cplx* T; PairClasses pc; const FillDedupe* dedupe; hipStream_t st;
};

#pragma GCC visibility push(hidden)   // between the units of one library: none of these is exported
// ---- kernels_tables.hip
// pair tables of the upper pairs b < bp in the layout `mode` (d_tab: the ball tables, read by PT_REDUCED only); with rep_flag only
// of the pairs it marks.  No launch for B <= 1
int launch_pair_tables(const biem_plan* p, int nb, int B, const double* d_k, const double* d_centers, int geom_batched, const double* d_tab,
                       PairTableMode mode, const int* rep_flag, cplx* T, hipStream_t st);
// classes of the B (B - 1) / 2 upper pairs into pc (on: by displacement, radius, alpha, beta; off: every pair its own class)
int launch_pair_classes(const biem_plan* p, int nb, int B, const double* d_centers, int geom_batched, const FillDedupe* dedupe,
                        const PairClasses& pc, hipStream_t st);
// both for a symmetric fill: the classes, then the pair tables of the class heads only (the fill reads no others; the serial radial
// recurrence of a pair's table is the expensive part of a 2-D fill)
int launch_classes_and_tables(const SymFill& c, PairTableMode mode);
// ---- kernels_fill.hip
int launch_fill2d_sym(const SymFill& c);          // launch_fill_sym's form DIRECT2D
FillSymForm fill_sym_form(const biem_plan* p);    // (DIRECT2D: launch_fill runs its list-free 2-D kernel as well)
bool plan_2d_direct(const biem_plan* p);      // the list-free 2-D kernels index the table row directly: the plan's table order allows it
#pragma GCC visibility pop

}  // namespace biem
