// plan.hpp -- host + device tables of one (tree, n_end): labels, boundary-data quadrature, projection
// matrix and the translation terms of the closed form.  All k- and geometry-independent.
#pragma once
#include <vector>
#include <cstdint>
#include "special.hpp"

constexpr int kChainNodeTab = 4096;        // doubles of node-factor tables the chain kernels keep in LDS
constexpr int kLists2dMax = 160;            // 2-D plans up to this order also carry term lists (tests, the generic fill forms)

// The table list: every std::vector of a plan once, as DEV(type, name) - it has the device mirror d_<name> - or HOST(type, name).
// The mirrors' declarations, plan_upload, plan_free and the digests of tools/plan_digest.cpp are generated from it, so a table
// cannot be uploaded and not freed, or built and not compared.  (tidx: the fills read tidx16, biem_plan_terms the host vector.)
#define BIEM_PLAN_TABLES(DEV, HOST) \
  DEV(int, labels) DEV(int, deg) DEV(int, labels2) DEV(int, deg2) DEV(int, units) HOST(double, qy) HOST(double, qw) DEV(double, W) \
  DEV(uint32_t, ptr) DEV(double, coef) HOST(int32_t, tidx) DEV(uint16_t, tidx16) DEV(int, chunk_ent) \
  DEV(int, spos) DEV(int, hpos) DEV(uint32_t, qptr) DEV(double, qcoef) DEV(uint16_t, qidx16) \
  DEV(int, lin2) DEV(uint32_t, q2ptr) DEV(double, q2coef) DEV(uint16_t, q2idx16) DEV(int, qchunk) \
  DEV(int, red_of) DEV(int, red_first) HOST(int, red_label) DEV(int, ph_mu) HOST(int, ph_of_unit) \
  DEV(double, rcoef) DEV(uint16_t, ridx) DEV(uint16_t, rphsel) DEV(int, rchunk) DEV(int, rcrow) DEV(int, rwrow) DEV(int, schunk)
// the force tables in a list of their own: plan_build_force builds and uploads them on the first request, not with the plan
#define BIEM_PLAN_FORCE_TABLES(DEV, HOST) \
  HOST(uint32_t, fptr) DEV(int32_t, fcol) HOST(int32_t, fcomp) DEV(double, fval) DEV(uint32_t, fptr_comp)

struct biem_plan {
  int tree = 0, d = 0, n_end = 0, n2 = 0;   // n2 = 2 n_end - 1 (degrees of the translation table)
  int H = 0, H2 = 0, Q = 0;
  double Cd = 0.0;                          // (2 pi)^{d/2} sqrt(2/pi)
  // host tables
  int lw = 3;                               // label width: 3 (a, ba, bba, caa), d - 1 (chain trees)
  std::vector<int> labels, deg;             // [H][lw], [H]
  std::vector<int> labels2, deg2;           // [H2][lw], [H2]
  std::vector<int> units;                   // [U][2]: harmonics (h, p) with conj Y_h = Y_p, h <= p (h == p: real harmonic)
  std::vector<double> qy, qw;               // [Q][d], [Q]
  std::vector<double> W;                    // [Q][H] complex128 interleaved
  std::vector<uint32_t> ptr;                // [H*H + 1]
  std::vector<double> coef;                 // [terms]
  std::vector<int32_t> tidx;                // [terms]
  std::vector<uint16_t> tidx16;             // same, 16-bit copy the fill kernel keeps in LDS
  std::vector<int> chunk_ent;               // fill chunks: entries e = h*H + h' in [chunk_ent[c], chunk_ent[c+1]); sized to the LDS budget
  int chunk_terms_max = 0;                  // largest number of terms in one chunk
  int chunk_ents_max = 0;                   // largest number of entries in one chunk
  bool lists_built = true;                  // false: 2-D beyond kLists2dMax - no term lists (ptr / coef / q* / r* are empty), only the 2-D fills run
  bool fill_table_global = false;           // general fill: the pair table stays in global memory (it does not fit LDS beside the term slice)
  // the symmetric (real-harmonic) fill: unit pairs (u, u') in row-major order, four term lists ("slots") per pair for the entries
  // (h,h'), (h,p'), (p,h'), (p,p') of the units (h,p), (h',p') - empty where h == p or h' == p' - so one thread forms a whole
  // 2 x 2 block of R W^H M W R^-1.  Internal order of the unknowns of a ball in that path: the U "cosine" combinations first
  // (slot u), then the "sine" combinations of the units with h != p (slot U + spos[u]); hpos[h] = slot holding harmonic h before
  // the transform (h -> u, p -> U + spos[u]).
  std::vector<int> spos, hpos;              // [U], [H]
  std::vector<uint32_t> qptr;               // [4 U U + 1]
  std::vector<double> qcoef;
  std::vector<uint16_t> qidx16;
  // entry-per-lane form: conjugation pairs the lists - (p,p') has the coefficients of (h,h') with every table index replaced by
  // its conjugate partner's, (p,h') those of (h,p') - so a unit pair carries TWO lists (A: (h,h'), B: (h,p'), B only when both units
  // are doubles) and the pair table is stored with partners adjacent: lin2[l] = 2e for the first member of unit e of the degree
  // < 2 n_end - 1 labels, 2e + 1 for its partner (a self-conjugate label fills both), so the partner's entry is index ^ 1.
  std::vector<int> lin2;                    // [H2]
  int H2lin = 0;                            // 2 * (number of units among the H2 labels)
  bool pair_lists_ok = false;               // the pairing was verified on every unit pair of this plan
  std::vector<uint32_t> q2ptr;              // [2 U U + 1]
  std::vector<double> q2coef;
  std::vector<uint16_t> q2idx16;            // indices into the paired table layout
  std::vector<int> qchunk;                  // chunks of unit pairs: [qchunk[c], qchunk[c+1]), at most FILL_SYM_THREADS pairs each
  int qchunk_terms_max = 0, qchunk_pairs_max = 0;
  // ---- reduced-table form of the entry-per-lane symmetric fill (k_fill_sym) ----
  // Every term of one entry (h, h') carries the same azimuthal order vector mu = m' - m, so T[l] = T'[e(l)] * e^{+-i mu.phi} with the
  // REAL-angular-factor table T'[e] = C_d h_{n''}(k|t|) |Y_l|-amplitude shared by a label and its conjugate partner (e = unit of
  // the label among the degree < 2 n_end - 1 labels) and the phase leaves the sum:  S(h,h') = phase * sum_p coef[p] T'[e[p]],  and
  // the conjugate entry (p,p') is conj(phase) times the SAME sum.  One chain per list instead of two, half the table.
  // Table row of a (pair, system): T'[0 .. E) then the NP phases e^{i mu_id . phi} of the distinct azimuthal vectors of first members.
  int E = 0, NP = 0;                        // E = H2lin / 2 label units, NP phase ids
  std::vector<int> red_of;                  // [H2] unit e of label l
  std::vector<int> red_first;               // [H2] 1: l is the first member of its unit (or self-conjugate), 0: the partner
  std::vector<int> red_label;               // [E] the first member's label index
  std::vector<int> ph_mu;                   // [NP][2] azimuthal orders of phase id (second entry: caa only)
  std::vector<int> ph_of_unit;              // [E] phase id of the unit's first member
  // term lists per wave of 64 consecutive unit pairs, TRANSPOSED and padded to the wave's longest list: row r holds term number
  // (r - start) of the 64 lanes (coefficient 0, index 0 where a lane's list has run out), so the per-step reads of a wave are
  // contiguous (no LDS bank conflicts).  Lists are padded to multiples of 4 rows; the indices of a group of 4 rows are packed per
  // lane (ridx[(group * 64 + lane) * 4 + k]: one 8-byte read per lane and group).  Chunk c = unit pairs [rchunk[c], rchunk[c+1]) (at most 1024 = 16 waves), its rows
  // [rcrow[c], rcrow[c+1]); rwrow[c * 33 + 2 w + {0, 1, 2}] = first row of wave w's list A, of its list B, end (relative to the chunk).
  bool red_lists_ok = false;
  int red_waves = 16, red_nc = 2;           // workgroup of k_fill_red (waves) and combinations per iteration the chunks were cut for (experiments: BIEM_FILL_RED_WAVES=8, BIEM_FILL_NC=1 at plan build)
  std::vector<double> rcoef;                // [rows][64]
  std::vector<uint16_t> ridx;               // [rows][64] indices e into T'
  std::vector<uint16_t> rphsel;             // [U U][2]: phase selector of list A, of list B: 2 * phase id + (1: conjugate phase)
  std::vector<int> rchunk, rcrow, rwrow;
  int rchunk_rows_max = 0;
  double red_gather_cycles = 0.0;           // LDS cycles per row and ds_read_b128 lane group of the table gather (1 = conflict-free)
  // the same lists cut into small chunks for the systems-in-lanes form of the symmetric fill (k_fill_sys: no LDS ceiling on H2)
  std::vector<int> schunk;
  int schunk_terms_max = 0, schunk_pairs_max = 0;
  // ---- coupling table of the radiation force (kernels_force.hip), built on the first request (plan_build_force) ----
  // T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega, i = 0 .. d-1 along the plan's axes: Hermitian in (h', h), nonzero only for |n - n'| = 1.
  // CSR over the rows h'; the entries of a row are ordered by (component, column).
  bool force_built = false, force_uploaded = false;
  std::vector<uint32_t> fptr;               // [H + 1]
  std::vector<int32_t> fcol, fcomp;         // [entries] column h, component i
  std::vector<double> fval;                 // [entries] complex128 interleaved
  std::vector<uint32_t> fptr_comp;          // [H * d + 1]: the entries of (row h', component i) are [fptr_comp[h' d + i], fptr_comp[h' d + i + 1])
  // device mirrors d_<table> of the table lists above (null until uploaded)
  int device = -1;
#define BIEM_PLAN_MIRROR(T, name) T* d_##name = nullptr;
#define BIEM_PLAN_HOST_ONLY(T, name)
  BIEM_PLAN_TABLES(BIEM_PLAN_MIRROR, BIEM_PLAN_HOST_ONLY)
  BIEM_PLAN_FORCE_TABLES(BIEM_PLAN_MIRROR, BIEM_PLAN_HOST_ONLY)
#undef BIEM_PLAN_MIRROR
#undef BIEM_PLAN_HOST_ONLY
};

namespace biem {
int plan_build_host(biem_plan* p, int tree, int n_end);   // returns BIEM_* status
// the translation terms of entry (row h, column h') of bba / caa at order n_end, by the code the plan build runs, without a plan
int plan_entry_terms(int tree, int n_end, int hp, int h, std::vector<double>& coef, std::vector<int>& tidx);
int plan_build_chain_host(biem_plan* p, int d, int n_end);  // the standard chain tree "b" * (d - 2) + "a", 3 <= d <= kChainDimMax
int plan_upload(biem_plan* p);
int plan_build_force(biem_plan* p);         // the force coupling table, and its device mirror if the plan is uploaded; a no-op once built
void plan_free(biem_plan* p);
void set_error(const char* fmt, ...);
}  // namespace biem
