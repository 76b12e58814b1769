// plan_build.hpp -- private to the units that build a plan: plan_tree.cpp (what depends on the coordinate tree: labels, units, boundary-data
// quadrature, projection matrix, term lists; the chain trees), plan_fill.cpp (the fill's tables behind the labels and term lists, the same
// for every tree) and plan.cpp (device mirrors, force coupling table, error text).
#pragma once
#include "plan.hpp"
#include "../../include/biem_mi355.h"

namespace biem {

static inline int iabs(int v) { return v < 0 ? -v : v; }

#pragma GCC visibility push(hidden)   // between the units of one library: none of these is exported
// ---- plan_tree.cpp: the two rules every tree-dependent decision of the fill tables goes through
// conj Y_h = Y_p with the orders of all type-a nodes negated (every tree built here has real non-azimuthal factors and no sign:
// tests/test_oracle_golden.py::test_translation_block_matrix_is_complex_symmetric...): the label of p from the label of h, in place
void conjugate_label(int tree, int lw, int* label);
// the azimuthal orders of a label (m2: the second type-a node of caa, 0 elsewhere)
void azimuthal_orders(int tree, int lw, const int* label, int& m1, int& m2);
// partner[l] = index of the conjugate of label l among `count` labels of width lw; false at the first label without one (-1 from there on)
bool conjugate_partners(int tree, int lw, const std::vector<int>& labels, int count, std::vector<int>& partner);
// ---- plan_fill.cpp: every table from tidx16 on (plan.hpp), from tree, lw, n_end, H, H2, labels2, units, lists_built, ptr, coef, tidx
int plan_build_fill_tables(biem_plan* p);
#pragma GCC visibility pop

}  // namespace biem
