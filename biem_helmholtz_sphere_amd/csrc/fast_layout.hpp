// fast_layout.hpp -- the LDS layout of the per-lane field kernels (kernels_uscat.hip, kernels_uinterior.hip).
#pragma once
#include "common.hpp"

// The LDS layout, the recurrence tables and the staging of a ball's coefficients of the per-lane kernels.  k_uscat_fast and the gradient
// kernel k_uscat_grad_fast share them as ONE text expanded in both (macros, not device functions: the compiler contracts multiply-adds
// after inlining, and a value kernel built from inlined helpers differed from its predecessor in the last bit of some results; the
// expansion is token for token the text the value kernel had, so its code object does not change).
// They expect n_end, H, labels, tid, T and (staging) cs in scope and define ra, rb, cmm, ga, gia, g0, jA, jB, jC, jN, sC, K2, ncaa, ms, nC.
#define BIEM_FAST_LAYOUT() \
  extern __shared__ double sfast[]; \
  /* 3-D: ra[q * n_end + m], rb[q * n_end + m] (q > m), cm[m]; then the ball's coefficients sC[pos] */ \
  constexpr bool LEG = TREE == TREE_BA || TREE == TREE_BBA;   /* a Legendre factor Pbar_l^m */ \
  double* ra = sfast; \
  double* rb = ra + (LEG ? n_end * n_end : 0); \
  double* cmm = rb + (LEG ? n_end * n_end : 0); \
  double* ga = cmm + (LEG ? ((n_end + 1) & ~1) : 0);   /* bba: Gegenbauer a_q of order lam = l + 1 at [l * n_end + q] */ \
  double* gia = ga + (TREE == TREE_BBA ? n_end * n_end : 0);   /*      1 / a_q */ \
  double* g0 = gia + (TREE == TREE_BBA ? n_end * n_end : 0);   /*      p_0 = 1 / sqrt(h_0(l)) */ \
  /* caa: the Jacobi recurrence p_{m+1} = (jA x + jB) p_m - jC p_{m-1} of cbar_single and its norm, at [(a * n_end + b) * K2 + m] */ \
  const int K2 = (n_end + 1) / 2, ncaa = TREE == TREE_CAA ? n_end * n_end * K2 : 0; \
  double* jA = g0 + (TREE == TREE_BBA ? ((n_end + 1) & ~1) : 0); \
  double* jB = jA + ncaa; \
  double* jC = jB + ncaa; \
  double* jN = jC + ncaa; \
  cplx* sC = (cplx*)(jN + ncaa); \
  const int ms = 2 * n_end - 1; \
  const int nC = TREE == TREE_BA ? n_end * n_end : TREE == TREE_BBA ? n_end * n_end * ms : TREE == TREE_CAA ? n_end * ms * ms : ms;
#define BIEM_FAST_TABLES() \
  if (LEG) { \
    for (int e = tid; e < n_end * n_end; e += T) { \
      const int q = e / n_end, m = e - q * n_end; \
      double a = 0.0, b = 0.0; \
      if (q > m) { \
        a = sqrt((double)(4 * q * q - 1) / (double)(q * q - m * m)); \
        b = sqrt((double)((q - 1) * (q - 1) - m * m) / (double)(4 * (q - 1) * (q - 1) - 1)); \
      } \
      ra[e] = a; rb[e] = b; \
    } \
    for (int m = tid; m < n_end; m += T) cmm[m] = m == 0 ? 0.0 : sqrt((double)(2 * m + 1) / (double)(2 * m)); \
  } \
  if (TREE == TREE_CAA) { \
    for (int e = tid; e < ncaa; e += T) { \
      const int a = e / (n_end * K2), b = (e / K2) % n_end, m = e % K2; \
      const double al = (double)b, be = (double)a;   /* Jacobi P^{(alpha = b, beta = a)} */ \
      double A, Bc, C; \
      if (m == 0) { A = 0.5 * (al + be + 2.0); Bc = (al + 1.0) - A; C = 0.0; } \
      else { \
        const double t = 2.0 * m + al + be, den = 2.0 * (m + 1.0) * (m + al + be + 1.0) * t; \
        A = (t + 1.0) * (t + 2.0) * t / den; Bc = (t + 1.0) * (al * al - be * be) / den; C = 2.0 * (m + al) * (m + be) * (t + 2.0) / den; \
      } \
      double nr = 2.0 * (2.0 * m + a + b + 1.0); \
      for (int i = 1; i <= a; ++i) nr *= (double)(m + b + i) / (double)(m + i); \
      jA[e] = A; jB[e] = Bc; jC[e] = C; jN[e] = sqrt(nr); \
    } \
  } \
  if (TREE == TREE_BBA) {   /* the coefficients of gbar_single */ \
    for (int e = tid; e < n_end * n_end; e += T) { \
      const int l = e / n_end, q = e - l * n_end; \
      const double lam = (double)(l + 1); \
      const double aq = q == 0 ? 1.0 : 0.5 * sqrt((double)q * ((double)q + 2.0 * lam - 1.0) / (((double)q + lam - 1.0) * ((double)q + lam))); \
      ga[e] = q == 0 ? 0.0 : aq; gia[e] = 1.0 / aq; \
    } \
    for (int l = tid; l < n_end; l += T) { \
      double h0 = 0.5 * kPi; \
      for (int i = 1; i <= l; ++i) h0 *= ((double)i + 0.5) / ((double)i + 1.0); \
      g0[l] = 1.0 / sqrt(h0); \
    } \
  }
#define BIEM_FAST_STAGE() \
  for (int h = tid; h < H; h += T) { \
    int pos; \
    if (TREE == TREE_BA) { const int n = labels[3 * h], m = labels[3 * h + 1]; pos = n * n + n + m; } \
    else if (TREE == TREE_BBA) pos = (labels[3 * h] * n_end + labels[3 * h + 1]) * (2 * n_end - 1) + labels[3 * h + 2] + n_end - 1; \
    else if (TREE == TREE_CAA) pos = (labels[3 * h] * ms + labels[3 * h + 1] + n_end - 1) * ms + labels[3 * h + 2] + n_end - 1; \
    else pos = labels[3 * h] + n_end - 1; \
    sC[pos] = cs[h]; \
  }
