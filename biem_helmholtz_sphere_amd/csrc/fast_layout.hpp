// fast_layout.hpp -- the LDS layout of the per-lane field kernels (with its size and the tree dispatch for their launchers) and the
// harmonic loops of the value and of the gradient kernels (kernels_uscat.hip, kernels_uinterior.hip).
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

namespace biem {
// The dynamic LDS bytes of BIEM_FAST_LAYOUT for a workgroup of `threads` lanes: the tables, one ball's coefficients and, behind them, a
// row of `row` complex radial values per lane (the kernels' js; 0: no rows).  The launchers' one copy of what the macro lays out.
inline size_t fast_layout_lds_bytes(int tree, int n_end, int threads, size_t row) {
  const size_t ne = (size_t)n_end, ms = 2 * ne - 1, ne1 = (ne + 1) & ~(size_t)1;
  size_t tab = 0, nC = ms;                 // doubles of tables, complex of coefficients
  if (tree == TREE_BA) { tab = 2 * ne * ne + ne1; nC = ne * ne; }
  else if (tree == TREE_BBA) { tab = 4 * ne * ne + 2 * ne1; nC = ne * ne * ms; }
  else if (tree == TREE_CAA) { tab = 4 * ne * ne * ((ne + 1) / 2); nC = ne * ms * ms; }
  return tab * sizeof(double) + (nC + (size_t)threads * row) * sizeof(cplx);
}
}  // namespace biem
// STMT(TREE) for the per-lane tree of a plan (a, ba, bba or caa: the caller has excluded the chains), TREE a compile-time constant
#define BIEM_FAST_TREE_DISPATCH(tree, STMT) \
  if ((tree) == TREE_BA) { STMT(TREE_BA) } \
  else if ((tree) == TREE_BBA) { STMT(TREE_BBA) } \
  else if ((tree) == TREE_CAA) { STMT(TREE_CAA) } \
  else { STMT(TREE_A) }

// The harmonic loops of the value kernels: one text for k_uscat_fast (kernels_uscat.hip) and k_uinterior_fast (kernels_uinterior.hip),
// moved here token for token from the former.  Expects BIEM_FAST_LAYOUT's names, n_end, the offset u[4] from the ball's centre and its
// length r, and the caller's radial part: h0, h1 (the pair (h_0, h_1) of an upward recurrence, or zero), advance(hprev, hcur, two_q)
// (its next member) and radial(n, hup) giving the radial factor of degree n - hup, the recurrence's h_n, or the entry of a per-lane
// row.  Defines ar, ai: one ball's sum, without the common factor 1 / sqrt(2 pi).
#define BIEM_FIELD_HARMONICS() \
  double ar = 0.0, ai = 0.0; \
  if (TREE == TREE_A) { \
    /* Y_m = e^{i m theta} / sqrt(2 pi); degree n = |m| */ \
    const double e1x = r > 0.0 ? u[0] / r : 1.0, e1y = r > 0.0 ? u[1] / r : 0.0; \
    double ex = 1.0, ey = 0.0; \
    cplx hp = h0, hc = h1;               /* h_n, h_{n+1} */ \
    for (int n = 0; n < n_end; ++n) { \
      const cplx cp = sC[n_end - 1 + n]; \
      cplx t = make_double2(cp.x * ex - cp.y * ey, cp.x * ey + cp.y * ex); \
      if (n > 0) { const cplx cn = sC[n_end - 1 - n]; t.x += cn.x * ex + cn.y * ey; t.y += cn.y * ex - cn.x * ey; } \
      const cplx hv = radial(n, hp); \
      ar += hv.x * t.x - hv.y * t.y; ai += hv.x * t.y + hv.y * t.x; \
      const cplx hn = advance(hp, hc, 2.0 * n + 2.0); \
      hp = hc; hc = hn; \
      const double nx = ex * e1x - ey * e1y; ey = ex * e1y + ey * e1x; ex = nx; \
    } \
  } else if (TREE == TREE_BBA) { \
    /* Y_{n l m} = s0^l g_{n-l}^{(l+1)}(c0) Pbar_l^{|m|}(c1) e^{i m phi} / sqrt(2 pi): three nested recurrences; (h_m, h_{m+1}) */ \
    /* runs along m, (h_l, h_{l+1}) along l from it, (h_n, h_{n+1}) along n from that - no restart from h_0 */ \
    const double rho2 = sqrt(u[2] * u[2] + u[3] * u[3]), rho1 = sqrt(u[1] * u[1] + rho2 * rho2); \
    const double c0 = r > 0.0 ? u[0] / r : 1.0, s0 = r > 0.0 ? rho1 / r : 0.0; \
    const double c1 = rho1 > 0.0 ? u[1] / rho1 : 1.0, s1 = rho1 > 0.0 ? rho2 / rho1 : 0.0; \
    const double e1x = rho2 > 0.0 ? u[2] / rho2 : 1.0, e1y = rho2 > 0.0 ? u[3] / rho2 : 0.0; \
    const int mstride = 2 * n_end - 1; \
    double ex = 1.0, ey = 0.0, pmm = 0.70710678118654752440, s0m = 1.0; \
    cplx hm = h0, hm1 = h1; \
    for (int m = 0; m < n_end; ++m) { \
      if (m > 0) { \
        pmm *= cmm[m] * s1; s0m *= s0; \
        const cplx hn = advance(hm, hm1, 2.0 * m); \
        hm = hm1; hm1 = hn; \
        const double nx = ex * e1x - ey * e1y; ey = ex * e1y + ey * e1x; ex = nx; \
      } \
      double p0 = 0.0, p1 = pmm, sl = s0m; \
      cplx hl = hm, hl1 = hm1; \
      double sr = 0.0, si = 0.0, qr = 0.0, qi = 0.0; \
      for (int l = m; l < n_end; ++l) { \
        double gp0 = 0.0, gp1 = g0[l]; \
        cplx hp = hl, hc = hl1; \
        const double alm = sl * p1; \
        for (int n = l; n < n_end; ++n) { \
          const double amp = alm * gp1; \
          const cplx hv = radial(n, hp); \
          const double wr = hv.x * amp, wi = hv.y * amp; \
          const cplx* cc = sC + (n * n_end + l) * mstride + n_end - 1; \
          const cplx cp = cc[m]; \
          sr += wr * cp.x - wi * cp.y; si += wr * cp.y + wi * cp.x; \
          if (m > 0) { const cplx cn = cc[-m]; qr += wr * cn.x - wi * cn.y; qi += wr * cn.y + wi * cn.x; } \
          const int q = n - l + 1; \
          if (n + 1 < n_end) { \
            const double gp2 = (c0 * gp1 - ga[l * n_end + q - 1] * gp0) * gia[l * n_end + q]; \
            gp0 = gp1; gp1 = gp2; \
            const cplx hn = advance(hp, hc, 2.0 * (n + 1)); \
            hp = hc; hc = hn; \
          } \
        } \
        const int ql = l + 1; \
        if (ql < n_end) { \
          const double p2 = ra[ql * n_end + m] * (c1 * p1 - rb[ql * n_end + m] * p0); \
          p0 = p1; p1 = p2; \
          sl *= s0; \
          const cplx hn = advance(hl, hl1, 2.0 * ql); \
          hl = hl1; hl1 = hn; \
        } \
      } \
      ar += sr * ex - si * ey + qr * ex + qi * ey; \
      ai += sr * ey + si * ex + qi * ex - qr * ey; \
    } \
  } else if (TREE == TREE_CAA) { \
    /* Y_{n m1 m2} = cos^a sin^b Pbar_k^{(b,a)}(cos 2 t0) e^{i (m1 t1 + m2 t2)} / (2 pi), a = |m1|, b = |m2|, n = a + b + 2 k: the */ \
    /* Jacobi recurrence runs along k inside (a, b); the four sign combinations share it and the radial factor */ \
    const double r01 = sqrt(u[0] * u[0] + u[1] * u[1]), r23 = sqrt(u[2] * u[2] + u[3] * u[3]); \
    const double c0 = r > 0.0 ? r01 / r : 1.0, s0 = r > 0.0 ? r23 / r : 0.0, xx = c0 * c0 - s0 * s0; \
    const double e1x = r01 > 0.0 ? u[0] / r01 : 1.0, e1y = r01 > 0.0 ? u[1] / r01 : 0.0; \
    const double e2x = r23 > 0.0 ? u[2] / r23 : 1.0, e2y = r23 > 0.0 ? u[3] / r23 : 0.0; \
    double ca = 1.0, eax = 1.0, eay = 0.0; \
    cplx ha = h0, ha1 = h1;              /* h_a, h_{a+1} */ \
    for (int a = 0; a < n_end; ++a) { \
      if (a > 0) { \
        ca *= c0; \
        const cplx hn = advance(ha, ha1, 2.0 * a); \
        ha = ha1; ha1 = hn; \
        const double nx = eax * e1x - eay * e1y; eay = eax * e1y + eay * e1x; eax = nx; \
      } \
      double sb = 1.0, ebx = 1.0, eby = 0.0; \
      cplx hb = ha, hb1 = ha1;           /* h_{a+b}, h_{a+b+1} */ \
      for (int b = 0; a + b < n_end; ++b) { \
        if (b > 0) { \
          sb *= s0; \
          const cplx hn = advance(hb, hb1, 2.0 * (a + b)); \
          hb = hb1; hb1 = hn; \
          const double nx = ebx * e2x - eby * e2y; eby = ebx * e2y + eby * e2x; ebx = nx; \
        } \
        const int tb = (a * n_end + b) * K2; \
        const double amp0 = ca * sb; \
        double p0 = 0.0, p1 = 1.0; \
        cplx hp = hb, hc = hb1; \
        double ppr = 0.0, ppi = 0.0, mpr = 0.0, mpi = 0.0, pmr = 0.0, pmi = 0.0, mmr = 0.0, mmi = 0.0;   /* sums of the (+-a, +-b) coefficients */ \
        for (int kq = 0, n = a + b; n < n_end; ++kq, n += 2) { \
          const cplx hv = radial(n, hp); \
          const double amp = amp0 * jN[tb + kq] * p1; \
          const double wr = hv.x * amp, wi = hv.y * amp; \
          const cplx* cc = sC + (n * ms + n_end - 1) * ms + n_end - 1; \
          { const cplx cv = cc[a * ms + b]; ppr += wr * cv.x - wi * cv.y; ppi += wr * cv.y + wi * cv.x; } \
          if (a > 0) { const cplx cv = cc[-a * ms + b]; mpr += wr * cv.x - wi * cv.y; mpi += wr * cv.y + wi * cv.x; } \
          if (b > 0) { const cplx cv = cc[a * ms - b]; pmr += wr * cv.x - wi * cv.y; pmi += wr * cv.y + wi * cv.x; } \
          if (a > 0 && b > 0) { const cplx cv = cc[-a * ms - b]; mmr += wr * cv.x - wi * cv.y; mmi += wr * cv.y + wi * cv.x; } \
          if (n + 2 < n_end) { \
            const double p2 = (jA[tb + kq] * xx + jB[tb + kq]) * p1 - jC[tb + kq] * p0; \
            p0 = p1; p1 = p2; \
            cplx hn = advance(hp, hc, 2.0 * (n + 1)); \
            hp = hc; hc = hn; \
            hn = advance(hp, hc, 2.0 * (n + 2)); \
            hp = hc; hc = hn; \
          } \
        } \
        /* e^{i (+-a t1 +- b t2)} */ \
        const double fx = eax * ebx - eay * eby, fy = eax * eby + eay * ebx;     /* e^{i (a t1 + b t2)} */ \
        const double gx = eax * ebx + eay * eby, gy = eax * eby - eay * ebx;     /* e^{i (-a t1 + b t2)} */ \
        ar += ppr * fx - ppi * fy + mmr * fx + mmi * fy + mpr * gx - mpi * gy + pmr * gx + pmi * gy; \
        ai += ppr * fy + ppi * fx + mmi * fx - mmr * fy + mpr * gy + mpi * gx + pmi * gx - pmr * gy; \
      } \
    } \
    ar *= kInvSqrt2Pi; ai *= kInvSqrt2Pi;   /* (the second 1 / sqrt(2 pi) below) */ \
  } else { \
    const double rxy = sqrt(u[1] * u[1] + u[2] * u[2]); \
    const double c0 = r > 0.0 ? u[0] / r : 1.0, s0 = r > 0.0 ? rxy / r : 0.0; \
    const double e1x = rxy > 0.0 ? u[1] / rxy : 1.0, e1y = rxy > 0.0 ? u[2] / rxy : 0.0; \
    double ex = 1.0, ey = 0.0, pmm = 0.70710678118654752440; \
    cplx hm = h0, hm1 = h1;              /* h_m, h_{m+1}: advanced by one per order m */ \
    for (int m = 0; m < n_end; ++m) { \
      if (m > 0) { \
        pmm *= cmm[m] * s0; \
        const cplx hn = advance(hm, hm1, 2.0 * m); \
        hm = hm1; hm1 = hn; \
        const double nx = ex * e1x - ey * e1y; ey = ex * e1y + ey * e1x; ex = nx; \
      } \
      cplx hp = hm, hc = hm1;            /* h_n, h_{n+1} for n = m .. */ \
      double p0 = 0.0, p1 = pmm; \
      double sr = 0.0, si = 0.0;         /* sum over n of h_n Pbar_n^m c_{n, +-m} (the e^{+- i m phi} factors applied once per m) */ \
      double qr = 0.0, qi = 0.0; \
      for (int n = m; n < n_end; ++n) { \
        const cplx cp = sC[n * n + n + m]; \
        const cplx hv = radial(n, hp); \
        const double wr = hv.x * p1, wi = hv.y * p1; \
        sr += wr * cp.x - wi * cp.y; si += wr * cp.y + wi * cp.x; \
        if (m > 0) { const cplx cn = sC[n * n + n - m]; qr += wr * cn.x - wi * cn.y; qi += wr * cn.y + wi * cn.x; } \
        const int q = n + 1; \
        if (q < n_end) { \
          const double p2 = ra[q * n_end + m] * (c0 * p1 - rb[q * n_end + m] * p0); \
          p0 = p1; p1 = p2; \
          const cplx hn = advance(hp, hc, 2.0 * q); \
          hp = hc; hc = hn; \
        } \
      } \
      ar += sr * ex - si * ey + qr * ex + qi * ey; \
      ai += sr * ey + si * ex + qi * ex - qr * ey; \
    } \
  }

// The harmonic loops of the gradient kernels: the solid-harmonic form of kernels_uscat.hip's header (grad (z_n Y_h) = alpha_n Y_h e +
// beta_n (grad S_h)(e), never divided by a sine), one text for k_uscat_grad_fast (kernels_uscat.hip) and k_uinterior_grad_fast
// (kernels_uinterior.hip), moved here token for token from the former.  Expects BIEM_FAST_LAYOUT's names, n_end, the unit vector e[4],
// zero, and the caller's radial part: h0, h1 (the pair (h_0, h_1) of an upward recurrence, or zero), advance(hprev, hcur, two_q) (its
// next member) and radial2(n, hn, hn1, al, be) giving (alpha_n, beta_n) - from that pair or from a per-lane row.  Defines g[4]: the
// gradient of one ball's sum in the plan's axes, without the common factor 1 / sqrt(2 pi).
#define BIEM_GRAD_HARMONICS() \
  cplx g[4] = {zero, zero, zero, zero}; \
  if (TREE == TREE_A) { \
    /* S_{+-n} = (e0 +- i e1)^n / sqrt(2 pi) */ \
    const cplx w = make_double2(e[0], e[1]); \
    cplx wn = make_double2(1.0, 0.0), wn1 = zero;       /* w^n, w^{n-1} */ \
    cplx hp = h0, hc = h1; \
    cplx R = zero;                                      /* coefficient of e */ \
    for (int n = 0; n < n_end; ++n) { \
      cplx al, be; \
      radial2(n, hp, hc, al, be); \
      const cplx cp = sC[n_end - 1 + n]; \
      cplx t = cmul(cp, wn); \
      if (n > 0) { \
        const cplx cn = sC[n_end - 1 - n]; \
        cacc_conj(t, cn, wn); \
        const cplx tp = cmul(cp, wn1), tm = cmulc(cn, wn1); \
        const cplx bn = cscale(be, (double)n); \
        cacc(g[0], bn, cadd(tp, tm)); \
        const cplx df = csub(tp, tm); \
        cacc(g[1], bn, make_double2(-df.y, df.x)); \
      } \
      cacc(R, al, t); \
      const cplx hn = advance(hp, hc, 2.0 * n + 2.0); \
      hp = hc; hc = hn; \
      wn1 = wn; wn = cmul(wn, w); \
    } \
    for (int i = 0; i < 2; ++i) cacc_real(g[i], R, e[i]); \
  } else if (TREE == TREE_BA) { \
    /* S_{n, +-m} = r^{n-m} Q_n^m(u0 / r) (u1 +- i u2)^m / sqrt(2 pi) */ \
    const double c0 = e[0]; \
    const cplx w = make_double2(e[1], e[2]); \
    cplx wm = make_double2(1.0, 0.0), wm1 = zero; \
    double qmm = 0.70710678118654752440; \
    cplx hm = h0, hm1 = h1; \
    cplx R = zero;                                      /* coefficient of e */ \
    for (int m = 0; m < n_end; ++m) { \
      if (m > 0) { \
        qmm *= cmm[m]; \
        const cplx hn = advance(hm, hm1, 2.0 * m); \
        hm = hm1; hm1 = hn; \
        wm1 = wm; wm = cmul(wm, w); \
      } \
      cplx hp = hm, hc = hm1; \
      double q0 = 0.0, q1 = qmm, d0 = 0.0, d1 = 0.0;    /* Q_n^m and its derivative */ \
      cplx A = zero, Bq = zero, C = zero, An = zero, Bn = zero, Cn = zero; \
      for (int n = m; n < n_end; ++n) { \
        cplx al, be; \
        radial2(n, hp, hc, al, be); \
        const cplx W3 = cscale(be, q1), W2 = cscale(be, d1); \
        const double nm = (double)(n - m); \
        const cplx W1 = make_double2(al.x * q1 + nm * W3.x, al.y * q1 + nm * W3.y); \
        const cplx cp = sC[n * n + n + m]; \
        cacc(A, W1, cp); cacc(Bq, W2, cp); cacc(C, W3, cp); \
        if (m > 0) { const cplx cn = sC[n * n + n - m]; cacc(An, W1, cn); cacc(Bn, W2, cn); cacc(Cn, W3, cn); } \
        const int q = n + 1; \
        if (q < n_end) { \
          const double a = ra[q * n_end + m], bb = rb[q * n_end + m]; \
          const double q2 = a * (c0 * q1 - bb * q0), d2 = a * (q1 + c0 * d1 - bb * d0); \
          q0 = q1; q1 = q2; d0 = d1; d1 = d2; \
          const cplx hn = advance(hp, hc, 2.0 * q); \
          hp = hc; hc = hn; \
        } \
      } \
      cplx T1 = cmul(A, wm), T2 = cmul(Bq, wm); \
      cacc_conj(T1, An, wm); cacc_conj(T2, Bn, wm); \
      R.x += T1.x - c0 * T2.x; R.y += T1.y - c0 * T2.y; \
      g[0].x += T2.x; g[0].y += T2.y; \
      if (m > 0) { \
        const cplx tp = cmul(C, wm1), tm = cmulc(Cn, wm1); \
        const double fm = (double)m; \
        g[1].x += fm * (tp.x + tm.x); g[1].y += fm * (tp.y + tm.y); \
        g[2].x -= fm * (tp.y - tm.y); g[2].y += fm * (tp.x - tm.x); \
      } \
    } \
    for (int i = 0; i < 3; ++i) cacc_real(g[i], R, e[i]); \
  } else if (TREE == TREE_BBA) { \
    /* S_{n l +-m} = r^{n-l} g_{n-l}^{(l+1)}(u0 / r) L_l(u1, u2, u3) (u2 +- i u3)^m / sqrt(2 pi) */ \
    const double c0 = e[0], u1 = e[1], tau = e[1] * e[1] + e[2] * e[2] + e[3] * e[3]; \
    const cplx w = make_double2(e[2], e[3]); \
    const int mstride = 2 * n_end - 1; \
    cplx wm = make_double2(1.0, 0.0), wm1 = zero; \
    double qmm = 0.70710678118654752440; \
    cplx hm = h0, hm1 = h1; \
    cplx R = zero, V = zero;                            /* coefficients of e and of (0, e1, e2, e3) */ \
    for (int m = 0; m < n_end; ++m) { \
      if (m > 0) { \
        qmm *= cmm[m]; \
        const cplx hn = advance(hm, hm1, 2.0 * m); \
        hm = hm1; hm1 = hn; \
        wm1 = wm; wm = cmul(wm, w); \
      } \
      double L0 = 0.0, L1 = qmm, a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;   /* L_l and grad L_l = a_l (0,1,0,0) + b_l (0, e1, e2, e3) */ \
      cplx hl = hm, hl1 = hm1; \
      cplx XU = zero, XE = zero, XA = zero, XV = zero, XM = zero, YU = zero, YE = zero, YA = zero, YV = zero, YM = zero;   /* +m, -m */ \
      for (int l = m; l < n_end; ++l) { \
        double gp0 = 0.0, gp1 = g0[l], gd0 = 0.0, gd1 = 0.0;   /* the Gegenbauer factor and its derivative */ \
        cplx hp = hl, hc = hl1; \
        cplx S1 = zero, S2 = zero, S3 = zero, N1 = zero, N2 = zero, N3 = zero; \
        for (int n = l; n < n_end; ++n) { \
          cplx al, be; \
          radial2(n, hp, hc, al, be); \
          const cplx W3 = cscale(be, gp1), W2 = cscale(be, gd1); \
          const double nl = (double)(n - l); \
          const cplx W1 = make_double2(al.x * gp1 + nl * W3.x, al.y * gp1 + nl * W3.y); \
          const cplx* cc = sC + (n * n_end + l) * mstride + n_end - 1; \
          const cplx cp = cc[m]; \
          cacc(S1, W1, cp); cacc(S2, W2, cp); cacc(S3, W3, cp); \
          if (m > 0) { const cplx cn = cc[-m]; cacc(N1, W1, cn); cacc(N2, W2, cn); cacc(N3, W3, cn); } \
          const int q = n - l + 1; \
          if (n + 1 < n_end) { \
            const double gq = ga[l * n_end + q - 1], gi = gia[l * n_end + q]; \
            const double gp2 = (c0 * gp1 - gq * gp0) * gi, gd2 = (gp1 + c0 * gd1 - gq * gd0) * gi; \
            gp0 = gp1; gp1 = gp2; gd0 = gd1; gd1 = gd2; \
            const cplx hn = advance(hp, hc, 2.0 * (n + 1)); \
            hp = hc; hc = hn; \
          } \
        } \
        cacc_real(XU, S1, L1); cacc_real(XE, S2, L1); cacc_real(XA, S3, a1); cacc_real(XV, S3, b1); cacc_real(XM, S3, L1); \
        if (m > 0) { cacc_real(YU, N1, L1); cacc_real(YE, N2, L1); cacc_real(YA, N3, a1); cacc_real(YV, N3, b1); cacc_real(YM, N3, L1); } \
        const int ql = l + 1; \
        if (ql < n_end) { \
          const double a = ra[ql * n_end + m], bb = rb[ql * n_end + m]; \
          const double L2 = a * (u1 * L1 - bb * tau * L0); \
          const double a2 = a * (L1 + u1 * a1 - bb * tau * a0); \
          const double b2 = a * (u1 * b1 - bb * (2.0 * L0 + tau * b0)); \
          L0 = L1; L1 = L2; a0 = a1; a1 = a2; b0 = b1; b1 = b2; \
          const cplx hn = advance(hl, hl1, 2.0 * ql); \
          hl = hl1; hl1 = hn; \
        } \
      } \
      cplx TU = cmul(XU, wm), TE = cmul(XE, wm), TA = cmul(XA, wm), TV = cmul(XV, wm); \
      cacc_conj(TU, YU, wm); cacc_conj(TE, YE, wm); cacc_conj(TA, YA, wm); cacc_conj(TV, YV, wm); \
      R.x += TU.x - c0 * TE.x; R.y += TU.y - c0 * TE.y; \
      g[0].x += TE.x; g[0].y += TE.y; \
      g[1].x += TA.x; g[1].y += TA.y; \
      V.x += TV.x; V.y += TV.y; \
      if (m > 0) { \
        const cplx tp = cmul(XM, wm1), tm = cmulc(YM, wm1); \
        const double fm = (double)m; \
        g[2].x += fm * (tp.x + tm.x); g[2].y += fm * (tp.y + tm.y); \
        g[3].x -= fm * (tp.y - tm.y); g[3].y += fm * (tp.x - tm.x); \
      } \
    } \
    for (int i = 0; i < 4; ++i) cacc_real(g[i], R, e[i]); \
    for (int i = 1; i < 4; ++i) cacc_real(g[i], V, e[i]); \
  } else { \
    /* caa: S_{n, +-a, +-b} = r^{2 k} Pbar_k^{(b,a)}(xx) (u0 +- i u1)^a (u2 +- i u3)^b / (2 pi), xx = (u0^2 + u1^2 - u2^2 - u3^2) / r^2, */ \
    /* n = a + b + 2 k; grad xx on the unit sphere = 2 (e0, e1, -e2, -e3) - 2 xx e */ \
    const double xx = (e[0] * e[0] + e[1] * e[1]) - (e[2] * e[2] + e[3] * e[3]); \
    const cplx w1 = make_double2(e[0], e[1]), w2 = make_double2(e[2], e[3]); \
    cplx wa = make_double2(1.0, 0.0), wa1 = zero; \
    cplx ha = h0, ha1 = h1; \
    cplx U = zero, V = zero;                            /* coefficients of e and of 2 (e0, e1, -e2, -e3) - 2 xx e */ \
    for (int a = 0; a < n_end; ++a) { \
      if (a > 0) { \
        const cplx hn = advance(ha, ha1, 2.0 * a); \
        ha = ha1; ha1 = hn; \
        wa1 = wa; wa = cmul(wa, w1); \
      } \
      cplx wb = make_double2(1.0, 0.0), wb1 = zero; \
      cplx hb = ha, hb1 = ha1; \
      for (int b2 = 0; a + b2 < n_end; ++b2) { \
        if (b2 > 0) { \
          const cplx hn = advance(hb, hb1, 2.0 * (a + b2)); \
          hb = hb1; hb1 = hn; \
          wb1 = wb; wb = cmul(wb, w2); \
        } \
        const int tb = (a * n_end + b2) * K2; \
        double p0 = 0.0, p1 = 1.0, d0 = 0.0, d1 = 0.0; \
        cplx hp = hb, hc = hb1; \
        /* sums of the (+-a, +-b) coefficients under the three weights: pp, mp (-a, +b), pm (+a, -b), mm */ \
        cplx pp1 = zero, pp2 = zero, pp3 = zero, mp1 = zero, mp2 = zero, mp3 = zero, pm1 = zero, pm2 = zero, pm3 = zero, mm1 = zero, \
             mm2 = zero, mm3 = zero; \
        for (int kq = 0, n = a + b2; n < n_end; ++kq, n += 2) { \
          cplx al, be; \
          radial2(n, hp, hc, al, be); \
          const double nr = jN[tb + kq], pv = nr * p1, dv = nr * d1; \
          const cplx W3 = cscale(be, pv), W2 = cscale(be, dv); \
          const double k2 = (double)(2 * kq); \
          const cplx W1 = make_double2(al.x * pv + k2 * W3.x, al.y * pv + k2 * W3.y); \
          const cplx* cc = sC + (n * ms + n_end - 1) * ms + n_end - 1; \
          { const cplx cv = cc[a * ms + b2]; cacc(pp1, W1, cv); cacc(pp2, W2, cv); cacc(pp3, W3, cv); } \
          if (a > 0) { const cplx cv = cc[-a * ms + b2]; cacc(mp1, W1, cv); cacc(mp2, W2, cv); cacc(mp3, W3, cv); } \
          if (b2 > 0) { const cplx cv = cc[a * ms - b2]; cacc(pm1, W1, cv); cacc(pm2, W2, cv); cacc(pm3, W3, cv); } \
          if (a > 0 && b2 > 0) { const cplx cv = cc[-a * ms - b2]; cacc(mm1, W1, cv); cacc(mm2, W2, cv); cacc(mm3, W3, cv); } \
          if (n + 2 < n_end) { \
            const double lin = jA[tb + kq] * xx + jB[tb + kq]; \
            const double p2 = lin * p1 - jC[tb + kq] * p0, d2 = jA[tb + kq] * p1 + lin * d1 - jC[tb + kq] * d0; \
            p0 = p1; p1 = p2; d0 = d1; d1 = d2; \
            cplx hn = advance(hp, hc, 2.0 * (n + 1)); \
            hp = hc; hc = hn; \
            hn = advance(hp, hc, 2.0 * (n + 2)); \
            hp = hc; hc = hn; \
          } \
        } \
        /* w1^{+-a} w2^{+-b} (a negative power is the conjugate's) */ \
        const cplx Epp = cmul(wa, wb), Emp = cmulc(wb, wa); \
        cacc(U, pp1, Epp); cacc_conj(U, mm1, Epp); cacc(U, mp1, Emp); cacc_conj(U, pm1, Emp); \
        cacc(V, pp2, Epp); cacc_conj(V, mm2, Epp); cacc(V, mp2, Emp); cacc_conj(V, pm2, Emp); \
        if (a > 0) {                       /* a w1^{+-(a-1)} (1, +-i, 0, 0) */ \
          const cplx Fpp = cmul(wa1, wb), Fmp = cmulc(wb, wa1); \
          cplx tp = cmul(pp3, Fpp), tm = cmul(mp3, Fmp); \
          cacc_conj(tp, pm3, Fmp); cacc_conj(tm, mm3, Fpp); \
          const double fa = (double)a; \
          g[0].x += fa * (tp.x + tm.x); g[0].y += fa * (tp.y + tm.y); \
          g[1].x -= fa * (tp.y - tm.y); g[1].y += fa * (tp.x - tm.x); \
        } \
        if (b2 > 0) {                      /* b w2^{+-(b-1)} (0, 0, 1, +-i) */ \
          const cplx Hpp = cmul(wa, wb1), Hmp = cmulc(wb1, wa); \
          cplx tp = cmul(pp3, Hpp), tm = cmulc(pm3, Hmp); \
          cacc(tp, mp3, Hmp); cacc_conj(tm, mm3, Hpp); \
          const double fb = (double)b2; \
          g[2].x += fb * (tp.x + tm.x); g[2].y += fb * (tp.y + tm.y); \
          g[3].x -= fb * (tp.y - tm.y); g[3].y += fb * (tp.x - tm.x); \
        } \
      } \
    } \
    const cplx R = make_double2(U.x - 2.0 * xx * V.x, U.y - 2.0 * xx * V.y); \
    for (int i = 0; i < 4; ++i) { cacc_real(g[i], R, e[i]); cacc_real(g[i], V, i < 2 ? 2.0 * e[i] : -2.0 * e[i]); } \
    for (int i = 0; i < 4; ++i) g[i] = cscale(g[i], kInvSqrt2Pi);   /* (the second 1 / sqrt(2 pi) below) */ \
  }
