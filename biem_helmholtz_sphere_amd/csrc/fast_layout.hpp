// fast_layout.hpp -- the LDS layout of the per-lane field kernels and the harmonic loops of the gradient kernels (kernels_uscat.hip,
// kernels_uinterior.hip).
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
