// plan.cpp -- host-side table builder (pure C++; the only HIP calls are the uploads).
#include "plan.hpp"
#include "../../include/biem_mi355.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <unordered_map>
#include <tuple>

namespace biem {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
const char* last_error() { return g_err; }

// ---- quadrature nodes ---------------------------------------------------------------------
static void gauss_legendre(int n, std::vector<double>& t, std::vector<double>& w) {
  t.assign(n, 0.0); w.assign(n, 0.0);
  for (int i = 0; i < n; ++i) {
    double x = cos(kPi * (i + 0.75) / (n + 0.5));
    double pp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = x;
      for (int k = 2; k <= n; ++k) { double p2 = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
      if (n == 1) { p0 = 1.0; p1 = x; }
      pp = n * (x * p1 - p0) / (x * x - 1.0);
      double dx = p1 / pp;
      x -= dx;
      if (fabs(dx) < 1e-16) break;
    }
    // final derivative at the converged node
    double p0 = 1.0, p1 = x;
    for (int k = 2; k <= n; ++k) { double p2 = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
    pp = n * (x * p1 - p0) / (x * x - 1.0);
    t[n - 1 - i] = x;                         // ascending
    w[n - 1 - i] = 2.0 / ((1.0 - x * x) * pp * pp);
  }
}
// Gauss-Jacobi(1/2,1/2): weight sqrt(1-t^2)
static void gauss_cheb2(int n, std::vector<double>& t, std::vector<double>& w) {
  t.assign(n, 0.0); w.assign(n, 0.0);
  for (int i = 1; i <= n; ++i) {
    double th = i * kPi / (n + 1);
    t[i - 1] = cos(th);
    w[i - 1] = kPi / (n + 1) * sin(th) * sin(th);
  }
}

// ---- labels -------------------------------------------------------------------------------
static void make_labels(int tree, int n, std::vector<int>& lab, std::vector<int>& deg) {
  lab.clear(); deg.clear();
  auto push = [&](int a, int b, int c, int dg) { lab.push_back(a); lab.push_back(b); lab.push_back(c); deg.push_back(dg); };
  if (tree == TREE_A) {
    for (int m = 0; m < n; ++m) push(m, 0, 0, m);
    for (int m = -(n - 1); m < 0; ++m) push(m, 0, 0, -m);
  } else if (tree == TREE_BA) {
    for (int q = 0; q < n; ++q) for (int m = -q; m <= q; ++m) push(q, m, 0, q);
  } else if (tree == TREE_BBA) {
    for (int q = 0; q < n; ++q) for (int l = 0; l <= q; ++l) for (int m = -l; m <= l; ++m) push(q, l, m, q);
  } else {  // caa: (n, m1, m2), n - |m1| - |m2| even >= 0
    for (int q = 0; q < n; ++q)
      for (int m1 = -q; m1 <= q; ++m1)
        for (int m2 = -(q - (m1 < 0 ? -m1 : m1)); m2 <= q - (m1 < 0 ? -m1 : m1); ++m2)
          if (((q - (m1 < 0 ? -m1 : m1) - (m2 < 0 ? -m2 : m2)) & 1) == 0) push(q, m1, m2, q);
  }
}

static inline int iabs(int v) { return v < 0 ? -v : v; }
static inline double isign_even(int e) { return ((e / 2) & 1) ? -1.0 : 1.0; }  // i^e for even e (either sign)

// G3[(l'm'),(lm),l''] real Gaunt-type integral over S^2 of Ybar' conj(Ybar) conj(Ybar''), m'' = m' - m,
// for l, l' < nmaxA and l'' < nmaxC; evaluated lazily through a dense Pbar table at Gauss-Legendre nodes.
struct Gaunt3 {
  int nq, nmax;                     // Pbar table for degrees < nmax
  std::vector<double> w;            // [nq]
  std::vector<double> P;            // [nmax][nmax][nq]
  void init(int nmax_, int nq_) {
    nmax = nmax_; nq = nq_;
    std::vector<double> t;
    gauss_legendre(nq, t, w);
    P.assign((size_t)nmax * nmax * nq, 0.0);
    for (int q = 0; q < nq; ++q) {
      double x = t[q], s = sqrt(1.0 - x * x);
      for (int n = 0; n < nmax; ++n)
        for (int m = 0; m <= n; ++m) P[((size_t)n * nmax + m) * nq + q] = pbar_single(n, m, x, s);
    }
  }
  double operator()(int lp, int mp, int l, int m, int lpp) const {
    int mu = iabs(mp - m);
    if (lpp < iabs(l - lp) || lpp > l + lp || ((l + lp + lpp) & 1) || mu > lpp) return 0.0;
    const double* a = &P[((size_t)lp * nmax + iabs(mp)) * nq];
    const double* b = &P[((size_t)l * nmax + iabs(m)) * nq];
    const double* c = &P[((size_t)lpp * nmax + mu) * nq];
    double acc = 0.0;
    for (int q = 0; q < nq; ++q) acc += w[q] * a[q] * b[q] * c[q];
    return acc * kInvSqrt2Pi;
  }
};

static int plan_build_tail(biem_plan* p);

int plan_build_host(biem_plan* p, int tree, int n_end) {
  if (tree < 0 || tree > 3) { set_error("unsupported coordinate tree id %d (built: a, ba, bba, caa)", tree); return BIEM_ERR_UNSUPPORTED; }
  if (n_end < 1 || n_end > 4096) { set_error("n_end=%d out of range", n_end); return BIEM_ERR_ARG; }
  p->tree = tree; p->d = tree_dim(tree); p->n_end = n_end; p->n2 = 2 * n_end - 1;
  p->H = harm_count(tree, n_end); p->H2 = harm_count(tree, p->n2);
  p->Cd = pow(2.0 * kPi, 0.5 * p->d) * sqrt(2.0 / kPi);
  make_labels(tree, n_end, p->labels, p->deg);
  make_labels(tree, p->n2, p->labels2, p->deg2);
  const int H = p->H, d = p->d, n = n_end;
  {
    // conjugate partners: conj Y_h = Y_p with the orders of all type-a nodes negated (every tree built here has real
    // non-azimuthal factors and no sign: tests/test_oracle_golden.py::test_translation_block_matrix_is_complex_symmetric...)
    std::map<std::tuple<int, int, int>, int> pos;
    for (int h = 0; h < H; ++h) pos[std::make_tuple(p->labels[3 * h], p->labels[3 * h + 1], p->labels[3 * h + 2])] = h;
    p->units.clear();
    for (int h = 0; h < H; ++h) {
      int a = p->labels[3 * h], b = p->labels[3 * h + 1], c = p->labels[3 * h + 2];
      if (tree == TREE_A) a = -a; else if (tree == TREE_BA) b = -b; else if (tree == TREE_BBA) c = -c; else { b = -b; c = -c; }
      auto it = pos.find(std::make_tuple(a, b, c));
      if (it == pos.end()) { set_error("internal: harmonic %d has no conjugate partner", h); return BIEM_ERR_ARG; }
      if (h <= it->second) { p->units.push_back(h); p->units.push_back(it->second); }
    }
  }

  // ---- boundary-data quadrature ----
  {
    std::vector<double> t0, w0, t1, w1;
    const int na = 2 * n;
    if (tree == TREE_A) {
      p->Q = na;
      p->qy.resize((size_t)p->Q * d); p->qw.resize(p->Q);
      for (int j = 0; j < na; ++j) { double ph = j * kPi / n; p->qy[2 * j] = cos(ph); p->qy[2 * j + 1] = sin(ph); p->qw[j] = kPi / n; }
    } else if (tree == TREE_BA) {
      gauss_legendre(n, t0, w0);
      p->Q = n * na;
      p->qy.resize((size_t)p->Q * d); p->qw.resize(p->Q);
      for (int i = 0; i < n; ++i) for (int j = 0; j < na; ++j) {
        int q = i * na + j; double ph = j * kPi / n, s = sqrt(1.0 - t0[i] * t0[i]);
        p->qy[3 * q] = t0[i]; p->qy[3 * q + 1] = s * cos(ph); p->qy[3 * q + 2] = s * sin(ph);
        p->qw[q] = w0[i] * kPi / n;
      }
    } else if (tree == TREE_CAA) {
      // type-c root over two type-a children: sin t cos t dt = dx / 4 with x = cos 2t -> Gauss-Legendre in x (pinned by the
      // jascome caa goldens); both azimuths 2 n_end equispaced points
      gauss_legendre(n, t0, w0);
      p->Q = n * na * na;
      p->qy.resize((size_t)p->Q * d); p->qw.resize(p->Q);
      for (int i = 0; i < n; ++i) for (int j1 = 0; j1 < na; ++j1) for (int j2 = 0; j2 < na; ++j2) {
        int q = (i * na + j1) * na + j2;
        double th = 0.5 * acos(t0[i]), p1 = j1 * kPi / n, p2 = j2 * kPi / n;
        p->qy[4 * q] = cos(th) * cos(p1); p->qy[4 * q + 1] = cos(th) * sin(p1);
        p->qy[4 * q + 2] = sin(th) * cos(p2); p->qy[4 * q + 3] = sin(th) * sin(p2);
        p->qw[q] = 0.25 * w0[i] * (kPi / n) * (kPi / n);
      }
    } else {
      gauss_cheb2(n, t0, w0); gauss_legendre(n, t1, w1);
      p->Q = n * n * na;
      p->qy.resize((size_t)p->Q * d); p->qw.resize(p->Q);
      for (int i = 0; i < n; ++i) for (int l = 0; l < n; ++l) for (int j = 0; j < na; ++j) {
        int q = (i * n + l) * na + j; double ph = j * kPi / n;
        double s0 = sqrt(1.0 - t0[i] * t0[i]), s1 = sqrt(1.0 - t1[l] * t1[l]);
        p->qy[4 * q] = t0[i]; p->qy[4 * q + 1] = s0 * t1[l]; p->qy[4 * q + 2] = s0 * s1 * cos(ph); p->qy[4 * q + 3] = s0 * s1 * sin(ph);
        p->qw[q] = w0[i] * w1[l] * kPi / n;
      }
    }
  }
  // ---- projection matrix W[q][h] = w_q conj(Y_h(y_q)) ----
  p->W.resize((size_t)p->Q * H * 2);
  for (int q = 0; q < p->Q; ++q) {
    Dir dir = make_dir(tree, &p->qy[(size_t)q * d]);
    for (int h = 0; h < H; ++h) {
      double re, im;
      harmonic_single(tree, p->labels[3 * h], p->labels[3 * h + 1], p->labels[3 * h + 2], dir, &re, &im);
      p->W[((size_t)q * H + h) * 2] = p->qw[q] * re;
      p->W[((size_t)q * H + h) * 2 + 1] = -p->qw[q] * im;
    }
  }
  // ---- translation terms ----
  // 2-D beyond kLists2dMax: no term lists at all (H^2 entries of one term each: 1.4 GB at the reference's n_end = 3444) - the 2-D
  // fills evaluate S(m, m') = i^{|m| + |mu| - |m'|} T[mu], mu = m' - m, directly (k_fill2d_sym / k_fill2d, any order)
  const bool lists = !(tree == TREE_A && n_end > kLists2dMax);
  p->lists_built = lists;
  p->ptr.assign(lists ? (size_t)H * H + 1 : 1, 0);
  p->coef.clear(); p->tidx.clear();
  if (!lists) {
  } else if (tree == TREE_A) {
    const int n2 = p->n2;
    for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
      int m = p->labels[3 * h], mp = p->labels[3 * hp], mu = mp - m;
      p->coef.push_back(isign_even(iabs(m) + iabs(mu) - iabs(mp)) * kInvSqrt2Pi);
      p->tidx.push_back(mu >= 0 ? mu : (2 * n2 - 1) + mu);
      p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
    }
  } else if (tree == TREE_BA) {
    Gaunt3 G; G.init(p->n2, 2 * n);
    for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
      int q = p->labels[3 * h], m = p->labels[3 * h + 1], qp = p->labels[3 * hp], mp = p->labels[3 * hp + 1], mu = mp - m;
      for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2) {
        if (q2 < iabs(mu)) continue;
        double g = G(qp, mp, q, m, q2);
        p->coef.push_back(isign_even(q + q2 - qp) * g);
        p->tidx.push_back(q2 * q2 + q2 + mu);
      }
      p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
    }
  } else if (tree == TREE_CAA) {
    // int Y' conj(Y) conj(Y'') = delta(m1'' = m1' - m1) delta(m2'' = m2' - m2) / (2 pi) * int cbar' cbar cbar'' sin cos dt;
    // the polar integrand is a polynomial of degree <= 2 n_end - 2 in x = cos 2t: Gauss-Legendre with 2 n_end nodes is exact
    const int nq = 2 * n;
    std::vector<double> xg, wg; gauss_legendre(nq, xg, wg);
    std::map<int, std::vector<double>> cb;      // key (n, a, b) -> values at the nodes
    auto key = [](int q, int a, int b) { return (q * 256 + a) * 256 + b; };
    for (size_t l = 0; l < p->deg2.size(); ++l) {
      int q = p->labels2[3 * l], a = iabs(p->labels2[3 * l + 1]), b = iabs(p->labels2[3 * l + 2]);
      auto& v = cb[key(q, a, b)];
      if (!v.empty()) continue;
      v.resize(nq);
      for (int i = 0; i < nq; ++i) { double th = 0.5 * acos(xg[i]); v[i] = cbar_single(q, a, b, cos(th), sin(th)); }
    }
    std::map<int, int> pos2;                    // signed label -> index among degrees < n2
    auto skey = [](int q, int m1, int m2) { return (q * 256 + (m1 + 128)) * 256 + (m2 + 128); };
    for (size_t l = 0; l < p->deg2.size(); ++l) pos2[skey(p->labels2[3 * l], p->labels2[3 * l + 1], p->labels2[3 * l + 2])] = (int)l;
    for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
      int q = p->labels[3 * h], m1 = p->labels[3 * h + 1], m2 = p->labels[3 * h + 2];
      int qp = p->labels[3 * hp], m1p = p->labels[3 * hp + 1], m2p = p->labels[3 * hp + 2];
      int mu1 = m1p - m1, mu2 = m2p - m2;
      const std::vector<double>& a = cb[key(qp, iabs(m1p), iabs(m2p))];
      const std::vector<double>& b = cb[key(q, iabs(m1), iabs(m2))];
      for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2) {
        if (q2 < iabs(mu1) + iabs(mu2)) continue;
        const std::vector<double>& c = cb[key(q2, iabs(mu1), iabs(mu2))];
        double acc = 0.0;
        for (int i = 0; i < nq; ++i) acc += 0.25 * wg[i] * a[i] * b[i] * c[i];
        if (fabs(acc) < 1e-14) continue;
        p->coef.push_back(isign_even(q + q2 - qp) * acc / (2.0 * kPi));
        p->tidx.push_back(pos2[skey(q2, mu1, mu2)]);
      }
      p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
    }
  } else {
    const int n2 = p->n2;
    Gaunt3 G; G.init(n2, 2 * n);
    // Abar[n][l][q] at Gauss-Chebyshev-2 nodes, degrees < n2
    std::vector<double> tc, wc; gauss_cheb2(2 * n, tc, wc);
    const int nq = 2 * n;
    std::vector<double> Ab((size_t)n2 * n2 * nq, 0.0);
    for (int qd = 0; qd < nq; ++qd) {
      double x = tc[qd], s = sqrt(1.0 - x * x);
      for (int l = 0; l < n2; ++l) {
        double sl = 1.0; for (int i = 0; i < l; ++i) sl *= s;
        for (int q = l; q < n2; ++q) Ab[((size_t)q * n2 + l) * nq + qd] = sl * gbar_single(q - l, l, x);
      }
    }
    auto off = [](int q) { return q * (q + 1) * (2 * q + 1) / 6; };
    for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
      int q = p->labels[3 * h], l = p->labels[3 * h + 1], m = p->labels[3 * h + 2];
      int qp = p->labels[3 * hp], lp = p->labels[3 * hp + 1], mp = p->labels[3 * hp + 2], mu = mp - m;
      const double* a = &Ab[((size_t)qp * n2 + lp) * nq];
      const double* b = &Ab[((size_t)q * n2 + l) * nq];
      for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2) {
        for (int l2 = iabs(l - lp); l2 <= l + lp && l2 <= q2; l2 += 2) {
          if (l2 < iabs(mu)) continue;
          double g3 = G(lp, mp, l, m, l2);
          if (g3 == 0.0) continue;
          const double* c = &Ab[((size_t)q2 * n2 + l2) * nq];
          double a4 = 0.0;
          for (int qd = 0; qd < nq; ++qd) a4 += wc[qd] * a[qd] * b[qd] * c[qd];
          // (quadrature noise of a polar integral that vanishes by a selection rule reaches 3e-14 at n_end = 15; integrals that do not
          // vanish are >= 1e-9 there: oracle/biem_oracle.py::_theta4)
          if (fabs(a4) < 1e-12) continue;
          double v = a4 * g3;
          if (fabs(v) < 1e-14) continue;   // vanishes by a selection rule; only quadrature rounding is left
          p->coef.push_back(isign_even(q + q2 - qp) * v);
          p->tidx.push_back(off(q2) + l2 * l2 + l2 + mu);
        }
      }
      p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
    }
  }
  return plan_build_tail(p);
}

// the tree-independent tables behind the labels and term lists: fill chunks, unit-pair lists, the reduced-table form
static int plan_build_tail(biem_plan* p) {
  const int tree = p->tree, n_end = p->n_end, H = p->H, lw = p->lw;
  const bool lists = p->lists_built;
  // ---- entry chunks of the fill kernel: term slice + row pointers + pair table + column factors must fit LDS ----
  p->tidx16.resize(p->tidx.size());
  for (size_t i = 0; i < p->tidx.size(); ++i) p->tidx16[i] = (uint16_t)p->tidx[i];
  {
    const int max_ents = 1024;                                     // = FILL_THREADS of the fill kernel: one entry per thread
    long long budget = 150 * 1024 - (long long)(p->H2 + 2 * H) * 16 - (long long)(max_ents + 1) * 4 - 64;
    // large orders (3-D n_end >= 40, 4-D >= 15): the pair table no longer leaves room for a useful slice of the term list - the
    // kernel then reads the pair table from global memory (L2) and LDS holds only the column factors and the term slice
    p->fill_table_global = budget < 2048 * 10;
    if (p->fill_table_global) budget = 150 * 1024 - (long long)(2 * H) * 16 - (long long)(max_ents + 1) * 4 - 64;
    long long cap_terms = budget > 0 ? budget / 10 : 0;            // 8-byte coefficient + 2-byte table index per term
    if (cap_terms > 16384) cap_terms = 16384;
    const long long total = (long long)H * H;
    p->chunk_ent.clear();
    p->chunk_ent.push_back(0);
    p->chunk_terms_max = 0; p->chunk_ents_max = 0;
    long long e0 = 0;
    while (lists && e0 < total) {
      long long e1 = e0 + 1;
      while (e1 < total && e1 - e0 < max_ents && (long long)(p->ptr[e1 + 1] - p->ptr[e0]) <= cap_terms) ++e1;
      int nt = (int)(p->ptr[e1] - p->ptr[e0]);
      if (nt > p->chunk_terms_max) p->chunk_terms_max = nt;
      if ((int)(e1 - e0) > p->chunk_ents_max) p->chunk_ents_max = (int)(e1 - e0);
      p->chunk_ent.push_back((int)e1);
      e0 = e1;
    }
  }
  // ---- unit-pair ("quad") term lists and chunks of the symmetric fill ----
  {
    const int U = (int)(p->units.size() / 2);
    p->spos.assign(U, -1); p->hpos.assign(H, 0);
    int ns = 0;
    for (int u = 0; u < U; ++u) {
      const int h = p->units[2 * u], pp = p->units[2 * u + 1];
      p->hpos[h] = u;
      if (pp != h) { p->spos[u] = ns; p->hpos[pp] = U + ns; ++ns; }
    }
    p->qptr.assign(lists ? (size_t)4 * U * U + 1 : 1, 0);
    p->qcoef.clear(); p->qidx16.clear();
    p->qcoef.reserve(p->coef.size()); p->qidx16.reserve(p->coef.size());
    for (int u = 0; u < (lists ? U : 0); ++u)
      for (int v = 0; v < U; ++v) {
        const int hh[2] = {p->units[2 * u], p->units[2 * u + 1]}, cc[2] = {p->units[2 * v], p->units[2 * v + 1]};
        for (int slot = 0; slot < 4; ++slot) {
          const int ri = slot >> 1, ci = slot & 1;
          const bool present = (ri == 0 || hh[1] != hh[0]) && (ci == 0 || cc[1] != cc[0]);
          if (present) {
            const size_t e = (size_t)hh[ri] * H + cc[ci];
            for (uint32_t q = p->ptr[e]; q < p->ptr[e + 1]; ++q) { p->qcoef.push_back(p->coef[q]); p->qidx16.push_back((uint16_t)p->tidx[q]); }
          }
          p->qptr[((size_t)u * U + v) * 4 + slot + 1] = (uint32_t)p->qcoef.size();
        }
      }
    // ---- the two-list form of the entry-per-lane kernel ----
    {
      std::map<std::vector<int>, int> pos2;
      const int H2 = p->H2;
      for (int l = 0; l < H2; ++l) pos2[std::vector<int>(&p->labels2[(size_t)lw * l], &p->labels2[(size_t)lw * l] + lw)] = l;
      std::vector<int> partner2(H2, -1);
      bool ok = true;
      for (int l = 0; l < H2 && ok; ++l) {
        std::vector<int> c(&p->labels2[(size_t)lw * l], &p->labels2[(size_t)lw * l] + lw);
        if (tree == TREE_A) c[0] = -c[0]; else if (tree == TREE_BA) c[1] = -c[1]; else if (tree == TREE_BBA) c[2] = -c[2];
        else if (tree == TREE_CHAIN) c[lw - 1] = -c[lw - 1]; else { c[1] = -c[1]; c[2] = -c[2]; }
        auto it = pos2.find(c);
        if (it == pos2.end()) ok = false; else partner2[l] = it->second;
      }
      p->lin2.assign(H2, 0);
      int ne = 0;
      for (int l = 0; l < H2 && ok; ++l)
        if (l <= partner2[l]) { p->lin2[l] = 2 * ne; if (partner2[l] != l) p->lin2[partner2[l]] = 2 * ne + 1; ++ne; }
      p->H2lin = 2 * ne;
      if (p->H2lin > 65535) ok = false;
      p->q2ptr.assign(lists ? (size_t)2 * U * U + 1 : 1, 0);
      p->q2coef.clear(); p->q2idx16.clear();
      const int Ul = lists ? U : 0;            // (no lists: the loops over unit pairs below do nothing)
      auto same_mirrored = [&](size_t ea, size_t eb) {      // list of entry eb == list of entry ea with partner indices?
        if (p->ptr[ea + 1] - p->ptr[ea] != p->ptr[eb + 1] - p->ptr[eb]) return false;
        for (uint32_t q = p->ptr[ea], r = p->ptr[eb]; q < p->ptr[ea + 1]; ++q, ++r) {
          if (fabs(p->coef[q] - p->coef[r]) > 1e-13 * (fabs(p->coef[q]) + 1e-300)) return false;
          if (partner2[p->tidx[q]] != p->tidx[r]) return false;
        }
        return true;
      };
      for (int u = 0; u < Ul && ok; ++u)
        for (int v = 0; v < U && ok; ++v) {
          const int h = p->units[2 * u], pp = p->units[2 * u + 1], ch = p->units[2 * v], cp = p->units[2 * v + 1];
          const bool r2 = pp != h, c2 = cp != ch;
          const size_t eA = (size_t)h * H + ch;
          for (uint32_t q = p->ptr[eA]; q < p->ptr[eA + 1]; ++q) { p->q2coef.push_back(p->coef[q]); p->q2idx16.push_back((uint16_t)p->lin2[p->tidx[q]]); }
          p->q2ptr[((size_t)u * U + v) * 2 + 1] = (uint32_t)p->q2coef.size();
          // the mirror of list A: (p,p') when both units are doubles, (p,h') when only the row unit is, (h,p') when only the column unit is
          if (r2 && c2) ok = ok && same_mirrored(eA, (size_t)pp * H + cp);
          else if (r2) ok = ok && same_mirrored(eA, (size_t)pp * H + ch);
          else if (c2) ok = ok && same_mirrored(eA, (size_t)h * H + cp);
          if (r2 && c2) {
            const size_t eB = (size_t)h * H + cp;
            for (uint32_t q = p->ptr[eB]; q < p->ptr[eB + 1]; ++q) { p->q2coef.push_back(p->coef[q]); p->q2idx16.push_back((uint16_t)p->lin2[p->tidx[q]]); }
            ok = ok && same_mirrored(eB, (size_t)pp * H + ch);
          }
          p->q2ptr[((size_t)u * U + v) * 2 + 2] = (uint32_t)p->q2coef.size();
        }
      p->pair_lists_ok = ok && lists;
      // ---- reduced-table form: T'[e] shared by a label and its partner, one phase per list (plan.hpp) ----
      bool rok = ok;
      p->E = ne; p->red_of.assign(H2, 0); p->red_first.assign(H2, 0); p->red_label.assign(ne, 0);
      for (int l = 0; l < H2 && rok; ++l) {
        p->red_of[l] = p->lin2[l] >> 1;
        p->red_first[l] = (l <= partner2[l]) ? 1 : 0;
        if (l <= partner2[l]) p->red_label[p->lin2[l] >> 1] = l;
      }
      // phase ids: one per distinct azimuthal order vector of the first members
      auto az_of = [&](int l, int& m1, int& m2) {
        m2 = 0;
        if (tree == TREE_CHAIN) { m1 = p->labels2[(size_t)lw * l + lw - 1]; return; }
        const int a = p->labels2[3 * l], b = p->labels2[3 * l + 1], c = p->labels2[3 * l + 2];
        if (tree == TREE_A) m1 = a; else if (tree == TREE_BA) m1 = b; else if (tree == TREE_BBA) m1 = c; else { m1 = b; m2 = c; }
      };
      std::map<std::pair<int, int>, int> phid;
      p->ph_mu.clear(); p->ph_of_unit.assign(ne, 0);
      for (int e = 0; e < ne && rok; ++e) {
        int m1, m2; az_of(p->red_label[e], m1, m2);
        auto it = phid.find(std::make_pair(m1, m2));
        if (it == phid.end()) { it = phid.insert(std::make_pair(std::make_pair(m1, m2), (int)phid.size())).first; p->ph_mu.push_back(m1); p->ph_mu.push_back(m2); }
        p->ph_of_unit[e] = it->second;
      }
      p->NP = (int)phid.size();
      if (p->E + p->NP > 65535 || p->NP > 32767) rok = false;
      // per list: all terms of one kind (first members / partners / self-conjugate) and of one phase id
      p->rphsel.assign(lists ? (size_t)2 * U * U : 0, 0);
      auto list_sel = [&](size_t e, uint16_t& sel) {     // phase selector of entry e's list; false if the list is not uniform
        int kind = -1, id = -1;
        for (uint32_t q = p->ptr[e]; q < p->ptr[e + 1]; ++q) {
          const int l = p->tidx[q], u2 = p->red_of[l];
          const int k2 = partner2[l] == l ? 0 : (p->red_first[l] ? 1 : 2);          // 0 self, 1 first, 2 partner
          if (kind < 0) { kind = k2; id = p->ph_of_unit[u2]; }
          else if (kind != k2 || id != p->ph_of_unit[u2]) return false;
        }
        if (kind < 0) { sel = 0; return true; }            // empty list: value 0 whatever the phase
        if (kind == 0) {                                    // self-conjugate labels: azimuthal vector 0, phase 1
          if (p->ph_mu[2 * id] != 0 || p->ph_mu[2 * id + 1] != 0) return false;
        }
        sel = (uint16_t)(2 * id + (kind == 2 ? 1 : 0));
        return true;
      };
      // transposed, padded lists per wave of 64 unit pairs; chunks of at most 16 waves within the LDS budget
      p->rcoef.clear(); p->ridx.clear(); p->rchunk.assign(1, 0); p->rcrow.assign(1, 0); p->rwrow.clear(); p->rchunk_rows_max = 0;
      const long long total_pairs = lists ? (long long)U * U : 0;
      { const char* ew = getenv("BIEM_FILL_RED_WAVES"); p->red_waves = (ew && atoi(ew) == 8) ? 8 : 16;
        const char* en = getenv("BIEM_FILL_NC"); p->red_nc = (en && en[0] == '1') ? 1 : 2; }
      // LDS of a workgroup: 16 waves - the CU to itself; 8 waves - two workgroups per CU (their phases overlap); red_nc table rows
      const long long lds_budget = (p->red_waves == 16 ? 156 : 76) * 1024 - p->red_nc * ((long long)(p->E + p->NP) * 16 + (long long)2 * n_end * 16) - 33 * 4 - 256;
      const long long cap_rows = lds_budget > 0 ? lds_budget / (64 * 10) : 0;          // a row: 64 x (8-byte coefficient + 2-byte index)
      std::vector<int> wr(33, 0);
      long long crows = 0; int cw = 0;                     // rows / waves of the open chunk
      // lanes of the four groups in which a ds_read_b128 is serviced (MI355X_MICROARCH.md, LDS table)
      static const int kB128Group[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                            {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                            {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                            {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
      const char* elo = getenv("BIEM_FILL_LIST_ORDER");
      const bool reorder_lists = !(elo && elo[0] == 'n');
      long long gather_cycles = 0, gather_groups = 0;
      auto close_chunk = [&](long long pair_end) {
        for (int w = cw; w < 16; ++w) { wr[2 * w + 1] = wr[2 * w]; wr[2 * w + 2] = wr[2 * w]; }
        for (int i = 0; i < 33; ++i) p->rwrow.push_back(wr[i]);
        p->rchunk.push_back((int)pair_end);
        p->rcrow.push_back((int)(p->rcoef.size() / 64));
        if (crows > p->rchunk_rows_max) p->rchunk_rows_max = (int)crows;
        crows = 0; cw = 0; wr.assign(33, 0);
      };
      for (long long w0 = 0; w0 < total_pairs && rok; w0 += 64) {
        const int nl = (int)((total_pairs - w0 < 64) ? total_pairs - w0 : 64);
        size_t eA[64], eB[64]; bool hasB[64];
        uint32_t LA = 0, LB = 0;
        for (int i = 0; i < nl; ++i) {
          const long long pi = w0 + i; const int u = (int)(pi / U), v = (int)(pi - (long long)u * U);
          const int h = p->units[2 * u], pp = p->units[2 * u + 1], ch = p->units[2 * v], cp = p->units[2 * v + 1];
          eA[i] = (size_t)h * H + ch; eB[i] = (size_t)h * H + cp; hasB[i] = (pp != h) && (cp != ch);
          uint16_t sA = 0, sB = 0;
          rok = rok && list_sel(eA[i], sA);
          if (hasB[i]) rok = rok && list_sel(eB[i], sB);
          p->rphsel[2 * (size_t)pi] = sA; p->rphsel[2 * (size_t)pi + 1] = sB;
          const uint32_t la = p->ptr[eA[i] + 1] - p->ptr[eA[i]], lb = hasB[i] ? p->ptr[eB[i] + 1] - p->ptr[eB[i]] : 0;
          if (la > LA) LA = la;
          if (lb > LB) LB = lb;
        }
        LA = (LA + 3) & ~3u; LB = (LB + 3) & ~3u;           // the kernel walks the lists in groups of four rows
        if (!rok) break;
        if ((long long)(LA + LB) > cap_rows) { rok = false; break; }                    // one wave alone exceeds the LDS budget
        if (cw == p->red_waves || crows + LA + LB > cap_rows) close_chunk(w0);
        wr[2 * cw] = (int)crows; wr[2 * cw + 1] = (int)(crows + LA); wr[2 * cw + 2] = (int)(crows + LA + LB);
        for (int pass = 0; pass < 2; ++pass) {
          const uint32_t L = pass ? LB : LA;
          const size_t base = p->rcoef.size();                // coefficients [row][lane]; indices [group of 4 rows][lane][4]
          p->rcoef.resize(base + (size_t)L * 64, 0.0); p->ridx.resize(base + (size_t)L * 64, 0);
          // The order of a lane's terms is free (a sum), and row t of the transposed list is ONE ds_read_b128 gather of the table
          // per combination: 16-byte entries, 16 slots of 4 banks per 256-byte bank row, serviced in four fixed groups of 16 lanes
          // (MI355X_MICROARCH.md, LDS); lanes of a group that read different entries of one slot take one more LDS cycle each.
          // So the terms are dealt to the rows group by group such that the lanes of a group meet on as few slots as possible
          // (greedy: lanes with the fewest choices first, each takes the term whose slot is least loaded in this row; equal entries
          // share a read).  Natural order: ~1.6 LDS cycles per group and row at cfg 3, i.e. 30 % of all LDS cycles of the kernel were
          // bank conflicts (profiles/r03_pmc_summary.txt).  BIEM_FILL_LIST_ORDER=natural keeps the natural order (A/B).
          std::vector<std::vector<std::pair<double, uint16_t>>> terms(64);
          for (int i = 0; i < nl; ++i)
            if (pass == 0 || hasB[i]) {
              const size_t e = pass ? eB[i] : eA[i];
              for (uint32_t q = p->ptr[e]; q < p->ptr[e + 1]; ++q) terms[i].push_back(std::make_pair(p->coef[q], (uint16_t)p->red_of[p->tidx[q]]));
            }
          std::vector<std::vector<std::pair<double, uint16_t>>> rowterm(L, std::vector<std::pair<double, uint16_t>>(64, std::make_pair(0.0, (uint16_t)0xffff)));
          if (!reorder_lists) {
            for (int i = 0; i < 64; ++i) for (size_t t = 0; t < terms[i].size(); ++t) rowterm[t][i] = terms[i][t];
          } else {
            for (int g = 0; g < 4; ++g) {
              std::vector<std::vector<char>> used(16);
              for (int q = 0; q < 16; ++q) used[q].assign(terms[kB128Group[g][q]].size(), 0);
              for (uint32_t t = 0; t < L; ++t) {
                int load[16] = {0};                           // distinct entries per slot in this row and group
                std::vector<uint16_t> chosen;                 // entries already read in this row and group
                // lanes in the order of their number of distinct remaining slots (fewest first)
                int order[16], nd[16];
                for (int q = 0; q < 16; ++q) {
                  order[q] = q;
                  bool seen[16] = {false}; nd[q] = 0;
                  const auto& tl = terms[kB128Group[g][q]];
                  for (size_t x = 0; x < tl.size(); ++x) if (!used[q][x] && !seen[tl[x].second & 15]) { seen[tl[x].second & 15] = true; ++nd[q]; }
                }
                std::stable_sort(order, order + 16, [&](int a, int b) { return nd[a] < nd[b]; });
                for (int oq = 0; oq < 16; ++oq) {
                  const int q = order[oq], lane_i = kB128Group[g][q];
                  const auto& tl = terms[lane_i];
                  int best = -1, best_cost = 1 << 30, best_cnt = -1;
                  int cnt[16] = {0};
                  for (size_t x = 0; x < tl.size(); ++x) if (!used[q][x]) ++cnt[tl[x].second & 15];
                  for (size_t x = 0; x < tl.size(); ++x) {
                    if (used[q][x]) continue;
                    const int sl = tl[x].second & 15;
                    bool shared = false;
                    for (uint16_t cix : chosen) if (cix == tl[x].second) { shared = true; break; }
                    const int cost = shared ? 0 : load[sl] * 2 + 1;      // a shared entry is free; then the least loaded slot
                    if (cost < best_cost || (cost == best_cost && cnt[sl] > best_cnt)) { best = (int)x; best_cost = cost; best_cnt = cnt[sl]; }
                  }
                  if (best < 0) continue;                     // this lane's list has run out
                  used[q][best] = 1;
                  rowterm[t][lane_i] = tl[best];
                  bool shared = false;
                  for (uint16_t cix : chosen) if (cix == tl[best].second) { shared = true; break; }
                  if (!shared) { chosen.push_back(tl[best].second); ++load[tl[best].second & 15]; }
                }
                // lanes without a term in this row (coefficient 0) read an entry somebody else of the group reads anyway: the one of
                // the lowest degree (T' is degree-major: the smallest index; entry 0 itself, h_0, was the padding before)
                uint16_t filler = 0;
                if (!chosen.empty()) { filler = chosen[0]; for (uint16_t cix : chosen) if (cix < filler) filler = cix; }
                for (int q = 0; q < 16; ++q) if (rowterm[t][kB128Group[g][q]].second == 0xffff) rowterm[t][kB128Group[g][q]] = std::make_pair(0.0, filler);
              }
            }
          }
          for (uint32_t t = 0; t < L; ++t)
            for (int i = 0; i < 64; ++i) {
              double cf = rowterm[t][i].first; uint16_t ix = rowterm[t][i].second;
              if (ix == 0xffff) { cf = 0.0; ix = 0; }
              p->rcoef[base + (size_t)t * 64 + i] = cf;
              p->ridx[base + ((size_t)(t >> 2) * 64 + i) * 4 + (t & 3)] = ix;
              // statistics of the gather (LDS cycles per row and group = most distinct entries on one slot)
            }
          for (uint32_t t = 0; t < L; ++t)
            for (int g = 0; g < 4; ++g) {
              int mx = 0;
              for (int sl = 0; sl < 16; ++sl) {
                uint16_t seen_e[16]; int ns = 0;
                for (int q = 0; q < 16; ++q) {
                  const uint16_t ix = p->ridx[base + ((size_t)(t >> 2) * 64 + kB128Group[g][q]) * 4 + (t & 3)];
                  if ((ix & 15) != sl) continue;
                  bool dup = false;
                  for (int z = 0; z < ns; ++z) if (seen_e[z] == ix) { dup = true; break; }
                  if (!dup) seen_e[ns++] = ix;
                }
                if (ns > mx) mx = ns;
              }
              gather_cycles += mx; gather_groups += 1;
            }
        }
        crows += LA + LB; ++cw;
      }
      if (rok && cw > 0) close_chunk(total_pairs);
      p->red_gather_cycles = gather_groups > 0 ? (double)gather_cycles / (double)gather_groups : 0.0;
      if (getenv("BIEM_PLAN_STATS")) fprintf(stderr, "plan tree %d n_end %d: table gather %.3f LDS cycles per row and lane group (1 = conflict-free), %lld rows\n", tree, n_end, p->red_gather_cycles, gather_groups / 4);
      p->red_lists_ok = rok && (int)p->rchunk.size() > 1;
      if (!p->red_lists_ok) { p->rcoef.clear(); p->ridx.clear(); p->rchunk.assign(1, 0); p->rcrow.assign(1, 0); p->rwrow.clear(); p->rchunk_rows_max = 0; }
    }
    // chunks: the paired pair table (H2lin complex), the per-degree factors of two balls, the list pointers and the term slice share LDS
    const int max_pairs = 1024;                                    // = FILL_SYM_THREADS: one unit pair per thread
    const long long budget = 158 * 1024 - (long long)p->H2lin * 16 - (long long)2 * n_end * 16 - (long long)(2 * max_pairs + 1) * 4 - 64;
    long long cap_terms = budget > 0 ? budget / 10 : 0;
    const long long total = lists ? (long long)U * U : 0;
    p->qchunk.clear(); p->qchunk.push_back(0);
    p->qchunk_terms_max = 0; p->qchunk_pairs_max = 0;
    long long e0 = 0;
    bool fits = cap_terms > 0 && p->pair_lists_ok;
    while (fits && e0 < total) {
      long long e1 = e0 + 1;
      if ((long long)(p->q2ptr[2 * e1] - p->q2ptr[2 * e0]) > cap_terms) { fits = false; break; }     // one pair alone exceeds the budget
      while (e1 < total && e1 - e0 < max_pairs && (long long)(p->q2ptr[2 * (e1 + 1)] - p->q2ptr[2 * e0]) <= cap_terms) ++e1;
      const int nt = (int)(p->q2ptr[2 * e1] - p->q2ptr[2 * e0]);
      if (nt > p->qchunk_terms_max) p->qchunk_terms_max = nt;
      if ((int)(e1 - e0) > p->qchunk_pairs_max) p->qchunk_pairs_max = (int)(e1 - e0);
      p->qchunk.push_back((int)e1);
      e0 = e1;
    }
    if (!fits) { p->qchunk.assign(1, 0); p->qchunk_terms_max = 0; p->qchunk_pairs_max = 0; }   // the systems-in-lanes form takes over
    // small chunks of the systems-in-lanes form: at most 3072 terms (36 KB of LDS: several workgroups per CU) and 256 unit pairs
    {
      const long long cap = 3072, maxp = 256;
      p->schunk.clear(); p->schunk.push_back(0);
      p->schunk_terms_max = 0; p->schunk_pairs_max = 0;
      long long a0 = 0;
      while (a0 < total) {
        long long a1 = a0 + 1;      // a single pair always fits: its four lists hold at most 4 * (2 n_end) * ... terms, checked at launch
        while (a1 < total && a1 - a0 < maxp && (long long)(p->qptr[4 * (a1 + 1)] - p->qptr[4 * a0]) <= cap) ++a1;
        const int nt = (int)(p->qptr[4 * a1] - p->qptr[4 * a0]);
        if (nt > p->schunk_terms_max) p->schunk_terms_max = nt;
        if ((int)(a1 - a0) > p->schunk_pairs_max) p->schunk_pairs_max = (int)(a1 - a0);
        p->schunk.push_back((int)a1);
        a0 = a1;
      }
    }
  }
  return BIEM_OK;
}

// ---- chain trees "b" * (d - 2) + "a" ----------------------------------------------------------
// n-point Gauss-Jacobi(a, a) rule (weight (1-x^2)^a; a = 0, 1/2 take the rules above, so a chain plan of ba / bba has their rule):
// nodes by Sturm-sequence bisection on the Jacobi matrix of the orthonormal Gegenbauer polynomials (lam = a + 1/2), weights by
// the Christoffel numbers 1 / sum_{k<n} p_k(x)^2
static void gauss_sym(int n, double a, std::vector<double>& t, std::vector<double>& w) {
  if (a == 0.0) { gauss_legendre(n, t, w); return; }
  if (a == 0.5) { gauss_cheb2(n, t, w); return; }
  const double lam = a + 0.5;
  std::vector<double> b2(n, 0.0);                 // squared off-diagonal a_k^2, k = 1 .. n-1
  for (int k = 1; k < n; ++k) b2[k] = 0.25 * (double)k * (k + 2.0 * lam - 1.0) / ((k + lam - 1.0) * (k + lam));
  auto below = [&](double x) {                    // number of eigenvalues < x
    int cnt = 0; double q = -x;
    if (q < 0) ++cnt;
    for (int k = 1; k < n; ++k) {
      if (q == 0.0) q = 1e-300;
      q = -x - b2[k] / q;
      if (q < 0) ++cnt;
    }
    return cnt;
  };
  t.assign(n, 0.0); w.assign(n, 0.0);
  const double h0 = sqrt(kPi) * exp(lgamma(lam + 0.5) - lgamma(lam + 1.0));
  for (int i = 0; i < n; ++i) {
    double lo = -1.0, hi = 1.0;
    for (int it = 0; it < 200 && hi - lo > 0.0; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (mid <= lo || mid >= hi) break;
      if (below(mid) > i) hi = mid; else lo = mid;
    }
    const double x = 0.5 * (lo + hi);
    t[i] = x;
    double p0 = 1.0 / sqrt(h0), s = p0 * p0, p1 = 0.0, aprev = 0.0;
    for (int k = 1; k < n; ++k) {
      const double ak = sqrt(b2[k]);
      const double p2 = (x * p0 - aprev * p1) / ak;
      p1 = p0; p0 = p2; aprev = ak; s += p0 * p0;
    }
    w[i] = 1.0 / s;
  }
}

// labels of degree < n in n-major order: (n, l_1 .. l_{d-3}, m), each label entry from 0 to the previous one, m from -l to l
static void chain_labels(int d, int n, std::vector<int>& lab, std::vector<int>& deg) {
  lab.clear(); deg.clear();
  const int lw = d - 1;
  std::vector<int> cur(lw, 0);
  std::function<void(int, int)> rec = [&](int j, int up) {
    if (j == lw - 1) {
      for (int m = -up; m <= up; ++m) { cur[j] = m; lab.insert(lab.end(), cur.begin(), cur.end()); deg.push_back(cur[0]); }
      return;
    }
    for (int l = 0; l <= up; ++l) { cur[j] = l; rec(j + 1, l); }
  };
  for (int q = 0; q < n; ++q) { cur[0] = q; rec(1, q); }
}

int plan_build_chain_host(biem_plan* p, int d, int n_end) {
  if (d < 3 || d > kChainDimMax) { set_error("unsupported chain tree dimension d=%d (built: 3 <= d <= %d)", d, kChainDimMax); return BIEM_ERR_UNSUPPORTED; }
  if (n_end < 1) { set_error("n_end=%d out of range", n_end); return BIEM_ERR_ARG; }
  const int n2 = 2 * n_end - 1, lw = d - 1;
  const long long H2ll = harm_count_d(d, n2);
  // every 16-bit index the fills keep (tidx16, qidx16, q2idx16, ridx) addresses the H2 table labels or fewer
  if (H2ll > 65535) {
    set_error("chain tree d=%d n_end=%d: %lld table labels (degree < 2 n_end - 1) exceed the 16-bit table index limit 65535 of the fill", d, n_end, H2ll);
    return BIEM_ERR_UNSUPPORTED;
  }
  // the chain kernels keep (d - 2) node tables of n2 x n2 doubles in LDS (pair tables) and the radial functions up to order n2 + shift
  if ((long long)(d - 2) * n2 * n2 > kChainNodeTab || n2 + kRadShiftMax + 6 > 2 * 320) {
    set_error("chain tree d=%d n_end=%d: the node tables (%d x %d x %d doubles) exceed the chain kernels' LDS limit %d", d, n_end, d - 2, n2, n2, kChainNodeTab);
    return BIEM_ERR_UNSUPPORTED;
  }
  p->tree = TREE_CHAIN; p->d = d; p->lw = lw; p->n_end = n_end; p->n2 = n2;
  p->H = (int)harm_count_d(d, n_end); p->H2 = (int)H2ll;
  p->Cd = pow(2.0 * kPi, 0.5 * d) * sqrt(2.0 / kPi);
  chain_labels(d, n_end, p->labels, p->deg);
  chain_labels(d, n2, p->labels2, p->deg2);
  const int H = p->H, n = n_end, np = d - 2;        // np polar nodes
  auto lab = [&](const std::vector<int>& L, int h, int j) { return j < lw - 1 ? L[(size_t)lw * h + j] : iabs(L[(size_t)lw * h + lw - 1]); };
  {
    // conjugate partners: the azimuthal order negated
    std::map<std::vector<int>, int> pos;
    for (int h = 0; h < H; ++h) pos[std::vector<int>(&p->labels[(size_t)lw * h], &p->labels[(size_t)lw * h] + lw)] = h;
    p->units.clear();
    for (int h = 0; h < H; ++h) {
      std::vector<int> c(&p->labels[(size_t)lw * h], &p->labels[(size_t)lw * h] + lw);
      c[lw - 1] = -c[lw - 1];
      auto it = pos.find(c);
      if (it == pos.end()) { set_error("internal: harmonic %d has no conjugate partner", h); return BIEM_ERR_ARG; }
      if (h <= it->second) { p->units.push_back(h); p->units.push_back(it->second); }
    }
  }
  // ---- boundary-data quadrature: n-point Gauss-Jacobi((d-j-3)/2, (d-j-3)/2) at polar node j, 2 n equispaced azimuths ----
  std::vector<std::vector<double>> tq(np), wq(np);
  for (int j = 0; j < np; ++j) gauss_sym(n, 0.5 * (d - j - 3), tq[j], wq[j]);
  const int na = 2 * n;
  long long Qll = na;
  for (int j = 0; j < np; ++j) Qll *= n;
  if (Qll * H > (1LL << 31)) { set_error("chain tree d=%d n_end=%d: projection matrix of %lld x %d entries too large", d, n_end, Qll, H); return BIEM_ERR_UNSUPPORTED; }
  p->Q = (int)Qll;
  p->qy.resize((size_t)p->Q * d); p->qw.resize(p->Q);
  // node factors of the harmonics at the rule's nodes: Fq[j][i][L][L1], L < n_end
  std::vector<double> Fq((size_t)np * n * n * n, 0.0);
  for (int j = 0; j < np; ++j)
    for (int i = 0; i < n; ++i) {
      const double c = tq[j][i], s = sqrt(1.0 - c * c);
      for (int L = 0; L < n; ++L) for (int L1 = 0; L1 <= L; ++L1) Fq[(((size_t)j * n + i) * n + L) * n + L1] = chain_node_factor(d, j, L, L1, c, s);
    }
  p->W.resize((size_t)p->Q * H * 2);
  std::vector<int> idx(np, 0);
  for (int q = 0; q < p->Q; ++q) {
    int r = q / na; const int jp = q % na;
    for (int j = np - 1; j >= 0; --j) { idx[j] = r % n; r /= n; }
    double* y = &p->qy[(size_t)q * d];
    double sp = 1.0, wt = kPi / n;
    for (int j = 0; j < np; ++j) {
      const double c = tq[j][idx[j]];
      y[j] = sp * c; sp *= sqrt(1.0 - c * c); wt *= wq[j][idx[j]];
    }
    const double ph = jp * kPi / n;
    y[d - 2] = sp * cos(ph); y[d - 1] = sp * sin(ph);
    p->qw[q] = wt;
    for (int h = 0; h < H; ++h) {
      double amp = kInvSqrt2Pi;
      for (int j = 0; j < np; ++j) amp *= Fq[(((size_t)j * n + idx[j]) * n + lab(p->labels, h, j)) * n + lab(p->labels, h, j + 1)];
      const double ang = p->labels[(size_t)lw * h + lw - 1] * ph;
      p->W[((size_t)q * H + h) * 2] = wt * amp * cos(ang);
      p->W[((size_t)q * H + h) * 2 + 1] = -wt * amp * sin(ang);
    }
  }
  // ---- translation terms ----
  // int Y' conj(Y) conj(Y'') = delta(m'' = m' - m) / sqrt(2 pi) * prod_j I_j, I_j = int (1-x^2)^{(d-j-3)/2} f'_j f_j f''_j dx over
  // the node factors f_j = sin^{l_{j+1}} Gbar_{l_j - l_{j+1}}: for the kept terms the powers of sin sum to an even number, so the
  // integrand is a polynomial of degree <= 4 n_end - 4 times the weight and the 2 n_end-point Gauss-Jacobi rule of the node is exact.
  // Terms are selected by the selection rules alone - at every node the triangle |l_j - l'_j| <= l''_j <= l_j + l'_j (l''_{j+1} <= l''_j)
  // and an even (l_j - l_{j+1}) + (l'_j - l'_{j+1}) + (l''_j - l''_{j+1}); at the azimuth |m''| <= l''_{d-3}.
  const int nq = 2 * n;
  std::vector<double> Ft((size_t)np * n2 * n2 * nq, 0.0), wt_((size_t)np * nq);
  for (int j = 0; j < np; ++j) {
    std::vector<double> t, w; gauss_sym(nq, 0.5 * (d - j - 3), t, w);
    for (int i = 0; i < nq; ++i) {
      wt_[(size_t)j * nq + i] = w[i];
      const double c = t[i], s = sqrt(1.0 - c * c);
      for (int L = 0; L < n2; ++L) for (int L1 = 0; L1 <= L; ++L1) Ft[(((size_t)j * n2 + L) * n2 + L1) * nq + i] = chain_node_factor(d, j, L, L1, c, s);
    }
  }
  auto node_int = [&](int j, int a0, int a1, int b0, int b1, int c0, int c1) {
    const double* fa = &Ft[(((size_t)j * n2 + a0) * n2 + a1) * nq];
    const double* fb = &Ft[(((size_t)j * n2 + b0) * n2 + b1) * nq];
    const double* fc = &Ft[(((size_t)j * n2 + c0) * n2 + c1) * nq];
    const double* w = &wt_[(size_t)j * nq];
    double acc = 0.0;
    for (int i = 0; i < nq; ++i) acc += w[i] * fa[i] * fb[i] * fc[i];
    return acc;
  };
  std::unordered_map<unsigned long long, int> pos2;           // label key -> index among the degrees < n2
  const unsigned long long base = 2ULL * n2 + 1;
  auto key = [&](const int* l) { unsigned long long k = 0; for (int j = 0; j < lw; ++j) k = k * base + (unsigned long long)(l[j] + n2); return k; };
  for (int l = 0; l < p->H2; ++l) pos2[key(&p->labels2[(size_t)lw * l])] = l;
  p->lists_built = true;
  p->ptr.assign((size_t)H * H + 1, 0);
  p->coef.clear(); p->tidx.clear();
  std::vector<int> a(np + 1), b(np + 1), c(lw);
  std::vector<double> pre(np + 1);
  bool too_many = false;
  for (int h = 0; h < H && !too_many; ++h)
    for (int hp = 0; hp < H; ++hp) {
      for (int j = 0; j <= np; ++j) { b[j] = lab(p->labels, h, j); a[j] = lab(p->labels, hp, j); }
      const int m = p->labels[(size_t)lw * h + lw - 1], mp = p->labels[(size_t)lw * hp + lw - 1], mu = mp - m;
      c[lw - 1] = mu;
      // choose l''_j node by node; pre[j] = product of the node integrals 0 .. j-1
      std::function<void(int)> rec = [&](int j) {
        const int lo = iabs(a[j] - b[j]), hi = std::min(a[j] + b[j], j == 0 ? n2 - 1 : c[j - 1]);
        for (int l2 = lo; l2 <= hi; ++l2) {
          if (j > 0 && (((a[j - 1] - a[j]) + (b[j - 1] - b[j]) + (c[j - 1] - l2)) & 1)) continue;
          c[j] = l2;
          pre[j] = j == 0 ? 1.0 : pre[j - 1] * node_int(j - 1, a[j - 1], a[j], b[j - 1], b[j], c[j - 1], l2);
          if (j < np - 1) { rec(j + 1); continue; }
          // last polar node: l''_{d-2} = |m''|
          if (l2 < iabs(mu) || (((a[j] - a[j + 1]) + (b[j] - b[j + 1]) + (l2 - iabs(mu))) & 1)) continue;
          const double v = pre[j] * node_int(j, a[j], a[j + 1], b[j], b[j + 1], l2, iabs(mu));
          p->coef.push_back(isign_even(b[0] + c[0] - a[0]) * v * kInvSqrt2Pi);
          p->tidx.push_back(pos2.at(key(c.data())));
        }
      };
      rec(0);
      if (p->coef.size() > 0x7fffffffULL) { too_many = true; break; }
      p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
    }
  if (too_many) { set_error("chain tree d=%d n_end=%d: more than 2^31 translation terms", d, n_end); return BIEM_ERR_UNSUPPORTED; }
  return plan_build_tail(p);
}

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s failed: %s", #x, hipGetErrorString(e_)); return BIEM_ERR_HIP; } } while (0)

template <class T> static int up(T** dst, const std::vector<T>& src) {
  if (src.empty()) { *dst = nullptr; return BIEM_OK; }
  HIPCHK(hipMalloc((void**)dst, src.size() * sizeof(T)));
  HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return BIEM_OK;
}

int plan_upload(biem_plan* p) {
  if (p->device >= 0) return BIEM_OK;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  int rc;
  if ((rc = up(&p->d_labels, p->labels))) return rc;
  if ((rc = up(&p->d_deg, p->deg))) return rc;
  if ((rc = up(&p->d_labels2, p->labels2))) return rc;
  if ((rc = up(&p->d_deg2, p->deg2))) return rc;
  if ((rc = up(&p->d_units, p->units))) return rc;
  if ((rc = up(&p->d_W, p->W))) return rc;
  if ((rc = up(&p->d_ptr, p->ptr))) return rc;
  if ((rc = up(&p->d_coef, p->coef))) return rc;
  if ((rc = up(&p->d_tidx, p->tidx))) return rc;
  if ((rc = up(&p->d_tidx16, p->tidx16))) return rc;
  if ((rc = up(&p->d_chunk_ent, p->chunk_ent))) return rc;
  if ((rc = up(&p->d_spos, p->spos))) return rc;
  if ((rc = up(&p->d_hpos, p->hpos))) return rc;
  if ((rc = up(&p->d_qptr, p->qptr))) return rc;
  if ((rc = up(&p->d_qcoef, p->qcoef))) return rc;
  if ((rc = up(&p->d_qidx16, p->qidx16))) return rc;
  if ((rc = up(&p->d_qchunk, p->qchunk))) return rc;
  if ((rc = up(&p->d_schunk, p->schunk))) return rc;
  if ((rc = up(&p->d_lin2, p->lin2))) return rc;
  if ((rc = up(&p->d_q2ptr, p->q2ptr))) return rc;
  if ((rc = up(&p->d_q2coef, p->q2coef))) return rc;
  if ((rc = up(&p->d_q2idx16, p->q2idx16))) return rc;
  if ((rc = up(&p->d_red_of, p->red_of))) return rc;
  if ((rc = up(&p->d_red_first, p->red_first))) return rc;
  if ((rc = up(&p->d_red_label, p->red_label))) return rc;
  if ((rc = up(&p->d_ph_mu, p->ph_mu))) return rc;
  if ((rc = up(&p->d_rcoef, p->rcoef))) return rc;
  if ((rc = up(&p->d_ridx, p->ridx))) return rc;
  if ((rc = up(&p->d_rphsel, p->rphsel))) return rc;
  if ((rc = up(&p->d_rchunk, p->rchunk))) return rc;
  if ((rc = up(&p->d_rcrow, p->rcrow))) return rc;
  if ((rc = up(&p->d_rwrow, p->rwrow))) return rc;
  p->device = dev;
  return BIEM_OK;
}

// ---- coupling table of the radiation force ------------------------------------------------------
// T^i_{h'h} = sum_q w_q y_i(q) Y_h(q) conj(Y_h'(q)) with the plan's own boundary-data rule and harmonics (W = w conj Y).  A kept entry
// has |n - n'| = 1, so its integrand is a polynomial of degree n + n' + 1 <= 2 n_end - 2: within the exactness of the rule, which
// projects data of degree < n_end onto harmonics of degree < n_end (degree 2 n_end - 2 as well) at every node of every tree.
// Candidates: |n - n'| = 1 and every label entry differing by at most 1 - y_i is a harmonic of degree 1, of degree <= 1 in every
// sub-sphere of the tree and of azimuthal orders <= 1, so the product y_i Y_h has no other components.
int plan_build_force(biem_plan* p) {
  static std::mutex mtx;
  std::lock_guard<std::mutex> lock(mtx);
  if (!p->force_built) {
    const int H = p->H, d = p->d, lw = p->lw, Q = p->Q;
    std::vector<std::vector<int>> cand(H);
    for (int hp = 0; hp < H; ++hp)
      for (int h = 0; h < H; ++h) {
        if (iabs(p->deg[h] - p->deg[hp]) != 1) continue;
        bool near = true;
        for (int j = 0; j < lw && near; ++j) near = iabs(p->labels[(size_t)lw * h + j] - p->labels[(size_t)lw * hp + j]) <= 1;
        if (near) cand[hp].push_back(h);
      }
    std::vector<size_t> first(H + 1, 0);
    for (int hp = 0; hp < H; ++hp) first[hp + 1] = first[hp] + cand[hp].size();
    std::vector<double> acc(first[H] * d * 2, 0.0);                   // [candidate][component] complex
    for (int q = 0; q < Q; ++q) {
      const double* Wq = &p->W[(size_t)q * H * 2];
      const double* y = &p->qy[(size_t)q * d];
      const double iw = 1.0 / p->qw[q];
      for (int hp = 0; hp < H; ++hp) {
        const double ar = Wq[2 * hp] * iw, ai = Wq[2 * hp + 1] * iw;  // conj(Y_h') (one weight taken back out)
        double* a = &acc[first[hp] * d * 2];
        for (int h : cand[hp]) {
          const double br = Wq[2 * h], bi = -Wq[2 * h + 1];          // w Y_h
          const double vr = ar * br - ai * bi, vi = ar * bi + ai * br;
          for (int i = 0; i < d; ++i) { a[2 * i] += y[i] * vr; a[2 * i + 1] += y[i] * vi; }
          a += 2 * d;
        }
      }
    }
    p->fptr.assign(H + 1, 0); p->fptr_comp.assign((size_t)H * d + 1, 0);
    p->fcol.clear(); p->fcomp.clear(); p->fval.clear();
    for (int hp = 0; hp < H; ++hp) {
      for (int i = 0; i < d; ++i) {
        for (size_t c = 0; c < cand[hp].size(); ++c) {
          const double vr = acc[((first[hp] + c) * d + i) * 2], vi = acc[((first[hp] + c) * d + i) * 2 + 1];
          const double mag = hypot(vr, vi);
          // the values are O(1) algebraic numbers or exact zeros: anything between is a rule that was not exact
          if (mag > 1e-14 && mag < 1e-10) {
            set_error("internal: force coupling entry (%d, %d) component %d of tree %d n_end %d has the size %.3e of neither a value nor rounding",
                      hp, cand[hp][c], i, p->tree, p->n_end, mag);
            p->fptr.clear(); p->fptr_comp.clear(); p->fcol.clear(); p->fcomp.clear(); p->fval.clear();
            return BIEM_ERR_ARG;
          }
          if (mag <= 1e-14) continue;
          p->fcol.push_back(cand[hp][c]); p->fcomp.push_back(i); p->fval.push_back(vr); p->fval.push_back(vi);
        }
        p->fptr_comp[(size_t)hp * d + i + 1] = (uint32_t)p->fcol.size();
      }
      p->fptr[hp + 1] = (uint32_t)p->fcol.size();
    }
    p->force_built = true;
  }
  if (p->device >= 0 && !p->force_uploaded) {
    int rc;
    if (!p->d_fptr_comp && (rc = up(&p->d_fptr_comp, p->fptr_comp))) return rc;
    if (!p->d_fcol && (rc = up(&p->d_fcol, p->fcol))) return rc;
    if (!p->d_fval && (rc = up(&p->d_fval, p->fval))) return rc;
    p->force_uploaded = true;
  }
  return BIEM_OK;
}

void plan_free(biem_plan* p) {
  if (p->device >= 0) {
    (void)hipFree(p->d_fptr_comp); (void)hipFree(p->d_fcol); (void)hipFree(p->d_fval);
    (void)hipFree(p->d_labels); (void)hipFree(p->d_deg); (void)hipFree(p->d_labels2); (void)hipFree(p->d_deg2); (void)hipFree(p->d_units);
    (void)hipFree(p->d_W); (void)hipFree(p->d_ptr); (void)hipFree(p->d_coef); (void)hipFree(p->d_tidx);
    (void)hipFree(p->d_tidx16); (void)hipFree(p->d_chunk_ent);
    (void)hipFree(p->d_spos); (void)hipFree(p->d_hpos); (void)hipFree(p->d_qptr); (void)hipFree(p->d_qcoef); (void)hipFree(p->d_qidx16);
    (void)hipFree(p->d_qchunk); (void)hipFree(p->d_schunk);
    (void)hipFree(p->d_lin2); (void)hipFree(p->d_q2ptr); (void)hipFree(p->d_q2coef); (void)hipFree(p->d_q2idx16);
    (void)hipFree(p->d_red_of); (void)hipFree(p->d_red_first); (void)hipFree(p->d_red_label); (void)hipFree(p->d_ph_mu);
    (void)hipFree(p->d_rcoef); (void)hipFree(p->d_ridx); (void)hipFree(p->d_rphsel); (void)hipFree(p->d_rchunk); (void)hipFree(p->d_rcrow); (void)hipFree(p->d_rwrow);
  }
  delete p;
}

}  // namespace biem
