// plan_tree.cpp -- what a plan holds per coordinate tree: labels, conjugate units, boundary-data quadrature, projection matrix and the
// translation term lists (pure C++).  One function per tree for the quadrature and one for the term lists, each reached through one
// switch; the fill tables behind them are the same for every tree (plan_fill.cpp).
#include "plan_build.hpp"
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>

namespace biem {

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

// ---- the partner rule and the azimuth rule --------------------------------------------------
// the label entries that hold azimuthal orders (the tree's type-a nodes): one, two for caa
static int azimuthal_slots(int tree, int lw, int slot[2]) {
  switch (tree) {
    case TREE_A: slot[0] = 0; return 1;
    case TREE_BA: slot[0] = 1; return 1;
    case TREE_BBA: slot[0] = 2; return 1;
    case TREE_CHAIN: slot[0] = lw - 1; return 1;
    default: slot[0] = 1; slot[1] = 2; return 2;   // caa
  }
}
void conjugate_label(int tree, int lw, int* label) {
  int slot[2];
  for (int i = azimuthal_slots(tree, lw, slot); i-- > 0;) label[slot[i]] = -label[slot[i]];
}
void azimuthal_orders(int tree, int lw, const int* label, int& m1, int& m2) {
  int slot[2];
  const int ns = azimuthal_slots(tree, lw, slot);
  m1 = label[slot[0]]; m2 = ns > 1 ? label[slot[1]] : 0;
}
bool conjugate_partners(int tree, int lw, const std::vector<int>& labels, int count, std::vector<int>& partner) {
  std::map<std::vector<int>, int> pos;
  for (int l = 0; l < count; ++l) pos[std::vector<int>(&labels[(size_t)lw * l], &labels[(size_t)lw * l] + lw)] = l;
  partner.assign(count, -1);
  for (int l = 0; l < count; ++l) {
    std::vector<int> c(&labels[(size_t)lw * l], &labels[(size_t)lw * l] + lw);
    conjugate_label(tree, lw, c.data());
    auto it = pos.find(c);
    if (it == pos.end()) return false;
    partner[l] = it->second;
  }
  return true;
}

// writes units; reads tree, lw, H, labels
static int build_units(biem_plan* p) {
  std::vector<int> partner;
  p->units.clear();
  if (!conjugate_partners(p->tree, p->lw, p->labels, p->H, partner)) {
    set_error("internal: harmonic %d has no conjugate partner", (int)(std::find(partner.begin(), partner.end(), -1) - partner.begin()));
    return BIEM_ERR_ARG;
  }
  for (int h = 0; h < p->H; ++h) if (h <= partner[h]) { p->units.push_back(h); p->units.push_back(partner[h]); }
  return BIEM_OK;
}

// ---- boundary-data quadrature: each writes Q, qy, qw; reads d, n_end (the chain rule H as well) --------------------------
static void quad_resize(biem_plan* p, int Q) { p->Q = Q; p->qy.resize((size_t)Q * p->d); p->qw.resize(Q); }

static void quadrature_a(biem_plan* p) {
  const int n = p->n_end, na = 2 * n;
  quad_resize(p, na);
  for (int j = 0; j < na; ++j) { double ph = j * kPi / n; p->qy[2 * j] = cos(ph); p->qy[2 * j + 1] = sin(ph); p->qw[j] = kPi / n; }
}
static void quadrature_ba(biem_plan* p) {
  const int n = p->n_end, na = 2 * n;
  std::vector<double> t0, w0;
  gauss_legendre(n, t0, w0);
  quad_resize(p, n * na);
  for (int i = 0; i < n; ++i) for (int j = 0; j < na; ++j) {
    int q = i * na + j; double ph = j * kPi / n, s = sqrt(1.0 - t0[i] * t0[i]);
    p->qy[3 * q] = t0[i]; p->qy[3 * q + 1] = s * cos(ph); p->qy[3 * q + 2] = s * sin(ph);
    p->qw[q] = w0[i] * kPi / n;
  }
}
static void quadrature_caa(biem_plan* p) {
  const int n = p->n_end, na = 2 * n;
  std::vector<double> t0, w0;
  // type-c root over two type-a children: sin t cos t dt = dx / 4 with x = cos 2t -> Gauss-Legendre in x (pinned by the
  // jascome caa goldens); both azimuths 2 n_end equispaced points
  gauss_legendre(n, t0, w0);
  quad_resize(p, n * na * na);
  for (int i = 0; i < n; ++i) for (int j1 = 0; j1 < na; ++j1) for (int j2 = 0; j2 < na; ++j2) {
    int q = (i * na + j1) * na + j2;
    double th = 0.5 * acos(t0[i]), p1 = j1 * kPi / n, p2 = j2 * kPi / n;
    p->qy[4 * q] = cos(th) * cos(p1); p->qy[4 * q + 1] = cos(th) * sin(p1);
    p->qy[4 * q + 2] = sin(th) * cos(p2); p->qy[4 * q + 3] = sin(th) * sin(p2);
    p->qw[q] = 0.25 * w0[i] * (kPi / n) * (kPi / n);
  }
}
static void quadrature_bba(biem_plan* p) {
  const int n = p->n_end, na = 2 * n;
  std::vector<double> t0, w0, t1, w1;
  gauss_cheb2(n, t0, w0); gauss_legendre(n, t1, w1);
  quad_resize(p, n * n * na);
  for (int i = 0; i < n; ++i) for (int l = 0; l < n; ++l) for (int j = 0; j < na; ++j) {
    int q = (i * n + l) * na + j; double ph = j * kPi / n;
    double s0 = sqrt(1.0 - t0[i] * t0[i]), s1 = sqrt(1.0 - t1[l] * t1[l]);
    p->qy[4 * q] = t0[i]; p->qy[4 * q + 1] = s0 * t1[l]; p->qy[4 * q + 2] = s0 * s1 * cos(ph); p->qy[4 * q + 3] = s0 * s1 * sin(ph);
    p->qw[q] = w0[i] * w1[l] * kPi / n;
  }
}

// the chain rule: n-point Gauss-Jacobi((d-j-3)/2, (d-j-3)/2) at polar node j, 2 n equispaced azimuths (the last index of a point)
static void chain_polar_rules(int d, int n, std::vector<std::vector<double>>& tq, std::vector<std::vector<double>>& wq) {
  tq.resize(d - 2); wq.resize(d - 2);
  for (int j = 0; j < d - 2; ++j) gauss_sym(n, 0.5 * (d - j - 3), tq[j], wq[j]);
}
// polar node indices idx[] of quadrature point q; returns its azimuth index
static int chain_point(int q, int n, std::vector<int>& idx) {
  int r = q / (2 * n);
  for (int j = (int)idx.size() - 1; j >= 0; --j) { idx[j] = r % n; r /= n; }
  return q % (2 * n);
}
static int quadrature_chain(biem_plan* p) {
  const int d = p->d, n = p->n_end, np = d - 2;
  std::vector<std::vector<double>> tq, wq;
  chain_polar_rules(d, n, tq, wq);
  long long Qll = 2 * n;
  for (int j = 0; j < np; ++j) Qll *= n;
  if (Qll * p->H > (1LL << 31)) { set_error("chain tree d=%d n_end=%d: projection matrix of %lld x %d entries too large", d, n, Qll, p->H); return BIEM_ERR_UNSUPPORTED; }
  quad_resize(p, (int)Qll);
  std::vector<int> idx(np, 0);
  for (int q = 0; q < p->Q; ++q) {
    const int jp = chain_point(q, n, idx);
    double* y = &p->qy[(size_t)q * d];
    double sp = 1.0, wt = kPi / n;
    for (int j = 0; j < np; ++j) {
      const double c = tq[j][idx[j]];
      y[j] = sp * c; sp *= sqrt(1.0 - c * c); wt *= wq[j][idx[j]];
    }
    const double ph = jp * kPi / n;
    y[d - 2] = sp * cos(ph); y[d - 1] = sp * sin(ph);
    p->qw[q] = wt;
  }
  return BIEM_OK;
}
static int build_quadrature(biem_plan* p) {
  switch (p->tree) {
    case TREE_A: quadrature_a(p); break;
    case TREE_BA: quadrature_ba(p); break;
    case TREE_BBA: quadrature_bba(p); break;
    case TREE_CAA: quadrature_caa(p); break;
    default: return quadrature_chain(p);
  }
  return BIEM_OK;
}

// ---- projection matrix W[q][h] = w_q conj(Y_h(y_q)): writes W; reads tree, d, H, Q, labels, qy, qw ----
// entry j of label h of a chain tree as a degree: the azimuthal order by its magnitude
static inline int chain_deg(const std::vector<int>& L, int lw, int h, int j) { return j < lw - 1 ? L[(size_t)lw * h + j] : iabs(L[(size_t)lw * h + lw - 1]); }

static void projection_chain(biem_plan* p) {
  const int d = p->d, n = p->n_end, np = d - 2, lw = p->lw, H = p->H;
  std::vector<std::vector<double>> tq, wq;
  chain_polar_rules(d, n, tq, wq);
  // node factors of the harmonics at the rule's nodes: Fq[j][i][L][L1], L < n_end
  std::vector<double> Fq((size_t)np * n * n * n, 0.0);
  for (int j = 0; j < np; ++j)
    for (int i = 0; i < n; ++i) {
      const double c = tq[j][i], s = sqrt(1.0 - c * c);
      for (int L = 0; L < n; ++L) for (int L1 = 0; L1 <= L; ++L1) Fq[(((size_t)j * n + i) * n + L) * n + L1] = chain_node_factor(d, j, L, L1, c, s);
    }
  std::vector<int> idx(np, 0);
  for (int q = 0; q < p->Q; ++q) {
    const int jp = chain_point(q, n, idx);
    const double ph = jp * kPi / n, wt = p->qw[q];
    for (int h = 0; h < H; ++h) {
      double amp = kInvSqrt2Pi;
      for (int j = 0; j < np; ++j) amp *= Fq[(((size_t)j * n + idx[j]) * n + chain_deg(p->labels, lw, h, j)) * n + chain_deg(p->labels, lw, h, j + 1)];
      const double ang = p->labels[(size_t)lw * h + lw - 1] * ph;
      p->W[((size_t)q * H + h) * 2] = wt * amp * cos(ang);
      p->W[((size_t)q * H + h) * 2 + 1] = -wt * amp * sin(ang);
    }
  }
}
static void build_projection(biem_plan* p) {
  const int tree = p->tree, d = p->d, H = p->H;
  p->W.resize((size_t)p->Q * H * 2);
  if (tree == TREE_CHAIN) { projection_chain(p); return; }
  for (int q = 0; q < p->Q; ++q) {
    Dir dir = make_dir(tree, &p->qy[(size_t)q * d]);
    for (int h = 0; h < H; ++h) {
      double re, im;
      harmonic_single(tree, p->labels[3 * h], p->labels[3 * h + 1], p->labels[3 * h + 2], dir, &re, &im);
      p->W[((size_t)q * H + h) * 2] = p->qw[q] * re;
      p->W[((size_t)q * H + h) * 2 + 1] = -p->qw[q] * im;
    }
  }
}

// ---- translation terms: each appends coef, tidx and sets ptr per entry (h, h'); reads n_end, n2, H, labels, labels2 ----
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

static void terms_a(biem_plan* p) {
  const int H = p->H, n2 = p->n2;
  for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
    int m = p->labels[3 * h], mp = p->labels[3 * hp], mu = mp - m;
    p->coef.push_back(isign_even(iabs(m) + iabs(mu) - iabs(mp)) * kInvSqrt2Pi);
    p->tidx.push_back(mu >= 0 ? mu : (2 * n2 - 1) + mu);
    p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
  }
}
static void terms_ba(biem_plan* p) {
  const int H = p->H, n = p->n_end;
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
}
// ---- the 4-D trees: term lists of bba and caa through one per-entry function ------------------------------------------------
// Both trees keep, besides the label rules (triangle and parity in the degrees, the azimuthal deltas), polar triple integrals that
// vanish with no rule behind them (zeros of the recoupling coefficient of SO(4)), and integrals that do not vanish fall with the
// order without bound (3e-13 at bba n_end 24), so no constant separates the two.  The integrals are therefore taken in long double -
// nodes, weights, node tables and the sum - and one counts as zero where it lies within the rounding bound of its own sum,
// kZeroSlack nq eps sum |w a b c|; everything else is a term.  The double that the list carries is that sum rounded once.
// The bound is 1.7e-16 of sum |w a b c| at n_end 24 (64-bit mantissa), and the smallest integrals that do not vanish fall by about 60
// for every three orders (5e-14 at bba n_end 24), so they reach it near n_end 30: from there on real terms are taken for zeros again -
// terms below 1e-15, far under what a double-precision contraction resolves, but that is the ceiling of this selection.
typedef long double ldbl;
static const ldbl kPiL = 3.14159265358979323846264338327950288L;
static const ldbl kZeroSlack = 32.0L;

static void gauss_legendre_l(int n, std::vector<ldbl>& t, std::vector<ldbl>& w) {
  t.assign(n, 0.0L); w.assign(n, 0.0L);
  for (int i = 0; i < n; ++i) {
    ldbl x = cosl(kPiL * (i + 0.75L) / (n + 0.5L)), pp = 1.0L;
    for (int it = 0; it < 100; ++it) {
      ldbl p0 = 1.0L, p1 = x;
      for (int k = 2; k <= n; ++k) { ldbl p2 = ((2.0L * k - 1.0L) * x * p1 - (k - 1.0L) * p0) / k; p0 = p1; p1 = p2; }
      pp = n * (x * p1 - p0) / (x * x - 1.0L);
      const ldbl dx = p1 / pp;
      x -= dx;
      if (it > 2 && fabsl(dx) < 4.0L * std::numeric_limits<ldbl>::epsilon()) break;
    }
    ldbl p0 = 1.0L, p1 = x;
    for (int k = 2; k <= n; ++k) { ldbl p2 = ((2.0L * k - 1.0L) * x * p1 - (k - 1.0L) * p0) / k; p0 = p1; p1 = p2; }
    pp = n * (x * p1 - p0) / (x * x - 1.0L);
    t[n - 1 - i] = x;                         // ascending
    w[n - 1 - i] = 2.0L / ((1.0L - x * x) * pp * pp);
  }
}
// pbar_single, gbar_single, cbar_single (special.hpp) in long double
static ldbl pbar_l(int n, int m, ldbl x, ldbl s) {
  ldbl pmm = sqrtl(0.5L);
  for (int i = 1; i <= m; ++i) pmm *= sqrtl((ldbl)(2 * i + 1) / (ldbl)(2 * i)) * s;
  if (n == m) return pmm;
  ldbl p1 = sqrtl((ldbl)(2 * m + 3)) * x * pmm, p0 = pmm;
  for (int q = m + 2; q <= n; ++q) {
    const ldbl a = sqrtl((ldbl)(4 * q * q - 1) / (ldbl)(q * q - m * m));
    const ldbl b = sqrtl((ldbl)((q - 1) * (q - 1) - m * m) / (ldbl)(4 * (q - 1) * (q - 1) - 1));
    const ldbl p2 = a * (x * p1 - b * p0);
    p0 = p1; p1 = p2;
  }
  return p1;
}
static ldbl gbar_l(int k, int l, ldbl x) {
  ldbl h0 = 0.5L * kPiL;
  for (int i = 1; i <= l; ++i) h0 *= ((ldbl)i + 0.5L) / ((ldbl)i + 1.0L);
  const ldbl lam = (ldbl)(l + 1);
  ldbl p0 = 1.0L / sqrtl(h0);
  if (k == 0) return p0;
  const ldbl a1 = 0.5L * sqrtl((2.0L * lam) / (lam * (1.0L + lam)));
  ldbl p1 = x * p0 / a1, aprev = a1;
  for (int q = 2; q <= k; ++q) {
    const ldbl aq = 0.5L * sqrtl((ldbl)q * ((ldbl)q + 2.0L * lam - 1.0L) / (((ldbl)q + lam - 1.0L) * ((ldbl)q + lam)));
    const ldbl p2 = (x * p1 - aprev * p0) / aq;
    p0 = p1; p1 = p2; aprev = aq;
  }
  return p1;
}
static ldbl cbar_l(int n, int a, int b, ldbl c, ldbl s) {
  const int k = (n - a - b) / 2;
  const ldbl x = c * c - s * s, al = (ldbl)b, be = (ldbl)a;
  ldbl p0 = 1.0L, p1 = 1.0L;
  if (k >= 1) {
    p1 = (al + 1.0L) + 0.5L * (al + be + 2.0L) * (x - 1.0L);
    for (int m = 1; m < k; ++m) {
      const ldbl t = 2.0L * m + al + be;
      const ldbl p2 = ((t + 1.0L) * ((t + 2.0L) * t * x + al * al - be * be) * p1 - 2.0L * (m + al) * (m + be) * (t + 2.0L) * p0) /
                      (2.0L * (m + 1.0L) * (m + al + be + 1.0L) * t);
      p0 = p1; p1 = p2;
    }
  }
  ldbl r = 2.0L * (2.0L * k + a + b + 1.0L);
  for (int i = 1; i <= a; ++i) r *= (ldbl)(k + b + i) / (ldbl)(k + i);
  ldbl f = sqrtl(r);
  for (int i = 0; i < a; ++i) f *= c;
  for (int i = 0; i < b; ++i) f *= s;
  return f * p1;
}
// sum_i w a b c, exactly 0.0 where the sum is within its own rounding bound
static double resolved_sum(int nq, const ldbl* w, const ldbl* a, const ldbl* b, const ldbl* c, ldbl scale) {
  ldbl acc = 0.0L, mag = 0.0L;
  for (int i = 0; i < nq; ++i) { const ldbl t = w[i] * a[i] * b[i] * c[i]; acc += t; mag += fabsl(t); }
  if (fabsl(acc) <= kZeroSlack * nq * std::numeric_limits<ldbl>::epsilon() * mag) return 0.0;
  return (double)(acc * scale);
}

// One (tree, n_end) of bba / caa: labels, node tables, and the integral tables the entries share - one polar table per pair of
// unsigned labels {(q'l'), (ql)} over its (q''l''), one S^2 table per {(l'|m'|), (l|m|)} and sign of m'm over its l'' - each filled
// when an entry first asks for it.  The plan build walks every entry; biem_plan_entry_terms asks for one.
struct Terms4 {
  int tree = -1, n = 0, n2 = 0, nq = 0, H = 0;
  std::vector<int> labels, deg, labels2, deg2;
  std::vector<ldbl> wp, Tp;                     // polar rule and node table: bba Abar[(q n2 + l) nq + i]; caa cbar[row(q,a,b) nq + i]
  std::vector<ldbl> wl, Pl;                     // bba: Gauss-Legendre rule and Pbar[(l n2 + m) nq + i]
  std::vector<int> crow;                        // caa: (q n2 + a) n2 + b -> row of Tp
  std::unordered_map<int, int> pos2;            // caa: signed label -> index among the degrees < n2
  std::unordered_map<unsigned long long, std::vector<double>> polar, gaunt;

  static int skey(int q, int m1, int m2) { return (q * 256 + (m1 + 128)) * 256 + (m2 + 128); }

  void init(int tree_, int n_end) {
    tree = tree_; n = n_end; n2 = 2 * n - 1; nq = 2 * n;
    make_labels(tree, n, labels, deg);
    make_labels(tree, n2, labels2, deg2);
    H = (int)deg.size();
    if (tree == TREE_BBA) {
      // Gauss-Chebyshev-2: weight sqrt(1 - x^2) = one sin of sin^2 dtheta; the integrand is a polynomial of degree <= 4 n_end - 4
      wp.resize(nq); Tp.assign((size_t)n2 * n2 * nq, 0.0L);
      for (int i = 0; i < nq; ++i) {
        const ldbl th = (i + 1) * kPiL / (nq + 1), x = cosl(th), s = sinl(th);
        wp[i] = kPiL / (nq + 1) * s * s;
        for (int l = 0; l < n2; ++l) {
          ldbl sl = 1.0L; for (int j = 0; j < l; ++j) sl *= s;
          for (int q = l; q < n2; ++q) Tp[((size_t)q * n2 + l) * nq + i] = sl * gbar_l(q - l, l, x);
        }
      }
      std::vector<ldbl> t; gauss_legendre_l(nq, t, wl);
      Pl.assign((size_t)n2 * n2 * nq, 0.0L);
      for (int i = 0; i < nq; ++i) {
        const ldbl x = t[i], s = sqrtl(1.0L - x * x);
        for (int l = 0; l < n2; ++l) for (int m = 0; m <= l; ++m) Pl[((size_t)l * n2 + m) * nq + i] = pbar_l(l, m, x, s);
      }
    } else {
      // sin t cos t dt = dx / 4 with x = cos 2t; the integrand is a polynomial of degree <= 2 n_end - 2 in x
      std::vector<ldbl> xg; gauss_legendre_l(nq, xg, wp);
      for (int i = 0; i < nq; ++i) wp[i] *= 0.25L;
      crow.assign((size_t)n2 * n2 * n2, -1);
      int rows = 0;
      for (size_t l = 0; l < deg2.size(); ++l) {
        int& r = crow[((size_t)labels2[3 * l] * n2 + iabs(labels2[3 * l + 1])) * n2 + iabs(labels2[3 * l + 2])];
        if (r < 0) r = rows++;
        pos2[skey(labels2[3 * l], labels2[3 * l + 1], labels2[3 * l + 2])] = (int)l;
      }
      Tp.assign((size_t)rows * nq, 0.0L);
      for (int q = 0; q < n2; ++q) for (int a = 0; a <= q; ++a) for (int b = 0; a + b <= q; ++b) {
        const int r = crow[((size_t)q * n2 + a) * n2 + b];
        if (r < 0) continue;
        for (int i = 0; i < nq; ++i) Tp[(size_t)r * nq + i] = cbar_l(q, a, b, sqrtl(0.5L * (1.0L + xg[i])), sqrtl(0.5L * (1.0L - xg[i])));
      }
    }
  }

  // bba: A4 over (q'' from |q - q'| in steps of 2, l'' from |l - l'| in steps of 2 while l'' <= min(l + l', q'')), the order of entry()
  const std::vector<double>& polar_bba(int qp, int lp, int q, int l) {
    int ka = qp * n2 + lp, kb = q * n2 + l;
    if (ka > kb) std::swap(ka, kb);
    std::vector<double>& v = polar[(unsigned long long)ka * n2 * n2 + kb];
    if (!v.empty()) return v;
    const ldbl* a = &Tp[(size_t)ka * nq]; const ldbl* b = &Tp[(size_t)kb * nq];
    for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2)
      for (int l2 = iabs(l - lp); l2 <= l + lp && l2 <= q2; l2 += 2)
        v.push_back(resolved_sum(nq, wp.data(), a, b, &Tp[((size_t)q2 * n2 + l2) * nq], 1.0L));
    return v;
  }
  // bba: the real Gaunt-type integral over S^2 of Ybar' conj(Ybar) conj(Ybar''), m'' = m' - m, over l'' from |l - l'| in steps of 2
  const std::vector<double>& gaunt_bba(int lp, int mp, int l, int m) {
    const int mu = iabs(mp - m);
    int ka = lp * n2 + iabs(mp), kb = l * n2 + iabs(m);
    if (ka > kb) std::swap(ka, kb);
    std::vector<double>& v = gaunt[((unsigned long long)ka * n2 * n2 + kb) * 2 + (mu == iabs(mp) + iabs(m) ? 1 : 0)];
    if (!v.empty()) return v;
    const ldbl* a = &Pl[(size_t)ka * nq]; const ldbl* b = &Pl[(size_t)kb * nq];
    const ldbl inv_sqrt_2pi = 1.0L / sqrtl(2.0L * kPiL);
    for (int l2 = iabs(l - lp); l2 <= l + lp; l2 += 2)
      v.push_back(l2 < mu ? 0.0 : resolved_sum(nq, wl.data(), a, b, &Pl[((size_t)l2 * n2 + mu) * nq], inv_sqrt_2pi));
    return v;
  }
  // caa: int cbar' cbar cbar'' sin cos dt over q'' from |q - q'| in steps of 2, (a'', b'') = (|m1' - m1|, |m2' - m2|)
  const std::vector<double>& polar_caa(int qp, int m1p, int m2p, int q, int m1, int m2) {
    const int a3 = iabs(m1p - m1), b3 = iabs(m2p - m2);
    int ka = crow[((size_t)qp * n2 + iabs(m1p)) * n2 + iabs(m2p)], kb = crow[((size_t)q * n2 + iabs(m1)) * n2 + iabs(m2)];
    if (ka > kb) std::swap(ka, kb);
    const unsigned long long rows = Tp.size() / nq;
    std::vector<double>& v = polar[(((unsigned long long)ka * rows + kb) * 2 + (a3 == iabs(m1p) + iabs(m1) ? 1 : 0)) * 2 + (b3 == iabs(m2p) + iabs(m2) ? 1 : 0)];
    if (!v.empty()) return v;
    const ldbl* a = &Tp[(size_t)ka * nq]; const ldbl* b = &Tp[(size_t)kb * nq];
    for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2)
      v.push_back(q2 < a3 + b3 ? 0.0 : resolved_sum(nq, wp.data(), a, b, &Tp[(size_t)crow[((size_t)q2 * n2 + a3) * n2 + b3] * nq], 1.0L));
    return v;
  }

  // appends the terms of entry (row h, column h') to coef, tidx
  void entry(int h, int hp, std::vector<double>& coef, std::vector<int>& tidx) {
    const int q = labels[3 * h], qp = labels[3 * hp];
    if (tree == TREE_BBA) {
      const int l = labels[3 * h + 1], m = labels[3 * h + 2], lp = labels[3 * hp + 1], mp = labels[3 * hp + 2], mu = mp - m;
      const std::vector<double>& A4 = polar_bba(qp, lp, q, l);
      const std::vector<double>& G3 = gaunt_bba(lp, mp, l, m);
      size_t k = 0;
      for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2)
        for (int l2 = iabs(l - lp), j = 0; l2 <= l + lp && l2 <= q2; l2 += 2, ++j, ++k) {
          const double v = A4[k] * G3[j];
          if (v == 0.0) continue;               // a rule (l'' < |m''|) or a resolved zero of either integral
          coef.push_back(isign_even(q + q2 - qp) * v);
          tidx.push_back(q2 * (q2 + 1) * (2 * q2 + 1) / 6 + l2 * l2 + l2 + mu);
        }
    } else {
      // int Y' conj(Y) conj(Y'') = delta(m1'' = m1' - m1) delta(m2'' = m2' - m2) / (2 pi) * the polar integral
      const int m1 = labels[3 * h + 1], m2 = labels[3 * h + 2], m1p = labels[3 * hp + 1], m2p = labels[3 * hp + 2];
      const std::vector<double>& I3 = polar_caa(qp, m1p, m2p, q, m1, m2);
      size_t k = 0;
      for (int q2 = iabs(q - qp); q2 <= q + qp; q2 += 2, ++k) {
        if (I3[k] == 0.0) continue;             // the rule q'' < |m1''| + |m2''| or a resolved zero
        coef.push_back(isign_even(q + q2 - qp) * I3[k] / (2.0 * kPi));
        tidx.push_back(pos2.at(skey(q2, m1p - m1, m2p - m2)));
      }
    }
  }
};

static int terms_4d(biem_plan* p) {
  Terms4 t; t.init(p->tree, p->n_end);
  const int H = p->H;
  for (int h = 0; h < H; ++h) for (int hp = 0; hp < H; ++hp) {
    t.entry(h, hp, p->coef, p->tidx);
    if (p->coef.size() > 0xffffffffULL) { set_error("n_end=%d: more than 2^32 translation terms", p->n_end); return BIEM_ERR_UNSUPPORTED; }
    p->ptr[(size_t)h * H + hp + 1] = (uint32_t)p->coef.size();
  }
  return BIEM_OK;
}

// the term list of one entry of bba / caa without a plan; the tables of the last (tree, n_end) asked for are kept between calls
int plan_entry_terms(int tree, int n_end, int hp, int h, std::vector<double>& coef, std::vector<int>& tidx) {
  static std::mutex mu;
  static std::unique_ptr<Terms4> kept;
  if (tree != TREE_BBA && tree != TREE_CAA) { set_error("biem_plan_entry_terms: tree id %d (built: bba, caa)", tree); return BIEM_ERR_UNSUPPORTED; }
  if (n_end < 1 || n_end > 64) { set_error("biem_plan_entry_terms: n_end=%d out of range (1 .. 64)", n_end); return BIEM_ERR_ARG; }
  std::lock_guard<std::mutex> lock(mu);
  if (!kept || kept->tree != tree || kept->n != n_end) { kept.reset(new Terms4()); kept->init(tree, n_end); }
  if (h < 0 || h >= kept->H || hp < 0 || hp >= kept->H) { set_error("biem_plan_entry_terms: entry (%d, %d) outside the %d harmonics of n_end=%d", hp, h, kept->H, n_end); return BIEM_ERR_ARG; }
  coef.clear(); tidx.clear();
  kept->entry(h, hp, coef, tidx);
  return BIEM_OK;
}

// int Y' conj(Y) conj(Y'') = delta(m'' = m' - m) / sqrt(2 pi) * prod_j I_j, I_j = int (1-x^2)^{(d-j-3)/2} f'_j f_j f''_j dx over
// the node factors f_j = sin^{l_{j+1}} Gbar_{l_j - l_{j+1}}: for the kept terms the powers of sin sum to an even number, so the
// integrand is a polynomial of degree <= 4 n_end - 4 times the weight and the 2 n_end-point Gauss-Jacobi rule of the node is exact.
// Terms are selected by the selection rules alone - at every node the triangle |l_j - l'_j| <= l''_j <= l_j + l'_j (l''_{j+1} <= l''_j)
// and an even (l_j - l_{j+1}) + (l'_j - l'_{j+1}) + (l''_j - l''_{j+1}); at the azimuth |m''| <= l''_{d-3}.
static int terms_chain(biem_plan* p) {
  const int d = p->d, n = p->n_end, n2 = p->n2, lw = p->lw, np = d - 2, H = p->H;
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
  std::vector<int> a(np + 1), b(np + 1), c(lw);
  std::vector<double> pre(np + 1);
  bool too_many = false;
  for (int h = 0; h < H && !too_many; ++h)
    for (int hp = 0; hp < H; ++hp) {
      for (int j = 0; j <= np; ++j) { b[j] = chain_deg(p->labels, lw, h, j); a[j] = chain_deg(p->labels, lw, hp, j); }
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
  if (too_many) { set_error("chain tree d=%d n_end=%d: more than 2^31 translation terms", d, n); return BIEM_ERR_UNSUPPORTED; }
  return BIEM_OK;
}
// writes lists_built, ptr, coef, tidx
static int build_terms(biem_plan* p) {
  // 2-D beyond kLists2dMax: no term lists at all (H^2 entries of one term each: 1.4 GB at the reference's n_end = 3444) - the 2-D
  // fills evaluate S(m, m') = i^{|m| + |mu| - |m'|} T[mu], mu = m' - m, directly (k_fill2d_sym / k_fill2d, any order)
  p->lists_built = !(p->tree == TREE_A && p->n_end > kLists2dMax);
  p->ptr.assign(p->lists_built ? (size_t)p->H * p->H + 1 : 1, 0);
  p->coef.clear(); p->tidx.clear();
  if (!p->lists_built) return BIEM_OK;
  switch (p->tree) {
    case TREE_A: terms_a(p); break;
    case TREE_BA: terms_ba(p); break;
    case TREE_BBA: case TREE_CAA: return terms_4d(p);
    default: return terms_chain(p);
  }
  return BIEM_OK;
}

// everything behind the scalars and labels: units, quadrature, projection, term lists, fill tables
static int build_tables(biem_plan* p) {
  int rc;
  if ((rc = build_units(p)) || (rc = build_quadrature(p))) return rc;
  build_projection(p);
  if ((rc = build_terms(p))) return rc;
  return plan_build_fill_tables(p);
}

int plan_build_host(biem_plan* p, int tree, int n_end) {
  if (tree < 0 || tree > 3) { set_error("unsupported coordinate tree id %d (built: a, ba, bba, caa)", tree); return BIEM_ERR_UNSUPPORTED; }
  if (n_end < 1 || n_end > 4096) { set_error("n_end=%d out of range", n_end); return BIEM_ERR_ARG; }
  p->tree = tree; p->d = tree_dim(tree); p->n_end = n_end; p->n2 = 2 * n_end - 1;
  p->H = harm_count(tree, n_end); p->H2 = harm_count(tree, p->n2);
  p->Cd = pow(2.0 * kPi, 0.5 * p->d) * sqrt(2.0 / kPi);
  make_labels(tree, n_end, p->labels, p->deg);
  make_labels(tree, p->n2, p->labels2, p->deg2);
  return build_tables(p);
}

// the standard chain tree "b" * (d - 2) + "a"
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
  return build_tables(p);
}

}  // namespace biem
