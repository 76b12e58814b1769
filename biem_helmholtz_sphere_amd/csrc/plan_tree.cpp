// plan_tree.cpp -- what a plan holds per coordinate tree: labels, conjugate units, boundary-data quadrature, projection matrix and the
// translation term lists (pure C++).  One function per tree for the quadrature and one for the term lists, each reached through one
// switch; the fill tables behind them are the same for every tree (plan_fill.cpp).
#include "plan_build.hpp"
#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
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
static void terms_caa(biem_plan* p) {
  const int H = p->H, n = p->n_end;
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
}
static void terms_bba(biem_plan* p) {
  const int H = p->H, n = p->n_end, n2 = p->n2;
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
    case TREE_BBA: terms_bba(p); break;
    case TREE_CAA: terms_caa(p); break;
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
