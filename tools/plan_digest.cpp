// plan_digest.cpp -- build plans on the host and print one line per plan: return code, scalar members, an FNV-1a digest of every
// table of the plan's table list (BIEM_PLAN_TABLES, plan.hpp) and the build time.  Links the plan sources only and calls no HIP function:
//   hipcc --offload-host-only -O1 -std=c++17 tools/plan_digest.cpp biem_helmholtz_sphere_amd/csrc/plan*.cpp -o plan_digest
//   plan_digest [--check] TREE N_END [TREE N_END ...]        TREE: a | ba | bba | caa | chain<d>
// Two builds of the plan sources agree when their lines differ in build_s alone.  --check verifies the structural invariants of the
// fill tables as well and exits with status 1 at the first violation, naming it.  A host program: sanitizers apply to it as to any other.
#include "../biem_helmholtz_sphere_amd/csrc/plan.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace biem { const char* last_error(); }

template <class T> static unsigned long long fnv1a(const std::vector<T>& v) {
  unsigned long long h = 1469598103934665603ULL;
  const unsigned char* b = (const unsigned char*)v.data();
  for (size_t i = 0, n = v.size() * sizeof(T); i < n; ++i) { h ^= b[i]; h *= 1099511628211ULL; }
  return h;
}

static std::string g_bad;      // the first violated invariant
static bool bad(const std::string& what) { if (g_bad.empty()) g_bad = what; return false; }

// bound[] starts at 0 and rises strictly; on: it ends at total; off: it is {0}
static bool check_bounds(const std::string& n, const std::vector<int>& bound, bool on, long long total) {
  if (bound.empty() || bound[0] != 0) return bad(n + " does not start at 0");
  if (!on) return bound.size() == 1 || bad(n + " is cut although its form is off");
  for (size_t c = 0; c + 1 < bound.size(); ++c) if (bound[c + 1] <= bound[c]) return bad(n + " is not strictly increasing");
  return bound.back() == total || bad(n + " does not end at its total");
}
// and the two maxima are those of the chunks cut (terms counted by the prefix sums pre[stride * item]), 0 when the form is off
template <class P> static bool check_chunks(const char* name, const std::vector<int>& bound, bool on, long long total, const std::vector<P>& pre,
                                            int stride, int terms_max, int items_max) {
  const std::string n(name);
  if (!check_bounds(n, bound, on, total)) return false;
  if ((size_t)bound.back() * stride >= pre.size()) return bad(n + " runs past its prefix sums");
  long long tm = 0, im = 0;
  for (size_t c = 0; c + 1 < bound.size(); ++c) {
    const long long nt = (long long)pre[(size_t)bound[c + 1] * stride] - (long long)pre[(size_t)bound[c] * stride];
    if (nt > tm) tm = nt;
    if (bound[c + 1] - bound[c] > im) im = bound[c + 1] - bound[c];
  }
  if (tm != terms_max) return bad(n + ": terms_max is not the largest chunk cut");
  return im == items_max || bad(n + ": items_max is not the largest chunk cut");
}

template <class P, class C> static bool check_ptr(const char* name, const std::vector<P>& ptr, const std::vector<C>& coef) {
  for (size_t i = 0; i + 1 < ptr.size(); ++i) if (ptr[i + 1] < ptr[i]) return bad(std::string(name) + " decreases");
  return (!ptr.empty() && ptr.back() == coef.size()) || bad(std::string(name) + " does not end at the size of its coefficient array");
}

static bool check_below(const char* name, const std::vector<uint16_t>& idx, long long limit) {
  for (uint16_t v : idx) if ((long long)v >= limit) return bad(std::string(name) + " holds an index past its table");
  return true;
}

static bool check_plan(const biem_plan& p) {
  const long long H = p.H, U = (long long)p.units.size() / 2;
  if (!check_ptr("ptr", p.ptr, p.coef) || !check_ptr("qptr", p.qptr, p.qcoef) || !check_ptr("q2ptr", p.q2ptr, p.q2coef)) return false;
  if (!check_chunks("chunk_ent", p.chunk_ent, p.lists_built, H * H, p.ptr, 1, p.chunk_terms_max, p.chunk_ents_max)) return false;
  if (!check_chunks("qchunk", p.qchunk, p.qchunk.size() > 1, U * U, p.q2ptr, 2, p.qchunk_terms_max, p.qchunk_pairs_max)) return false;
  if (p.qchunk.size() > 1 && !p.pair_lists_ok) return bad("qchunk is cut although the pair lists are off");
  if (!check_chunks("schunk", p.schunk, p.lists_built, U * U, p.qptr, 4, p.schunk_terms_max, p.schunk_pairs_max)) return false;
  if (!check_bounds("rchunk", p.rchunk, p.red_lists_ok, U * U)) return false;
  if (p.rcrow.size() != p.rchunk.size() || p.rcrow[0] != 0) return bad("rcrow does not match rchunk");
  int rows_max = 0;
  for (size_t c = 0; c + 1 < p.rcrow.size(); ++c) {
    if (p.rcrow[c + 1] <= p.rcrow[c]) return bad("rcrow is not increasing");
    if (p.rcrow[c + 1] - p.rcrow[c] > rows_max) rows_max = p.rcrow[c + 1] - p.rcrow[c];
  }
  if ((size_t)p.rcrow.back() != p.rcoef.size() / 64 || p.ridx.size() != p.rcoef.size()) return bad("rcrow does not end at rcoef.size() / 64");
  if (rows_max != p.rchunk_rows_max) return bad("rchunk_rows_max is not the largest chunk cut");
  if (p.rwrow.size() != 33 * (p.rchunk.size() - 1)) return bad("rwrow does not hold 33 entries per reduced chunk");
  for (size_t c = 0; c + 1 < p.rchunk.size(); ++c)
    for (int w = 0; w < 16; ++w) {
      const int* r = &p.rwrow[c * 33 + 2 * w];
      if (r[0] > r[1] || r[1] > r[2] || r[2] > p.rcrow[c + 1] - p.rcrow[c]) return bad("rwrow: a wave's rows are not ordered within its chunk");
    }
  if (!check_below("tidx16", p.tidx16, p.H2) || !check_below("qidx16", p.qidx16, p.H2) || !check_below("q2idx16", p.q2idx16, p.H2lin) ||
      !check_below("ridx", p.ridx, p.E)) return false;
  std::vector<char> seen(p.H2lin / 2, 0);          // lin2 of the first members (even values): every even number below H2lin once
  for (int v : p.lin2) {
    if (v < 0 || v >= p.H2lin) return bad("lin2 leaves the paired table");
    if (!(v & 1) && seen[v / 2]++) return bad("lin2 maps two first members to one slot");
  }
  for (char s : seen) if (!s) return bad("lin2 leaves a slot of the paired table without a first member");
  std::vector<char> hit(H, 0);
  for (int v : p.hpos) if (v < 0 || v >= H || hit[v]++) return bad("hpos is not a permutation of 0 .. H-1");
  return (long long)p.hpos.size() == H || bad("hpos is not a permutation of 0 .. H-1");
}

int main(int argc, char** argv) {
  bool check = false;
  int first = 1;
  if (argc > 1 && !strcmp(argv[1], "--check")) { check = true; first = 2; }
  if (argc <= first || ((argc - first) & 1)) { fprintf(stderr, "usage: %s [--check] TREE N_END [TREE N_END ...]   (TREE: a | ba | bba | caa | chain<d>)\n", argv[0]); return 2; }
  static const char* kTrees[4] = {"a", "ba", "bba", "caa"};
  for (int a = first; a + 1 < argc; a += 2) {
    const char* tname = argv[a];
    const int n_end = atoi(argv[a + 1]);
    int tree = -1;
    for (int t = 0; t < 4; ++t) if (!strcmp(tname, kTrees[t])) tree = t;
    if (tree < 0 && strncmp(tname, "chain", 5)) { fprintf(stderr, "unknown tree %s\n", tname); return 2; }
    biem_plan* p = new biem_plan();
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = tree >= 0 ? biem::plan_build_host(p, tree, n_end) : biem::plan_build_chain_host(p, atoi(tname + 5), n_end);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%s %d rc=%d", tname, n_end, rc);
    if (rc) printf(" error=\"%s\"", biem::last_error());
    printf(" tree=%d d=%d n_end=%d n2=%d H=%d H2=%d Q=%d Cd=%.17g lw=%d chunk_terms_max=%d chunk_ents_max=%d lists_built=%d fill_table_global=%d",
           p->tree, p->d, p->n_end, p->n2, p->H, p->H2, p->Q, p->Cd, p->lw, p->chunk_terms_max, p->chunk_ents_max, (int)p->lists_built, (int)p->fill_table_global);
    printf(" H2lin=%d pair_lists_ok=%d qchunk_terms_max=%d qchunk_pairs_max=%d E=%d NP=%d red_lists_ok=%d red_waves=%d red_nc=%d rchunk_rows_max=%d",
           p->H2lin, (int)p->pair_lists_ok, p->qchunk_terms_max, p->qchunk_pairs_max, p->E, p->NP, (int)p->red_lists_ok, p->red_waves, p->red_nc, p->rchunk_rows_max);
    printf(" red_gather_cycles=%.17g schunk_terms_max=%d schunk_pairs_max=%d", p->red_gather_cycles, p->schunk_terms_max, p->schunk_pairs_max);
#define DIGEST(T, name) printf(" " #name "=%zu:%016llx", p->name.size(), fnv1a(p->name));
    BIEM_PLAN_TABLES(DIGEST, DIGEST)
#undef DIGEST
    const bool ok = !check || rc != 0 || check_plan(*p);
    if (check && rc == 0) printf(" check=%s", ok ? "ok" : "FAILED");
    printf(" build_s=%.3f\n", secs);
    fflush(stdout);
    delete p;
    if (!ok) { fprintf(stderr, "%s %d: %s\n", tname, n_end, g_bad.c_str()); return 1; }
  }
  return 0;
}
