// plan.cpp -- a plan's device mirrors (upload and free, generated from the table lists of plan.hpp), the coupling table of the radiation
// force and the library's error text.  The host tables themselves: plan_tree.cpp (per tree) and plan_fill.cpp (the fill's forms).
#include "plan_build.hpp"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>

namespace biem {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
const char* last_error() { return g_err; }

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s failed: %s", #x, hipGetErrorString(e_)); return BIEM_ERR_HIP; } } while (0)

template <class T> static int up(T** dst, const std::vector<T>& src) {
  if (src.empty()) { *dst = nullptr; return BIEM_OK; }
  HIPCHK(hipMalloc((void**)dst, src.size() * sizeof(T)));
  HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return BIEM_OK;
}
// per entry of a table list (plan.hpp): upload what has no mirror yet; free what has one.  A failed upload leaves its earlier tables
// to plan_free, which does not ask whether the upload was completed.
#define UPLOAD(T, name) if (!p->d_##name && (rc = up(&p->d_##name, p->name))) return rc;
#define RELEASE(T, name) if (p->d_##name) (void)hipFree(p->d_##name);
#define HOST_ONLY(T, name)

int plan_upload(biem_plan* p) {
  if (p->device >= 0) return BIEM_OK;
  int dev = 0, rc;
  HIPCHK(hipGetDevice(&dev));
  BIEM_PLAN_TABLES(UPLOAD, HOST_ONLY)
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
          // the values are algebraic numbers or exact zeros.  They are not O(1): the smallest shrinks with order and dimension
          // (7.2e-3 at ba 50, 1.15e-3 at bba 16, 3.0e-4 at bbba 10), but at the order ceilings of the field kernels and two orders
          // above them it stays six decades above this band, and an independent rule leaves at most 3e-16 where an entry was dropped
          // (tests/test_force_table_full_order_host.py asserts both margins).  Anything between is a rule that was not exact
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
    BIEM_PLAN_FORCE_TABLES(UPLOAD, HOST_ONLY)
    p->force_uploaded = true;
  }
  return BIEM_OK;
}

void plan_free(biem_plan* p) {
  BIEM_PLAN_TABLES(RELEASE, HOST_ONLY)
  BIEM_PLAN_FORCE_TABLES(RELEASE, HOST_ONLY)
  delete p;
}

}  // namespace biem
