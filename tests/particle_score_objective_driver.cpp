// particle_score_objective_driver.cpp — csrc/gicp_pair_device.hpp's gicp_pair_cost beside gicp_pair_sums on the host, as a
// stand-alone program for the address and undefined-behaviour sanitizers (tests/test_particle_score_objective_cpu.py compiles
// and runs it the way tests/gicp_accum_driver.cpp is).  It checks itself and prints one line per group; exit status 1 and a
// line "FAIL ..." per finding otherwise.
//   adversarial pairs   parallel, orthogonal and skew normals, epsilon at both ends and at its default, delta finite and +inf:
//                       no NaN, 0 <= h, and the rho2 gicp_pair_cost sees is bitwise the one gicp_pair_sums folds: its return
//                       value is w = 1 (sqrt(rho2) <= delta) else delta / sqrt(rho2) and acc[28] is w * rho2 of that rho2
//   rejected pairs      zero normals, NaN and infinite points, ok == false: h, accepted and all 29 sums are exact zeros
//   the kink            rho at delta exactly and one ulp on either side: the two branches of h agree there to 2 ulp
//   delta = +inf        h is rho2 itself
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "gicp_pair_device.hpp"

using namespace svnicp;

static int failures = 0;
static void fail(const char* what, int i, double a, double b) {
  std::printf("FAIL %s (case %d): %.17g vs %.17g\n", what, i, a, b);
  ++failures;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static double ulp(double x) { return std::nextafter(std::fabs(x), std::numeric_limits<double>::infinity()) - std::fabs(x); }

struct Pair { double u[3], m[3], n[3]; };

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double r2 = std::sqrt(0.5), r3 = std::sqrt(1.0 / 3.0);
  const Pair pairs[] = {
      {{0.3, -0.2, 0.1}, {0, 0, 1}, {0, 0, 1}},                 // parallel
      {{0.3, -0.2, 0.1}, {0, 0, 1}, {0, 0, -1}},                // antiparallel
      {{0.3, -0.2, 0.1}, {0, 0, 1}, {1, 0, 0}},                 // orthogonal
      {{0.0, 0.0, 0.25}, {0, 0, 1}, {0, 1, 0}},                 // u along one normal
      {{0.25, 0.0, 0.0}, {0, 0, 1}, {0, 1, 0}},                 // u in both planes: rho2 = eps-free direction
      {{1e-9, -2e-9, 3e-9}, {r2, r2, 0}, {r2, -r2, 0}},         // tiny u
      {{0.9, 0.9, 0.9}, {r3, r3, r3}, {r3, r3, r3}},            // u along parallel normals: rho2 = |u|^2
      {{0.01, 0.4, -0.3}, {r3, -r3, r3}, {r2, 0, -r2}},         // skew
      {{0.0, 0.0, 0.0}, {0, 1, 0}, {1, 0, 0}},                  // u = 0
  };
  const double epss[] = {kGicpEpsilonMin, kGicpEpsilonDefault, 0.5, 1.0};
  const double deltas[] = {1e-3, 0.05, 0.3, inf};
  int i = 0, n_pairs = 0;
  for (const Pair& p : pairs)
    for (const double eps : epss)
      for (const double delta : deltas) {
        ++i; ++n_pairs;
        double accepted = -1.0, rho2 = -1.0;
        const double h = gicp_pair_cost(true, p.u[0], p.u[1], p.u[2], p.m[0], p.m[1], p.m[2], p.n[0], p.n[1], p.n[2], eps, delta, accepted, &rho2);
        double acc[kGicpSums] = {};
        const double w = gicp_pair_sums(acc, true, 1.5, -2.5, 0.5, p.u[0], p.u[1], p.u[2], p.m[0], p.m[1], p.m[2], p.n[0], p.n[1], p.n[2], eps, delta);
        if (!(h == h) || !(rho2 == rho2) || !(h >= 0.0) || !(rho2 >= 0.0)) fail("NaN or negative", i, h, rho2);
        if (accepted != 1.0 || acc[27] != 1.0) fail("accepted flag", i, accepted, acc[27]);
        const double rho = std::sqrt(rho2);
        const double w_want = rho <= delta ? 1.0 : delta / rho;
        if (!same_bits(w, w_want)) fail("gicp_pair_sums' weight is not that of gicp_pair_cost's rho2", i, w, w_want);
        if (!same_bits(acc[28], w * rho2)) fail("acc[28] is not w * rho2 of gicp_pair_cost's rho2", i, acc[28], w * rho2);
        const double u2 = (p.u[0] * p.u[0] + p.u[1] * p.u[1]) + p.u[2] * p.u[2];
        if (rho2 > u2 * (1.0 + 1e-9) + 0.0) fail("rho2 exceeds |u|^2: W's eigenvalues lie in [eps, 1]", i, rho2, u2);
        const double want = rho <= delta ? rho2 : delta * (2.0 * rho - delta);
        if (!same_bits(h, want)) fail("h", i, h, want);
        if (delta == inf && !same_bits(h, rho2)) fail("delta = inf: h is rho2 itself", i, h, rho2);
        for (int k = 0; k < kGicpSums; ++k)
          if (!(acc[k] == acc[k])) fail("NaN in the sums", i, (double)k, acc[k]);
      }
  std::printf("adversarial pairs: %d checked\n", n_pairs);

  // rejected pairs: every operand is selected to zero first
  const double bad[] = {nan, inf, -inf, 1e308, 0.0};
  int n_rej = 0;
  for (const double x : bad)
    for (const double delta : deltas) {
      ++i; ++n_rej;
      double accepted = -1.0, rho2 = -1.0;
      const double h = gicp_pair_cost(false, x, 0.1, x, x, 0.0, 1.0, 0.0, x, 0.0, kGicpEpsilonDefault, delta, accepted, &rho2);
      double acc[kGicpSums] = {};
      const double w = gicp_pair_sums(acc, false, x, x, x, x, 0.1, x, x, 0.0, 1.0, 0.0, x, 0.0, kGicpEpsilonDefault, delta);
      if (!same_bits(h, 0.0) || !same_bits(accepted, 0.0) || !same_bits(rho2, 0.0) || !same_bits(w, 0.0)) fail("a rejected pair is not exact zeros", i, h, rho2);
      for (int k = 0; k < kGicpSums; ++k)
        if (!same_bits(acc[k], 0.0)) fail("a rejected pair left a non-zero sum", i, (double)k, acc[k]);
    }
  // an accepted pair between zero normals (never formed by the kernels, whose `ok` asks for both): W = eps I, still finite
  {
    ++i;
    double accepted, rho2;
    const double h = gicp_pair_cost(true, 0.3, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 1e-3, inf, accepted, &rho2);
    if (!(h == h) || std::fabs(h - 1e-3 * 0.09) > 4 * ulp(1e-3 * 0.09)) fail("zero normals: W = eps I", i, h, 1e-3 * 0.09);
  }
  std::printf("rejected pairs: %d checked\n", n_rej);

  // the kink: eps = 1 makes W = I exactly, rho2 = x * x
  int n_kink = 0;
  double worst = 0.0;
  for (const double x : {0.05, 0.3, 1.0 / 3.0, 1e-3, 0.7071067811865476}) {
    double accepted, rho2;
    (void)gicp_pair_cost(true, x, 0.0, 0.0, 0, 0, 1, 0, 1, 0, 1.0, inf, accepted, &rho2);
    const double rho = std::sqrt(rho2);
    const double at[] = {rho, std::nextafter(rho, 0.0), std::nextafter(rho, inf)};
    for (const double delta : at) {
      ++i; ++n_kink;
      const double h = gicp_pair_cost(true, x, 0.0, 0.0, 0, 0, 1, 0, 1, 0, 1.0, delta, accepted, &rho2);
      const double inside = rho2, outside = delta * (2.0 * rho - delta);
      if (!same_bits(h, rho <= delta ? inside : outside)) fail("the kink: h is not the selected branch", i, h, inside);
      const double d = std::fabs(inside - outside) / ulp(inside);
      worst = d > worst ? d : worst;
      if (d > 2.0) fail("the kink: the two branches differ by more than 2 ulp", i, inside, outside);
      if (!same_bits(robust_cost(rho, rho2, delta), h)) fail("robust_cost", i, h, robust_cost(rho, rho2, delta));
    }
  }
  std::printf("the kink: %d checked, the branches agree to %.2f ulp\n", n_kink, worst);
  // the cap of a scoring is the same function of the gate: h(gate) with x2 = gate * gate
  for (const double gate : {0.3, 1.0})
    for (const double delta : deltas) {
      ++i;
      const double cap = robust_cost(gate, gate * gate, delta);
      const double want = gate <= delta ? gate * gate : delta * (2.0 * gate - delta);
      if (!same_bits(cap, want) || !(cap > 0.0) || !(cap <= gate * gate)) fail("cap", i, cap, want);
    }
  std::printf(failures ? "FAILED: %d findings\n" : "ok (%d findings)\n", failures);
  return failures ? 1 : 0;
}
