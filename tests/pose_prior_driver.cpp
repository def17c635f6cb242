// pose_prior_driver.cpp — svnicp::pose_prior::validate (csrc/pose_prior.hpp) on crafted means and information matrices, as a
// stand-alone host program: tests/test_pose_prior_cpu.py builds it with -fsanitize=address,undefined and reads its output,
// one line per case: name|return code|reason or "-"|largest asymmetry of the stored matrix|R_mu orthogonality defect.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pose_prior.hpp"

using svnicp::PosePrior;

struct Case { const char* name; double mean[6]; double L[36]; };

static void diag(double* L, double v) { std::memset(L, 0, 36 * sizeof(double)); for (int i = 0; i < 6; ++i) L[7 * i] = v; }

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name) -> Case& { cases.push_back(Case{}); cases.back().name = name; diag(cases.back().L, 1.0); return cases.back(); };
  add("identity");
  { Case& c = add("zero"); diag(c.L, 0.0); }
  { Case& c = add("huge"); diag(c.L, 1e12); c.L[1] = c.L[6] = 5e11; }
  { Case& c = add("rank1");   // v v^T, v = (1, 2, 0, 0, 0, -3): PSD, five zero eigenvalues
    const double v[6] = {1, 2, 0, 0, 0, -3};
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) c.L[6 * i + j] = v[i] * v[j]; }
  { Case& c = add("asymmetric"); c.L[1] = 0.5; c.L[6] = 0.5 + 1e-9; }
  { Case& c = add("asymmetric_within_tolerance"); diag(c.L, 4.0); c.L[1] = 0.5; c.L[6] = 0.5 + 2e-12; }
  { Case& c = add("nan_entry"); c.L[8] = std::numeric_limits<double>::quiet_NaN(); }
  { Case& c = add("inf_entry"); c.L[35] = std::numeric_limits<double>::infinity(); }
  { Case& c = add("nan_mean"); c.mean[2] = std::numeric_limits<double>::quiet_NaN(); }
  { Case& c = add("negative_diagonal"); c.L[14] = -1e-3; }
  { Case& c = add("eigenvalue_-1e-6");   // [[1, 1 + 1e-6], [1 + 1e-6, 1]] in (x, y): eigenvalues 2 + 1e-6 and -1e-6, no negative diagonal
    c.L[1] = c.L[6] = 1.0 + 1e-6; }
  { Case& c = add("eigenvalue_-1e-13_relative");   // below the 1e-12 max|Lambda| allowance: accepted
    diag(c.L, 1e3); c.L[0] = c.L[7] = 1.0; c.L[1] = c.L[6] = 1.0 + 1e-10; }
  { Case& c = add("mean_rotation_pi"); c.mean[3] = 3.14159265358979323846; }
  { Case& c = add("mean_rotation_3.1"); c.mean[4] = 3.1; }
  { Case& c = add("mean_general"); c.mean[0] = 1e3; c.mean[3] = 0.1; c.mean[4] = -0.2; c.mean[5] = 0.05; }
  for (const Case& c : cases) {
    PosePrior out;
    std::memset(&out, 0, sizeof out);
    const char* why = nullptr;
    const int rc = svnicp::pose_prior::validate(c.mean, c.L, &out, &why);
    double asym = 0.0, orth = 0.0;
    if (rc == 0) {
      for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) asym = std::fmax(asym, std::fabs(out.L[6 * i + j] - out.L[6 * j + i]));
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += out.Rmu[3 * k + i] * out.Rmu[3 * k + j];
        orth = std::fmax(orth, std::fabs(s - (i == j ? 1.0 : 0.0)));
      }
    }
    std::printf("%s|%d|%s|%.3g|%.3g\n", c.name, rc, why ? why : "-", asym, orth);
  }
  const char* why = nullptr;
  PosePrior out;
  const int rc_null = svnicp::pose_prior::validate(nullptr, nullptr, &out, &why);
  std::printf("null|%d|%s|0|0\n", rc_null, why ? why : "-");
  return 0;
}
