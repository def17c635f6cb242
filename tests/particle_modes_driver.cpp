// particle_modes_driver.cpp — svnicp_particle_modes through the C++ shim (svn-icp_amd/host/svnicp_hip_shim.hpp) on a caller's
// particle set; tests/test_particle_modes_gpu.py compiles it and compares what it prints with the Python binding's struct.
//   particle_modes_driver in.bin link_trans link_rot max_modes
// in.bin : int32 P, int32 has_weights, f64 [6][P] particles, f64 [P] weights when has_weights
// prints : "modes particles nonfinite n_modes n_reported has_scores", one line per reported mode
//          "mode k label count best mass cost_min cost_mean mean[6] cov[36] R[9] t[3]" (%.17g), then "labels l0 l1 ..."
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svnicp_hip_shim.hpp"

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s in.bin link_trans link_rot max_modes\n", argv[0]); return 64; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 65; }
  int32_t P = 0, has_w = 0;
  if (fread(&P, 4, 1, f) != 1 || fread(&has_w, 4, 1, f) != 1 || P < 1) return 66;
  std::vector<double> x((size_t)6 * P), w((size_t)P);
  if (fread(x.data(), 8, x.size(), f) != x.size()) return 66;
  if (has_w && fread(w.data(), 8, w.size(), f) != w.size()) return 66;
  fclose(f);
  try {
    svnicp::SteinICPParam prm;
    svnicp::SVNICP s(prm, std::vector<double>(6, 0.0));   // no clouds, no registration: the set is the caller's
    const svnicp_modes m = s.particle_modes(atof(argv[2]), atof(argv[3]), atoi(argv[4]), x.data(), P, has_w ? w.data() : nullptr);
    printf("modes %d %d %d %d %d\n", (int)m.particles, (int)m.nonfinite, (int)m.n_modes, (int)m.n_reported, (int)m.has_scores);
    for (int k = 0; k < m.n_reported; ++k) {
      printf("mode %d %d %d %d %.17g %.17g %.17g", k, (int)m.label[k], (int)m.count[k], (int)m.best[k], m.mass[k], m.cost_min[k], m.cost_mean[k]);
      for (int i = 0; i < 6; ++i) printf(" %.17g", m.mean[k][i]);
      for (int i = 0; i < 36; ++i) printf(" %.17g", m.cov[k][i]);
      for (int i = 0; i < 9; ++i) printf(" %.17g", m.R[k][i]);
      for (int i = 0; i < 3; ++i) printf(" %.17g", m.t[k][i]);
      printf("\n");
    }
    printf("labels");
    for (int32_t l : s.get_mode_labels()) printf(" %d", (int)l);
    printf("\n");
  } catch (const std::exception& e) {
    fprintf(stderr, "svnicp: %s\n", e.what());
    return 3;
  }
  return 0;
}
