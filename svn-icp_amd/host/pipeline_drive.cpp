// pipeline_drive.cpp — runs svnicp::RegistrationPipeline (registration_pipeline.hpp) over a recorded sequence of scans and
// dumps, per scan, what the pipeline handed to the solver and what it got back.  Used by tests/test_pipeline_gpu.py, which
// replays the dumped solver inputs through the CPU oracle and through svn-icp_amd/pipeline.py.
//   g++ -std=c++17 -I include -I svn-icp_amd/host pipeline_drive.cpp -L svn-icp_amd -lsvnicp_hip -o pipeline_drive
//   pipeline_drive scans.bin out.bin P iterations knn voxel [particles.bin|-] [gpu_map 0|1|2] [deskew 0|1] [segment 0|1] [map_normals 0|1] [eval_dist] [information off|point|plane|gicp] [modes off|mean|heaviest link_trans link_rot] [clear 0|1]
//     (gpu_map 2: device map + device pre-processing; deskew 1: PipelineConfig::deskew, OdometryPipeline.cpp:551-554;
//      segment 1: PipelineConfig::segmentation with the HDL-64E sensor, USE_Segmentation, :328-355;
//      map_normals 1: the point-to-plane residual with the normals of the device map's own voxels, needs gpu_map 1 or 2;
//      map_normals 2: the generalized-ICP residual, the target's normals from the map as with 1, the source's from the solver's pass;
//      eval_dist > 0: PipelineConfig::eval_dist, every registered scan is evaluated and one more line per scan is printed:
//      "eval <scan>: fitness inlier_rmse plane_rmse plane_inliers" with %.17g, -1 where a figure does not exist;
//      information point|plane|gicp: PipelineConfig::information (needs eval_dist > 0; gicp needs map_normals 2), one more line per registered scan:
//      "info <scan>: pairs rank eigval[0] ... eigval[5]" with %.17g;
//      modes mean|heaviest link_trans link_rot: PipelineConfig::mode_link_* / mode_select_heaviest, one more line per registered scan:
//      "modes <scan>: n_modes n_reported nonfinite has_scores" and per reported mode " | label count best mass mean[0..5]" with %.17g;
//      clear 1: PipelineConfig::clear_seen_through with its defaults (window 1 x 1, margins 0.3 m / 0.02) and the HDL-64E sensor,
//      one more line per registered scan: "clear <scan>: points_removed";
//      after those, seven more: seed_levels seed_keep seed_skip_fitness extent_xy extent_yaw step_xy step_yaw -- seed_levels > 0 turns
//      PipelineConfig::seed_grid on with that x / y / yaw grid (1 = the flat grid, > 1 = the coarse-to-fine search), one more line per
//      seeded scan: "seed <scan>: searched levels nodes_scored fitness_zero cost_zero cost correction[x] [y] [yaw]" with %.17g;
//      after those, seven more: prior_point_sigma sx sy sz srx sry srz -- prior_point_sigma > 0 turns PipelineConfig::prior_sigma on
//      with those standard deviations, one more line per registered scan: "prior <scan>: prior_chi2" with %.17g;
//      after those, three more: weight_dist weight_temperature weight_cost -- weight_dist > 0 turns PipelineConfig::weight_dist /
//      weight_temperature on, weight_cost point|solved is PipelineConfig::weight_cost)
// scans.bin : int32 n_scans, then per scan { f64 stamp, int32 n, n x 3 float32 } — with deskew 1 followed by n x f64 point stamps
// particles : optional f64 [n_scans][6][P] (otherwise the built-in uniform prior sampler)
// out.bin   : per scan { int32 aligned, f64 pose[12], guess[12], corr[6], var[6], cov[36], int64 B, M, f64 src[3B], tgt[3M], init[6P] }
//             — with map_normals 1 followed, for a registered scan, by int64 with_normal
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "registration_pipeline.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: %s scans.bin out.bin P iterations knn voxel [particles.bin]\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 65; }
  svnicp::PipelineConfig cfg;
  cfg.particle_count = atoi(argv[3]);
  cfg.solver.iterations = atoi(argv[4]); cfg.solver.KNN_count = atoi(argv[5]);
  cfg.solver.lr = 1.0; cfg.solver.max_dist = 1.0; cfg.solver.SVN_full_grad = false;
  cfg.voxel_size = cfg.map_voxel_size = atof(argv[6]);
  cfg.min_range = 1.0; cfg.max_range = 80.0; cfg.map_range = 100.0; cfg.map_voxel_max_points = 20;
  FILE* fp = (argc > 7 && argv[7][0] != '-') ? fopen(argv[7], "rb") : nullptr;
  cfg.gpu_map = argc > 8 && atoi(argv[8]) != 0;
  cfg.gpu_prep = argc > 8 && atoi(argv[8]) >= 2;
  cfg.deskew = argc > 9 && atoi(argv[9]) != 0;
  cfg.segmentation = argc > 10 && atoi(argv[10]) != 0;
  cfg.map_normals = argc > 11 && atoi(argv[11]) != 0;
  cfg.gicp = cfg.map_normals && atoi(argv[11]) == 2;
  cfg.plane = cfg.map_normals && !cfg.gicp;
  cfg.eval_dist = argc > 12 ? atof(argv[12]) : 0.0;
  if (argc > 13) cfg.information = argv[13];
  if (argc > 16 && std::string(argv[14]) != "off") {
    cfg.mode_link_trans = atof(argv[15]); cfg.mode_link_rot = atof(argv[16]);
    cfg.mode_select_heaviest = std::string(argv[14]) == "heaviest";
  }
  cfg.clear_seen_through = argc > 17 && atoi(argv[17]) != 0;
  if (argc > 24 && atoi(argv[18]) > 0) {
    const double exy = atof(argv[21]), eyaw = atof(argv[22]), sxy = atof(argv[23]), syaw = atof(argv[24]);
    cfg.seed_grid = std::make_pair(std::array<double, 6>{exy, exy, 0, 0, 0, eyaw}, std::array<double, 6>{sxy, sxy, 0, 0, 0, syaw});
    cfg.seed_levels = atoi(argv[18]); cfg.seed_keep = atoi(argv[19]); cfg.seed_skip_fitness = atof(argv[20]);
  }
  if (argc > 31 && atof(argv[25]) > 0) {
    cfg.prior_point_sigma = atof(argv[25]);
    cfg.prior_sigma = std::array<double, 6>{atof(argv[26]), atof(argv[27]), atof(argv[28]), atof(argv[29]), atof(argv[30]), atof(argv[31])};
  }
  if (argc > 34) { cfg.weight_dist = atof(argv[32]); cfg.weight_temperature = atof(argv[33]); cfg.weight_cost = argv[34]; }
  try {
    svnicp::RegistrationPipeline pipe(cfg);
    svnicp::Tap tap;
    pipe.set_tap(&tap);
    std::vector<double> injected((size_t)6 * cfg.particle_count);
    if (fp) pipe.set_particle_source([&](int P, double* out) { for (int i = 0; i < 6 * P; ++i) out[i] = injected[i]; });
    int32_t n_scans = 0;
    if (!rd(fi, &n_scans, 1)) return 66;
    for (int s = 0; s < n_scans; ++s) {
      double stamp; int32_t n;
      if (!rd(fi, &stamp, 1) || !rd(fi, &n, 1)) return 66;
      svnicp::Cloud pts((size_t)n);
      if (!rd(fi, &pts[0][0], (size_t)3 * n)) return 66;
      std::vector<double> point_stamps(cfg.deskew ? (size_t)n : 0);
      if (cfg.deskew && !rd(fi, point_stamps.data(), (size_t)n)) return 66;
      if (fp && !rd(fp, injected.data(), injected.size())) return 66;
      tap = svnicp::Tap{};
      const svnicp::ScanResult r = cfg.deskew ? pipe.process_scan(pts, stamp, point_stamps) : pipe.process_scan(pts, stamp);
      const int32_t aligned = r.aligned ? 1 : 0;
      wr(fo, &aligned, 1);
      double pose[12], guess[12];
      for (int i = 0; i < 9; ++i) { pose[i] = r.pose.R[i]; guess[i] = r.initial_guess.R[i]; }
      for (int i = 0; i < 3; ++i) { pose[9 + i] = r.pose.t[i]; guess[9 + i] = r.initial_guess.t[i]; }
      wr(fo, pose, 12); wr(fo, guess, 12);
      std::vector<double> cov = r.cov; cov.resize(36, 0.0);
      wr(fo, r.correction.data(), 6); wr(fo, r.variance.data(), 6); wr(fo, cov.data(), 36);
      const int64_t B = (int64_t)tap.source.size() / 3, M = (int64_t)tap.target.size() / 3;
      wr(fo, &B, 1); wr(fo, &M, 1);
      wr(fo, tap.source.data(), tap.source.size()); wr(fo, tap.target.data(), tap.target.size());
      tap.particles.resize((size_t)6 * cfg.particle_count, 0.0);
      wr(fo, tap.particles.data(), tap.particles.size());
      if (cfg.map_normals && r.aligned) wr(fo, &r.with_normal, 1);
      printf("scan %d: aligned %d  B %lld  M %lld  voxels %zu  h2d bytes so far %zu  pose t = %.4f %.4f %.4f\n", s, aligned, (long long)B,
             (long long)M, pipe.map_voxels(), pipe.bytes_h2d(), r.pose.t[0], r.pose.t[1], r.pose.t[2]);
      if (cfg.eval_dist > 0)
        printf("eval %d: %.17g %.17g %.17g %lld\n", s, r.fitness, r.inlier_rmse, r.plane_rmse, (long long)r.plane_inliers);
      if (r.information) {
        const svnicp_information& in = *r.information;
        printf("info %d: %lld %d %.17g %.17g %.17g %.17g %.17g %.17g\n", s, (long long)in.pairs, (int)in.rank, in.eigval[0], in.eigval[1],
               in.eigval[2], in.eigval[3], in.eigval[4], in.eigval[5]);
      }
      if (cfg.clear_seen_through && r.aligned) printf("clear %d: %lld\n", s, (long long)r.cleared);
      if (r.seed)
        printf("seed %d: %d %d %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", s, r.seed->searched ? 1 : 0, r.seed->levels,
               (long long)r.seed->nodes_scored, r.seed->fitness_zero, r.seed->cost_zero, r.seed->cost, r.seed->correction[0],
               r.seed->correction[1], r.seed->correction[5]);
      if (cfg.prior_sigma && r.aligned) printf("prior %d: %.17g\n", s, r.prior_chi2);
      if (r.modes) {
        const svnicp_modes& m = *r.modes;
        printf("modes %d: %d %d %d %d", s, (int)m.n_modes, (int)m.n_reported, (int)m.nonfinite, (int)m.has_scores);
        for (int k = 0; k < m.n_reported; ++k)
          printf(" | %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g", (int)m.label[k], (int)m.count[k], (int)m.best[k], m.mass[k], m.mean[k][0],
                 m.mean[k][1], m.mean[k][2], m.mean[k][3], m.mean[k][4], m.mean[k][5]);
        printf("\n");
      }
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "svnicp: %s\n", e.what());
    return 3;  // e.g. no gfx950 device: the library has no CPU path
  }
  fclose(fo); fclose(fi);
  return 0;
}
