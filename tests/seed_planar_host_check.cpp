// Stand-alone check of the planar half of csrc/seed_host.cpp, built by tests/test_seed_planar_cpu.py with
// -fsanitize=address,undefined and linked with that file only:
//
//   seed_planar_host_check records.txt seeds.txt
//
// It prints the defaults of ilcc_default_seed_planar_params, the squared thresholds (%.17g) and the frame-size bound's two sides,
// checks the refusals of seed_planar_thresholds, and then ranks records as tests/seed_host_check.cpp does, under the planar
// defaults: records.txt holds per frame "n" and n lines of 11 integers, seeds.txt gets per frame the count and one line per seed:
// key n l1 l2 rms score cx cy cz (%.17g).  Records and seeds sit in heap blocks of exactly their size.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "k15_seed.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "r");
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  ilcc_params p;
  std::memset(&p, 0, sizeof(p));
  p.cluster_tol = 0.12;
  p.cluster_min = 100;
  p.ransac_thresh = 0.03;
  p.board_w = 6;
  p.board_h = 8;
  p.grid_length = 0.15;
  ilcc_seed_params sp, plain;
  ilcc_seed_planar_params pp;
  ilcc_default_seed_params(&p, &plain);
  ilcc_default_seed_planar_params(&p, &sp, &pp);
  std::printf("defaults %.17g %.17g %.17g %.17g\n", sp.max_rms, pp.planar_rms, pp.min_spread, pp.own_rms);
  plain.max_rms = sp.max_rms;
  if (std::memcmp(&plain, &sp, sizeof(sp)) != 0) return 3;   // the rest of sp is as ilcc_default_seed_params sets it
  ilcc_default_seed_planar_params(nullptr, &sp, &pp);         // null arguments: nothing is written
  ilcc_default_seed_planar_params(&p, nullptr, &pp);
  ilcc_default_seed_planar_params(&p, &sp, nullptr);

  double a = -1, b = -1, c = -1;
  if (!ilcc::seed_planar_thresholds(pp, &a, &b, &c)) return 3;
  std::printf("thresholds %.17g %.17g %.17g\n", a, b, c);
  for (int k = 0; k < 3; ++k)
    for (double bad : {0.0, -0.01, (double)NAN, (double)INFINITY}) {
      ilcc_seed_planar_params q = pp;
      (k == 0 ? q.planar_rms : k == 1 ? q.min_spread : q.own_rms) = bad;
      double x = 7, y = 7, z = 7;
      if (ilcc::seed_planar_thresholds(q, &x, &y, &z)) return 4;
    }

  ilcc::SeedGrid g;
  if (!ilcc::seed_grid(sp, 1u << 20, &g) || g.cq != 123) return 3;
  // n 2 cq < 2^31: 8 729 608 points fit at the default cell, 8 729 609 do not
  std::printf("fits %d %d %d\n", (int)ilcc::seed_planar_frame_fits(8729608u, g), (int)ilcc::seed_planar_frame_fits(8729609u, g),
              (int)ilcc::seed_planar_frame_fits(1ull << 28, g));

  int n = 0, frames = 0;
  while (std::fscanf(in, "%d", &n) == 1) {
    int64_t* rec = (int64_t*)std::malloc(sizeof(int64_t) * ILCC_SEED_RECORD_WORDS * (size_t)(n ? n : 1));
    for (int k = 0; k < n * ILCC_SEED_RECORD_WORDS; ++k)
      if (std::fscanf(in, "%" SCNd64, &rec[k]) != 1) return 2;
    ilcc_seed* seeds = (ilcc_seed*)std::malloc(sizeof(ilcc_seed) * (size_t)sp.max_seeds);
    const int32_t got = ilcc::seed_rank(n ? rec : nullptr, n, sp, seeds);
    std::fprintf(out, "%d\n", got);
    for (int32_t k = 0; k < got; ++k)
      std::fprintf(out, "%u %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", seeds[k].key, seeds[k].n, seeds[k].l1, seeds[k].l2, seeds[k].rms,
                   seeds[k].score, (double)seeds[k].centroid[0], (double)seeds[k].centroid[1], (double)seeds[k].centroid[2]);
    std::free(seeds);
    std::free(rec);
    ++frames;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("frames %d\n", frames);
  return 0;
}
