// Stand-alone check of csrc/seed_host.cpp, built by tests/test_seed_cpu.py with -fsanitize=address,undefined and linked with
// that file only:
//
//   seed_host_check records.txt seeds.txt
//
// records.txt: one line "max_seeds size_lo size_hi max_rms", then per frame "n" and n lines of 11 integers (the records the
// restatement dumped, sorted by key).  The frame's records sit in a heap block of exactly their size, and the seeds in one of
// exactly max_seeds, so a read or write past either is a sanitizer report.  seeds.txt: per frame the count, then one line per seed:
// key n l1 l2 rms score cx cy cz (%.17g).  Every other parameter is ilcc_default_seed_params of ilcc_default_params' board.
#include <cinttypes>
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
  ilcc_seed_params sp;
  ilcc_default_seed_params(&p, &sp);
  if (std::fscanf(in, "%d %lf %lf %lf", &sp.max_seeds, &sp.size_lo, &sp.size_hi, &sp.max_rms) != 4) return 2;
  ilcc::SeedGrid g;
  if (!ilcc::seed_grid(sp, 1u << 20, &g) || g.range_q != 20480 || g.cq != 123 || g.off != 167 || g.N != 335) return 3;
  sp.range = 1e6;
  if (ilcc::seed_grid(sp, 1u << 20, &g)) return 3;   // range / cell too large
  sp.range = 20.0;
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
