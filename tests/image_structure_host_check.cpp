// Stand-alone check of the structure recovery in csrc/image_corners_host.cpp, built by tests/test_image_structure_cpu.py with
// -fsanitize=address,undefined and linked with that file only (the two names it takes from the rest of the library are stood in
// for below):
//
//   image_structure_host_check corners.txt boards.txt
//
// corners.txt: per case a line "n board_w board_h", then n lines "u v v1x v1y v2x v2y" (%.17g).  The corners sit in a heap block of
// exactly their size and every index output in one of exactly the size it is announced with, so a read or write past either is a
// sanitizer report.  boards.txt: per case "status rows cols" and the index matrix of ilcc_chessboard_from_corners on one line, then
// per seed "rows cols energy" (%.17g) and the indices of ilcc_chessboard_seed_board.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ilcc_hip.h"
#include "ilcc_image_corners.h"
#include "ilcc_image_structure.h"

namespace ilcc {
void set_global_error(const std::string&) {}
int32_t image_corners(const void*, int32_t, int32_t, int32_t, ilcc_image_corner*, int32_t, int32_t*, ilcc_image_corner_stages*, void*) {
  return ILCC_HIP_ERROR;   // ilcc_find_chessboard_device is not under test: no device here
}
}  // namespace ilcc

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "r");
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  int n = 0, bw = 0, bh = 0, cases = 0;
  while (std::fscanf(in, "%d %d %d", &n, &bw, &bh) == 3) {
    ilcc_image_corner* c = (ilcc_image_corner*)std::malloc(sizeof(ilcc_image_corner) * (size_t)(n ? n : 1));
    for (int i = 0; i < n; ++i) {
      if (std::fscanf(in, "%lf %lf %lf %lf %lf %lf", &c[i].u, &c[i].v, &c[i].v1[0], &c[i].v1[1], &c[i].v2[0], &c[i].v2[1]) != 6) return 2;
      c[i].score = 1.0;
    }
    int32_t* idx = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)bw * bh);
    int32_t rows = -1, cols = -1;
    const int32_t st = ilcc_chessboard_from_corners(n ? c : nullptr, n, bw, bh, &rows, &cols, idx);
    std::fprintf(out, "%d %d %d", st, rows, cols);
    for (int k = 0; st == ILCC_OK && k < rows * cols; ++k) std::fprintf(out, " %d", idx[k]);
    std::fprintf(out, "\n");
    std::free(idx);
    for (int seed = 0; seed < n; ++seed) {
      double e = 0;
      // first with room for nothing: the shape comes back with ILCC_CAPACITY, then a block of exactly that size
      int32_t s = ilcc_chessboard_seed_board(c, n, seed, &rows, &cols, nullptr, 0, &e);
      if (s != ILCC_OK && s != ILCC_CAPACITY) return 3;
      if ((s == ILCC_CAPACITY) != (rows * cols > 0)) return 3;
      int32_t* cells = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)(rows * cols ? rows * cols : 1));
      if (ilcc_chessboard_seed_board(c, n, seed, &rows, &cols, cells, rows * cols, &e) != ILCC_OK) return 3;
      std::fprintf(out, "%d %d %.17g", rows, cols, e);
      for (int k = 0; k < rows * cols; ++k) std::fprintf(out, " %d", cells[k]);
      std::fprintf(out, "\n");
      std::free(cells);
    }
    if (n > 0) {   // refusals read nothing
      double e = 0;
      if (ilcc_chessboard_seed_board(c, n, n, &rows, &cols, nullptr, 0, &e) != ILCC_BAD_ARGUMENT) return 3;
      if (ilcc_chessboard_seed_board(c, n, -1, &rows, &cols, nullptr, 0, &e) != ILCC_BAD_ARGUMENT) return 3;
      if (ilcc_chessboard_seed_board(nullptr, n, 0, &rows, &cols, nullptr, 0, &e) != ILCC_BAD_ARGUMENT) return 3;
    }
    std::free(c);
    ++cases;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("cases %d\n", cases);
  return 0;
}
