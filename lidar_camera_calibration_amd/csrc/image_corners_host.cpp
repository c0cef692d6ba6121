// Structure recovery and the corner-file writer of include/ilcc_image_corners.h, on the host: a few
// hundred corners, sequential by nature.  Restated from libcbdetect/matching: chessboardsFromCorners.m
// (seeds in corner order, growth while the energy falls, keep below -10, the overlap rule),
// initChessboard.m, growChessboard.m, chessboardEnergy.m, and the dump of plotChessboards.m:48-68.
// Boards are rows x cols matrices of 0-based corner indices, stored row-major.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_image_corners.h"
#include "ilcc_image_structure.h"   // ilcc_chessboard_seed_board

namespace ilcc {

int32_t image_corners(const void* d_image, int32_t w, int32_t h, int32_t stride, ilcc_image_corner* corners, int32_t capacity,
                      int32_t* n_corners, ilcc_image_corner_stages* stages, void* stream);

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();

struct Board {
  int rows = 0, cols = 0;
  std::vector<int> idx;   // row-major; -1 = empty (initChessboard's 0)
  int& at(int r, int c) { return idx[(size_t)r * cols + c]; }
  int at(int r, int c) const { return idx[(size_t)r * cols + c]; }
  bool empty() const { return idx.empty(); }
};

struct Pt {
  double x, y;
};

struct Corners {
  std::vector<Pt> p, v1, v2;
};

// chessboardEnergy.m: -(corner count) + count * (worst collinearity ratio over row and column triples)
double energy(const Board& b, const Corners& C) {
  double es = 0;
  auto triple = [&](int i0, int i1, int i2) {
    const Pt a = C.p[i0], m = C.p[i1], c = C.p[i2];
    const double nx = a.x + c.x - 2 * m.x, ny = a.y + c.y - 2 * m.y, dx = a.x - c.x, dy = a.y - c.y;
    es = std::fmax(es, std::sqrt(nx * nx + ny * ny) / std::sqrt(dx * dx + dy * dy));
  };
  for (int r = 0; r < b.rows; ++r)
    for (int c = 0; c + 2 < b.cols; ++c) triple(b.at(r, c), b.at(r, c + 1), b.at(r, c + 2));
  for (int c = 0; c < b.cols; ++c)
    for (int r = 0; r + 2 < b.rows; ++r) triple(b.at(r, c), b.at(r + 1, c), b.at(r + 2, c));
  const double n = (double)b.rows * b.cols;
  return -n + n * es;
}

std::vector<int> unused_of(const Board& b, int n) {
  std::vector<char> used(n, 0);
  for (int i : b.idx)
    if (i >= 0) used[i] = 1;
  std::vector<int> u;
  for (int i = 0; i < n; ++i)
    if (!used[i]) u.push_back(i);
  return u;
}

// initChessboard.m directionalNeighbor: the unused corner minimising (distance along v) + 5 (distance
// off the line); corners behind count as inf; first minimum wins
int directional_neighbor(int idx, Pt v, const Board& b, const Corners& C, double& min_dist) {
  const std::vector<int> un = unused_of(b, (int)C.p.size());
  int best = un.empty() ? -1 : un[0];
  min_dist = kInf;
  bool first = true;
  for (int k : un) {
    const double dx = C.p[k].x - C.p[idx].x, dy = C.p[k].y - C.p[idx].y;
    const double d = dx * v.x + dy * v.y;
    const double ex = dx - d * v.x, ey = dy - d * v.y;
    const double de = std::sqrt(ex * ex + ey * ey);
    const double s = (d < 0 ? kInf : d) + 5 * de;
    if (first || s < min_dist) {
      min_dist = s;
      best = k;
      first = false;
    }
  }
  return best;
}

double mean(const std::vector<double>& v) {
  double s = 0;
  for (double x : v) s += x;
  return s / v.size();
}

double stdev(const std::vector<double>& v) {   // N - 1
  const double m = mean(v);
  double s = 0;
  for (double x : v) s += (x - m) * (x - m);
  return std::sqrt(s / (v.size() - 1));
}

Board init_board(const Corners& C, int idx) {
  Board b;
  if (C.p.size() < 9) return b;
  b.rows = b.cols = 3;
  b.idx.assign(9, -1);
  const Pt v1 = C.v1[idx], v2 = C.v2[idx], m1 = {-v1.x, -v1.y}, m2 = {-v2.x, -v2.y};
  b.at(1, 1) = idx;
  std::vector<double> d1(2), d2(6);
  b.at(1, 2) = directional_neighbor(idx, v1, b, C, d1[0]);
  b.at(1, 0) = directional_neighbor(idx, m1, b, C, d1[1]);
  b.at(2, 1) = directional_neighbor(idx, v2, b, C, d2[0]);
  b.at(0, 1) = directional_neighbor(idx, m2, b, C, d2[1]);
  b.at(0, 0) = directional_neighbor(b.at(1, 0), m2, b, C, d2[2]);
  b.at(2, 0) = directional_neighbor(b.at(1, 0), v2, b, C, d2[3]);
  b.at(0, 2) = directional_neighbor(b.at(1, 2), m2, b, C, d2[4]);
  b.at(2, 2) = directional_neighbor(b.at(1, 2), v2, b, C, d2[5]);
  for (double d : d1)
    if (std::isinf(d)) return Board();
  for (double d : d2)
    if (std::isinf(d)) return Board();
  if (stdev(d1) / mean(d1) > 0.3 || stdev(d2) / mean(d2) > 0.3) return Board();
  return b;
}

// growChessboard.m predictCorners: replica prediction from three points per row / column
Pt predict(Pt p1, Pt p2, Pt p3) {
  const double v1x = p2.x - p1.x, v1y = p2.y - p1.y, v2x = p3.x - p2.x, v2y = p3.y - p2.y;
  const double a1 = std::atan2(v1y, v1x), a2 = std::atan2(v2y, v2x), a3 = 2 * a2 - a1;
  const double s1 = std::sqrt(v1x * v1x + v1y * v1y), s2 = std::sqrt(v2x * v2x + v2y * v2y), s3 = 2 * s2 - s1;
  return {p3.x + 0.75 * s3 * std::cos(a3), p3.y + 0.75 * s3 * std::sin(a3)};
}

// assignClosestCorners: greedy global minimum of the distance matrix (first in column-major order);
// false when there are fewer candidates than predictions
bool assign_closest(const Corners& C, const std::vector<int>& cand, const std::vector<Pt>& pred, std::vector<int>& out) {
  const size_t nc = cand.size(), np = pred.size();
  if (nc < np) return false;
  std::vector<double> D(nc * np);   // D[col * nc + row]
  for (size_t j = 0; j < np; ++j)
    for (size_t i = 0; i < nc; ++i) {
      const double dx = C.p[cand[i]].x - pred[j].x, dy = C.p[cand[i]].y - pred[j].y;
      D[j * nc + i] = std::sqrt(dx * dx + dy * dy);
    }
  out.assign(np, -1);
  for (size_t it = 0; it < np; ++it) {
    size_t best = 0;
    for (size_t k = 1; k < D.size(); ++k)
      if (D[k] < D[best]) best = k;
    const size_t row = best % nc, col = best / nc;
    out[col] = cand[row];
    for (size_t j = 0; j < np; ++j) D[j * nc + row] = kInf;
    for (size_t i = 0; i < nc; ++i) D[col * nc + i] = kInf;
  }
  return true;
}

// border 1: new last column, 2: new last row, 3: new first column, 4: new first row
Board grow(const Board& b, const Corners& C, int border) {
  if (b.empty()) return b;
  const std::vector<int> un = unused_of(b, (int)C.p.size());
  std::vector<Pt> pred;
  const bool col = border == 1 || border == 3;
  const int len = col ? b.rows : b.cols;
  for (int k = 0; k < len; ++k) {
    int i1, i2, i3;
    if (border == 1) { i1 = b.at(k, b.cols - 3); i2 = b.at(k, b.cols - 2); i3 = b.at(k, b.cols - 1); }
    else if (border == 2) { i1 = b.at(b.rows - 3, k); i2 = b.at(b.rows - 2, k); i3 = b.at(b.rows - 1, k); }
    else if (border == 3) { i1 = b.at(k, 2); i2 = b.at(k, 1); i3 = b.at(k, 0); }
    else { i1 = b.at(2, k); i2 = b.at(1, k); i3 = b.at(0, k); }
    pred.push_back(predict(C.p[i1], C.p[i2], C.p[i3]));
  }
  std::vector<int> got;
  if (!assign_closest(C, un, pred, got)) return b;
  Board n;
  n.rows = b.rows + (col ? 0 : 1);
  n.cols = b.cols + (col ? 1 : 0);
  n.idx.assign((size_t)n.rows * n.cols, -1);
  const int r0 = border == 4 ? 1 : 0, c0 = border == 3 ? 1 : 0;
  for (int r = 0; r < b.rows; ++r)
    for (int c = 0; c < b.cols; ++c) n.at(r + r0, c + c0) = b.at(r, c);
  for (int k = 0; k < len; ++k) {
    if (border == 1) n.at(k, n.cols - 1) = got[k];
    else if (border == 2) n.at(n.rows - 1, k) = got[k];
    else if (border == 3) n.at(k, 0) = got[k];
    else n.at(0, k) = got[k];
  }
  return n;
}

// the board seed i grows to while the energy falls (empty: initChessboard rejected it, or its 3 x 3 board is above 0)
Board seed_board(const Corners& C, int i) {
  Board b = init_board(C, i);
  if (b.empty() || energy(b, C) > 0) return Board();
  for (;;) {
    const double e = energy(b, C);
    Board prop[4];
    double pe[4];
    for (int j = 0; j < 4; ++j) {
      prop[j] = grow(b, C, j + 1);
      pe[j] = energy(prop[j], C);
    }
    int mi = 0;
    for (int j = 1; j < 4; ++j)
      if (pe[j] < pe[mi]) mi = j;
    if (pe[mi] < e) b = prop[mi];
    else break;
  }
  return b;
}

std::vector<Board> chessboards_from_corners(const Corners& C) {
  std::vector<Board> boards;
  for (int i = 0; i < (int)C.p.size(); ++i) {
    const Board b = seed_board(C, i);
    if (b.empty()) continue;
    const double eb = energy(b, C);
    if (!(eb < -10)) continue;
    std::vector<int> over;
    std::vector<double> over_e;
    for (size_t j = 0; j < boards.size(); ++j) {
      bool hit = false;
      for (int a : boards[j].idx) {
        for (int c : b.idx) hit |= a == c;
        if (hit) break;
      }
      if (hit) {
        over.push_back((int)j);
        over_e.push_back(energy(boards[j], C));
      }
    }
    if (over.empty()) {
      boards.push_back(b);
    } else {
      bool keep_old = false;
      for (double oe : over_e) keep_old |= oe <= eb;
      if (!keep_old) {
        for (size_t k = over.size(); k-- > 0;) boards.erase(boards.begin() + over[k]);
        boards.push_back(b);
      }
    }
  }
  return boards;
}

}  // namespace
}  // namespace ilcc

extern "C" int32_t ilcc_chessboard_from_corners(const ilcc_image_corner* corners, int32_t n_corners, int32_t board_w,
                                                int32_t board_h, int32_t* rows, int32_t* cols, int32_t* board_index) {
  if ((n_corners > 0 && !corners) || n_corners < 0 || !rows || !cols || !board_index || board_w < 3 || board_h < 3)
    return ilcc::fail(ILCC_BAD_ARGUMENT, "ilcc_chessboard_from_corners: bad argument");
  ilcc::Corners C;
  for (int i = 0; i < n_corners; ++i) {
    C.p.push_back({corners[i].u, corners[i].v});
    C.v1.push_back({corners[i].v1[0], corners[i].v1[1]});
    C.v2.push_back({corners[i].v2[0], corners[i].v2[1]});
  }
  const std::vector<ilcc::Board> boards = ilcc::chessboards_from_corners(C);
  const ilcc::Board* hit = nullptr;
  int n_hit = 0;
  for (const auto& b : boards)
    if ((b.rows == board_w && b.cols == board_h) || (b.rows == board_h && b.cols == board_w)) {
      hit = &b;
      ++n_hit;
    }
  *rows = *cols = 0;
  if (n_hit == 0)
    return ilcc::fail(ILCC_BOARD_NOT_FOUND, "no " + std::to_string(board_w) + " x " + std::to_string(board_h) + " board among " +
                                                std::to_string(boards.size()) + " recovered from " + std::to_string(n_corners) + " corners");
  if (n_hit > 1)
    return ilcc::fail(ILCC_AMBIGUOUS, std::to_string(n_hit) + " boards of " + std::to_string(board_w) + " x " + std::to_string(board_h) + " recovered");
  *rows = hit->rows;
  *cols = hit->cols;
  for (size_t k = 0; k < hit->idx.size(); ++k) board_index[k] = hit->idx[k];
  return ILCC_OK;
}

extern "C" int32_t ilcc_chessboard_seed_board(const ilcc_image_corner* corners, int32_t n_corners, int32_t seed, int32_t* rows,
                                              int32_t* cols, int32_t* index, int32_t cap, double* energy) {
  if (!corners || n_corners <= 0 || seed < 0 || seed >= n_corners || !rows || !cols || !energy || cap < 0 || (cap > 0 && !index))
    return ilcc::fail(ILCC_BAD_ARGUMENT, "ilcc_chessboard_seed_board: bad argument");
  ilcc::Corners C;
  for (int i = 0; i < n_corners; ++i) {
    C.p.push_back({corners[i].u, corners[i].v});
    C.v1.push_back({corners[i].v1[0], corners[i].v1[1]});
    C.v2.push_back({corners[i].v2[0], corners[i].v2[1]});
  }
  const ilcc::Board b = ilcc::seed_board(C, seed);
  *rows = b.rows;
  *cols = b.cols;
  *energy = b.empty() ? 0.0 : ilcc::energy(b, C);
  if (b.empty()) {
    *rows = *cols = 0;
    return ILCC_OK;
  }
  if ((size_t)cap < b.idx.size()) return ilcc::fail(ILCC_CAPACITY, "ilcc_chessboard_seed_board: the board has more cells than index holds");
  for (size_t k = 0; k < b.idx.size(); ++k) index[k] = b.idx[k];
  return ILCC_OK;
}

extern "C" int32_t ilcc_find_chessboard_device(const void* d_image, int32_t width, int32_t height, int32_t stride,
                                               int32_t board_w, int32_t board_h, int32_t* rows, int32_t* cols, double* xy,
                                               void* hip_stream) {
  if (!rows || !cols || !xy || board_w < 3 || board_h < 3) return ilcc::fail(ILCC_BAD_ARGUMENT, "ilcc_find_chessboard_device: bad argument");
  *rows = *cols = 0;
  std::vector<ilcc_image_corner> c(4096);
  int32_t n = 0;
  int32_t st = ilcc::image_corners(d_image, width, height, stride, c.data(), (int32_t)c.size(), &n, nullptr, hip_stream);
  if (st == ILCC_CAPACITY) {
    c.resize((size_t)n);
    st = ilcc::image_corners(d_image, width, height, stride, c.data(), n, &n, nullptr, hip_stream);
  }
  if (st != ILCC_OK) return st;
  std::vector<int32_t> idx((size_t)board_w * board_h);
  int32_t r = 0, k = 0;
  st = ilcc_chessboard_from_corners(c.data(), n, board_w, board_h, &r, &k, idx.data());
  if (st != ILCC_OK) return st;
  for (size_t i = 0; i < idx.size(); ++i) {
    xy[2 * i] = c[idx[i]].u;
    xy[2 * i + 1] = c[idx[i]].v;
  }
  *rows = r;
  *cols = k;
  return ILCC_OK;
}

extern "C" int32_t ilcc_save_cam_corners(const char* filename, int32_t rows, int32_t cols, const double* xy) {
  if (!filename || !xy || rows <= 0 || cols <= 0) return ilcc::fail(ILCC_BAD_ARGUMENT, "ilcc_save_cam_corners: bad argument");
  FILE* f = std::fopen(filename, "wb");
  if (!f) return ilcc::fail(ILCC_IO_ERROR, std::string("cannot write ") + filename);
  for (int axis = 0; axis < 2; ++axis)
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        std::fprintf(f, c + 1 < cols ? "%.5g " : "%.5g\n", xy[2 * ((size_t)r * cols + c) + axis] + 1);
  if (std::fclose(f) != 0) return ilcc::fail(ILCC_IO_ERROR, std::string("cannot write ") + filename);
  return ILCC_OK;
}
