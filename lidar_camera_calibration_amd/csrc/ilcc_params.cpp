// ilcc_params.cpp -- the part of the C-ABI (include/ilcc_hip.h) that needs neither a handle nor the HIP runtime: the parameter
// set (defaults, validation, the camera YAML's three keys), the status texts, the ABI version, and the two corner-file contracts.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "host_util.h"
#include "ilcc_internal.h"   // (the kernels' limits that params_ok enforces: kGridTableMax, kCoverageCellsMax)

namespace ilcc {

// what ilcc_create / ilcc_set_params accept: everything the kernels can run
bool params_ok(const ilcc_params& p, std::string& why) {
  auto bad = [&](const char* m) {
    why = m;
    return false;
  };
  if (!(p.grid_length > 0)) return bad("grid_length must be > 0");
  if (p.board_w < 2 || p.board_h < 2 || p.board_w > p.board_h) return bad("board_w/board_h: need 2 <= w <= h");
  if ((p.board_w - 1) * (p.board_h - 1) > ILCC_MAX_CORNERS) return bad("too many corners");
  if (p.hist_bins < 1 || p.hist_bins > 4096) return bad("hist_bins out of range");
  if (!(p.gray_rate > 0) || !(p.huber_delta > 0)) return bad("gray_rate / huber_delta must be > 0");
  if (p.ransac_hyp < 1 || p.ransac_hyp > 65536) return bad("ransac_hyp out of range");
  if (!(p.ransac_probability == p.ransac_probability) || p.ransac_probability >= 1.0) return bad("ransac_probability must be < 1");
  if (!(p.cluster_tol > 0) || p.cluster_min < 1 || p.cluster_max < p.cluster_min) return bad("cluster params");
  if (p.solver != ILCC_SOLVER_REFERENCE_LOCAL && p.solver != ILCC_SOLVER_GRID) return bad("solver");
  if (p.phase_mode < 0 || p.phase_mode > 2) return bad("phase_mode");
  if (p.grid_prune != 0 && p.grid_prune != 1) return bad("grid_prune must be 0 or 1");
  if (p.max_iterations < 0 || p.max_iterations > 100000) return bad("max_iterations");
  if (p.n_th < 1 || p.n_ty < 1 || p.n_tz < 1) return bad("grid sizes must be >= 1");
  if (p.n_th > 4096 || p.n_ty > 4096 || p.n_tz > 4096) return bad("grid axes are limited to 4096 candidates");
  // K6 keeps the (ty, tz) tables in LDS behind the staged points: the raised dynamic-LDS limit covers kGridTableMax floats
  if (p.n_ty + p.n_tz > kGridTableMax) return bad("n_ty + n_tz exceeds the LDS table capacity of the grid kernel");
  if (p.refine_div < 0 || p.refine_div > 64 || (p.refine_div & (p.refine_div - 1)) != 0)
    return bad("refine_div must be 0 or a power of two <= 64");
  if (p.refine_max_rounds < 0 || p.refine_max_rounds > 4096) return bad("refine_max_rounds");
  if (p.refine_th_margin < 0 || p.refine_th_margin > 4096) return bad("refine_th_margin");
  if (!(p.online_cluster_tol > 0)) return bad("online_cluster_tol must be > 0");
  if (!(p.ambiguity_eps == p.ambiguity_eps)) return bad("ambiguity_eps is NaN");
  if (!(p.min_cell_coverage == p.min_cell_coverage) || p.min_cell_coverage > 1.0) return bad("min_cell_coverage must be <= 1");
  if (p.board_w * p.board_h > kCoverageCellsMax) return bad("board has more squares than the coverage mask holds");
  if ((uint64_t)p.n_th * p.n_ty * p.n_tz * 2ull >= 0xFFFFFFFFull) return bad("grid too large");
  if (!(p.th_step > 0) || !(p.ty_step > 0) || !(p.tz_step > 0)) return bad("grid steps must be > 0");
  {
    // K7r's basin check compares with the positions ONE SQUARE away: lround(g / (step / div)) lattice units.  A step so
    // coarse that this rounds to 0 would compare the centre with itself (margin 0: every frame ILCC_AMBIGUOUS)
    const double div = (double)(p.refine_div > 0 ? p.refine_div : 1);
    if (std::lround(p.grid_length / (p.ty_step / div)) < 1 || std::lround(p.grid_length / (p.tz_step / div)) < 1)
      return bad("ty_step / tz_step too coarse: one board square is less than half a refinement-lattice step");
  }
  return true;
}

}  // namespace ilcc

extern "C" {

int32_t ilcc_abi_version(void) { return ILCC_ABI_VERSION; }

const char* ilcc_strerror(int32_t status) {
  switch (status) {
    case ILCC_OK: return "ok";
    case ILCC_NO_ROI_POINTS: return "no points inside the ROI box around the click";
    case ILCC_NO_CLUSTER: return "no Euclidean cluster of admissible size";
    case ILCC_NO_PLANE: return "could not estimate a planar model";
    case ILCC_DEGENERATE_HIST: return "intensity histogram is degenerate (no bin on one side of the mean)";
    case ILCC_TOO_FEW_POINTS: return "too few points";
    case ILCC_BAD_ARGUMENT: return "bad argument";
    case ILCC_CAPACITY: return "handle capacity exceeded";
    case ILCC_HIP_ERROR: return "HIP runtime error";
    case ILCC_IO_ERROR: return "file I/O error";
    case ILCC_BOARD_NOT_FOUND: return "no chessboard plane of sufficient size around the given point";
    case ILCC_AMBIGUOUS: return "board position ambiguous: a basin one square away costs about the same";
    default: return "unknown status";
  }
}

void ilcc_default_params(ilcc_params* p) {
  std::memset(p, 0, sizeof(*p));
  p->roi_half[0] = 1.0;
  p->roi_half[1] = 1.5;
  p->roi_half[2] = 2.0;
  p->cluster_tol = 0.12;
  p->cluster_min = 100;
  p->cluster_max = 25000;
  p->ransac_thresh = 0.03;
  p->ransac_hyp = 50;            // SACSegmentation: max_iterations_
  p->ransac_probability = 0.99;  // SACSegmentation: probability_
  p->ransac_seed = 12345u;
  p->hist_bins = 100;
  p->gray_rate = 2.5;
  p->huber_delta = 0.1;
  p->grid_length = 0.15;
  p->board_w = 6;
  p->board_h = 8;
  p->solver = ILCC_SOLVER_GRID;
  p->phase_mode = 2;
  p->max_iterations = 50;
  p->grid_prune = 1;
  const double kPi = 3.14159265358979323846;
  p->n_th = 61;
  p->th_step = 0.5 * kPi / 180.0;
  p->th_min = -15.0 * kPi / 180.0;
  p->n_ty = 40;
  p->ty_step = 0.15 / 20.0;
  p->ty_min = -0.15;
  p->n_tz = 40;
  p->tz_step = 0.15 / 20.0;
  p->tz_min = -0.15;
  p->refine_div = 16;
  p->refine_max_rounds = 64;
  p->refine_th_margin = 32;
  p->ambiguity_eps = 1.0;
  p->online_cluster_tol = 0.10;   // LidarCornersEst.cpp:80
  p->min_cell_coverage = 0.9;
}

// Minimal OpenCV-FileStorage YAML reader for the three scalar keys the path uses
// (cv::FileStorage is not available; ilcc2/config/pointgrey.yaml:17-19).
int32_t ilcc_set_chessboard_param(ilcc_params* p, const char* cam_yaml) {
  if (!p || !cam_yaml) return ILCC_BAD_ARGUMENT;
  std::ifstream in(cam_yaml);
  if (!in.is_open()) {
    ilcc::set_global_error(std::string("can not open ") + cam_yaml);   // LidarCornersEst.cpp:27
    return ILCC_IO_ERROR;
  }
  double grid_length = -1;
  long cx = -1, cy = -1;
  std::string line;
  while (std::getline(in, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    const size_t colon = line.find(':');
    if (colon == std::string::npos) continue;
    std::string key = line.substr(0, colon), val = line.substr(colon + 1);
    auto trim = [](std::string& s) {
      const size_t a = s.find_first_not_of(" \t\r\n");
      const size_t b = s.find_last_not_of(" \t\r\n");
      s = (a == std::string::npos) ? std::string() : s.substr(a, b - a + 1);
    };
    trim(key);
    trim(val);
    if (val.empty()) continue;
    char* endp = nullptr;
    if (key == "grid_length") grid_length = std::strtod(val.c_str(), &endp);
    else if (key == "corner_in_x") cx = (long)std::strtod(val.c_str(), &endp);
    else if (key == "corner_in_y") cy = (long)std::strtod(val.c_str(), &endp);
  }
  if (!(grid_length > 0) || cx < 1 || cy < 1) {
    ilcc::set_global_error("grid_length / corner_in_x / corner_in_y missing or invalid");
    return ILCC_BAD_ARGUMENT;
  }
  int32_t w = (int32_t)cx + 1, hh = (int32_t)cy + 1;   // :31-32
  if (w > hh) std::swap(w, hh);                        // :35-39
  // keep the default grid's meaning (one cell either way, g/20 steps) when the square size changes
  const double scale = grid_length / p->grid_length;
  p->grid_length = grid_length;
  p->board_w = w;
  p->board_h = hh;
  if (scale > 0 && scale != 1.0) {
    p->ty_min *= scale;
    p->ty_step *= scale;
    p->tz_min *= scale;
    p->tz_step *= scale;
  }
  return ILCC_OK;
}

// get_lidar_corners.cpp:27-36 -- ofstream(trunc), `x << " " << y << " " << z << endl` with the
// stream's default float formatting (precision 6).
int32_t ilcc_save_corners2txt(const float* corners_xyz, uint32_t n_corners, const char* filename) {
  if (!corners_xyz || !filename) return ILCC_BAD_ARGUMENT;
  std::ofstream outfile(filename, std::ios_base::trunc);
  if (!outfile.is_open()) return ILCC_IO_ERROR;
  for (uint32_t i = 0; i < n_corners; ++i)
    outfile << corners_xyz[3 * i] << " " << corners_xyz[3 * i + 1] << " " << corners_xyz[3 * i + 2] << std::endl;
  outfile.close();
  return outfile.fail() ? ILCC_IO_ERROR : ILCC_OK;
}

// ImageCornersEst.cpp:281-299 -- `float x,y,z; infile >> x >> y >> z` until eof or num corners
int32_t ilcc_read_lidar_corners(const char* filename, uint32_t num, double* out_xyz) {
  if (!filename || !out_xyz) return -ILCC_BAD_ARGUMENT;
  std::ifstream infile(filename);
  if (!infile.is_open()) return -ILCC_IO_ERROR;
  uint32_t counter = 0;
  while (!infile.eof() && counter < num) {
    float x = 0, y = 0, z = 0;
    infile >> x >> y >> z;
    if (infile.fail()) break;
    out_xyz[3 * counter] = x;
    out_xyz[3 * counter + 1] = y;
    out_xyz[3 * counter + 2] = z;
    ++counter;
  }
  return (int32_t)counter;
}

}  // extern "C"
