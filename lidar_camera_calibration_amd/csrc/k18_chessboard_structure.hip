// K18 chessboard structure recovery of a BATCH of corner lists (include/ilcc_image_structure.h): chessboardsFromCorners.m as
// image_corners_host.cpp restates it, with every (image, seed corner) pair grown on a wavefront of its own.
//
//   k18_grow    grid (seed groups, images), 4 wavefronts a workgroup, all on seeds of ONE image whose positions the workgroup
//               stages once in LDS (16 B a corner; 4 096 corners are 64 KB).  A wavefront keeps its state in registers: the "used"
//               set as one 64-bit word per lane (corner k is bit k / 64 of lane k % 64), the board as four cells per lane (cell c
//               is slot c / 64 of lane c % 64, read with a cross-lane shuffle).  init_board, then the grow loop; the seed's board
//               and energy go to the plan's per-seed store.
//   k18_select  grid (images), one wavefront: the seeds in corner order through the keep-below--10 test and the overlap rule with
//               an owner[corner] array in LDS, then the one board of the requested shape.
//
// Every loop has a static bound: n_corners grow steps a seed, one assignment round per prediction (<= 64), 64 seeds per ballot
// word.  A seed that meets a bound or whose proposal exceeds a board capacity marks its image; the host recomputes marked images
// with ilcc_chessboard_from_corners.  Compiled with -ffp-contract=off like the host file: the energies are the host's bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "host_util.h"
#include "ilcc_image_structure.h"

using namespace ilcc;

namespace {

constexpr int kWave = 64, kGrowWaves = 4;
constexpr int kMaxCorners = ILCC_STRUCTURE_MAX_CORNERS, kMaxCells = ILCC_STRUCTURE_MAX_CELLS, kMaxSide = ILCC_STRUCTURE_MAX_SIDE;
static_assert(kMaxCorners == kWave * 64, "the used set is one 64-bit word per lane");
static_assert(kMaxCells == kWave * 4, "the board is four cells per lane");
static_assert(kMaxSide <= kWave, "one prediction per lane");
static_assert(kMaxCorners <= 32767, "cells are stored as int16");

struct PackedCorner {   // what the device reads of an ilcc_image_corner
  double u, v, v1x, v1y, v2x, v2y;
};
struct ImageRow {
  uint32_t first;   // of the image's corners in the packed list
  int32_t n;        // corners on the device path (0 for an image the host marked)
  int32_t flag;     // != 0: marked, the host recomputes it
  int32_t pad;
};
struct SeedMeta {
  double energy;
  int32_t rows, cols;   // 0: the seed has no board
};
struct ImageOut {
  int32_t status, rows, cols, flag;
  int32_t idx[kMaxCells];
};

struct BoardRegs {
  int c[4];
};

__device__ inline double dinf() { return __longlong_as_double(0x7ff0000000000000ll); }

// cell `cell` (any per lane, 0 .. 255) of the board; every lane of the wavefront must call it
__device__ inline int board_get(const BoardRegs& b, int cell) {
  const int src = cell & 63, s = cell >> 6;
  const int v0 = __shfl(b.c[0], src), v1 = __shfl(b.c[1], src), v2 = __shfl(b.c[2], src), v3 = __shfl(b.c[3], src);
  return s == 0 ? v0 : s == 1 ? v1 : s == 2 ? v2 : v3;
}

__device__ inline void board_set(BoardRegs& b, int cell, int value, int lane) {   // cell, value: wave-uniform
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (lane == (cell & 63) && (cell >> 6) == s) b.c[s] = value;
}

// the least (d, j, k) in lexicographic order over the wavefront, in every lane; a lane without a candidate holds (inf, INT_MAX, INT_MAX)
__device__ inline void wave_min(double& d, int& j, int& k) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double od = __shfl_xor(d, off);
    const int oj = __shfl_xor(j, off), ok = __shfl_xor(k, off);
    if (od < d || (od == d && (oj < j || (oj == j && ok < k)))) {
      d = od;
      j = oj;
      k = ok;
    }
  }
  d = __shfl(d, 0);
  j = __shfl(j, 0);
  k = __shfl(k, 0);
}

// directionalNeighbor: the unused corner minimising (distance along v) + 5 (distance off the line); corners behind count as inf; the
// first minimum in ascending corner index, the lowest unused corner when every score is inf
__device__ inline int neighbor(const double2* pos, int n, int idx, double vx, double vy, uint64_t used, int lane, double* min_dist) {
  const double2 b = pos[idx];
  double bs = dinf();
  int bk = INT_MAX, bj = 0;
  for (int i = 0, k = lane; k < n; ++i, k += kWave) {
    if ((used >> i) & 1) continue;
    const double2 p = pos[k];
    const double dx = p.x - b.x, dy = p.y - b.y;
    const double d = dx * vx + dy * vy;
    const double ex = dx - d * vx, ey = dy - d * vy;
    const double de = __dsqrt_rn(ex * ex + ey * ey);
    const double s = (d < 0 ? dinf() : d) + 5 * de;
    if (bk == INT_MAX || s < bs) {
      bs = s;
      bk = k;
    }
  }
  wave_min(bs, bj, bk);
  *min_dist = bs;
  return bk;
}

// chessboardEnergy: -(cells) + cells * (worst collinearity ratio over row triples, then column triples); a maximum, so the lanes take
// the triples in any order
__device__ inline double board_energy(const double2* pos, const BoardRegs& b, int R, int C, int lane) {
  const int nrow = R * (C - 2), total = nrow + C * (R - 2);
  double es = 0;
  for (int t0 = 0; t0 < total; t0 += kWave) {
    const bool live = t0 + lane < total;
    const int t = live ? t0 + lane : 0;
    int c0, step;
    if (t < nrow) {
      c0 = (t / (C - 2)) * C + t % (C - 2);
      step = 1;
    } else {
      const int u = t - nrow;
      c0 = (u % (R - 2)) * C + u / (R - 2);
      step = C;
    }
    const int i0 = board_get(b, c0), i1 = board_get(b, c0 + step), i2 = board_get(b, c0 + 2 * step);
    if (live) {
      const double2 a = pos[i0], m = pos[i1], c = pos[i2];
      const double nx = a.x + c.x - 2 * m.x, ny = a.y + c.y - 2 * m.y, dx = a.x - c.x, dy = a.y - c.y;
      es = fmax(es, __ddiv_rn(__dsqrt_rn(nx * nx + ny * ny), __dsqrt_rn(dx * dx + dy * dy)));
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) es = fmax(es, __shfl_xor(es, off));
  const double n = (double)R * C;
  return -n + n * es;
}

// growChessboard predictCorners
__device__ inline double2 predict(double2 p1, double2 p2, double2 p3) {
  const double v1x = p2.x - p1.x, v1y = p2.y - p1.y, v2x = p3.x - p2.x, v2y = p3.y - p2.y;
  const double a1 = atan2(v1y, v1x), a2 = atan2(v2y, v2x), a3 = 2 * a2 - a1;
  const double s1 = __dsqrt_rn(v1x * v1x + v1y * v1y), s2 = __dsqrt_rn(v2x * v2x + v2y * v2y), s3 = 2 * s2 - s1;
  return make_double2(p3.x + 0.75 * s3 * cos(a3), p3.y + 0.75 * s3 * sin(a3));
}

enum { kProposed = 0, kNoProposal = 1, kOver = 2 };

// growChessboard on border 1 .. 4 (new last column, last row, first column, first row): lane k's *got is the corner of the border's
// entry k, *taken the used set with the border in it.  assignClosestCorners is the greedy global minimum, once per prediction, with
// the distances computed again every round; the first minimum in column-major order is the lower prediction, then the lower corner.
__device__ inline int propose(const double2* pos, int n, const BoardRegs& b, int R, int C, int border, uint64_t used, int lane, int* got,
                              uint64_t* taken_out) {
  const bool col = border == 1 || border == 3;
  const int len = col ? R : C;
  if (n - R * C < len) return kNoProposal;   // fewer candidates than predictions: the host leaves the board as it is
  if (len > kMaxSide || (R + (col ? 0 : 1)) * (C + (col ? 1 : 0)) > kMaxCells) return kOver;
  const int k = lane < len ? lane : 0;
  int c1, c2, c3;
  if (border == 1) { c1 = k * C + C - 3; c2 = c1 + 1; c3 = c1 + 2; }
  else if (border == 2) { c1 = (R - 3) * C + k; c2 = c1 + C; c3 = c2 + C; }
  else if (border == 3) { c1 = k * C + 2; c2 = c1 - 1; c3 = c1 - 2; }
  else { c1 = 2 * C + k; c2 = C + k; c3 = k; }
  const int i1 = board_get(b, c1), i2 = board_get(b, c2), i3 = board_get(b, c3);
  const double2 pred = predict(pos[i1], pos[i2], pos[i3]);
  uint64_t taken = used, live = len == 64 ? ~0ull : (1ull << len) - 1;
  int mine = -1;
  for (int it = 0; it < len; ++it) {
    double bd = dinf();
    int bj = INT_MAX, bk = INT_MAX;
    for (int j = 0; j < len; ++j) {
      if (!((live >> j) & 1)) continue;
      const double qx = __shfl(pred.x, j), qy = __shfl(pred.y, j);
      for (int i = 0, kk = lane; kk < n; ++i, kk += kWave) {
        if ((taken >> i) & 1) continue;
        const double2 p = pos[kk];
        const double dx = p.x - qx, dy = p.y - qy;
        const double d = __dsqrt_rn(dx * dx + dy * dy);
        if (d < bd) {
          bd = d;
          bj = j;
          bk = kk;
        }
      }
    }
    wave_min(bd, bj, bk);
    if (bk == INT_MAX) return kOver;   // no finite distance left: not a case the host's matrix is defined for
    if (lane == bj) mine = bk;
    if ((bk & 63) == lane) taken |= 1ull << (bk >> 6);
    live &= ~(1ull << bj);
  }
  *got = mine;
  *taken_out = taken;
  return kProposed;
}

// the board with the proposal's border attached
__device__ inline BoardRegs with_border(const BoardRegs& b, int R, int C, int border, int got, int lane) {
  const bool col = border == 1 || border == 3;
  const int R2 = R + (col ? 0 : 1), C2 = C + (col ? 1 : 0), r0 = border == 4 ? 1 : 0, c0 = border == 3 ? 1 : 0;
  BoardRegs nb;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cell = s * kWave + lane;
    const bool valid = cell < R2 * C2;
    const int r = valid ? cell / C2 : 0, c = valid ? cell % C2 : 0;
    const int ro = r - r0, co = c - c0;
    const bool inside = ro >= 0 && ro < R && co >= 0 && co < C;
    const int old = board_get(b, inside ? ro * C + co : 0);
    const int g = __shfl(got, (col ? r : c) & 63);
    nb.c[s] = !valid ? -1 : inside ? old : g;
  }
  return nb;
}

__global__ __launch_bounds__(kWave* kGrowWaves) void k18_grow(ImageRow* images, const PackedCorner* corners, SeedMeta* meta, int16_t* cells,
                                                              uint32_t max_c, uint32_t cell_stride) {
  extern __shared__ double2 pos[];
  const uint32_t img = blockIdx.y;
  const int n = images[img].n;
  const int seed0 = (int)blockIdx.x * kGrowWaves;
  if (seed0 >= n) return;   // the whole workgroup
  const PackedCorner* pc = corners + images[img].first;
  for (int i = threadIdx.x; i < n; i += kWave * kGrowWaves) pos[i] = make_double2(pc[i].u, pc[i].v);
  __syncthreads();
  const int lane = threadIdx.x & 63, seed = seed0 + (int)(threadIdx.x >> 6);
  if (seed >= n) return;   // the whole wavefront; no barrier below
  SeedMeta* out = meta + (size_t)img * max_c + seed;
  int16_t* out_cells = cells + ((size_t)img * max_c + seed) * cell_stride;
  if (lane == 0) *out = SeedMeta{0.0, 0, 0};
  if (n < 9) return;

  // initChessboard
  const double v1x = pc[seed].v1x, v1y = pc[seed].v1y, v2x = pc[seed].v2x, v2y = pc[seed].v2y;
  uint64_t used = 0;
  BoardRegs b = {{-1, -1, -1, -1}};
  double d1[2], d2[6];
  bool rejected = false;
  auto take = [&](int cell, int from, double vx, double vy, double* dist) -> int {
    const int k = neighbor(pos, n, from, vx, vy, used, lane, dist);
    if (k == INT_MAX) {   // no unused corner: cannot happen with n >= 9, and must not index anything if it does
      rejected = true;
      return from;
    }
    if ((k & 63) == lane) used |= 1ull << (k >> 6);
    board_set(b, cell, k, lane);
    rejected |= isinf(*dist);
    return k;
  };
  board_set(b, 4, seed, lane);
  if ((seed & 63) == lane) used |= 1ull << (seed >> 6);
  const int right = take(5, seed, v1x, v1y, &d1[0]);
  if (rejected) return;
  const int left = take(3, seed, -v1x, -v1y, &d1[1]);
  if (rejected) return;
  take(7, seed, v2x, v2y, &d2[0]);
  if (rejected) return;
  take(1, seed, -v2x, -v2y, &d2[1]);
  if (rejected) return;
  take(0, left, -v2x, -v2y, &d2[2]);
  if (rejected) return;
  take(6, left, v2x, v2y, &d2[3]);
  if (rejected) return;
  take(2, right, -v2x, -v2y, &d2[4]);
  if (rejected) return;
  take(8, right, v2x, v2y, &d2[5]);
  if (rejected) return;
  {   // mean and N - 1 standard deviation, summed in index order as the host does
    double s = 0;
    s += d1[0];
    s += d1[1];
    const double m1 = __ddiv_rn(s, 2.0);
    s = 0;
    s += (d1[0] - m1) * (d1[0] - m1);
    s += (d1[1] - m1) * (d1[1] - m1);
    const double sd1 = __dsqrt_rn(__ddiv_rn(s, 1.0));
    s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += d2[i];
    const double m2 = __ddiv_rn(s, 6.0);
    s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += (d2[i] - m2) * (d2[i] - m2);
    const double sd2 = __dsqrt_rn(__ddiv_rn(s, 5.0));
    if (__ddiv_rn(sd1, m1) > 0.3 || __ddiv_rn(sd2, m2) > 0.3) return;
  }
  int R = 3, C = 3;
  double e = board_energy(pos, b, R, C, lane);
  if (e > 0) return;

  // the grow loop of chessboardsFromCorners: the best of the four proposals while it lowers the energy
  bool over = false;
  int step = 0;
  for (; step < n; ++step) {
    double best_e = e;   // a border without a proposal leaves the board, and its energy, as they are
    int best_border = 0;
    BoardRegs best_b = b;
    uint64_t best_used = used;
    for (int border = 1; border <= 4; ++border) {
      int got = -1;
      uint64_t taken = used;
      const int st = propose(pos, n, b, R, C, border, used, lane, &got, &taken);
      if (st == kOver) {
        over = true;
        break;
      }
      double pe = e;
      BoardRegs nb = b;
      if (st == kProposed) {
        const bool col = border == 1 || border == 3;
        nb = with_border(b, R, C, border, got, lane);
        pe = board_energy(pos, nb, R + (col ? 0 : 1), C + (col ? 1 : 0), lane);
      }
      if (border == 1 || pe < best_e) {   // the first minimum: the lowest border wins a tie
        best_e = pe;
        best_border = st == kProposed ? border : 0;
        best_b = nb;
        best_used = taken;
      }
    }
    if (over || !(best_e < e)) break;
    b = best_b;
    used = best_used;
    e = best_e;
    if (best_border == 1 || best_border == 3) ++C;
    else ++R;
  }
  if (over || step == n) {   // a capacity or the loop bound: the host takes the image
    if (lane == 0) images[img].flag = 1;
    return;
  }
  if (lane == 0) *out = SeedMeta{e, R, C};
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s * kWave + lane < R * C) out_cells[s * kWave + lane] = (int16_t)b.c[s];
}

__global__ __launch_bounds__(kWave) void k18_select(const ImageRow* images, const SeedMeta* meta, const int16_t* cells, ImageOut* outs, uint32_t max_c,
                                                    uint32_t cell_stride, int board_w, int board_h) {
  __shared__ int16_t owner[kMaxCorners];   // the seed whose stored board holds the corner; -1: none
  __shared__ uint8_t alive[kMaxCorners];   // the seed's board is stored
  const uint32_t img = blockIdx.x;
  const int n = images[img].n, lane = threadIdx.x;
  for (int k = lane; k < n; k += kWave) {
    owner[k] = -1;
    alive[k] = 0;
  }
  __syncthreads();
  const SeedMeta* M = meta + (size_t)img * max_c;
  const int16_t* image_cells = cells + (size_t)img * max_c * cell_stride;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    uint64_t keep = __ballot(i < n && M[i].rows > 0 && M[i].energy < -10);
    for (int guard = 0; guard < kWave && keep; ++guard) {
      const int s = base + __ffsll((unsigned long long)keep) - 1;
      keep &= keep - 1;
      const double eb = M[s].energy;
      const int ncell = M[s].rows * M[s].cols;
      const int16_t* bc = image_cells + (size_t)s * cell_stride;
      int mine[4];
      bool hit = false, keep_old = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cell = q * kWave + lane;
        mine[q] = cell < ncell ? bc[cell] : -1;
        const int o = mine[q] >= 0 ? owner[mine[q]] : -1;
        if (o >= 0) {
          hit = true;
          keep_old |= M[o].energy <= eb;
        }
      }
      const bool any_hit = __any(hit), any_keep = __any(keep_old);
      if (any_hit && any_keep) continue;   // wave-uniform
      if (any_hit) {   // every overlapping board is worse: they all go
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (mine[q] >= 0 && owner[mine[q]] >= 0) alive[owner[mine[q]]] = 0;
        __syncthreads();
        for (int k = lane; k < n; k += kWave)
          if (owner[k] >= 0 && !alive[owner[k]]) owner[k] = -1;
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (mine[q] >= 0) owner[mine[q]] = (int16_t)s;
      if (lane == 0) alive[s] = 1;
      __syncthreads();
    }
  }
  // the one stored board of the requested shape
  int count = 0, found = -1;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    bool match = false;
    if (i < n && alive[i]) {
      const int r = M[i].rows, c = M[i].cols;
      match = (r == board_w && c == board_h) || (r == board_h && c == board_w);
    }
    const uint64_t m = __ballot(match);
    if (m && found < 0) found = base + __ffsll((unsigned long long)m) - 1;
    count += __popcll(m);
  }
  ImageOut* o = outs + img;
  if (lane == 0) {
    o->status = count == 0 ? ILCC_BOARD_NOT_FOUND : count > 1 ? ILCC_AMBIGUOUS : ILCC_OK;
    o->rows = count == 1 ? M[found].rows : 0;
    o->cols = count == 1 ? M[found].cols : 0;
    o->flag = images[img].flag;
  }
  if (count == 1) {
    const int16_t* bc = image_cells + (size_t)found * cell_stride;
    for (int cell = lane; cell < board_w * board_h; cell += kWave) o->idx[cell] = bc[cell];
  }
}

}  // namespace

// One device allocation, [image rows][packed corners][seed meta][image outputs][seed cells], and one page-locked one with the first
// two parts (up) and the outputs (down).
struct ilcc_structure_plan {
  uint32_t max_images = 0, max_corners = 0;
  uint32_t dev_corners = 0;   // min(max_corners, kMaxCorners): what the device parts are sized for
  uint32_t cell_stride = 0;   // int16 cells per seed: min(dev_corners, kMaxCells)
  int device = 0;
  uint8_t* d_buf = nullptr;
  uint8_t* h_buf = nullptr;
  uint64_t at_corners = 0, at_meta = 0, at_out = 0, at_cells = 0, d_total = 0, h_out = 0;
  uint32_t launches = 0, fallbacks = 0, allocations = 0;
  uint32_t last_n = 0;
};

extern "C" {

ilcc_structure_plan* ilcc_structure_plan_create(uint32_t max_images, uint32_t max_corners_per_image) {
  if (max_images == 0 || max_images > 65535u || max_corners_per_image == 0 || max_corners_per_image > (uint32_t)INT32_MAX) {
    set_global_error("ilcc_structure_plan_create: 1 .. 65535 images of at least one corner");
    return nullptr;
  }
  ilcc_structure_plan* p = new (std::nothrow) ilcc_structure_plan;
  if (!p) {
    set_global_error("ilcc_structure_plan_create: out of memory");
    return nullptr;
  }
  if (hipGetDevice(&p->device) != hipSuccess || p->device < 0) {
    delete p;
    (void)no_device();
    return nullptr;
  }
  p->max_images = max_images;
  p->max_corners = max_corners_per_image;
  p->dev_corners = std::min<uint32_t>(max_corners_per_image, kMaxCorners);
  p->cell_stride = std::min<uint32_t>(p->dev_corners, kMaxCells);
  const uint64_t n = max_images, seeds = n * p->dev_corners;
  p->at_corners = align256(n * sizeof(ImageRow));
  p->at_meta = p->at_corners + align256(seeds * sizeof(PackedCorner));
  p->at_out = p->at_meta + align256(seeds * sizeof(SeedMeta));
  p->at_cells = p->at_out + align256(n * sizeof(ImageOut));
  p->d_total = p->at_cells + align256(seeds * p->cell_stride * sizeof(int16_t));
  p->h_out = p->at_meta;   // the page-locked buffer: [image rows][packed corners][image outputs]
  hipError_t e = hipMalloc((void**)&p->d_buf, p->d_total);
  if (e == hipSuccess) {
    ++p->allocations;
    e = hipHostMalloc((void**)&p->h_buf, p->h_out + align256(n * sizeof(ImageOut)), hipHostMallocDefault);
  }
  if (e != hipSuccess) {
    (void)fail(ILCC_HIP_ERROR, std::string("ilcc_structure_plan_create: plan buffers: ") + hipGetErrorString(e));
    ilcc_structure_plan_destroy(p);
    return nullptr;
  }
  ++p->allocations;
  return p;
}

void ilcc_structure_plan_destroy(ilcc_structure_plan* plan) {
  if (!plan) return;
  if (plan->d_buf) (void)hipFree(plan->d_buf);
  if (plan->h_buf) (void)hipHostFree(plan->h_buf);
  delete plan;
}

uint32_t ilcc_structure_plan_launches(const ilcc_structure_plan* plan) { return plan ? plan->launches : 0; }
uint32_t ilcc_structure_plan_fallbacks(const ilcc_structure_plan* plan) { return plan ? plan->fallbacks : 0; }
uint32_t ilcc_structure_plan_allocations(const ilcc_structure_plan* plan) { return plan ? plan->allocations : 0; }

int32_t ilcc_chessboards_from_corners_batch(const ilcc_image_corner* corners, int32_t capacity, const int32_t* n_corners, uint32_t n_images,
                                            int32_t board_w, int32_t board_h, int32_t* status, int32_t* rows, int32_t* cols, int32_t* board_index,
                                            ilcc_structure_plan* plan, void* stream) {
  const char* name = "ilcc_chessboards_from_corners_batch: ";
  if (!plan) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "null plan");
  if (board_w < 3 || board_h < 3 || (int64_t)board_w * board_h > ILCC_MAX_CORNERS)
    return fail(ILCC_BAD_ARGUMENT, std::string(name) + "the board must have 3 x 3 .. ILCC_MAX_CORNERS corners");
  if (capacity < 0) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "negative capacity");
  if (n_images > plan->max_images)
    return fail(ILCC_BAD_ARGUMENT, std::string(name) + std::to_string(n_images) + " images, the plan holds " + std::to_string(plan->max_images));
  if (n_images == 0) {
    plan->launches = plan->fallbacks = plan->last_n = 0;
    return ILCC_OK;
  }
  if (!n_corners || !status || !rows || !cols || !board_index) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "null counts or outputs");
  for (uint32_t m = 0; m < n_images; ++m) {
    if (n_corners[m] < 0 || n_corners[m] > capacity)
      return fail(ILCC_BAD_ARGUMENT, std::string(name) + "image " + std::to_string(m) + " has " + std::to_string(n_corners[m]) + " corners, capacity is " +
                                         std::to_string(capacity));
    if ((uint32_t)n_corners[m] > plan->max_corners)
      return fail(ILCC_BAD_ARGUMENT, std::string(name) + "image " + std::to_string(m) + " has " + std::to_string(n_corners[m]) + " corners, the plan holds " +
                                         std::to_string(plan->max_corners));
    if (n_corners[m] > 0 && !corners) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "null corners");
  }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != plan->device) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "the plan belongs to another device");

  ilcc_structure_plan* p = plan;
  hipStream_t s = (hipStream_t)stream;
  // pack: what the device reads of every image that it can take; the others are marked here
  ImageRow* h_rows = reinterpret_cast<ImageRow*>(p->h_buf);
  PackedCorner* h_corners = reinterpret_cast<PackedCorner*>(p->h_buf + p->at_corners);
  uint32_t total = 0;
  int32_t n_max = 0;
  for (uint32_t m = 0; m < n_images; ++m) {
    const ilcc_image_corner* c = corners + (size_t)m * capacity;
    const int32_t n = n_corners[m];
    bool ok = n <= (int32_t)p->dev_corners;
    for (int32_t i = 0; ok && i < n; ++i) {
      const double v[6] = {c[i].u, c[i].v, c[i].v1[0], c[i].v1[1], c[i].v2[0], c[i].v2[1]};
      for (double x : v) ok &= std::fabs(x) <= ILCC_STRUCTURE_MAX_ABS;   // false for a NaN
      h_corners[total + i] = PackedCorner{v[0], v[1], v[2], v[3], v[4], v[5]};
    }
    h_rows[m] = ImageRow{total, ok ? n : 0, ok ? 0 : 1, 0};
    if (ok) {
      total += (uint32_t)n;
      n_max = std::max(n_max, n);
    }
  }
  const uint64_t up = p->at_corners + (uint64_t)total * sizeof(PackedCorner);
  hipError_t e = hipMemcpyAsync(p->d_buf, p->h_buf, up, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(e);
  ImageRow* d_rows = reinterpret_cast<ImageRow*>(p->d_buf);
  const PackedCorner* d_corners = reinterpret_cast<const PackedCorner*>(p->d_buf + p->at_corners);
  SeedMeta* d_meta = reinterpret_cast<SeedMeta*>(p->d_buf + p->at_meta);
  ImageOut* d_out = reinterpret_cast<ImageOut*>(p->d_buf + p->at_out);
  int16_t* d_cells = reinterpret_cast<int16_t*>(p->d_buf + p->at_cells);
  const uint32_t groups = (uint32_t)std::max(1, (n_max + kGrowWaves - 1) / kGrowWaves);
  const size_t lds = (size_t)std::max(n_max, 1) * sizeof(double2);   // <= 64 KB: n_max <= kMaxCorners
  hipLaunchKernelGGL(k18_grow, dim3(groups, n_images), dim3(kWave * kGrowWaves), lds, s, d_rows, d_corners, d_meta, d_cells, p->dev_corners, p->cell_stride);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k18_select, dim3(n_images), dim3(kWave), 0, s, d_rows, d_meta, d_cells, d_out, p->dev_corners, p->cell_stride, board_w, board_h);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  ImageOut* h_out = reinterpret_cast<ImageOut*>(p->h_buf + p->h_out);
  if ((e = hipMemcpyAsync(h_out, d_out, (size_t)n_images * sizeof(ImageOut), hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e);
  p->launches = 2;
  p->last_n = n_images;

  const size_t cells = (size_t)board_w * board_h;
  uint32_t fallbacks = 0;
  for (uint32_t m = 0; m < n_images; ++m) {
    h_rows[m].flag = h_out[m].flag;   // what ilcc_structure_plan_seed_board asks
    if (h_out[m].flag) {   // above a capacity or a loop bound: the host code's answer, from the host code
      ++fallbacks;
      status[m] = ilcc_chessboard_from_corners(corners + (size_t)m * capacity, n_corners[m], board_w, board_h, &rows[m], &cols[m], board_index + m * cells);
      if (status[m] != ILCC_OK && status[m] != ILCC_BOARD_NOT_FOUND && status[m] != ILCC_AMBIGUOUS) {
        p->fallbacks = fallbacks;
        return status[m];
      }
      continue;
    }
    status[m] = h_out[m].status;
    rows[m] = h_out[m].rows;
    cols[m] = h_out[m].cols;
    if (status[m] == ILCC_OK) std::memcpy(board_index + m * cells, h_out[m].idx, cells * sizeof(int32_t));
  }
  p->fallbacks = fallbacks;
  return ILCC_OK;
}

int32_t ilcc_structure_plan_seed_board(ilcc_structure_plan* plan, uint32_t image, uint32_t seed, int32_t* rows, int32_t* cols, int32_t* index,
                                       int32_t cap, double* energy) {
  const char* name = "ilcc_structure_plan_seed_board: ";
  if (!plan || !rows || !cols || !energy || cap < 0 || (cap > 0 && !index)) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "bad argument");
  if (image >= plan->last_n) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "image outside the plan's last call");
  const ImageRow row = reinterpret_cast<const ImageRow*>(plan->h_buf)[image];
  if (row.flag) return fail(ILCC_CAPACITY, std::string(name) + "the image was recomputed on the host");
  if (seed >= (uint32_t)row.n) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "seed outside the image's corners");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != plan->device) return fail(ILCC_BAD_ARGUMENT, std::string(name) + "the plan belongs to another device");
  const uint64_t at = (uint64_t)image * plan->dev_corners + seed;
  SeedMeta m;
  hipError_t e = hipMemcpy(&m, plan->d_buf + plan->at_meta + at * sizeof(SeedMeta), sizeof(m), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e);
  *rows = m.rows;
  *cols = m.cols;
  *energy = m.energy;
  const int32_t n = m.rows * m.cols;
  if (n == 0) return ILCC_OK;
  if (n < 0 || n > kMaxCells) return fail(ILCC_HIP_ERROR, std::string(name) + "the seed store holds no board shape");
  if (cap < n) return fail(ILCC_CAPACITY, std::string(name) + "the board has more cells than index holds");
  int16_t c16[kMaxCells];
  e = hipMemcpy(c16, plan->d_buf + plan->at_cells + at * plan->cell_stride * sizeof(int16_t), (size_t)n * sizeof(int16_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e);
  for (int32_t k = 0; k < n; ++k) index[k] = c16[k];
  return ILCC_OK;
}

}  // extern "C"
