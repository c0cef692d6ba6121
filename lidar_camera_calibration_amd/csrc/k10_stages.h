// The stages of libcbdetect's findCorners as __device__ bodies, ONE implementation each, called by the single-image
// kernels (k10_image_corners.hip) and by the batch kernels (k10b_image_corners_batch.hip).  Both files are compiled with
// -ffp-contract=off, so a stage gives the same bits whichever kernel calls it.  Also here: the template taps in
// constant memory (one copy per translation unit, uploaded by ensure_taps) and the host finishing of
// findCorners.m:97-125.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "host_util.h"
#include "ilcc_image_corners.h"

namespace ilcc {

namespace {

constexpr int kNmsN = 3, kNmsMargin = 5;
constexpr double kNmsTau = 0.025, kScoreTau = 0.01;
constexpr int kRefineR = 10, kRefineW = 2 * kRefineR + 1;
constexpr int kMaxTemplateR = 12;
constexpr int kMinSide = 2 * kMaxTemplateR + 2 * kNmsMargin;
constexpr int kTile = 16, kHalo = kMaxTemplateR, kTileIn = kTile + 2 * kHalo;
constexpr int kMaxTaps = 2048;
constexpr int kWave = 64;

struct Tap {
  int8_t oy, ox;   // input offset (conv2 flips the kernel: offset = radius - kernel index)
  int16_t pad;
  float w;
};
__constant__ Tap c_taps[kMaxTaps];
__constant__ int32_t c_seg[6 * 4 + 1];   // class c, quadrant q (a1, a2, b1, b2): taps [seg[4c+q], seg[4c+q+1])

struct Record {   // per candidate after refineCorners + scoreCorners: 1-based position
  double p[2], v1[2], v2[2], score;
};

// what refinement and scoring read of one image
struct RefineImage {
  const uint8_t* img;
  const short2* grad;
  const uint32_t* mm;   // [0] min, [1] max
  int w, h, stride;
};

// scan blocks of nonMaximumSuppression.m along a side of `side` pixels (n = 3, margin 5)
inline int nms_blocks(int side) {
  const int n = kNmsN;
  return (side - n - kNmsMargin) >= (n + 1 + kNmsMargin) ? (side - n - kNmsMargin - (n + 1 + kNmsMargin)) / (n + 1) + 1 : 0;
}

// createCorrelationPatch.m:1-49: membership of window pixel (du, dv) (offsets from the centre) and its
// unnormalised weight; -1 = inside the +-0.1 band around either edge
__host__ __device__ inline int quadrant(double du, double dv, double n1u, double n1v, double n2u, double n2v) {
  const double s1 = du * n1u + dv * n1v, s2 = du * n2u + dv * n2v;
  if (s1 <= -0.1 && s2 <= -0.1) return 0;
  if (s1 >= 0.1 && s2 >= 0.1) return 1;
  if (s1 <= -0.1 && s2 >= 0.1) return 2;
  if (s1 >= 0.1 && s2 <= -0.1) return 3;
  return -1;
}

__host__ __device__ inline double normpdf(double x, double sigma) {
  const double z = x / sigma;
  return exp(-0.5 * z * z) / (sqrt(2.0 * M_PI) * sigma);
}

__device__ __forceinline__ double wave_sum(double x) {
  for (int m = kWave / 2; m > 0; m >>= 1) x += __shfl_xor(x, m, kWave);
  return x;
}

// grid-stride min / max of one image by workgroup `block` of `nblocks` (findCorners.m:45-49); mm = {min, max}
__device__ __forceinline__ void minmax_body(const uint8_t* img, int w, int h, int stride, uint32_t* mm, unsigned block, unsigned nblocks) {
  uint32_t lo = 255, hi = 0;
  const size_t n = (size_t)w * h;
  for (size_t k = (size_t)block * blockDim.x + threadIdx.x; k < n; k += (size_t)nblocks * blockDim.x) {
    const uint32_t x = img[(k / w) * (size_t)stride + k % w];
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
  }
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, m, kWave), h2 = __shfl_xor(hi, m, kWave);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    atomicMin(&mm[0], lo);
    atomicMax(&mm[1], hi);
  }
}

// img_du = conv2(I, [-1 0 1; -1 0 1; -1 0 1], 'same') * 255: left column minus right column, zero outside
__device__ __forceinline__ void gradients_body(const uint8_t* img, int w, int h, int stride, short2* grad, int x, int y) {
  if (x >= w || y >= h) return;
  auto at = [&](int yy, int xx) -> int { return (xx >= 0 && xx < w && yy >= 0 && yy < h) ? (int)img[(size_t)yy * stride + xx] : 0; };
  int du = 0, dv = 0;
  for (int d = -1; d <= 1; ++d) {
    du += at(y + d, x - 1) - at(y + d, x + 1);
    dv += at(y - 1, x + d) - at(y + 1, x + d);
  }
  grad[(size_t)y * w + x] = make_short2((short)du, (short)dv);
}

// tile (bx, by) of the likelihood map: 16 x 16 outputs over a 40 x 40 LDS tile of (I - min), zero outside THIS image
__device__ __forceinline__ void likelihood_body(const uint8_t* img, int w, int h, int stride, const uint32_t* mm, float* L, int bx, int by,
                                                float (*tile)[kTileIn]) {
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * kTile + tx;
  const int x0 = bx * kTile - kHalo, y0 = by * kTile - kHalo;
  const float lo = (float)mm[0];
  for (int k = t; k < kTileIn * kTileIn; k += kTile * kTile) {
    const int yy = y0 + k / kTileIn, xx = x0 + k % kTileIn;
    tile[k / kTileIn][k % kTileIn] = (xx >= 0 && xx < w && yy >= 0 && yy < h) ? (float)img[(size_t)yy * stride + xx] - lo : 0.f;
  }
  __syncthreads();
  const int x = bx * kTile + tx, y = by * kTile + ty;
  if (x >= w || y >= h) return;
  float best = 0.f;
  for (int c = 0; c < 6; ++c) {
    float a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float acc = 0.f;
      for (int i = c_seg[4 * c + q]; i < c_seg[4 * c + q + 1]; ++i) {
        const Tap tp = c_taps[i];
        acc += tp.w * tile[ty + kHalo + tp.oy][tx + kHalo + tp.ox];
      }
      a[q] = acc;
    }
    const float mu = (a[0] + a[1] + a[2] + a[3]) / 4.f;
    const float c1 = fminf(fminf(a[0] - mu, a[1] - mu), fminf(mu - a[2], mu - a[3]));
    const float c2 = fminf(fminf(mu - a[0], mu - a[1]), fminf(a[2] - mu, a[3] - mu));
    best = fmaxf(best, fmaxf(c1, c2));
  }
  const uint32_t range = mm[1] - mm[0];
  // a constant image: the reference divides by zero and finds nothing; a zero map finds nothing too
  L[(size_t)y * w + x] = range ? best / (float)range : 0.f;
}

// nonMaximumSuppression.m: block b = bx * nby + by starts at 1-based (i, j) = (9 + 4 bx, 9 + 4 by); true when the block's
// maximum (1-based (maxi, maxj)) reaches tau and nothing within n of it, outside the block, is larger
__device__ __forceinline__ bool nms_block(const float* L, int w, int h, int nby, int b, int& maxi, int& maxj) {
  const int n = kNmsN;
  const int i = n + 1 + kNmsMargin + (b / nby) * (n + 1), j = n + 1 + kNmsMargin + (b % nby) * (n + 1);
  auto at = [&](int jj, int ii) { return L[(size_t)(jj - 1) * w + (ii - 1)]; };
  maxi = i;
  maxj = j;
  float maxval = at(j, i);
  for (int i2 = i; i2 <= i + n; ++i2)
    for (int j2 = j; j2 <= j + n; ++j2) {
      const float cv = at(j2, i2);
      if (cv > maxval) {
        maxi = i2;
        maxj = j2;
        maxval = cv;
      }
    }
  if (!((double)maxval >= kNmsTau)) return false;
  const int ie = min(maxi + n, w - kNmsMargin), je = min(maxj + n, h - kNmsMargin);
  for (int i2 = maxi - n; i2 <= ie; ++i2)
    for (int j2 = maxj - n; j2 <= je; ++j2)
      if (at(j2, i2) > maxval && (i2 < i || i2 > i + n || j2 < j || j2 > j + n)) return false;
  return true;
}

// unit eigenvector of the smaller eigenvalue of [[a, b], [b, c]] (eig's first column; its sign is
// irrelevant to every later use: |o . v|, projections, and the sign rules of findCorners.m:115-122)
__device__ inline void small_eigvec(double a, double b, double c, double& ex, double& ey) {
  if (b == 0.0) {
    if (a <= c) { ex = 1.0; ey = 0.0; } else { ex = 0.0; ey = 1.0; }
    return;
  }
  const double hm = 0.5 * (a + c), hd = 0.5 * (a - c);
  const double lam = hm - sqrt(hd * hd + b * b);
  double x1 = b, y1 = lam - a, x2 = lam - c, y2 = b;   // two forms of the same eigenvector
  const double n1 = x1 * x1 + y1 * y1, n2 = x2 * x2 + y2 * y2;
  if (n1 >= n2) { const double s = sqrt(n1); ex = x1 / s; ey = y1 / s; }
  else { const double s = sqrt(n2); ex = x2 / s; ey = y2 / s; }
}

// cornerCorrelationScore.m on the (2r+1)^2 window centred at 1-based (u, v); every lane returns it
__device__ inline double window_score(const RefineImage& A, int u, int v, int r, const double* v1, const double* v2, double lo, double inv) {
  const int n = 2 * r + 1, N = n * n, lane = threadIdx.x;
  auto wt_at = [&](int k) {   // column-major over the window: k = x * n + y
    const short2 g = A.grad[(size_t)(v - r - 1 + k % n) * A.w + (u - r - 1 + k / n)];
    const double du = g.x / 255.0, dv = g.y / 255.0;
    return sqrt(du * du + dv * dv);
  };
  auto filt_at = [&](int k) {
    const double px = k / n - r, py = k % n - r;
    const double q1 = px * v1[0] + py * v1[1], q2 = px * v2[0] + py * v2[1];
    const double e1x = px - q1 * v1[0], e1y = py - q1 * v1[1], e2x = px - q2 * v2[0], e2y = py - q2 * v2[1];
    return (sqrt(e1x * e1x + e1y * e1y) <= 1.5 || sqrt(e2x * e2x + e2y * e2y) <= 1.5) ? 1.0 : -1.0;
  };
  double sw = 0, sf = 0;
  for (int k = lane; k < N; k += kWave) { sw += wt_at(k); sf += filt_at(k); }
  const double mw = wave_sum(sw) / N, mf = wave_sum(sf) / N;
  double qw = 0, qf = 0, qwf = 0;
  for (int k = lane; k < N; k += kWave) {
    const double a = wt_at(k) - mw, b = filt_at(k) - mf;
    qw += a * a;
    qf += b * b;
    qwf += a * b;
  }
  const double stw = sqrt(wave_sum(qw) / (N - 1)), stf = sqrt(wave_sum(qf) / (N - 1));
  double g = wave_sum(qwf) / (stw * stf) / (N - 1);
  g = g > 0.0 ? g : 0.0;   // max(NaN, 0) is 0 in the reference
  // intensity: createCorrelationPatch(atan2(v1), atan2(v2), r) against the normalised image
  const double a1 = atan2(v1[1], v1[0]), a2 = atan2(v2[1], v2[0]);
  const double n1u = -sin(a1), n1v = cos(a1), n2u = -sin(a2), n2v = cos(a2);
  double sg[4] = {0, 0, 0, 0}, sgi[4] = {0, 0, 0, 0};
  for (int k = lane; k < N; k += kWave) {
    const int px = k / n - r, py = k % n - r;
    const int q = quadrant(px, py, n1u, n1v, n2u, n2v);
    if (q < 0) continue;
    const double gw = normpdf(sqrt((double)(px * px + py * py)), r / 2.0);
    const double im = ((double)A.img[(size_t)(v - 1 + py) * A.stride + (u - 1 + px)] - lo) * inv;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
      if (qq == q) { sg[qq] += gw; sgi[qq] += gw * im; }
  }
  double a[4];
  bool empty = false;
  for (int q = 0; q < 4; ++q) {
    const double s = wave_sum(sg[q]), si = wave_sum(sgi[q]);
    empty |= !(s > 0.0);
    a[q] = si / s;
  }
  if (empty) return 0.0;   // an empty quadrant makes the reference's responses NaN: intensity score 0
  const double mu = (a[0] + a[1] + a[2] + a[3]) / 4;
  const double s1 = fmin(fmin(a[0] - mu, a[1] - mu), fmin(mu - a[2], mu - a[3]));
  const double s2 = fmin(fmin(mu - a[0], mu - a[1]), fmin(a[2] - mu, a[3] - mu));
  const double si = fmax(fmax(s1, s2), 0.0);
  return g * si;
}

// one wavefront (a workgroup of kWave threads) on the candidate at 1-based (cu, cv) of image A: edgeOrientations +
// findModesMeanShift, the orientation and position refinement and scoreCorners; lane 0 writes *out
__device__ inline void refine_score_body(const RefineImage& A, int cu, int cv, Record* out) {
  __shared__ double s_ang[kRefineW * kRefineW], s_wt[kRefineW * kRefineW];
  __shared__ short2 s_g[kRefineW * kRefineW];
  __shared__ double s_hist[32];
  __shared__ double s_v[4];
  __shared__ int s_ok;
  __shared__ double hs[32], mv[32];   // lane 0's mean-shift state (kept out of scratch)
  __shared__ int mb[32];
  const int lane = threadIdx.x;
  const int u0 = max(cu - kRefineR, 1), u1 = min(cu + kRefineR, A.w), v0 = max(cv - kRefineR, 1), v1e = min(cv + kRefineR, A.h);
  const int nv = v1e - v0 + 1, N = (u1 - u0 + 1) * nv;   // column-major window, as img(:) is
  for (int i = lane; i < N; i += kWave) {
    const int u = u0 + i / nv, v = v0 + i % nv;
    const short2 g = A.grad[(size_t)(v - 1) * A.w + (u - 1)];
    const double du = g.x / 255.0, dv = g.y / 255.0;
    double an = atan2(dv, du);
    if (an < 0) an += M_PI;
    if (an > M_PI) an -= M_PI;
    s_g[i] = g;
    s_ang[i] = an;
    s_wt[i] = sqrt(du * du + dv * dv);
  }
  __syncthreads();
  // edgeOrientations: lane b sums bin b in the window's own order
  if (lane < 32) {
    double hb = 0;
    for (int i = 0; i < N; ++i) {
      double a = s_ang[i] + M_PI / 2;
      if (a > M_PI) a -= M_PI;
      const int bin = max(min((int)floor(a / (M_PI / 32)), 31), 0);
      if (bin == lane) hb += s_wt[i];
    }
    s_hist[lane] = hb;
  }
  __syncthreads();
  if (lane == 0) {
    // findModesMeanShift(hist, 1): 5-tap circular smoothing, hill climbing from every bin
    for (int i = 0; i < 32; ++i) {
      double s = 0;
      for (int j = -2; j <= 2; ++j) s += s_hist[(i + j + 32) % 32] * normpdf((double)j, 1.0);
      hs[i] = s;
    }
    bool flat = true;   // the reference's vector `if` holds only when every bin is within 1e-5 of bin 1
    for (int i = 0; i < 32; ++i) flat &= fabs(hs[i] - hs[0]) < 1e-5;
    int nm = 0;
    if (!flat) {
      for (int i = 0; i < 32; ++i) {
        int j = i;
        for (;;) {
          const double h0 = hs[j];
          const int j1 = (j + 1) % 32, j2 = (j + 31) % 32;
          const double h1 = hs[j1], h2 = hs[j2];
          if (h1 >= h0 && h1 >= h2) j = j1;
          else if (h2 > h0 && h2 > h1) j = j2;
          else break;
        }
        bool seen = false;
        for (int m = 0; m < nm; ++m) seen |= mb[m] == j;
        if (!seen) { mb[nm] = j; mv[nm] = hs[j]; ++nm; }
      }
      for (int a = 1; a < nm; ++a)   // stable sort, value descending
        for (int b = a; b > 0 && mv[b] > mv[b - 1]; --b) {
          const double t = mv[b]; mv[b] = mv[b - 1]; mv[b - 1] = t;
          const int ti = mb[b]; mb[b] = mb[b - 1]; mb[b - 1] = ti;
        }
    }
    int ok = 0;
    if (nm >= 2) {
      double t0 = mb[0] * M_PI / 32, t1 = mb[1] * M_PI / 32;   // (bin - 1) * pi / 32 with 1-based bins
      if (t1 < t0) { const double t = t0; t0 = t1; t1 = t; }
      if (fmin(t1 - t0, t0 + M_PI - t1) > 0.3) {
        ok = 1;
        s_v[0] = cos(t0); s_v[1] = sin(t0); s_v[2] = cos(t1); s_v[3] = sin(t1);
      }
    }
    s_ok = ok;
  }
  __syncthreads();
  Record rec;
  rec.p[0] = cu; rec.p[1] = cv;
  rec.v1[0] = rec.v1[1] = rec.v2[0] = rec.v2[1] = 0.0;
  rec.score = 0.0;
  if (!s_ok) {
    if (lane == 0) *out = rec;
    return;
  }
  double e1[2] = {s_v[0], s_v[1]}, e2[2] = {s_v[2], s_v[3]};
  // orientation refinement (refineCorners.m:35-65)
  double a00 = 0, a01 = 0, a11 = 0, b00 = 0, b01 = 0, b11 = 0;
  for (int i = lane; i < N; i += kWave) {
    const double du = s_g[i].x / 255.0, dv = s_g[i].y / 255.0;
    const double nr = sqrt(du * du + dv * dv);
    if (nr < 0.1) continue;
    const double ou = du / nr, ov = dv / nr;
    if (fabs(ou * e1[0] + ov * e1[1]) < 0.25) { a00 += du * du; a01 += du * dv; a11 += dv * dv; }
    if (fabs(ou * e2[0] + ov * e2[1]) < 0.25) { b00 += du * du; b01 += du * dv; b11 += dv * dv; }
  }
  a00 = wave_sum(a00); a01 = wave_sum(a01); a11 = wave_sum(a11);
  b00 = wave_sum(b00); b01 = wave_sum(b01); b11 = wave_sum(b11);
  small_eigvec(a00, a01, a11, e1[0], e1[1]);
  small_eigvec(b00, b01, b11, e2[0], e2[1]);
  // position refinement (refineCorners.m:71-120)
  double g00 = 0, g01 = 0, g11 = 0, r0 = 0, r1 = 0;
  for (int i = lane; i < N; i += kWave) {
    const double du = s_g[i].x / 255.0, dv = s_g[i].y / 255.0;
    const double nr = sqrt(du * du + dv * dv);
    if (nr < 0.1) continue;
    const int u = u0 + i / nv, v = v0 + i % nv;
    if (u == cu && v == cv) continue;
    const double ou = du / nr, ov = dv / nr;
    const double wu = u - cu, wv = v - cv;
    const double p1 = wu * e1[0] + wv * e1[1], p2 = wu * e2[0] + wv * e2[1];
    const double d1 = sqrt((wu - p1 * e1[0]) * (wu - p1 * e1[0]) + (wv - p1 * e1[1]) * (wv - p1 * e1[1]));
    const double d2 = sqrt((wu - p2 * e2[0]) * (wu - p2 * e2[0]) + (wv - p2 * e2[1]) * (wv - p2 * e2[1]));
    if ((d1 < 3 && fabs(ou * e1[0] + ov * e1[1]) < 0.25) || (d2 < 3 && fabs(ou * e2[0] + ov * e2[1]) < 0.25)) {
      g00 += du * du; g01 += du * dv; g11 += dv * dv;
      r0 += du * du * u + du * dv * v;
      r1 += dv * du * u + dv * dv * v;
    }
  }
  g00 = wave_sum(g00); g01 = wave_sum(g01); g11 = wave_sum(g11); r0 = wave_sum(r0); r1 = wave_sum(r1);
  // rank(G) == 2: smaller singular value above 2 * eps(larger)
  const double hm = 0.5 * (g00 + g11), hd = 0.5 * (g00 - g11), rt = sqrt(hd * hd + g01 * g01);
  const double smax = fmax(fabs(hm + rt), fabs(hm - rt)), smin = fmin(fabs(hm + rt), fabs(hm - rt));
  const double tol = 2.0 * (nextafter(smax, INFINITY) - smax);
  bool valid = smax > 0.0 && smin > tol;
  if (valid) {
    const double det = g00 * g11 - g01 * g01;
    rec.p[0] = (g11 * r0 - g01 * r1) / det;
    rec.p[1] = (g00 * r1 - g01 * r0) / det;
    const double dx = rec.p[0] - cu, dy = rec.p[1] - cv;
    valid = !(sqrt(dx * dx + dy * dy) >= 4);
  }
  if (valid) {
    rec.v1[0] = e1[0]; rec.v1[1] = e1[1]; rec.v2[0] = e2[0]; rec.v2[1] = e2[1];
    const double lo = A.mm[0], inv = 1.0 / ((double)A.mm[1] - (double)A.mm[0]);
    const double ru = round(rec.p[0]), rv = round(rec.p[1]);
    double best = 0.0;
    for (int ri = 0; ri < 3; ++ri) {
      const int r = 4 * (ri + 1);
      double s = 0.0;
      if (ru > r && ru <= A.w - r && rv > r && rv <= A.h - r) s = window_score(A, (int)ru, (int)rv, r, e1, e2, lo, inv);
      best = ri == 0 ? s : fmax(best, s);
    }
    rec.score = best;
  }
  if (lane == 0) *out = rec;
}

// the 6 x 4 quadrant kernels of findCorners.m:52, normalised, as taps with conv2's flipped offsets
struct TapTable {
  std::vector<Tap> taps;
  int32_t seg[25];
};

TapTable build_taps() {
  static const double props[6][3] = {{0, M_PI / 2, 4}, {M_PI / 4, -M_PI / 4, 4}, {0, M_PI / 2, 8},
                                     {M_PI / 4, -M_PI / 4, 8}, {0, M_PI / 2, 12}, {M_PI / 4, -M_PI / 4, 12}};
  TapTable t;
  for (int c = 0; c < 6; ++c) {
    const int r = (int)props[c][2], n = 2 * r + 1;
    const double n1u = -sin(props[c][0]), n1v = cos(props[c][0]), n2u = -sin(props[c][1]), n2v = cos(props[c][1]);
    for (int q = 0; q < 4; ++q) {
      t.seg[4 * c + q] = (int32_t)t.taps.size();
      double sum = 0;
      std::vector<std::pair<int, double>> cells;   // (ky * n + kx, weight)
      for (int kx = 0; kx < n; ++kx)
        for (int ky = 0; ky < n; ++ky) {
          if (quadrant(kx - r, ky - r, n1u, n1v, n2u, n2v) != q) continue;
          const double g = normpdf(sqrt((double)((kx - r) * (kx - r) + (ky - r) * (ky - r))), r / 2.0);
          cells.push_back({ky * n + kx, g});
          sum += g;
        }
      for (auto& cell : cells) {
        Tap tp;
        tp.oy = (int8_t)(r - cell.first / n);
        tp.ox = (int8_t)(r - cell.first % n);
        tp.pad = 0;
        tp.w = (float)(cell.second / sum);
        t.taps.push_back(tp);
      }
    }
  }
  t.seg[24] = (int32_t)t.taps.size();
  return t;
}

std::mutex g_taps_mu;
bool g_taps_ready[16] = {};

inline int32_t k10_hip_fail(const char* what, hipError_t e) {
  set_global_error(std::string("k10 ") + what + ": " + hipGetErrorString(e));
  return ILCC_HIP_ERROR;
}

// this translation unit's copy of the template taps, uploaded once per device
int32_t ensure_taps(int dev) {
  std::lock_guard<std::mutex> lock(g_taps_mu);
  if (g_taps_ready[dev]) return ILCC_OK;
  const TapTable t = build_taps();
  if (t.taps.size() > (size_t)kMaxTaps) {
    set_global_error("k10: template taps exceed the constant table");
    return ILCC_HIP_ERROR;
  }
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_taps), t.taps.data(), sizeof(Tap) * t.taps.size());
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_seg), t.seg, sizeof(t.seg));
  if (e != hipSuccess) return k10_hip_fail("template upload", e);
  g_taps_ready[dev] = true;
  return ILCC_OK;
}

// findCorners.m:97-125 on one image's records: drop corners without edges and below tau, v1 sign, right-handed v2,
// 0-based.  Fills corners[0 .. min(count, capacity)) and returns the full count.
inline int32_t finish_corners(const Record* rec, uint32_t nc, ilcc_image_corner* corners, int32_t capacity) {
  int32_t cnt = 0;
  for (uint32_t i = 0; i < nc; ++i) {
    const Record& r = rec[i];
    if (r.v1[0] == 0 && r.v1[1] == 0) continue;
    if (r.score < kScoreTau) continue;
    double v1x = r.v1[0], v1y = r.v1[1];
    if (v1x + v1y < 0) { v1x = -v1x; v1y = -v1y; }
    const double d = v1y * r.v2[0] + (-v1x) * r.v2[1];
    const double flip = d > 0 ? -1.0 : (d < 0 ? 1.0 : 0.0);
    if (cnt < capacity) {
      ilcc_image_corner& o = corners[cnt];
      o.u = r.p[0] - 1; o.v = r.p[1] - 1;
      o.v1[0] = v1x; o.v1[1] = v1y;
      o.v2[0] = r.v2[0] * flip; o.v2[1] = r.v2[1] * flip;
      o.score = r.score;
    }
    ++cnt;
  }
  return cnt;
}

}  // namespace
}  // namespace ilcc
