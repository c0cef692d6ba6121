// K7a local_solve (ILCC_SOLVER_REFERENCE_LOCAL): ONE WAVEFRONT per (frame, colour phase); a 256-thread workgroup holds
//      kSolveWaves such solves (the two phases of a frame share one staged copy of its labelled points in LDS).
//  (1) starts at (0,0,0), the reference's own start;
//  (2) runs the reference's two local solves, pass A (useOutofBoard = true) then pass B (false)
//      -- LidarCornersEst::get_corners, ilcc2/src/LidarCornersEst.cpp:398-409 --
//      each a restatement of what ceres::Solve does for Optimization::get_theta_t
//      (ilcc2/src/Optimization.cpp:94-160): TRUST_REGION, DOGLEG/SUBSPACE_DOGLEG,
//      DENSE_NORMAL_CHOLESKY, HuberLoss(0.1) through Ceres' Corrector, Jacobi scaling, Ceres 1.14
//      default tolerances.  The 64 lanes stride over the points (residual + Jacobian in double), sums are
//      combined with a DPP / permlane butterfly (no LDS, no barrier: after the staging barrier the wavefronts of a
//      workgroup never meet again), and the 3-parameter trust-region bookkeeping runs once per wavefront on
//      wave-uniform values.  Round 6 (profiles/r06a_*): the 4-wavefront-per-solve layout of rounds 1-5 issued the
//      dogleg FOUR times per iteration -- 60 % of the kernel's 1.02 G wave-instructions per 1024 frames -- and at 203
//      VGPRs held two wavefronts per SIMD; the kernel was VALU-issue bound (VALU busy 70 %), not latency bound.
//      The arithmetic is unchanged value for value: divisions by a divisor that is used many times (g; the dogleg's
//      diagonal, Cholesky pivots, norms) are one true division for RN(1/d) plus Markstein's correction (exactly the
//      correctly rounded quotient), sqrt(r * r) of Huber is |r| (exact in binary floating point).
// The GRID mode's solver is K7r (k7r_pattern_refine.hip); K7b (k7b_corners.hip) turns either solver's records into corners.
#include "k7_common.h"

namespace ilcc {

// ------------------------------------------------------------------ residual (Optimization.h:31-107)
// a / d, correctly rounded, for a divisor that divides many numerators: y = RN(1 / d) costs one true division, every
// quotient after that is q = RN(a y); r = a - q d (exact, one FMA); RN(q + r y) -- Markstein's theorem: with y the
// correctly rounded reciprocal and q within an ulp of a / d the corrected quotient IS RN(a / d) (the sequence the
// hardware's own v_div_* expansion ends with; tools/ubench/markstein_check.c compares it with `/` on 6e8 samples).
// Numerators here are finite and far from the over/underflow range (board coordinates, trust-region bookkeeping).
struct Divisor {
  double d, y;
};
__device__ __forceinline__ Divisor make_divisor(double d) { return Divisor{d, 1.0 / d}; }
__device__ __forceinline__ double div_by(double a, const Divisor& v) {
  const double q = a * v.y;
  const double r = __builtin_fma(-q, v.d, a);
  return __builtin_fma(r, v.y, q);
}

// the board with the constants the residual needs
struct SolveBoard {
  double W, H, delta;
  double Wg2, Hg2;   // W * g / 2.0, H * g / 2.0 (Optimization.h:45-46)
  Divisor g;
};
__device__ __forceinline__ SolveBoard make_board(const ilcc_params& p) {
  SolveBoard b;
  b.W = (double)p.board_w;
  b.H = (double)p.board_h;
  b.delta = p.huber_delta;
  b.Wg2 = b.W * p.grid_length / 2.0;
  b.Hg2 = b.H * p.grid_length / 2.0;
  b.g = make_divisor(p.grid_length);
  return b;
}

// raw residual; jac = d r / d(theta, ty, tz) when JAC.  cs = (cos theta, sin theta).  Value for value the oracle's
// residual_cs (oracle/ilcc_oracle.c): (floor(i) even) is read off the integer instead of floor(ifl / 2) * 2 == ifl,
// ceil(i) of a non-integer i is floor(i) + 1, d i / d theta = -(s y + c z) / g = -rz / g and d j / d theta = ry / g
// reuse the rotated point (the same products, the same sums), +-1 / g is +-RN(1 / g).
template <bool JAC>
__device__ __forceinline__ double residual(const double x[3], double c, double s, double y, double z,
                                           const SolveBoard& bd, bool tlw, bool laser_white, bool use_oob,
                                           double jac[3]) {
  // written without a branch (round 6): a divergent `if` costs the wavefront both sides plus the exec-mask bookkeeping.
  // min(frac, 1 - frac) IS the in-board distance of :70-78 -- frac = i - floor(i) is exact, and for frac > 1/2 both ceil(i) - i and
  // 1 - frac are exact (Sterbenz) and equal; min(|i|, |i - W|) IS the out-of-board distance of :86-97
  const double ry = c * y - s * z;
  const double rz = s * y + c * z;
  const double i = div_by((ry + x[1]) + bd.Wg2, bd.g);
  const double j = div_by((rz + x[2]) + bd.Hg2, bd.g);
  const bool inside = (int)(i > 0) & (int)(i < bd.W) & (int)(j > 0) & (int)(j < bd.H);
  const double ifl = floor(i), jfl = floor(j);
  const double fi = i - ifl, fj = j - jfl;
  const double res_in = fmin(fi, 1.0 - fi) + fmin(fj, 1.0 - fj);
  const bool odd = ((((int)ifl) ^ ((int)jfl)) & 1) != 0;
  const bool white = odd != tlw;   // same parity: topleftWhite, else its opposite (:57-61)
  const double iw = i - bd.W, jh = j - bd.H;
  double res_out = 0.0;
  if (use_oob) res_out = fmin(fabs(i), fabs(iw)) + fmin(fabs(j), fabs(jh));   // (wave-uniform: pass B never computes it)
  const bool take_in = (int)inside & (int)(laser_white != white), take_out = (int)!inside & (int)use_oob;
  if (JAC) {
    // d r / d i, d r / d j: -1 past the middle of a cell; out of board the sign of the nearer edge's offset (:86-97)
    const double si_in = fi > 0.5 ? -1.0 : 1.0, sj_in = fj > 0.5 ? -1.0 : 1.0;
    const double si_out = ((fabs(i) < fabs(iw) ? i : iw) < 0) ? -1.0 : 1.0, sj_out = ((fabs(j) < fabs(jh) ? j : jh) < 0) ? -1.0 : 1.0;
    const double si = take_in ? si_in : (take_out ? si_out : 0.0), sj = take_in ? sj_in : (take_out ? sj_out : 0.0);
    const double dith = -div_by(rz, bd.g), djth = div_by(ry, bd.g);
    jac[0] = si * dith + sj * djth;
    jac[1] = si * bd.g.y;
    jac[2] = sj * bd.g.y;
  }
  return take_in ? res_in : (take_out ? res_out : 0.0);
}

// HuberLoss(a) on s = r * r with r >= 0 (the residual is a sum of distances): sqrt(s) is r itself -- for binary floating point
// sqrt(RN(r * r)) == |r| barring over/underflow (Boldo 2015; the oracle calls sqrt) -- so no square root is taken
__device__ __forceinline__ void huber(double a, double r, double s, double& rho0, double& rho1) {
  const double b = a * a;
  const bool outlier = s > b;
  rho0 = outlier ? 2.0 * a * r - b : s;
  rho1 = outlier ? fmax(a / r, 2.2250738585072014e-308) : 1.0;   // (only the Jacobian pass reads rho1: the cost pass drops the division)
}

// ------------------------------------------------------------------ wavefront-wide evaluation
constexpr int kSolveWaves = kSolveThreads / ILCC_WAVE;   // solves per K7a workgroup
#ifndef ILCC_K7A_WIDE_MAX
#define ILCC_K7A_WIDE_MAX 256
#endif
constexpr int kSolveWideMaxFrames = ILCC_K7A_WIDE_MAX;    // K7a: batches up to this size give every solve a whole workgroup

struct Problem {
  const float2* yz;      // LDS or global
  const uint8_t* lab;
  uint32_t n;
  SolveBoard bd;
  bool tlw, oob;
  double* red;           // WIDE only -- LDS: 2 x kSolveRedDoubles (double-buffered partial sums)
  int* flip;             // WIDE only -- per-thread toggle (register copy lives in the caller)
};

// butterfly in the order 32, 16, 8, 4, 2, 1: identical in every lane (each step adds the same two operands
// in both partners)
__device__ __forceinline__ double wave_allsum(double v) {
  v += xor_lane_f64<32>(v);
  v += xor_lane_f64<16>(v);
  v += xor_lane_f64<8>(v);
  v += xor_lane_f64<4>(v);
  v += xor_lane_f64<2>(v);
  v += xor_lane_f64<1>(v);
  return v;
}

// sums[0] = cost ; if JAC: sums[1..3] = J^T r, sums[4..9] = upper J^T J (00,01,02,11,12,22),
// with Ceres' Corrector applied (rows scaled by sqrt(rho')).  The same value in every lane on return.
// ONE summation order for both layouts, so that a frame's result does not depend on the size of the batch it came in:
// lane l owns the points l, l + 64, l + 128, ...; the point l + 64 m goes to the lane's partial sum a[m mod 4] (each
// partial adds its points in increasing order); the lane's sum is ((a0 + a1) + a2) + a3; the 64 lane sums are
// combined by the butterfly.
//   WIDE = false: one wavefront per solve.  The cost alone keeps the four partials in registers (one walk over the
//   points); the Jacobian pass (one evaluation in six) walks the four residue classes one after the other.
//   WIDE = true (small batches, where latency counts and the chip is not full): the whole 256-thread workgroup works
//   on ONE solve, wavefront w computes the partials a[w]; wavefronts -> LDS -> everyone, ONE barrier per call
//   (double-buffered slots); every thread then runs the trust-region bookkeeping redundantly.
template <bool JAC>
__device__ __forceinline__ void add_point(const Problem& q, const double x[3], double cs, double sn, uint32_t p, double acc[10]) {
  const float2 v = q.yz[p];
  double jac[3];
  const double res = residual<JAC>(x, cs, sn, (double)v.x, (double)v.y, q.bd, q.tlw, q.lab[p] != 0, q.oob, jac);
  double r0, r1;
  huber(q.bd.delta, res, res * res, r0, r1);
  acc[0] += 0.5 * r0;
  if (JAC) {
    const double sr = sqrt(r1);
    const double rc = sr * res;
    const double j0 = sr * jac[0], j1 = sr * jac[1], j2 = sr * jac[2];
    acc[1] += j0 * rc;
    acc[2] += j1 * rc;
    acc[3] += j2 * rc;
    acc[4] += j0 * j0;
    acc[5] += j0 * j1;
    acc[6] += j0 * j2;
    acc[7] += j1 * j1;
    acc[8] += j1 * j2;
    acc[9] += j2 * j2;
  }
}
// the partial sums a[w] of this lane: points first, first + 256, ...
template <bool JAC>
__device__ __forceinline__ void accumulate_class(const Problem& q, const double x[3], double cs, double sn, uint32_t first,
                                                 double acc[10]) {
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  // (the Jacobian pass is one evaluation in six and carries 10 sums: not unrolled, its registers set the kernel's occupancy)
#pragma unroll 1
  for (uint32_t p = first; p < q.n; p += (uint32_t)(4 * ILCC_WAVE)) add_point<JAC>(q, x, cs, sn, p, acc);
}

constexpr int kSolveRedDoubles = 10 * 4 * ILCC_WAVE;   // WIDE: one exchange buffer (10 sums x 4 partials x 64 lanes)

template <bool JAC, bool WIDE>
__device__ __forceinline__ void evaluate(const Problem& q, const double x[3], double sums[10]) {
  static_assert(kSolveThreads == 4 * ILCC_WAVE, "the summation order is defined on four partial sums per lane");
  double sn, cs;
  sincos(x[0], &sn, &cs);
  constexpr int NV = JAC ? 10 : 1;
  const uint32_t lane = (uint32_t)lane_id();
  double tot[10];
  if (WIDE) {
    double acc[10];
    accumulate_class<JAC>(q, x, cs, sn, threadIdx.x, acc);
    *q.flip ^= 1;
    double* slot = q.red + (*q.flip) * kSolveRedDoubles;
#pragma unroll
    for (int k = 0; k < NV; ++k) slot[(k * 4 + wave_id()) * ILCC_WAVE + lane] = acc[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double* sk = slot + k * 4 * ILCC_WAVE + lane;
      tot[k] = ((sk[0] + sk[ILCC_WAVE]) + sk[2 * ILCC_WAVE]) + sk[3 * ILCC_WAVE];
    }
  } else if (JAC) {
#pragma nounroll
    for (int w = 0; w < 4; ++w) {
      double acc[10];
      accumulate_class<true>(q, x, cs, sn, (uint32_t)w * ILCC_WAVE + lane, acc);
#pragma unroll
      for (int k = 0; k < NV; ++k) tot[k] = (w == 0) ? acc[k] : tot[k] + acc[k];
    }
  } else {
    double a0[10], a1[10], a2[10], a3[10];   // ([0] only: the cost)
    a0[0] = a1[0] = a2[0] = a3[0] = 0.0;
    for (uint32_t p = lane; p < q.n; p += (uint32_t)(4 * ILCC_WAVE)) {
      add_point<false>(q, x, cs, sn, p, a0);
      if (p + ILCC_WAVE < q.n) add_point<false>(q, x, cs, sn, p + ILCC_WAVE, a1);
      if (p + 2 * ILCC_WAVE < q.n) add_point<false>(q, x, cs, sn, p + 2 * ILCC_WAVE, a2);
      if (p + 3 * ILCC_WAVE < q.n) add_point<false>(q, x, cs, sn, p + 3 * ILCC_WAVE, a3);
    }
    tot[0] = ((a0[0] + a1[0]) + a2[0]) + a3[0];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) sums[k] = wave_allsum(tot[k]);
}

// ------------------------------------------------------------------ dogleg bookkeeping (wave-uniform values)
struct Dog {
  double radius, mu;
  int reuse;
  Divisor d0, d1, d2;       // diagonal (divides the gradient, the basis and every step)
  double g0, g1, g2;        // scaled gradient
  double n0, n1, n2;        // Gauss-Newton step (scaled space)
  double alpha, step_norm;
  int one_dim;
  double b00, b01, b10, b11, b20, b21;   // subspace basis (3x2)
  double sg0, sg1, sB00, sB01, sB11;
  double A00, A01, A02, A11, A12, A22;   // J^T J of the column-scaled Jacobian
  double r0, r1, r2;                     // J^T r of the column-scaled Jacobian
  // min_on_circle's radius-independent half (eigen-decomposition of the 2x2 subspace model), computed at the first
  // boundary step of a linearisation point and kept while the rejected steps only shrink the radius
  int eig_ready;
  double e_l1, e_l2, e_v1x, e_v1y, e_v2x, e_v2y, e_g1, e_g2, e_gn;
};

// (A + diag(e)) x = b by Cholesky; false on a non-positive pivot (Eigen LLT NumericalIssue)
__device__ __forceinline__ bool chol3_solve(double a00, double a01, double a02, double a11, double a12,
                                            double a22, double b0, double b1, double b2, double& x0,
                                            double& x1, double& x2) {
  if (!(a00 > 0.0)) return false;
  const Divisor l00 = make_divisor(sqrt(a00));
  const double l10 = div_by(a01, l00), l20 = div_by(a02, l00);
  const double s11 = a11 - l10 * l10;
  if (!(s11 > 0.0)) return false;
  const Divisor l11 = make_divisor(sqrt(s11));
  const double l21 = div_by(a12 - l20 * l10, l11);
  const double s22 = a22 - l20 * l20 - l21 * l21;
  if (!(s22 > 0.0)) return false;
  const Divisor l22 = make_divisor(sqrt(s22));
  const double y0 = div_by(b0, l00);
  const double y1 = div_by(b1 - l10 * y0, l11);
  const double y2 = div_by(b2 - l20 * y0 - l21 * y1, l22);
  x2 = div_by(y2, l22);
  x1 = div_by(y1 - l21 * x2, l11);
  x0 = div_by(y0 - l10 * x1 - l20 * x2, l00);
  return isfinite(x0) && isfinite(x1) && isfinite(x2);
}

// argmin of 1/2 y'By + g'y on |y| = radius, B symmetric PSD 2x2 (Ceres: quartic roots; here
// eigen-decomposition + Newton on the secular equation, More-Sorensen; oracle/ilcc_oracle.c min_on_circle).
// First half: everything that does not depend on the radius.
__device__ __forceinline__ void circle_eigen(Dog& s) {
  const double B00 = s.sB00, B01 = s.sB01, B11 = s.sB11, gx = s.sg0, gy = s.sg1;
  const double d = 0.5 * (B00 - B11), e = B01;
  const double h = sqrt(d * d + e * e), mean = 0.5 * (B00 + B11);
  s.e_l1 = mean - h;
  s.e_l2 = mean + h;
  double v2x, v2y;
  if (h == 0.0) {
    v2x = 1.0;
    v2y = 0.0;
  } else if (d >= 0.0) {
    v2x = d + h;
    v2y = e;
  } else {
    v2x = e;
    v2y = h - d;
  }
  {
    const double nv = sqrt(v2x * v2x + v2y * v2y);
    if (nv > 0.0) {
      v2x /= nv;
      v2y /= nv;
    } else {
      v2x = 1.0;
      v2y = 0.0;
    }
  }
  const double v1x = -v2y, v1y = v2x;
  s.e_v1x = v1x;
  s.e_v1y = v1y;
  s.e_v2x = v2x;
  s.e_v2y = v2y;
  s.e_g1 = v1x * gx + v1y * gy;
  s.e_g2 = v2x * gx + v2y * gy;
  s.e_gn = sqrt(s.e_g1 * s.e_g1 + s.e_g2 * s.e_g2);
  s.eig_ready = 1;
}
// Second half: the multiplier for this radius
__device__ __forceinline__ void min_on_circle(Dog& s, double radius, double& yx, double& yy) {
  if (!s.eig_ready) circle_eigen(s);
  const double l1 = s.e_l1, l2 = s.e_l2, g1 = s.e_g1, g2 = s.e_g2;
  const Divisor rad = make_divisor(radius);
  const double gnr = div_by(s.e_gn, rad);
  double lo = fmax(0.0, -l1);
  lo = fmax(lo, gnr - l2);
  const double hi = gnr - l1;
  double lam = lo;
  if (!(l1 + lam > 0.0)) lam = lo + 1e-12 * fmax(1.0, fabs(hi));
  for (int it = 0; it < 60; ++it) {
    const double a1 = l1 + lam, a2 = l2 + lam;
    const double y1 = -g1 / a1, y2 = -g2 / a2;
    const double ny = sqrt(y1 * y1 + y2 * y2);
    const double qq = g1 * g1 / (a1 * a1 * a1) + g2 * g2 / (a2 * a2 * a2);
    if (!(qq > 0.0) || !isfinite(ny)) break;
    const double dl = (ny * ny / qq) * div_by(ny - radius, rad);
    double nl = lam + dl;
    if (!(l1 + nl > 0.0)) nl = 0.5 * (lam + fmax(0.0, -l1));
    if (fabs(nl - lam) <= 1e-15 * fmax(1.0, fabs(nl))) {
      lam = nl;
      break;
    }
    lam = nl;
  }
  const double a1 = l1 + lam, a2 = l2 + lam;
  double y1 = (a1 > 0.0) ? -g1 / a1 : 0.0, y2 = (a2 > 0.0) ? -g2 / a2 : 0.0;
  double ny = sqrt(y1 * y1 + y2 * y2);
  if (ny < radius * (1.0 - 1e-9) && !(a1 > 1e-300 * fmax(1.0, l2))) {
    y1 = sqrt(fmax(0.0, radius * radius - y2 * y2));
    ny = radius;
  }
  if (ny > 0.0) {
    const double k = radius / ny;
    y1 *= k;
    y2 *= k;
  }
  yx = s.e_v1x * y1 + s.e_v2x * y2;
  yy = s.e_v1y * y1 + s.e_v2y * y2;
}

__device__ __forceinline__ double nrm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

__device__ __forceinline__ void dogleg_traditional(Dog& s, double& s0, double& s1, double& s2) {
  const double gnn = nrm3(s.n0, s.n1, s.n2), gn_ = nrm3(s.g0, s.g1, s.g2);
  if (gnn <= s.radius) {
    s0 = div_by(s.n0, s.d0);
    s1 = div_by(s.n1, s.d1);
    s2 = div_by(s.n2, s.d2);
    s.step_norm = gnn;
    return;
  }
  if (gn_ * s.alpha >= s.radius) {
    const double k = -(s.radius / gn_);
    s0 = div_by(k * s.g0, s.d0);
    s1 = div_by(k * s.g1, s.d1);
    s2 = div_by(k * s.g2, s.d2);
    s.step_norm = s.radius;
    return;
  }
  const double a0 = -s.alpha * s.g0, a1 = -s.alpha * s.g1, a2 = -s.alpha * s.g2;
  const double bdota = a0 * s.n0 + a1 * s.n1 + a2 * s.n2;
  const double a2n = a0 * a0 + a1 * a1 + a2 * a2;
  const double bma2 = (s.n0 - a0) * (s.n0 - a0) + (s.n1 - a1) * (s.n1 - a1) + (s.n2 - a2) * (s.n2 - a2);
  const double cc = bdota - a2n;
  const double d = sqrt(cc * cc + bma2 * (s.radius * s.radius - a2n));
  const double beta = (cc <= 0) ? (d - cc) / bma2 : (s.radius * s.radius - a2n) / (d + cc);
  s0 = div_by(a0 + beta * (s.n0 - a0), s.d0);
  s1 = div_by(a1 + beta * (s.n1 - a1), s.d1);
  s2 = div_by(a2 + beta * (s.n2 - a2), s.d2);
  s.step_norm = s.radius;
}

// quadratic form u' A v with the symmetric 3x3 stored in Dog
__device__ __forceinline__ double qform(const Dog& s, double u0, double u1, double u2, double v0, double v1,
                                        double v2) {
  const double w0 = s.A00 * v0 + s.A01 * v1 + s.A02 * v2;
  const double w1 = s.A01 * v0 + s.A11 * v1 + s.A12 * v2;
  const double w2 = s.A02 * v0 + s.A12 * v1 + s.A22 * v2;
  return u0 * w0 + u1 * w1 + u2 * w2;
}

// DoglegStrategy::ComputeStep; A / r (scaled Jacobian) must be current when !reuse.
__device__ __forceinline__ bool dogleg_compute_step(Dog& s, double& s0, double& s1, double& s2) {
  if (!s.reuse) {
    s.reuse = 1;
    s.eig_ready = 0;
    s.d0 = make_divisor(sqrt(fmin(fmax(s.A00, 1e-6), 1e32)));
    s.d1 = make_divisor(sqrt(fmin(fmax(s.A11, 1e-6), 1e32)));
    s.d2 = make_divisor(sqrt(fmin(fmax(s.A22, 1e-6), 1e32)));
    s.g0 = div_by(s.r0, s.d0);
    s.g1 = div_by(s.r1, s.d1);
    s.g2 = div_by(s.r2, s.d2);
    {
      const double u0 = div_by(s.g0, s.d0), u1 = div_by(s.g1, s.d1), u2 = div_by(s.g2, s.d2);
      const double num = s.g0 * s.g0 + s.g1 * s.g1 + s.g2 * s.g2;
      s.alpha = num / qform(s, u0, u1, u2, u0, u1, u2);
    }
    bool ok = false;
    while (s.mu < 1.0) {
      const double sm = sqrt(s.mu);
      const double e0 = s.d0.d * sm, e1 = s.d1.d * sm, e2 = s.d2.d * sm;
      if (chol3_solve(s.A00 + e0 * e0, s.A01, s.A02, s.A11 + e1 * e1, s.A12, s.A22 + e2 * e2, s.r0, s.r1, s.r2,
                      s.n0, s.n1, s.n2)) {
        ok = true;
        break;
      }
      s.mu *= 10.0;
    }
    if (!ok) return false;
    s.n0 *= -s.d0.d;
    s.n1 *= -s.d1.d;
    s.n2 *= -s.d2.d;
    {
      const double q0 = s.g0 * s.g0 + s.g1 * s.g1 + s.g2 * s.g2;
      const double q1 = s.n0 * s.n0 + s.n1 * s.n1 + s.n2 * s.n2;
      const bool gfirst = q0 >= q1;
      const double nfv = sqrt(fmax(q0, q1));
      const Divisor nf = make_divisor(nfv);
      const double f0 = (gfirst ? s.g0 : s.n0), f1 = (gfirst ? s.g1 : s.n1), f2 = (gfirst ? s.g2 : s.n2);
      const double t0 = (gfirst ? s.n0 : s.g0), t1 = (gfirst ? s.n1 : s.g1), t2 = (gfirst ? s.n2 : s.g2);
      const double v00 = div_by(f0, nf), v01 = div_by(f1, nf), v02 = div_by(f2, nf);
      const double dot = t0 * v00 + t1 * v01 + t2 * v02;
      double v10 = t0 - dot * v00, v11 = t1 - dot * v01, v12 = t2 - dot * v02;
      const double nrv = nrm3(v10, v11, v12);
      s.one_dim = !(nrv > 3.0 * 2.220446049250313e-16 * nfv);
      if (!s.one_dim) {
        const Divisor nr = make_divisor(nrv);
        v10 = div_by(v10, nr);
        v11 = div_by(v11, nr);
        v12 = div_by(v12, nr);
        s.b00 = v00;
        s.b10 = v01;
        s.b20 = v02;
        s.b01 = v10;
        s.b11 = v11;
        s.b21 = v12;
        const double ua0 = div_by(v00, s.d0), ua1 = div_by(v01, s.d1), ua2 = div_by(v02, s.d2);
        const double ub0 = div_by(v10, s.d0), ub1 = div_by(v11, s.d1), ub2 = div_by(v12, s.d2);
        s.sg0 = v00 * s.g0 + v01 * s.g1 + v02 * s.g2;
        s.sg1 = v10 * s.g0 + v11 * s.g1 + v12 * s.g2;
        s.sB00 = qform(s, ua0, ua1, ua2, ua0, ua1, ua2);
        s.sB01 = qform(s, ua0, ua1, ua2, ub0, ub1, ub2);
        s.sB11 = qform(s, ub0, ub1, ub2, ub0, ub1, ub2);
      }
    }
  }
  const double gnn = nrm3(s.n0, s.n1, s.n2);
  if (gnn <= s.radius) {
    s0 = div_by(s.n0, s.d0);
    s1 = div_by(s.n1, s.d1);
    s2 = div_by(s.n2, s.d2);
    s.step_norm = gnn;
    return true;
  }
  if (s.one_dim) {
    const double k = -(s.radius / nrm3(s.g0, s.g1, s.g2));
    s0 = div_by(k * s.g0, s.d0);
    s1 = div_by(k * s.g1, s.d1);
    s2 = div_by(k * s.g2, s.d2);
    s.step_norm = s.radius;
    return true;
  }
  double yx, yy;
  min_on_circle(s, s.radius, yx, yy);
  if (!isfinite(yx) || !isfinite(yy)) {
    dogleg_traditional(s, s0, s1, s2);
    return true;
  }
  s0 = div_by(s.b00 * yx + s.b01 * yy, s.d0);
  s1 = div_by(s.b10 * yx + s.b11 * yy, s.d1);
  s2 = div_by(s.b20 * yx + s.b21 * yy, s.d2);
  s.step_norm = s.radius;
  return true;
}

// TrustRegionMinimizer::Minimize for 3 parameters, one wavefront, every lane on the same control flow.
#ifdef ILCC_K7_TIMING
__device__ unsigned long long g_k7_t[4];
#define K7_T0 const unsigned long long k7t0 = __builtin_readcyclecounter()
#define K7_ACC(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_k7_t[k] += __builtin_readcyclecounter() - k7t0; } while (0)
#else
#define K7_T0 do {} while (0)
#define K7_ACC(k) do {} while (0)
#endif

// One call site per evaluate<> flavour: the Jacobian pass of the start and of every accepted step is the `relinearise`
// block at the head of the loop (DoglegStrategy::StepAccepted's radius / mu updates do not read it, so running them
// first changes nothing) -- the kernel's code stays within the instruction cache.
template <bool WIDE>
__device__ __forceinline__ int trust_region_minimize(const Problem& q, double x[3], double& final_cost, int max_iter, Dog& s) {
  if (q.n == 0) {
    final_cost = 0.0;
    return 0;
  }
  double sums[10];
  // (s: this wavefront's dogleg state in LDS -- ~60 doubles that would otherwise stay live in VGPRs across every evaluation of
  // the points: 226 VGPRs, two wavefronts per SIMD; the wavefront reads them back, wave-uniform addresses, where the dogleg needs them)
  s.radius = 1e4;
  s.mu = 1e-8;
  s.reuse = 0;
  s.step_norm = 0.0;
  s.one_dim = 0;
  s.eig_ready = 0;
  double x_cost = 0.0, x_norm = 0.0;
  double gr0 = 0.0, gr1 = 0.0, gr2 = 0.0;
  double sc0 = 0.0, sc1 = 0.0, sc2 = 0.0;   // jacobi scaling from the initial Jacobian, kept for the whole solve
  int iter = 0, invalid = 0;
  bool relinearise = true, first = true;
  for (;;) {
    if (relinearise) {
      {
        K7_T0;
        evaluate<true, WIDE>(q, x, sums);
        K7_ACC(2);
      }
      x_cost = sums[0];
      x_norm = nrm3(x[0], x[1], x[2]);
      gr0 = sums[1];
      gr1 = sums[2];
      gr2 = sums[3];
      if (first) {
        sc0 = 1.0 / (1.0 + sqrt(sums[4]));
        sc1 = 1.0 / (1.0 + sqrt(sums[7]));
        sc2 = 1.0 / (1.0 + sqrt(sums[9]));
        first = false;
      }
      s.A00 = sums[4] * sc0 * sc0;
      s.A01 = sums[5] * sc0 * sc1;
      s.A02 = sums[6] * sc0 * sc2;
      s.A11 = sums[7] * sc1 * sc1;
      s.A12 = sums[8] * sc1 * sc2;
      s.A22 = sums[9] * sc2 * sc2;
      s.r0 = gr0 * sc0;
      s.r1 = gr1 * sc1;
      s.r2 = gr2 * sc2;
      relinearise = false;
    }
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (iter >= max_iter) break;
    if (fmax(fabs(gr0), fmax(fabs(gr1), fabs(gr2))) <= 1e-10) break;
    if (s.radius <= 1e-32) break;
    ++iter;
    double st0 = 0, st1 = 0, st2 = 0;
    bool valid;
    {
      K7_T0;
      valid = dogleg_compute_step(s, st0, st1, st2);
      K7_ACC(0);
    }
    double mcc = 0;
    if (valid) {
      // model_cost_change = -(J step)'(r + J step/2) = -(g' step + step' JtJ step / 2)
      const double gs = s.r0 * st0 + s.r1 * st1 + s.r2 * st2;
      mcc = -(gs + 0.5 * qform(s, st0, st1, st2, st0, st1, st2));
      valid = mcc > 0.0;
    }
    if (!valid) {
      if (++invalid >= 5) break;
      s.mu *= 10.0;   // StepIsInvalid
      s.reuse = 0;
      continue;
    }
    invalid = 0;
    const double cand[3] = {x[0] + st0 * sc0, x[1] + st1 * sc1, x[2] + st2 * sc2};
    double cs[10];
    {
      K7_T0;
      evaluate<false, WIDE>(q, cand, cs);
      K7_ACC(1);
    }
    const double cand_cost = cs[0];
    const double step_norm = nrm3(x[0] - cand[0], x[1] - cand[1], x[2] - cand[2]);
    if (step_norm <= 1e-8 * (x_norm + 1e-8)) break;            // ParameterToleranceReached
    const double cost_change = x_cost - cand_cost;
    if (fabs(cost_change) <= 1e-6 * x_cost) break;             // FunctionToleranceReached
    const double rel = cost_change / mcc;
    if (rel > 1e-3) {                                          // HandleSuccessfulStep
      x[0] = cand[0];
      x[1] = cand[1];
      x[2] = cand[2];
      relinearise = true;
      if (rel < 0.25) s.radius *= 0.5;                         // DoglegStrategy::StepAccepted
      if (rel > 0.75) s.radius = fmax(s.radius, 3.0 * s.step_norm);
      if (s.radius > 1e16) s.radius = 1e16;
      s.mu = fmax(1e-8, 2.0 * s.mu / 10.0);
      s.reuse = 0;
    } else {                                                   // StepRejected
      s.radius *= 0.5;
      s.reuse = 1;
    }
  }
  final_cost = x_cost;
  return iter;
}

// ------------------------------------------------------------------ K7a
// pass A then pass B of (frame f, phase slot) on the points q.yz / q.lab: one wavefront (WIDE = false) or the whole workgroup
template <bool WIDE>
__device__ __forceinline__ void solve_wave(const Ctx& c, Problem& q, uint32_t f, uint32_t slot, SolveRec* out, Dog& dog) {
  double x[3] = {0.0, 0.0, 0.0};
  int phase = (int)slot;
  if (c.p.phase_mode != 2) {
    phase = (c.p.phase_mode == 1) ? 1 : 0;
  }
  q.tlw = phase != 0;
  double cost[2] = {0.0, 0.0};
  int iters[2] = {0, 0};
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {
    q.oob = pass == 0;   // pass A: useOutofBoard (LidarCornersEst.cpp:403-405), pass B: not (:406-408)
    double fc = 0.0;
    const int it = trust_region_minimize<WIDE>(q, x, fc, c.p.max_iterations, dog);
    cost[pass] = fc;
    iters[pass] = it;
  }
#ifdef ILCC_K7_TIMING
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    printf("K7a f0 slot %d: iters %d + %d; cycles dogleg %llu, evaluate<false> %llu, evaluate<true> %llu\n", (int)slot, iters[0], iters[1], g_k7_t[0], g_k7_t[1], g_k7_t[2]);
    g_k7_t[0] = g_k7_t[1] = g_k7_t[2] = 0;
  }
#endif
  q.oob = true;
  double cs[10];
  evaluate<false, WIDE>(q, x, cs);
  if (WIDE ? threadIdx.x == 0 : lane_id() == 0) {
    out->x[0] = x[0];
    out->x[1] = x[1];
    out->x[2] = x[2];
    out->cost_a = cost[0];
    out->cost_b = cost[1];
    out->sel = cs[0];
    out->iters_a = iters[0];
    out->iters_b = iters[1];
    out->phase = phase;
    out->valid = 1;
    out->margin = 0.0;
    out->flags = 0;
    out->ties = 0;
  }
}

// grid: ceil(n_frames * n_slots / kSolveWaves) workgroups; wavefront w of workgroup b runs solve b * kSolveWaves + w =
// (frame, slot) = (solve / n_slots, solve % n_slots): with two slots the wavefronts 2k and 2k + 1 share a frame and its
// staged points.  Dynamic LDS: staged_points_bytes(grid_lds_points, kSolveWaves / n_slots).
#ifndef ILCC_K7A_WAVES_PER_EU
#define ILCC_K7A_WAVES_PER_EU 3
#endif
__global__ __launch_bounds__(kSolveThreads) __attribute__((amdgpu_waves_per_eu(ILCC_K7A_WAVES_PER_EU, ILCC_K7A_WAVES_PER_EU))) void k7a_local_solve(Ctx c, SolveRec* rec, int n_slots) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ Dog s_dog[kSolveWaves];   // one dogleg state per wavefront (= per solve)
  const uint32_t wave = (uint32_t)wave_id();
  const uint32_t solve = blockIdx.x * (uint32_t)kSolveWaves + wave;
  const uint32_t f = solve / (uint32_t)n_slots, slot = solve % (uint32_t)n_slots;
  const bool live = f < c.n_frames && c.res[f].status == ILCC_OK;
  const uint32_t n = live ? c.n_lab[f] : 0u;
  const bool in_lds = n <= c.grid_lds_points;
  // staging: the n_slots wavefronts of a frame copy its points together
  const StagedPoints st = staged_points(smem, c.grid_lds_points, (uint32_t)(kSolveWaves / n_slots), wave / (uint32_t)n_slots);
  const uint64_t beg = live ? c.off[f] : 0u;
  if (live && in_lds) {
    for (uint32_t i = slot * ILCC_WAVE + (uint32_t)lane_id(); i < n; i += (uint32_t)n_slots * ILCC_WAVE) {
      st.yz[i] = c.yz[beg + i];
      st.lab[i] = c.lab[beg + i];
    }
  }
  __syncthreads();   // the only barrier: from here on every wavefront is on its own
  if (f >= c.n_frames) return;
  SolveRec* out = &rec[2 * f + slot];
  if (!live) {
    if (lane_id() == 0) out->valid = 0;
    return;
  }
  Problem q;
  q.n = n;
  q.bd = make_board(c.p);
  // (two calls, not one on selected pointers: each shows the compiler the address space of yz and lab)
  if (in_lds) {
    q.yz = st.yz;
    q.lab = st.lab;
    solve_wave<false>(c, q, f, slot, out, s_dog[wave]);
  } else {   // a frame above the handle's LDS capacity (it grows after the batch): the points stay in HBM / L2
    q.yz = c.yz + beg;
    q.lab = c.lab + beg;
    solve_wave<false>(c, q, f, slot, out, s_dog[wave]);
  }
}

// Small batches (n_frames <= kSolveWideMaxFrames: fewer solves than SIMDs): one 256-thread workgroup per (frame, slot), the
// layout of rounds 1-5 on this round's arithmetic -- 128 frames alone on the chip: 0.62 ms (round 5), 1.11 ms (one wavefront per
// solve), see profiles/README.md for this variant.  Both layouts add the same terms in the same order (evaluate<>): a frame's
// result does not depend on the batch it came in.
__global__ __launch_bounds__(kSolveThreads) void k7a_local_solve_wide(Ctx c, SolveRec* rec) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double s_red[2 * kSolveRedDoubles];
  __shared__ Dog s_dog[kSolveWaves];   // every wavefront keeps its own copy of the (identical) dogleg state: no cross-wavefront hazards
  const uint32_t f = blockIdx.x, slot = blockIdx.y;
  SolveRec* out = &rec[2 * f + slot];
  if (c.res[f].status != ILCC_OK) {
    if (threadIdx.x == 0) out->valid = 0;
    return;
  }
  const StagedPoints st = staged_points(smem, c.grid_lds_points, 1, 0);
  const uint64_t beg = c.off[f];
  const uint32_t n = c.n_lab[f];
  int flip = 0;
  Problem q;
  q.n = n;
  q.bd = make_board(c.p);
  q.red = s_red;
  q.flip = &flip;
  // (two calls, as in k7a_local_solve: the address space of yz and lab stays visible)
  if (n <= c.grid_lds_points) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      st.yz[i] = c.yz[beg + i];
      st.lab[i] = c.lab[beg + i];
    }
    __syncthreads();
    q.yz = st.yz;
    q.lab = st.lab;
    solve_wave<true>(c, q, f, slot, out, s_dog[wave_id()]);
  } else {
    q.yz = c.yz + beg;
    q.lab = c.lab + beg;
    solve_wave<true>(c, q, f, slot, out, s_dog[wave_id()]);
  }
}

// test entry: one solve (one wavefront) on frame 0's labelled points (global memory)
__global__ __launch_bounds__(ILCC_WAVE) void k7_local_solve_test(Ctx c, int tlw, int use_oob, double* theta_t,
                                                                 double* cost_iters) {
  Problem q;
  q.yz = c.yz;
  q.lab = c.lab;
  q.n = c.n_lab[0];
  q.bd = make_board(c.p);
  q.tlw = tlw != 0;
  q.oob = use_oob != 0;
  __shared__ Dog s_dog1;
  double x[3] = {theta_t[0], theta_t[1], theta_t[2]};
  double cost = 0;
  const int it = trust_region_minimize<false>(q, x, cost, c.p.max_iterations, s_dog1);
  if (threadIdx.x == 0) {
    theta_t[0] = x[0];
    theta_t[1] = x[1];
    theta_t[2] = x[2];
    cost_iters[0] = cost;
    cost_iters[1] = (double)it;
  }
}

hipError_t set_kernel_attributes_k7a() {
  // (k7a_local_solve stages up to kSolveWaves frames per workgroup; launch_reference_solve falls back to the global-memory
  // path -- LDS capacity 0 -- when they would not fit the 160 KB of a CU)
  hipError_t e = hipFuncSetAttribute((const void*)k7a_local_solve, hipFuncAttributeMaxDynamicSharedMemorySize, kSolveLdsMax);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)k7a_local_solve_wide, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)staged_points_bytes(kGridLdsPointsMax, 1));
  return e;
}

void launch_reference_solve(const Ctx& c, hipStream_t s) {
  const int n_slots = solve_slots(c.p);
  if (c.n_frames <= (uint32_t)kSolveWideMaxFrames) {
    hipLaunchKernelGGL(k7a_local_solve_wide, dim3(c.n_frames, n_slots), dim3(kSolveThreads), staged_points_bytes(c.grid_lds_points, 1),
                       s, c, c.solve_rec);
    return;
  }
  Ctx ck = c;
  size_t lds = staged_points_bytes(c.grid_lds_points, (uint32_t)(kSolveWaves / n_slots));
  if (lds > (size_t)kSolveLdsMax) {   // very large frames: the points stay in HBM / L2
    ck.grid_lds_points = 0;
    lds = 0;
  }
  const uint32_t solves = c.n_frames * (uint32_t)n_slots;
  hipLaunchKernelGGL(k7a_local_solve, dim3((solves + kSolveWaves - 1) / kSolveWaves), dim3(kSolveThreads), lds, s, ck, c.solve_rec, n_slots);
}

void launch_local_solve(const Ctx& c, hipStream_t s, int32_t tlw, int32_t use_oob, double* theta_t,
                        double* cost_iters) {
  hipLaunchKernelGGL(k7_local_solve_test, dim3(1), dim3(ILCC_WAVE), 0, s, c, tlw, use_oob, theta_t, cost_iters);
}

}  // namespace ilcc
