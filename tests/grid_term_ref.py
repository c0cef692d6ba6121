"""K6's fp32 per-point term restated in numpy, operation for operation: the tables of upload_tables (ilcc_api.cpp), rotate()
(k5w_walk_order.h), accumulate<OOB> and accumulate_interior (k6_common.h), and the order of better() -- with every fmaf as ONE
rounding (fma32) and every other operation as the float32 operation numpy has for it.

Plain module beside constructed_bounds.py (no fixtures).  Nothing here is tuned against the kernels.

What a candidate's value is.  A lane adds its points' terms with A = fmaf(T, w, A), w in {0, 1/2}: T w is exact (a power of two
times a float32), so the lane's sum is a sum of the float32 values T w, rounded once per addition; the four lanes of a quad are added
by two more additions and the volume holds twice that.  volume_ref returns, per candidate, the EXACT sum of those float32 values
(times two), as Python integers in units of 2^-150 -- every float32 is a whole number of 2^-149 -- and the same numbers as Python
floats (int / int: correctly rounded).  The terms are non-negative, so the sum is also S, the sum of their magnitudes.

Where every term of a candidate is a whole number of 2^-k and the sum stays below 2^(24 - k), every partial sum in any order is a
float32: the kernel's value IS the exact sum, whatever the form that computed it.  Elsewhere a value computed with at most n
additions differs from the exact sum by at most n 2^-24 S (each addition rounds by at most 2^-24 of a partial sum, and a partial sum
of non-negative terms is at most S).
"""
from collections import namedtuple

import numpy as np

import constructed_bounds as cb

F = np.float32
UNIT_LOG2 = 150                 # the integers of volume_ref count 2^-150
POINT_CHUNK = 1024              # points per block of the evaluation (memory only)
MUTANTS = ("outline_gt", "parity_without_hw", "no_min", "interior_on_border", "last_point_out", "clamp_short")

Volume = namedtuple("Volume", "num val n_points interior")   # num: object [n_th, n_ty, n_tz, 2] of Python ints; val: float64, the same


# ---------------------------------------------------------------------------------------------------------------- one rounding
def fma32(a, b, c):
    """fmaf on float32 arrays: a * b + c rounded ONCE.  The product of two float32 is exact in float64; the float64 sum s and its
    exact error e (Knuth's two-sum) give the real value s + e; s is moved to the neighbour with an odd last bit when e != 0
    (rounding to odd), after which the rounding to float32 (29 bits shorter) is the rounding of the real value."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s, e = np.broadcast_arrays(s, e)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(F)


def fract32(x):
    """v_fract_f32 on the values the term gives it (multiples of 1/2 of small magnitude): x - floor(x)"""
    x = np.asarray(x, F)
    return x - np.floor(x)


# ---------------------------------------------------------------------------------------------------------------- tables, rotation
def tables32(p):
    """upload_tables: cos / g, sin / g, (t + W g / 2) / g in double, then float -> (cth, sth, ay, az) float32, (c_th, c_ty, c_tz)"""
    g = float(p.grid_length)
    th = np.array([p.th_min + k * p.th_step for k in range(p.n_th)], np.float64)
    cth, sth = (np.cos(th) / g).astype(F), (np.sin(th) / g).astype(F)
    ay = np.array([((p.ty_min + a * p.ty_step) + p.board_w * g / 2.0) / g for a in range(p.n_ty)], np.float64).astype(F)
    az = np.array([((p.tz_min + b * p.tz_step) + p.board_h * g / 2.0) / g for b in range(p.n_tz)], np.float64).astype(F)
    return cth, sth, ay, az, cb.tables(p)[4]


def rotate32(yz, cth, sth):
    """rotate(): (fmaf(-sth, z, cth * y), fmaf(cth, z, sth * y)) -- the products in front rounded on their own"""
    y, z = np.asarray(yz[:, 0], F), np.asarray(yz[:, 1], F)
    return fma32(-F(sth), z, F(cth) * y), fma32(F(cth), z, F(sth) * y)


def interior_class(p, yz):
    """which points K6 hands to accumulate_interior: K5w's interior class, for a frame that has a walk layout (at most
    kGridLdsPointsMax points); a larger frame is walked through accumulate<OOB> alone"""
    if len(yz) == 0 or len(yz) > cb.K_GRID_LDS_POINTS_MAX:
        return np.zeros(len(yz), bool)
    return cb.walk_classes(p, yz)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the term
def point_terms(pi, pj, hw, ay, az, Wh, Hh, delta, interior, use_oob, mutant=None):
    """accumulate<OOB> / accumulate_interior for points (pi, pj, hw)[m] under translations ay[na] x az[nb] -> (T w0, T w1), float32
    [m, na, nb]: what the two fmaf of a call add to A0 and A1 (exact products: w is 0 or 1/2)."""
    half, one, zero = F(0.5), F(1.0), F(0.0)
    i = pi[:, None] + ay[None, :]                          # [m, na]
    j = pj[:, None] + az[None, :]                          # [m, nb]
    fi, fj = np.floor(i), np.floor(j)
    ai, aj = (i - fi) - half, (j - fj) - half
    Rin = one - (np.abs(ai)[:, :, None] + np.abs(aj)[:, None, :])
    fsum = fi[:, :, None] + fj[:, None, :]
    hw3 = zero if mutant == "parity_without_hw" else hw[:, None, None]
    mf = fract32(fma32(half, fsum, hw3))
    nmf = half - mf
    ui, uj = np.abs(i - Wh) - Wh, np.abs(j - Hh) - Hh
    umax = np.maximum(ui[:, :, None], uj[:, None, :])
    oob = (umax > zero) if mutant == "outline_gt" else (umax >= zero)
    inner = np.ones(len(pi), bool) if mutant == "interior_on_border" else interior
    oob = oob & ~inner[:, None, None]                      # accumulate_interior has no out-of-board side
    if use_oob:
        R = np.where(oob, np.abs(ui)[:, :, None] + np.abs(uj)[:, None, :], Rin)
        w0, w1 = np.where(oob, half, mf), np.where(oob, half, nmf)
    else:
        R = np.where(oob, zero, Rin)
        w0, w1 = mf, nmf
    Q = R if mutant == "no_min" else np.minimum(R, delta)
    T = Q * fma32(-half, Q, R)
    return T * w0, T * w1


class _ExactSum:
    """sums of float32 values over axis 0, exactly: every value is cut into four limbs of 40 bits (float64 operations that are exact on
    a 24-bit significand), the limbs are added as int64 and put together as Python integers in units of 2^-UNIT_LOG2"""

    def __init__(self, shape):
        self.limbs = [np.zeros(shape, np.int64) for _ in range(4)]

    def add(self, t):
        x = t.astype(np.float64)
        assert (x >= 0).all() and (x < 2.0 ** 10).all()   # (the top limb then stays below 2^40 like the others)
        x = x * 2.0 ** UNIT_LOG2
        for n, sh in enumerate((120, 80, 40)):
            top = np.floor(x * 2.0 ** -sh)
            self.limbs[n] += top.astype(np.int64).sum(axis=0)
            x = x - top * 2.0 ** sh
            if not x.any():
                return
        self.limbs[3] += x.astype(np.int64).sum(axis=0)

    def total(self):
        out = self.limbs[0].astype(object) << 120
        for n, sh in enumerate((80, 40, 0), start=1):
            out = out + (self.limbs[n].astype(object) << sh)
        return out


def _as_floats(num):
    flat = np.array([n / (1 << UNIT_LOG2) for n in num.ravel()], np.float64)   # int / int: correctly rounded
    return flat.reshape(num.shape)


def volume_ref(p, yz, lab, use_oob, mutant=None, thetas=None, exact=None):
    """The restated cost volume [n_th, n_ty, n_tz, 2] of K6 for the labelled points (yz, lab) under the parameters p: per candidate
    and colour phase, twice the exact sum of the restated float32 terms (= S, the terms are non-negative) -> Volume.  thetas: the
    slices to evaluate (the others stay 0).  exact = (k, n): asserts that every term of slice k is a whole number of 2^-n."""
    yz, lab = np.asarray(yz, F).reshape(-1, 2), np.asarray(lab, np.uint8)
    cth, sth, ay, az, _ = tables32(p)
    if mutant == "clamp_short":
        ay, az = ay.copy(), az.copy()
        ay[-1], az[-1] = ay[max(len(ay) - 2, 0)], az[max(len(az) - 2, 0)]
    interior = interior_class(p, yz)
    m = len(lab) - 1 if (mutant == "last_point_out" and len(lab)) else len(lab)
    Wh, Hh, delta = F(0.5) * F(p.board_w), F(0.5) * F(p.board_h), F(p.huber_delta)
    hw = np.where(lab != 0, F(0.5), F(0.0)).astype(F)
    num = np.zeros((p.n_th, p.n_ty, p.n_tz, 2), object)
    for k in (range(p.n_th) if thetas is None else thetas):
        pi, pj = rotate32(yz, cth[k], sth[k])
        acc = (_ExactSum((p.n_ty, p.n_tz)), _ExactSum((p.n_ty, p.n_tz)))
        for lo in range(0, m, POINT_CHUNK):
            s = slice(lo, min(lo + POINT_CHUNK, m))
            t0, t1 = point_terms(pi[s], pj[s], hw[s], ay, az, Wh, Hh, delta, interior[s], use_oob, mutant)
            if exact is not None and exact[0] == k:
                for t in (t0, t1):
                    u = t.astype(np.float64) * 2.0 ** exact[1]
                    assert np.array_equal(u, np.floor(u)), "a term of the exact slice is no whole number of units"
            acc[0].add(t0)
            acc[1].add(t1)
        num[k, :, :, 0] = acc[0].total() * 2
        num[k, :, :, 1] = acc[1].total() * 2
    return Volume(num, _as_floats(num), len(lab), interior)


def float32_bits(num):
    """the candidates' exact values as float32 bit patterns -- asserts that each IS a float32 (an exact frame)"""
    val = _as_floats(num)
    f = val.astype(F)
    back = np.array([int(v) for v in (f.astype(np.float64) * 2.0 ** UNIT_LOG2).ravel()], object).reshape(num.shape)
    assert (back == num).all(), "a candidate's exact value is no float32"
    return f.view(np.uint32)


def term_units(num, unit_log2):
    """the candidates' values in whole units of 2^-unit_log2 (asserts that they are whole) -> object array of Python ints"""
    sh = UNIT_LOG2 - unit_log2
    assert all(n % (1 << sh) == 0 for n in num.ravel())
    return num >> sh


# ---------------------------------------------------------------------------------------------------------------- the argmin
def argmin_ref(p, volume):
    """better()'s order over a whole volume [n_th, n_ty, n_tz, 2] (numbers that compare as the kernel's float32 do): cost, then the
    squared index distance to the table entries nearest zero, then the flat index -> flat index"""
    c_th, c_ty, c_tz = cb.tables(p)[4]
    k, a, b = np.meshgrid(np.arange(p.n_th), np.arange(p.n_ty), np.arange(p.n_tz), indexing="ij")
    d2 = np.repeat(((k - c_th) ** 2 + (a - c_ty) ** 2 + (b - c_tz) ** 2).ravel(), 2)
    v = np.asarray(volume).reshape(-1)
    best = None
    for flat in np.flatnonzero(v == v.min()):
        key = (int(d2[flat]), int(flat))
        if best is None or key < best:
            best = key
    return best[1]
