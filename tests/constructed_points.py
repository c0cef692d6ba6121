"""Constructed labelled points for the GRID back end (K6's argmin, the near-tie recount, K7r): inputs that the labelled points
of synthetic frames never are -- noise-free boards whose cost is exactly 0 on a whole block of candidates, coordinates exactly on
the branches of the per-point term, point counts at wavefront and staging edges, 64-point chunks with a chosen number of points
that the refinement's stencil may skip -- and `exact_cost_q`, the fixed-point cost in exact rational arithmetic.

Plain module beside cbdetect_ref.py (no fixtures).  Every generator returns (float32 yz[m, 2], uint8 label[m]) and is deterministic
from its seed.  `p` is any parameter struct with board_w, board_h and grid_length (the library's or the oracle's).

A pose (th, ty, tz) is the solver's unknown: a point with board coordinate (i, j) squares under that pose has
  ry = i g - W g / 2 - ty,  rz = j g - H g / 2 - tz,  (y, z) = R(-th) (ry, rz),
so that the functor's (cos th y - sin th z + ty + W g / 2) / g gives i back.
"""
import functools
from fractions import Fraction

import numpy as np


def from_board(p, i, j, pose=(0.0, 0.0, 0.0)):
    """board coordinates (squares) under `pose` -> float32 yz[m, 2]"""
    th, ty, tz = pose
    W, H, g = p.board_w, p.board_h, p.grid_length
    ry = np.asarray(i, np.float64) * g - W * g / 2 - ty
    rz = np.asarray(j, np.float64) * g - H * g / 2 - tz
    y = np.cos(th) * ry + np.sin(th) * rz
    z = -np.sin(th) * ry + np.cos(th) * rz
    return np.stack([y, z], axis=1).astype(np.float32)


def board_coords(p, yz, x):
    """fp64 board coordinates (i, j) of float32 points under theta_t = x, with the term's own expressions"""
    W, H, g = float(p.board_w), float(p.board_h), p.grid_length
    y, z = yz[:, 0].astype(np.float64), yz[:, 1].astype(np.float64)
    c, s = np.cos(x[0]), np.sin(x[0])
    inv_g = 1.0 / g
    return ((c * y - s * z + x[1]) + W * g / 2.0) * inv_g, ((s * y + c * z + x[2]) + H * g / 2.0) * inv_g


def nearest_lattice(p, pose):
    """the refinement-lattice point nearest a pose"""
    div = p.refine_div if p.refine_div > 0 else 1
    return [int(round((pose[0] - p.th_min) / (p.th_step / div))), int(round((pose[1] - p.ty_min) / (p.ty_step / div))),
            int(round((pose[2] - p.tz_min) / (p.tz_step / div)))]


def ideal_board(p, J, K, seed, pose=(0.0, 0.0, 0.0)):
    """K points in every cell (ci, cj) at (ci + 1/2 + U(-J, J), cj + 1/2 + U(-J, J)), label (ci + cj) & 1 (phase 0): a noise-free,
    correctly labelled board.  Every candidate that keeps all points inside their cells costs exactly 0."""
    rng = np.random.default_rng(seed)
    W, H = p.board_w, p.board_h
    ci, cj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    ci, cj = np.repeat(ci.ravel(), K), np.repeat(cj.ravel(), K)
    i = ci + 0.5 + rng.uniform(-J, J, len(ci))
    j = cj + 0.5 + rng.uniform(-J, J, len(ci))
    return from_board(p, i, j, pose), ((ci + cj) & 1).astype(np.uint8)


def noisy_board(p, m, seed, pose=(0.0, 0.0, 0.0)):
    """m points in random cells at uniform in-cell positions; 10 % of the labels flipped, 10 % of the points moved 0-1.5 squares
    outside the outline: any m, a unique positive minimum near `pose`."""
    rng = np.random.default_rng(seed)
    W, H = p.board_w, p.board_h
    ci, cj = rng.integers(0, W, m), rng.integers(0, H, m)
    i, j = ci + rng.uniform(0, 1, m), cj + rng.uniform(0, 1, m)
    lab = (ci + cj) & 1
    lab = np.where(rng.random(m) < 0.1, 1 - lab, lab)
    out, side, far = rng.random(m) < 0.1, rng.integers(0, 4, m), rng.uniform(0, 1.5, m)
    i = np.where(out & (side == 0), -far, np.where(out & (side == 1), W + far, i))
    j = np.where(out & (side == 2), -far, np.where(out & (side == 3), H + far, j))
    return from_board(p, i, j, pose), lab.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- dyadic board
DYADIC = dict(board_w=6, board_h=8, grid_length=0.25, huber_delta=0.125,
              n_th=21, th_step=2.0 ** -6, th_min=-10 * 2.0 ** -6,
              n_ty=32, ty_step=2.0 ** -6, ty_min=-0.25, n_tz=32, tz_step=2.0 ** -6, tz_min=-0.25)


def dyadic_params():
    """Parameter fields of a board on which the term is exactly computable: every length a power of two (or a small multiple), so
    that with points on multiples of 2^-10 m and theta = 0 (lattice row 10 * div) every board coordinate is an exact dyadic number
    and can sit EXACTLY on a branch of the term.  Returned as {field: value}; the caller sets them on its parameter struct."""
    return dict(DYADIC)


def apply_fields(p, fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def dyadic_points(seed):
    """600 points on multiples of 2^-10 m for dyadic_params(): 100 with i an exact integer at t = 0 (both outlines i = 0 and i = W
    among them), 100 the same for j, 50 on exact half cells, 50 with fr_i = fr_j = 1/16 (a wrong-colour point there has
    res == delta exactly), the rest random; labels random."""
    W, H, g = DYADIC["board_w"], DYADIC["board_h"], DYADIC["grid_length"]
    rng = np.random.default_rng(seed)
    m = 600
    y = rng.integers(-1228, 1229, m) / 1024.0
    z = rng.integers(-1536, 1537, m) / 1024.0
    y[:100] = (rng.integers(0, W + 1, 100) - W / 2) * g
    y[0], y[1] = -W / 2 * g, W / 2 * g
    z[100:200] = (rng.integers(0, H + 1, 100) - H / 2) * g
    z[100], z[101] = -H / 2 * g, H / 2 * g
    y[200:250] = (rng.integers(0, W, 50) + 0.5 - W / 2) * g
    y[250:300] = (rng.integers(0, W, 50) + 1 / 16 - W / 2) * g
    z[250:300] = (rng.integers(0, H, 50) + 1 / 16 - H / 2) * g
    return np.stack([y, z], axis=1).astype(np.float32), rng.integers(0, 2, m).astype(np.uint8)


def dyadic_points_symmetric(seed):
    """The first 300 points of dyadic_points(seed) and their images under (y, z) -> (-y, -z), labels kept: the 6 x 8 board maps
    onto itself with its colours under that half turn, and negation is exact in floating point, so the cost at (th, ty, tz) equals
    the cost at (th, -ty, -tz) EXACTLY.  On the line ty = tz = 0 the 26 neighbours of a stencil come in tied pairs."""
    yz, lab = dyadic_points(seed)
    return np.concatenate([yz[:300], -yz[:300]]), np.concatenate([lab[:300], lab[:300]])


# ---------------------------------------------------------------------------------------------------------------- queue fills
def chunk_counts(seed, n=44):
    """Active points per 64-point chunk, over {0, 1, 63, 64}.  Chunks 0-6 are 63, 64, 64, 64, 0, 0, 1: a wavefront that takes every
    chunk (192 threads) has 127 points in flight after chunk 1 and again after chunks 2 and 3 -- the ring of 128 slots wraps -- and
    then meets two empty chunks.  A wavefront that takes every 4th chunk from chunk 0 (768 threads) sees 63, 0, 1, 64, 0 (two
    drains, nothing left) and then 63, 64, 64 at chunks 20, 24, 28.  The other entries are seeded draws."""
    rng = np.random.default_rng(seed)
    counts = [int(v) for v in rng.choice([0, 1, 63, 64], n)]
    counts[0:7] = [63, 64, 64, 64, 0, 0, 1]
    counts[8], counts[12], counts[16], counts[20], counts[24], counts[28] = 1, 64, 0, 63, 64, 64
    return counts


def chunk_pattern(p, counts, seed, pose=(0.0, 0.0, 0.0)):
    """m = 64 len(counts) + 17 points.  In 64-point chunk c of the input order exactly counts[c] points are ACTIVE -- the wrong
    colour for their cell, at least 0.2 square from each of its borders: their term is positive under every candidate of a stencil
    near `pose`, so a dropped or repeated point changes a sum -- at seeded positions of the chunk, and the others are SILENT: their
    own colour, within +-0.25 square of the cell's centre.  The 17 points of the tail alternate, starting active.
    -> (yz, label, active[m])"""
    rng = np.random.default_rng(seed)
    W, H = p.board_w, p.board_h
    m = 64 * len(counts) + 17
    active = np.zeros(m, bool)
    for c, k in enumerate(counts):
        active[64 * c + rng.permutation(64)[:k]] = True
    active[64 * len(counts)::2] = True
    ci, cj = rng.integers(0, W, m), rng.integers(0, H, m)
    half = np.where(active, 0.3, 0.25)
    i = ci + 0.5 + rng.uniform(-1, 1, m) * half
    j = cj + 0.5 + rng.uniform(-1, 1, m) * half
    lab = ((ci + cj) & 1) ^ active
    return from_board(p, i, j, pose), lab.astype(np.uint8), active


def silent_mask(p, yz, label, lat, phase, stride, cs=None):
    """stencil_sweep's silence test in fp64 numpy for the stencil centred on lattice point `lat` with this stride, for the theta
    lat[0] (cs = (cos, sin) of it, by default of the lattice angle): one cell, strictly inside the board, under both extreme
    translations, and the label is that cell's colour."""
    W, H, g = float(p.board_w), float(p.board_h), p.grid_length
    div = float(p.refine_div if p.refine_div > 0 else 1)
    c, s = cs if cs is not None else (np.cos(p.th_min + lat[0] * (p.th_step / div)), np.sin(p.th_min + lat[0] * (p.th_step / div)))
    y, z = yz[:, 0].astype(np.float64), yz[:, 1].astype(np.float64)
    ry, rz = c * y - s * z, s * y + c * z
    inv_g = 1.0 / g
    x1 = [p.ty_min + float(lat[1] + d * stride) * (p.ty_step / div) for d in (-1, 1)]
    x2 = [p.tz_min + float(lat[2] + d * stride) * (p.tz_step / div) for d in (-1, 1)]
    i0, i2 = ((ry + x1[0]) + W * g / 2.0) * inv_g, ((ry + x1[1]) + W * g / 2.0) * inv_g
    j0, j2 = ((rz + x2[0]) + H * g / 2.0) * inv_g, ((rz + x2[1]) + H * g / 2.0) * inv_g
    fi, fj = np.floor(i0), np.floor(j0)
    one_cell = (i0 > 0) & (i2 < W) & (j0 > 0) & (j2 < H) & (fi == np.floor(i2)) & (fj == np.floor(j2))
    odd = (fi.astype(np.int64) ^ fj.astype(np.int64)) & 1
    white = np.where(odd == 0, phase != 0, phase == 0)
    return one_cell & ((np.asarray(label) != 0) == white)


def far_points(m, lo, hi, seed):
    """m points with y and z uniform in [lo, hi) m -- off the default board's corner -- and random labels: out-of-board terms only,
    the largest the term has for a given distance."""
    rng = np.random.default_rng(seed)
    yz = np.stack([rng.uniform(lo, hi, m), rng.uniform(lo, hi, m)], axis=1).astype(np.float32)
    return yz, rng.integers(0, 2, m).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- exact reference
def _rint_half_even(q):
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return f


@functools.lru_cache(maxsize=1 << 16)
def _axis(c, t, n, g):
    """one axis of one point: float32 coordinate c, translation t, n squares of side g -> (strictly inside, floor odd, distance to
    the nearer border of the cell, distance to the nearer outline); cached: the costs of a stencil share their axes"""
    v = (Fraction(c) + t + n * g / 2) / g
    fl = v.numerator // v.denominator
    fr = v - fl
    return 0 < v < n, fl % 2 == 1, (fl + 1 - v if fr > Fraction(1, 2) else fr), min(abs(v), abs(v - n))


def exact_cost_q(p, yz, label, ty, tz, phase):
    """The fixed-point pass-A cost at theta = 0 in exact rational arithmetic, independent of the oracle: the functor's residual
    (strictly inside the board: the in-cell distance of a wrong-colour point, else 0; outside: the distance to the nearer outline
    per axis), Huber's rho on r, rint half-to-even of 1/2 rho 2^40, summed with Python integers.  Equals what IEEE doubles compute
    wherever every intermediate value is exactly representable: dyadic parameters and points (dyadic_params / dyadic_points)."""
    W, H = p.board_w, p.board_h
    g, d = Fraction(p.grid_length), Fraction(p.huber_delta)
    ty, tz = Fraction(ty), Fraction(tz)
    tot = 0
    for (y, z), lab in zip(yz, label):
        in_i, odd_i, di, ei = _axis(float(y), ty, W, g)
        in_j, odd_j, dj, ej = _axis(float(z), tz, H, g)
        res = Fraction(0)
        if in_i and in_j:
            white = bool(phase) if odd_i == odd_j else not phase
            if bool(lab) != white:
                res = di + dj
        else:
            res = ei + ej
        rho = 2 * d * res - d * d if res > d else res * res
        tot += _rint_half_even(rho * 2 ** 39)
    return tot
