"""Constructed labelled frames for the VALUES K6 computes (tests/test_grid_cost_values.py).

EXACT frames.  Board squares of 0.25 m, huber_delta 0.125, translations in steps of 2^-6 m = 1/16 square, points on multiples of
1/16 square, theta = 0 (cos / g = 4, sin / g = 0): every board coordinate under every candidate is a multiple of 1/16, every residual
R a multiple of 1/16, every term T = Q (R - Q / 2) a multiple of 2^-9 and T w one of 2^-10.  As long as a candidate's sum stays below
2^24 units of 2^-12 (asserted with integers by the CPU tests), every partial sum in ANY order is a float32 and the kernel's value is
the exact sum whichever of its forms computed it.  The theta table is {0} (n_th = 1), or the 21 thetas of
constructed_points.dyadic_params() / the 9 of PRODUCTION, of which only the slice at theta = 0 is exact.

Boards: 6 x 8, and the 7 x 5 board as the library takes it (board_w <= board_h: 5 wide, 7 high; W / 2 and H / 2 are then half
squares).  Translation tables 32 x 32, 30 x 29 (last tiles 2 and 1 candidates wide), 3 x 3 and 1 x 1, centred on translation 0.

GENERAL frames: test_gpu_parity's _rand_points on its 7 x 9 x 10 grid (the default board), theta != 0, nothing exact.

Plain module (no fixtures); every frame is deterministic from its name.  Nothing here is tuned against the kernels.
"""
import functools
from collections import namedtuple

import numpy as np

import constructed_bounds as cb
import constructed_points as cp

STEP = 2.0 ** -6                # translation step (m) = 1/16 square
G, DELTA = 0.25, 0.125
SUB = 16                        # lattice positions per square
REACH = 2                       # squares outside the outline the points reach
EXACT_UNIT_LOG2 = 12            # the unit the exactness condition counts in

Frame = namedtuple("Frame", "name fields yz lab exact_k kind")   # exact_k: the theta slice that is exact


def fields(W, H, n_ty, n_tz, thetas=1, th_step=STEP):
    """the parameter fields of an exact grid: tables centred on translation 0 (index n // 2), theta table {0} or 2 k + 1 thetas
    th_step (2^-6 rad) apart around 0"""
    half = (thetas - 1) // 2
    return dict(board_w=W, board_h=H, grid_length=G, huber_delta=DELTA, n_th=thetas, th_step=th_step, th_min=-half * th_step,
                n_ty=n_ty, ty_step=STEP, ty_min=-(n_ty // 2) * STEP, n_tz=n_tz, tz_step=STEP, tz_min=-(n_tz // 2) * STEP)


# what the pipeline's launches need: a seed grid (every axis >= 8), a theta group of 7.  Thetas 2^-4 rad apart: a step moves the points of
# the outer cells by 3/16 square, across cell borders -- the minimum then lies in the slice theta = 0 by a margin, not by noise
PRODUCTION = fields(6, 8, 14, 13, thetas=9, th_step=2.0 ** -4)


def _params(f):
    from types import SimpleNamespace
    return SimpleNamespace(**f)


# ---------------------------------------------------------------------------------------------------------------- points
def _special(W, H):
    """board coordinates (sixteenths of a square) at translation 0 that sit ON the term's branches: i or j an exact integer, both
    outlines of both axes, exact half cells, R == delta in the board (1/16 + 1/16 and 1/8 + 0 from the cell borders) and outside it,
    and points left of and below the board whose floors add up to a negative odd number"""
    s = SUB
    return [(0, 3 * s + 5), (W * s, 2 * s + 7), (2 * s + 3, 0), (s + 9, H * s),             # the four outlines
            (0, 0), (W * s, H * s), (0, H * s),                                              # corners of the outline
            (2 * s, 3 * s + 4), (3 * s + 11, 5 * s), (4 * s, 4 * s),                         # i / j / both exact integers inside
            (s + 8, 2 * s + 8), (3 * s + 8, 6 * s + 3), (2 * s + 5, 4 * s + 8),              # exact half cells
            (s + 1, 2 * s + 1), (2 * s + 15, 3 * s + 1), (4 * s + 2, 5 * s), (s + 14, s + 16),   # in the board, R == delta
            (-1, 1), (W * s + 1, H * s - 1), (2, -0), (-2, 3 * s),                           # out of the board, R == delta
            (-s - 3, -5), (-7, -2 * s + 4), (-s - 8, 2 * s + 8), (3 * s + 2, -s - 9),        # negative floors, odd sums among them
            (-2 * s, -2 * s), ((W + 2) * s, (H + 2) * s)]                                    # the far corners


def _draw(rng, W, H, n):
    return rng.integers(-REACH * SUB, (W + REACH) * SUB + 1, n), rng.integers(-REACH * SUB, (H + REACH) * SUB + 1, n)


def lattice_points(f, m, seed, kind="mixed", colour=None, shift=(0, 0)):
    """m labelled points on the lattice for the fields f.  kind: "mixed" -- the special points first, then uniform over the board and
    REACH squares around it; "no_interior" / "only_interior" -- drawn until K5w's class rule (constructed_bounds.walk_classes) gives
    none / only interior-class points; "outside" -- more than a square outside the outline, out of the board under every
    translation; "board" -- a noisy board (constructed_points.noisy_board on the lattice: random cells, in-cell positions on the
    lattice, 10 % of the labels flipped, 10 % moved outside), translated by `shift` sixteenths: a unique minimum near that
    translation.  colour: None random labels, 0 / 1 one colour.  -> (yz float32 [m, 2], lab uint8 [m])"""
    p = _params(f)
    W, H = p.board_w, p.board_h
    rng = np.random.default_rng(seed)
    to_yz = lambda i16, j16: cp.from_board(p, np.asarray(i16, np.float64) / SUB, np.asarray(j16, np.float64) / SUB)
    lab = None
    if kind == "mixed":
        sp = _special(W, H)[:m]
        ri, rj = _draw(rng, W, H, m - len(sp))
        i16 = np.concatenate([np.array([v[0] for v in sp], np.int64), ri])
        j16 = np.concatenate([np.array([v[1] for v in sp], np.int64), rj])
        order = rng.permutation(m)      # (the special points anywhere in the frame's order)
        i16, j16 = i16[order], j16[order]
    elif kind == "board":
        ci, cj = rng.integers(0, W, m), rng.integers(0, H, m)
        i16, j16 = ci * SUB + rng.integers(0, SUB, m), cj * SUB + rng.integers(0, SUB, m)
        lab = (ci + cj) & 1
        lab = np.where(rng.random(m) < 0.1, 1 - lab, lab)
        out, side, far = rng.random(m) < 0.1, rng.integers(0, 4, m), rng.integers(0, 3 * SUB // 2 + 1, m)
        i16 = np.where(out & (side == 0), -far, np.where(out & (side == 1), W * SUB + far, i16))
        j16 = np.where(out & (side == 2), -far, np.where(out & (side == 3), H * SUB + far, j16))
        i16, j16 = i16 - shift[0], j16 - shift[1]
    else:
        i16, j16 = np.zeros(0, np.int64), np.zeros(0, np.int64)
        while len(i16) < m:
            ci, cj = _draw(rng, W, H, 4 * m + 64)
            if kind == "outside":
                keep = (ci < -SUB) | (ci > (W + 1) * SUB) | (cj < -SUB) | (cj > (H + 1) * SUB)
            else:
                keep = (cb.walk_classes(p, to_yz(ci, cj))[0] == 0) == (kind == "only_interior")
            i16, j16 = np.concatenate([i16, ci[keep]]), np.concatenate([j16, cj[keep]])
        i16, j16 = i16[:m], j16[:m]
    if lab is None:
        lab = rng.integers(0, 2, m)
    if colour is not None:
        lab = np.full(m, colour)
    yz = to_yz(i16, j16)
    assert np.array_equal(yz.astype(np.float64) * (SUB / G) % 0.5, np.zeros_like(yz, np.float64))   # on the lattice, exactly
    return np.ascontiguousarray(yz, np.float32), np.ascontiguousarray(lab, np.uint8)


# ---------------------------------------------------------------------------------------------------------------- exact frames
B68, B75 = (6, 8), (5, 7)
# name: (M, board, table, thetas, kind, colour)
EXACT = {
    "m0": (0, B68, (32, 32), 1, "mixed", None),
    "m1_outline": (1, B75, (3, 3), 1, "mixed", None),
    "m63": (63, B68, (30, 29), 1, "mixed", None),
    "m64_no_interior": (64, B75, (32, 32), 1, "no_interior", None),
    "m65_one_candidate": (65, B68, (1, 1), 1, "mixed", None),
    "m255_only_interior": (255, B75, (30, 29), 1, "only_interior", None),
    "m256_outside": (256, B68, (32, 32), 1, "outside", None),
    "m257_thetas": (257, B68, (32, 32), 21, "mixed", None),
    "m1023_white": (1023, B75, (32, 32), 1, "mixed", 1),
    "m1024_black": (1024, B68, (30, 29), 1, "mixed", 0),
    "m1025_thetas": (1025, B68, (30, 29), 21, "mixed", None),
    "m2049": (2049, B75, (32, 32), 1, "mixed", None),
    "m2833_no_interior": (2833, B68, (32, 32), 1, "no_interior", None),
    "m8192": (8192, B68, (32, 32), 1, "mixed", None),
    "m8193": (8193, B75, (30, 29), 1, "mixed", None),
    "m600_3x3": (600, B68, (3, 3), 1, "mixed", None),
}
EXACT_M = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 2833, 8192, 8193)


@functools.lru_cache(maxsize=None)
def exact_frame(name):
    m, (W, H), (n_ty, n_tz), thetas, kind, colour = EXACT[name]
    f = fields(W, H, n_ty, n_tz, thetas)
    yz, lab = lattice_points(f, m, 1000 + m, kind, colour)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return Frame(name, f, yz, lab, (thetas - 1) // 2, kind)


# ---------------------------------------------------------------------------------------------------------------- production frames
# noisy boards under PRODUCTION, each at a translation of its own (sixteenths of a square): M, shift
PRODUCED = {"p65": (65, (2, -3)), "p257": (257, (-4, 1)), "p1025": (1025, (3, 4)), "p2833": (2833, (-1, -2)), "p8193": (8193, (5, 0))}


@functools.lru_cache(maxsize=None)
def produced_frame(name):
    m, shift = PRODUCED[name]
    yz, lab = lattice_points(PRODUCTION, m, 3000 + m, "board", shift=shift)   # (seeds 2000 + m: the 65 points' minimum is at another theta)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return Frame(name, PRODUCTION, yz, lab, (PRODUCTION["n_th"] - 1) // 2, "board")


def batch_of(n_frames, names):
    """n_frames frames taking `names` in turn -> [(yz, lab)], [name]"""
    picks = [names[f % len(names)] for f in range(n_frames)]
    return [(produced_frame(n).yz, produced_frame(n).lab) for n in picks], picks


# ---------------------------------------------------------------------------------------------------------------- general frames
GENERAL_GRID = dict(n_th=7, n_ty=9, n_tz=10, th_min=-0.12, th_step=0.04, ty_min=-0.12, ty_step=0.03, tz_min=-0.15, tz_step=0.03)
GENERAL_M = (1, 63, 64, 65, 257, 1000, 2500)


@functools.lru_cache(maxsize=None)
def general_frame(m):
    """test_gpu_parity's _rand_points, with its seed"""
    from test_gpu_parity import _rand_points
    yz, lab = _rand_points(np.random.default_rng(100 + m), m)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return Frame("g%d" % m, GENERAL_GRID, yz, lab, None, "random")
