"""Constructed inputs for the reference-trajectory solver (K7a) and K7b's phase choice: frames whose exact cost is known as a
rational number and in which every point counts, and solve cases whose trajectory through the trust-region minimiser is known --
which dogleg branches run, how the solve ends -- and stable under tiny changes of the start.

Plain module beside constructed_points.py (no fixtures).  Every generator returns (float32 yz[m, 2], uint8 label[m]) and is
deterministic from its arguments.  `p` is any parameter struct with board_w, board_h, grid_length and huber_delta (the library's
or the oracle's).
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import constructed_points as cp

# every labelled-point count at which K7a's loops change shape: one lane, a wavefront (64), the four residue classes of a lane
# (256), the strides beyond, the handle's first staging capacity (1024) and the first frame past it
M_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
M_MAX, FRAMES_MAX = 1025, 261


# ---------------------------------------------------------------------------------------------------------------- exact cost
def exact_cost(p, yz, label, ty, tz, phase, use_oob):
    """1/2 sum rho(r^2) of the double functor at theta = 0, as a Fraction with no rounding step anywhere: the residual of
    VirtualboardError (strictly inside the board: the in-cell distance of a wrong-colour point, else 0; outside: the distance to
    the nearer outline per axis when use_oob, else 0) and Huber's rho(s) = s (s <= delta^2) else 2 delta sqrt(s) - delta^2 with
    sqrt(r^2) = r.  The doubles of orc_cost / K7a equal it wherever every intermediate value is representable: the dyadic board
    with points on multiples of 2^-10 m and dyadic translations -- whatever the order of summation."""
    W, H = p.board_w, p.board_h
    g, d = Fraction(p.grid_length), Fraction(p.huber_delta)
    ty, tz = Fraction(ty), Fraction(tz)
    tot = Fraction(0)
    for (y, z), lab in zip(yz, label):
        in_i, odd_i, di, ei = cp._axis(float(y), ty, W, g)
        in_j, odd_j, dj, ej = cp._axis(float(z), tz, H, g)
        res = Fraction(0)
        if in_i and in_j:
            white = bool(phase) if odd_i == odd_j else not phase
            if bool(lab) != white:
                res = di + dj
        elif use_oob:
            res = ei + ej
        tot += (2 * d * res - d * d if res * res > d * d else res * res) / 2
    return tot


def as_exact_double(q):
    """the double that equals the Fraction q; asserts that there is one"""
    v = float(q)
    assert Fraction(v) == q, q
    return v


# ---------------------------------------------------------------------------------------------------------------- active frames
def active_frame(m, seed, phase=0):
    """m points of the dyadic board (constructed_points.dyadic_params), each in a random cell at an in-cell position on multiples
    of 1/256 square within [1/8, 7/8] on both axes, labelled with the WRONG colour for its cell under `phase`: at theta = t = 0
    every term of that phase's cost is positive (at least rho(1/4 square)), exactly representable, and under the other phase
    every term is 0.  A point dropped from, or added twice to, a sum changes it."""
    W, H, g = cp.DYADIC["board_w"], cp.DYADIC["board_h"], cp.DYADIC["grid_length"]
    rng = np.random.default_rng([seed, m, phase])
    ci, cj = rng.integers(0, W, m), rng.integers(0, H, m)
    ki, kj = rng.integers(32, 225, m), rng.integers(32, 225, m)
    y = (ci + ki / 256.0) * g - W * g / 2
    z = (cj + kj / 256.0) * g - H * g / 2
    right = ((ci + cj) & 1) ^ (1 if phase else 0)     # phase 0: an odd cell is white (label 1)
    return np.stack([y, z], axis=1).astype(np.float32), (1 - right).astype(np.uint8)


def outline_frame(seed, m=96):
    """Dyadic-board points whose in/out decision and cell are exact at theta = t = 0 and sit ON the branches: the outlines i = 0,
    i = W, j = 0, j = H (outside: the test is strict), interior cell borders (the cell is floor's), the four corners, and points
    just inside / outside by one 2^-10 m step; random labels."""
    W, H, g = cp.DYADIC["board_w"], cp.DYADIC["board_h"], cp.DYADIC["grid_length"]
    rng = np.random.default_rng([seed, 7])
    y = rng.integers(-800, 801, m) / 1024.0
    z = rng.integers(-1100, 1101, m) / 1024.0
    q = m // 8
    y[0 * q:1 * q] = -W * g / 2                                          # i == 0
    y[1 * q:2 * q] = W * g / 2                                           # i == W
    z[2 * q:3 * q] = -H * g / 2                                          # j == 0
    z[3 * q:4 * q] = H * g / 2                                           # j == H
    y[4 * q:5 * q] = (rng.integers(1, W, q) - W / 2) * g                 # interior borders of i
    z[5 * q:6 * q] = (rng.integers(1, H, q) - H / 2) * g                 # ... of j
    y[6 * q:6 * q + 4], z[6 * q:6 * q + 4] = np.array([-1, 1, -1, 1]) * W * g / 2, np.array([-1, -1, 1, 1]) * H * g / 2
    y[6 * q + 4:7 * q] = np.where(rng.random(q - 4) < 0.5, -1, 1) * (W * g / 2 - rng.integers(-1, 2, q - 4) / 1024.0)
    return np.stack([y, z], axis=1).astype(np.float32), rng.integers(0, 2, m).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- solve cases
# What a case must run, by the oracle's trace (oracle/binding.py TRACE_NAMES).  NOISY: what every noisy-board solve runs.
NOISY = ("gauss_newton_inside", "subspace_boundary", "boundary_reused", "rejected", "accepted_grow")
POSE = (0.03, 0.02, -0.03)
START = (1e-3, 2e-3, -1e-3)

# name; fields: parameter overrides on the defaults; points: (generator, arguments); start: where the four single-pass solves
# (both phases x OOB on / off, ilcc_get_theta_t's shape) begin -- the two-pass solves of the batch entry always begin at 0;
# expects: the branches those six solves must reach between them
Case = namedtuple("Case", "name fields points start expects")
AT_0 = ("end_gradient_tolerance_at_0",)


def _noisy(m, seed):
    return Case("noisy_m%d_s%d" % (m, seed), {}, ("noisy_board", m, seed, POSE), START, NOISY)


_COLUMN = ("column_of_cells", 40, 5)
_ROW = ("row_of_cells", 40, 6)

CASES = tuple(_noisy(m, seed) for m in (63, 64, 65, 255, 256, 257, 300, 769, 1025) for seed in (1, 2, 3)) + (
    # a correctly labelled noise-free board in its own phase costs exactly 0 (gradient tolerance before the first iteration); the
    # other phase of the same points is an ordinary solve
    Case("ideal_board", {}, ("ideal_board", 0.3, 2, 3), (0.0, 0.0, 0.0), AT_0 + NOISY),
    # two points: the phase they fit ends before the first iteration, the other one after a single step
    Case("noisy_m2_s2", {}, ("noisy_board", 2, 2, POSE), START, AT_0),
    Case("noisy_m2_s3", {}, ("noisy_board", 2, 3, POSE), START, AT_0),
    # rank-deficient sets: one column / one row of cells
    Case("one_column", {}, _COLUMN, START, NOISY),
    Case("one_row", {}, _ROW, START, NOISY),
    # a Huber delta so small that the corrected gradient is below the gradient tolerance at once / after some iterations
    Case("huber_1e-14", dict(huber_delta=1e-14), ("noisy_board", 65, 1, POSE), START, AT_0),
    Case("huber_1e-11", dict(huber_delta=1e-11), ("noisy_board", 65, 1, POSE), START, ("end_gradient_tolerance", "rejected")),
    Case("huber_5", dict(huber_delta=5.0), ("noisy_board", 65, 1, POSE), START, NOISY),
    # no iteration cap to speak of: every solve ends on a tolerance
    Case("iterations_100000", dict(max_iterations=100000), ("noisy_board", 65, 1, POSE), START, NOISY + ("end_function_tolerance",)),
    Case("iterations_1", dict(max_iterations=1), ("noisy_board", 257, 2, POSE), START, ("end_iteration_cap",)),
    # a far start in theta: |x| = 1e8, the first step is below 1e-8 |x| (parameter tolerance)
    Case("far_theta_start", {}, ("noisy_board", 65, 1, POSE), (1e8, 0.0, 0.0), ("end_parameter_tolerance",)),
    # one point 1e30 m off the board: the Gauss-Newton step lies outside the first radius and is parallel to the gradient (a
    # Jacobian of one row), so the step is taken along the gradient; the cost changes by less than 1e-6 of itself
    Case("one_far_point", {}, ("literal", ((1e30, 0.1),), (1,)), (0.0, 0.0, 0.0), ("one_dim_subspace", "end_function_tolerance")),
)
# over the whole list, beyond what each case states for itself
REACHED_SOMEWHERE = ("accepted_halve", "accepted_keep", "end_function_tolerance", "end_iteration_cap", "end_gradient_tolerance_at_0",
                     "end_gradient_tolerance", "end_parameter_tolerance", "one_dim_subspace")
# branches no finite input in the solver's domain reaches (tests/test_reference_solver_constructed.py says why)
NEVER_REACHED = ("mu_escalation", "linear_solver_failure", "traditional_fallback", "invalid_step", "end_invalid_steps", "end_min_radius")


def cells_line(p, m, seed, column):
    """m points with random labels in ONE column (i in cell 2) or ONE row (j in cell 4) of cells"""
    rng = np.random.default_rng([seed, int(column)])
    a, b = rng.uniform(0, p.board_h if column else p.board_w, m), (2.5 if column else 4.3) + rng.uniform(-0.4, 0.4, m)
    i, j = (b, a) if column else (a, b)
    return cp.from_board(p, i, j), rng.integers(0, 2, m).astype(np.uint8)


def case_points(p, case):
    kind, *args = case.points
    if kind == "noisy_board":
        return cp.noisy_board(p, *args)
    if kind == "ideal_board":
        return cp.ideal_board(p, *args)
    if kind in ("column_of_cells", "row_of_cells"):
        return cells_line(p, args[0], args[1], kind == "column_of_cells")
    if kind == "literal":
        yz, lab = args
        return np.asarray(yz, np.float32).reshape(-1, 2), np.asarray(lab, np.uint8)
    raise KeyError(kind)


# A case qualifies only if the ORACLE's own result is good to a tenth of the comparison tolerances: its solves are repeated with the
# points in other orders, which changes nothing but the rounding of the sums -- the least two correct implementations differ by.
# Small or degenerate frames can fail this however stable they are under moves of the start: the regularised normal equations
# (mu = 1e-8) return a rounding error multiplied by up to 1 / mu when the Jacobian loses rank along the way.  noisy_board(4, 1)
# moves its costs by 1e-7 relative; Huber delta 1e-12 on 65 points leaves the first gradient AT the gradient tolerance, and the
# order of the sum decides whether the solve starts at all.  Neither is a case.
PERMUTATIONS = 3
PERMUTED_COST_REL, PERMUTED_COST_ABS = 1e-10, 1e-13   # (and x within the 1e-9 of the stability condition)


def nudged_starts(start, eps=1e-11):
    """the six neighbours of a start: each coordinate moved by +-eps"""
    out = []
    for k in range(3):
        for sgn in (-1.0, 1.0):
            s = list(start)
            s[k] += sgn * eps
            out.append(tuple(s))
    return out
