"""The GRID back end -- K6's argmin, the near-tie recount, K7r's pattern search and basin check -- on CONSTRUCTED labelled points
(tests/constructed_points.py), where the rest of the suite feeds it the ~950 noisy points of synthetic frames: boards that cost
exactly 0 on a plateau of candidates, coordinates exactly on the term's branches, point counts at wavefront and staging edges,
chosen fills of the refinement's active-point queue, and sums at the edge of what a double adds exactly.

Every GPU assertion is `==` against the CPU oracle or against exact_cost_q (exact rationals, independent of the oracle).  The CPU
tests (no marker) check that the constructed inputs ARE what the GPU tests take them for: the plateau sizes, the distance of every
point from a cell border where ILCC_FLAG_BORDER_RISK must stay clear, which points a stencil may skip, the per-lane sums.
Nothing here is tuned against the kernels: seeds and poses were picked on those CPU conditions alone.
"""
import functools

import numpy as np
import pytest

import constructed_points as cp

K_TIE_CAP = 256          # ilcc_internal.h kTieCap
K_REFINE_LIST = 32       # kRefineList


# ------------------------------------------------------------------------------------------------------------------ parameters
def _oparams(ob, fields=None):
    p = ob.default_params()
    p.solver = ob.SOLVER_GRID
    return cp.apply_fields(p, fields or {})


def _nparams(fields=None):
    from lidar_camera_calibration_amd import _native as N
    p = N.default_params()
    p.solver = N.SOLVER_GRID
    return cp.apply_fields(p, fields or {})


def _small_grid(p):
    """test_gpu_parity's _SMALL_GRID on the default board: 21 thetas 1.5 degrees apart, 16 x 16 translations over [-g, g)"""
    n_th, th_step = 21, 1.5 * np.pi / 180
    return dict(n_th=n_th, th_step=th_step, th_min=-0.5 * (n_th - 1) * th_step, n_ty=16, n_tz=16,
                ty_step=2 * p.grid_length / 16, tz_step=2 * p.grid_length / 16, ty_min=-p.grid_length, tz_min=-p.grid_length)


def _cut_grid(p):
    """the default grid's steps on 9 x 12 x 12 candidates around zero: the same stencils as the default grid's, an exhaustive
    oracle search 80 x shorter"""
    return dict(n_th=9, th_min=-4 * p.th_step, n_ty=12, ty_min=-6 * p.ty_step, n_tz=12, tz_min=-6 * p.tz_step)


def _cell(p, flat):
    c = flat >> 1
    return c // (p.n_ty * p.n_tz), (c // p.n_tz) % p.n_ty, c % p.n_tz


def _i8(lab):
    return lab.astype(np.int8)


def _o_refine(ob, op, yz, lab, lat, ph):
    q, ph, cq, aq, rounds, hops = ob.pattern_refine(yz[:, 0], yz[:, 1], _i8(lab), op, lat, ph)
    return tuple(int(v) for v in q), ph, cq, aq, rounds, hops


def _g_refine(est, yz, lab, lat, ph):
    q, ph, cq, aq, rounds, hops = est.pattern_refine(yz, lab, lat, ph)
    return tuple(int(v) for v in q), ph, cq, aq, rounds, hops


def _assert_downstream(ob, op, yz, lab, got):
    """everything downstream of the solver's OWN grid argmin == the oracle's refinement from that start"""
    div = op.refine_div if op.refine_div > 0 else 1
    start = [div * v for v in _cell(op, got["grid_index"])]
    want = _o_refine(ob, op, yz, lab, start, got["grid_index"] & 1)
    assert (tuple(int(v) for v in got["lat"]), got["phase"], got["cost_q"], got["alt_cost_q"], got["rounds"], got["hops"]) == want, \
        (got, want)


# ------------------------------------------------------------------------------------------------------------------ the cases
# D: (J, seed, pose, class of the zero-cost plateau).  K = 8 points per cell, m = 384.
PLATEAUS = {
    "few_centre": (0.45, 8, (0.0, 0.0, 0.0), "one_sweep"),
    "few_posed": (0.45, 7, (0.056, 0.04, -0.06), "one_sweep"),
    "several_centre": (0.40, 7, (0.0, 0.0, 0.0), "several_sweeps"),
    "several_posed": (0.40, 7, (0.056, 0.04, -0.06), "several_sweeps"),
    "overflow_centre": (0.30, 7, (0.0, 0.0, 0.0), "overflow"),
    "overflow_posed": (0.30, 7, (0.02, 0.10, 0.09), "overflow"),
    "one_point": (None, 0, (0.0, 0.0, 0.0), "overflow"),
}
_CLASS = {"one_sweep": (2, K_REFINE_LIST), "several_sweeps": (K_REFINE_LIST + 1, 128), "overflow": (K_TIE_CAP + 1, 1 << 30)}


def _plateau_points(p, name):
    J, seed, pose, _ = PLATEAUS[name]
    if J is None:   # one point at the centre of cell (2, 3), its own colour
        return cp.from_board(p, [2.5], [3.5], pose), np.array([(2 + 3) & 1], np.uint8)
    return cp.ideal_board(p, J, 8, seed, pose)


@functools.lru_cache(maxsize=None)
def _plateau_ref(ob, name):
    """-> (yz, lab, oracle argmin flat index, its cost, candidates that cost exactly 0): computed once, shared, never modified"""
    op = _oparams(ob)
    yz, lab = _plateau_points(op, name)
    flat, cost, vol = ob.grid_search(yz[:, 0], yz[:, 1], _i8(lab), op, 1, want_volume=True)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return yz, lab, flat, cost, int((vol == 0).sum())


# B / C / E inputs
POSE_B = (0.021, 0.013, -0.022)
M_REFINE = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 767, 768, 769)
M_SOLVE_DEFAULT = (1, 65, 769)
M_SOLVE_SMALL = (8192, 8193)       # the last staged size (kGridLdsPointsMax) and the first global-memory size
POSE_C = (-0.017, 0.021, 0.012)
FAR_IN = dict(huber_delta=5.0, m=8000, lo=0.3, hi=0.9, seed=3)       # inside the documented domain of the double sums
FAR_OUT = dict(huber_delta=5.0, m=28800, lo=1.0, hi=2.0, seed=1)     # outside it at the 64-point stride of the pattern rounds
FAR_OUT_192 = dict(huber_delta=50.0, m=28800, lo=1.0, hi=2.0, seed=1)   # ... and at the 192-point stride of the basin check
FAR_ROUNDS = 6   # refine_max_rounds of E's tests: the search walks towards the points for 150 rounds otherwise, every one alike


def _terms(ob, op, yz, lab, lat, ph):
    x = ob.lattice_point(op, lat)
    return [ob.cost_q(x, yz[k:k + 1, 0], yz[k:k + 1, 1], _i8(lab[k:k + 1]), op, ph, 1) for k in range(len(lab))]


# A: starts on the line ty = tz = 0 of the symmetric dyadic set, where the first round's cheapest neighbours are a tied pair
TIE_STARTS = [([96, 256, 256], 0), ([112, 256, 256], 1), ([144, 256, 256], 1), ([212, 256, 256], 0)]


# ================================================================================================================== CPU tests
_LATTICE_DIV16 = [(la, lb, ph) for la in (0, 1, 255, 256, 257, 300, 511) for lb in (0, 256, 259, 511) for ph in (0, 1)]


def test_exact_rational_cost_matches_the_oracle_on_the_dyadic_board(ob):
    """exact_cost_q (fractions.Fraction, Python integers) == orc_cost_q on dyadic_points(11): at the 56 lattice points of the
    refine_div = 16 lattice (theta row 160 = 0.0 exactly) and on the grid-step lattice of refine_div = 0 (row 10).  Two
    independent statements of the term agree where every branch tie of it occurs: i or j an exact integer (the outlines
    included), exact half cells, res == delta."""
    yz, lab = cp.dyadic_points(11)
    for div, row, pts in ((16, 160, _LATTICE_DIV16), (0, 10, [(la, lb, ph) for la in (0, 1, 16, 31) for lb in (0, 15, 16) for ph in (0, 1)])):
        op = _oparams(ob, dict(cp.dyadic_params(), refine_div=div))
        for la, lb, ph in pts:
            x = ob.lattice_point(op, [row, la, lb])
            assert x[0] == 0.0
            assert ob.cost_q(x, yz[:, 0], yz[:, 1], _i8(lab), op, ph, 1) == cp.exact_cost_q(op, yz, lab, x[1], x[2], ph), (div, la, lb, ph)
    # the set holds what it claims at t = 0
    op = _oparams(ob, cp.dyadic_params())
    i, j = cp.board_coords(op, yz, (0.0, 0.0, 0.0))
    assert (i[:100] == np.rint(i[:100])).all() and 0.0 in i[:100] and float(op.board_w) in i[:100]
    assert (j[100:200] == np.rint(j[100:200])).all() and 0.0 in j[100:200] and float(op.board_h) in j[100:200]
    assert (i[200:250] - np.floor(i[200:250]) == 0.5).all()
    assert (i[250:300] - np.floor(i[250:300]) == 0.0625).all() and (j[250:300] - np.floor(j[250:300]) == 0.0625).all()
    assert op.huber_delta == 0.0625 + 0.0625


def test_symmetric_dyadic_set_ties_the_cheapest_neighbours(ob):
    """From every start of TIE_STARTS the first round's minimum over the 26 neighbours is attained twice, at the same distance, and
    lies below the centre: the move is decided by "first in (dk, da, db) order".  From at least one start the oracle ends off the
    symmetric line, so that the other choice would end at the mirrored point."""
    op = _oparams(ob, dict(cp.dyadic_params(), refine_div=16))
    yz, lab = cp.dyadic_points_symmetric(11)

    def cost(lat, ph):
        return ob.cost_q(ob.lattice_point(op, lat), yz[:, 0], yz[:, 1], _i8(lab), op, ph, 1)

    offs = [(dk, da, db) for dk in (-1, 0, 1) for da in (-1, 0, 1) for db in (-1, 0, 1) if (dk, da, db) != (0, 0, 0)]
    ends_off_line = 0
    for lat, ph in TIE_STARTS:
        v = [cost([lat[0] + 16 * dk, lat[1] + 16 * da, lat[2] + 16 * db], ph) for dk, da, db in offs]
        best = [o for o, c in zip(offs, v) if c == min(v)]
        assert len(best) == 2 and min(v) < cost(lat, ph), (lat, ph, best)
        assert best[0][0] == best[1][0] and best[0][1:] == tuple(-d for d in best[1][1:])
        q = _o_refine(ob, op, yz, lab, lat, ph)[0]
        ends_off_line += q[1:] != (256, 256)
    assert ends_off_line >= 1


@pytest.mark.parametrize("name", list(PLATEAUS))
def test_plateau_classes(ob, name):
    """The zero-cost candidates of every plateau case, counted on the oracle's whole cost volume, fall in the class the GPU test
    uses the case for: 2-32 (one recount sweep, a count that does not divide 64), 33-128 (full sweeps of 32 and a remainder),
    more than 256 (the near-tie list overflows).  The oracle's argmin costs 0 and its refinement stays there."""
    op = _oparams(ob)
    yz, lab, flat, cost, zeros = _plateau_ref(ob, name)
    lo, hi = _CLASS[PLATEAUS[name][3]]
    print("plateau %s: m %d, zero-cost candidates %d, oracle argmin %s" % (name, len(lab), zeros, _cell(op, flat) + (flat & 1,)))
    assert lo <= zeros <= hi, (name, zeros)
    if PLATEAUS[name][3] == "one_sweep":
        assert 64 % zeros != 0
    if PLATEAUS[name][3] == "several_sweeps":
        assert zeros % K_REFINE_LIST != 0 and 64 % (zeros % K_REFINE_LIST) != 0
    assert cost == 0.0 and (flat & 1) == 0
    start = [16 * v for v in _cell(op, flat)]
    q, ph, cq, aq, rounds, hops = _o_refine(ob, op, yz, lab, start, 0)
    assert (q, ph, cq, rounds, hops) == (tuple(start), 0, 0, 5, 0)
    assert (aq > 0) == (len(lab) > 1)   # (one point alone: a square further it sits in a cell of the flipped colour)


@pytest.mark.parametrize("name", list(PLATEAUS))
def test_plateau_points_keep_their_distance_from_cell_borders(ob, name):
    """Where the GPU test wants ILCC_FLAG_BORDER_RISK clear: every point's fp64 board coordinate under the 3 thetas x (3 + 3)
    translations of the oracle argmin's grid neighbourhood lies at least 1e-4 square from an integer -- 25 x the flag's window
    (kBorderRisk = 4e-6), where fp32 and fp64 coordinates differ by about 1e-6."""
    op = _oparams(ob)
    yz, lab, flat, _, _ = _plateau_ref(ob, name)
    k, a, b = _cell(op, flat)
    assert 0 < k < op.n_th - 1 and 0 < a < op.n_ty - 1 and 0 < b < op.n_tz - 1
    worst = 1.0
    for dk in (-1, 0, 1):
        for d in (-1, 0, 1):
            i, j = cp.board_coords(op, yz, (op.th_min + (k + dk) * op.th_step, op.ty_min + (a + d) * op.ty_step, op.tz_min + (b + d) * op.tz_step))
            worst = min(worst, np.abs(i - np.rint(i)).min(), np.abs(j - np.rint(j)).min())
    print("plateau %s: nearest cell border %.2e square" % (name, worst))
    assert worst >= 1e-4, (name, worst)


def test_chunk_pattern_is_what_it_claims(ob):
    """With stencil_sweep's own silence test in fp64: from both starts of the GPU test, for the first round's three thetas and
    its extreme translations (stride = refine_div), every designated silent point is silent and every active one is not; the
    counts per 64-point chunk are the requested ones."""
    op = _oparams(ob, _cut_grid(_oparams(ob)))
    counts = cp.chunk_counts(5)
    yz, lab, active = cp.chunk_pattern(op, counts, 5, POSE_C)
    assert len(counts) >= 40 and set(counts) == {0, 1, 63, 64} and len(lab) == 64 * len(counts) + 17
    assert any(counts[k:k + 3] == [63, 64, 64] for k in range(len(counts))) and any(counts[k:k + 4] == [64, 0, 0, 1] for k in range(len(counts)))
    assert [int(active[64 * c:64 * c + 64].sum()) for c in range(len(counts))] == counts
    near = cp.nearest_lattice(op, POSE_C)
    for lat in (near, [near[0] + 8, near[1] - 8, near[2] + 8]):
        for dk in (-1, 0, 1):
            silent = cp.silent_mask(op, yz, lab, [lat[0] + dk * op.refine_div, lat[1], lat[2]], 0, op.refine_div)
            assert np.array_equal(silent, ~active), (lat, dk)
    # an active point's term is positive under every candidate of that stencil: 0.2 square from the borders less the stencil's reach
    i, j = cp.board_coords(op, yz, POSE_C)
    fi, fj = i - np.floor(i), j - np.floor(j)
    assert (np.minimum(fi, 1 - fi)[active] > 0.19).all() and (np.minimum(fj, 1 - fj)[active] > 0.19).all()


def test_far_points_lie_on_either_side_of_the_double_sums_domain(ob):
    """stencil_sweep's doubles are exact while a lane's sum of rint(1/2 rho 2^40) stays below 2^53: P x rho(r_max) < 2^14 for
    P points per lane.  FAR_IN lies inside at every stride by that bound, one more square of distance per axis for the basin
    check included; FAR_OUT drives a lane of the 64-stride partition past 2^53 and FAR_OUT_192 one of the 192-stride partition
    (all their points are off the board: every one is evaluated, in input order)."""
    for case, stride in ((FAR_IN, 0), (FAR_OUT, 64), (FAR_OUT_192, 192)):
        op = _oparams(ob, dict(huber_delta=case["huber_delta"]))
        yz, lab = cp.far_points(case["m"], case["lo"], case["hi"], case["seed"])
        t = _terms(ob, op, yz, lab, [480, 320, 320], 0)
        lane_max = {n: max(sum(t[l::n]) for l in range(n)) for n in (64, 192, 256, 768)}
        i, j = cp.board_coords(op, yz, (0.0, 0.0, 0.0))
        r_max = float((np.maximum(i - op.board_w, 0) + np.maximum(j - op.board_h, 0)).max()) + 2.0
        d = op.huber_delta
        rho = 2 * d * r_max - d * d if r_max > d else r_max * r_max
        P = -(-case["m"] // 64)
        print("far points m %d delta %g: largest term %.3e, largest lane sum %s (2^53 = %.3e), P x rho(r_max) = %d x %.1f" %
              (case["m"], d, float(max(t)), {n: "%.3e" % float(v) for n, v in lane_max.items()}, 2.0 ** 53, P, rho))
        # what a kernel that adds each lane's terms in a double and the lanes as integers would report
        as_doubles = {n: sum(int(functools.reduce(lambda a, v: a + float(v), t[l::n], 0.0)) for l in range(n)) - sum(t) for n in lane_max}
        print("   double sums - integer sum:", as_doubles)
        if stride == 0:
            assert P * rho < 2 ** 14 and max(lane_max.values()) < 2 ** 53 and not any(as_doubles.values())
        else:
            assert P * rho >= 2 ** 14 and lane_max[stride] >= 2 ** 53 and as_doubles[stride] != 0


# ================================================================================================================== GPU tests
@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, 28800, _nparams())
    yield e
    e.close()


def _flags():
    from lidar_camera_calibration_amd import _native as N
    return N.FLAG_TIE_OVERFLOW, N.FLAG_BORDER_RISK


# ---- A: exact branch ties
@pytest.mark.gpu
def test_branch_ties_cost_and_basin_check_equal_the_exact_rational_cost(ob, est):
    """dyadic board, refine_div = 0 (the start is kept, the basin check still runs): at 20 starts on the theta = 0 row the
    kernel's cost_q is exact_cost_q at the start and alt_cost_q the minimum of exact_cost_q over the eight hop neighbours (16
    grid steps along y and / or z, the phase flipped on odd shifts) -- with points exactly on i, j integer (outlines included),
    on half cells and on res == delta."""
    fields = dict(cp.dyadic_params(), refine_div=0)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab = cp.dyadic_points(11)

    @functools.lru_cache(maxsize=None)
    def exact(la, lb, ph):
        return cp.exact_cost_q(op, yz, lab, op.ty_min + la * op.ty_step, op.tz_min + lb * op.tz_step, ph)

    hop = 16
    assert round(op.grid_length / op.ty_step) == hop and round(op.grid_length / op.tz_step) == hop
    n = 0
    for la in (0, 1, 16, 17):
        for lb in (0, 3, 16, 19, 31):
            ph = n & 1
            n += 1
            q, gph, cq, aq, rounds, hops = _g_refine(est, yz, lab, [10, la, lb], ph)
            alt = min(exact(la + da * hop, lb + db * hop, ph ^ ((da + db) & 1)) for da in (-1, 0, 1) for db in (-1, 0, 1) if (da, db) != (0, 0))
            assert (q, gph, rounds, hops) == ((10, la, lb), ph, 0, 0)
            assert (cq, aq) == (exact(la, lb, ph), alt), (la, lb, ph)
    assert n == 20


@pytest.mark.gpu
def test_branch_ties_pattern_search_equals_the_oracle(ob, est):
    """dyadic board, refine_div = 16, from starts on the theta = 0 row (160) and off it: the whole tuple == orc_pattern_refine.
    The silence test meets its own branches exactly (i0 == 0, i2 == W, i2 an integer: floor(i0) != floor(i2) with i2 on the
    border itself).  Then the symmetric set, whose stencils on the line ty = tz = 0 hold exactly tied pairs of neighbours: the
    tie-break "nearer, then first" decides the first move from every start of TIE_STARTS."""
    fields = dict(cp.dyadic_params(), refine_div=16)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab = cp.dyadic_points(11)
    starts = [([160, la, lb], ph) for la, lb, ph in _LATTICE_DIV16[::5]] + \
             [([160, 256, 256], 0), ([160, 256, 256], 1), ([144, 256, 256], 0), ([171, 250, 263], 1), ([0, 16, 500], 0), ([320, 511, 0], 1), ([163, 255, 257], 0)]
    for lat, ph in starts:
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)
    yz, lab = cp.dyadic_points_symmetric(11)   # exact cost ties: the cheapest of the 26 neighbours is a tied pair
    for lat, ph in TIE_STARTS:
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)


# ---- B: point counts
@pytest.mark.gpu
def test_point_counts_at_wavefront_edges_pattern_refine(ob, est):
    """K7r's own entry (192 threads: 64-point slices per theta, 192-point slices in the basin check) at every m around 64, 128,
    192, 256 and 768, from a start within 3 lattice units of the pose and from one a square off with the colours swapped."""
    est.set_params(_nparams())
    op = _oparams(ob)
    near = cp.nearest_lattice(op, POSE_B)
    hop_y = round(op.grid_length / (op.ty_step / op.refine_div))
    for m in M_REFINE:
        yz, lab = cp.noisy_board(op, m, 100 + m, POSE_B)
        for lat, ph in (([near[0] + 2, near[1] - 3, near[2] + 1], 0), ([near[0], near[1] + hop_y, near[2]], 1)):
            assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (m, lat, ph)


def _solve_case(ob, est, op, yz, lab):
    """-> (the solver's record, True when its grid argmin is the oracle's)"""
    got = est.grid_solve(yz, lab)
    _assert_downstream(ob, op, yz, lab, got)
    flat, _, _ = ob.grid_search(yz[:, 0], yz[:, 1], _i8(lab), op, 1)
    _, border_risk = _flags()
    assert got["grid_index"] == flat or (got["flags"] & border_risk), (got, flat)
    return got, got["grid_index"] == flat


_excused = []   # B's grid_solve cases whose argmin relied on ILCC_FLAG_BORDER_RISK


@pytest.mark.gpu
@pytest.mark.parametrize("m", M_SOLVE_DEFAULT + M_SOLVE_SMALL)
def test_point_counts_grid_solve(ob, m):
    """The pipeline's solver (768-thread K7r: 256-point slices per theta, 768 in the basin check) at m = 1, 65, 769 on the default
    grid and at 8192 / 8193 on a small grid -- the last size K7r stages in LDS and the first it reads from global memory.
    Everything downstream of the solver's own grid argmin == the oracle; the argmin == the oracle's, or ILCC_FLAG_BORDER_RISK is
    set, which at most one of the five cases may rely on."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    fields = _small_grid(_oparams(ob)) if m in M_SOLVE_SMALL else {}
    op = _oparams(ob, fields)
    yz, lab = cp.noisy_board(op, m, 200 + m, POSE_B)
    e = LidarCornersBatch(1, 8448, _nparams(fields))
    try:
        got, same = _solve_case(ob, e, op, yz, lab)
    finally:
        e.close()
    print("grid_solve m %d: flags %d ties %d argmin == oracle: %s" % (m, got["flags"], got["ties"], same))
    if not same:
        _excused.append(m)
    assert len(_excused) <= 1, _excused


# ---- C: queue fills
@pytest.mark.gpu
def test_queue_fills_pattern_refine_and_grid_solve(ob, est):
    """chunk_pattern: 0, 1, 63 or 64 active points per 64-point chunk, 63 + 64 + 64 in a row (127 in flight, the ring wraps) and
    64, 0, 0, 1; through K7r's entry (one wavefront per theta takes every chunk) from the pose's nearest lattice point and from 8
    lattice units away, and through the solver (four wavefronts per theta take every fourth chunk).  The grid is the default one
    cut to 9 x 12 x 12 candidates (the same steps, so the same stencils: the oracle's exhaustive search stays short)."""
    fields = _cut_grid(_oparams(ob))
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab, _ = cp.chunk_pattern(op, cp.chunk_counts(5), 5, POSE_C)
    near = cp.nearest_lattice(op, POSE_C)
    for lat in (near, [near[0] + 8, near[1] - 8, near[2] + 8]):
        assert _g_refine(est, yz, lab, lat, 0) == _o_refine(ob, op, yz, lab, lat, 0), lat
    got, same = _solve_case(ob, est, op, yz, lab)
    print("queue fills grid_solve: flags %d ties %d argmin == oracle: %s" % (got["flags"], got["ties"], same))


# ---- D: zero-cost plateaus
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLATEAUS))
def test_zero_cost_plateaus(ob, est, name):
    """A noise-free board: the frame's bound, every pruning limit of K6, the near-tie threshold and the recount's window are all
    exactly 0, and the near ties are the candidates that cost exactly 0 -- a few (one recount sweep), several dozen (sweeps of 32
    and a remainder), or more than the list holds (overflow: K6's own (cost, d2, flat) order on exactly-zero fp32 costs is the
    oracle's rule).  One point alone: most of the grid ties at 0."""
    est.set_params(_nparams())
    op = _oparams(ob)
    tie_overflow, border_risk = _flags()
    yz, lab, flat, _, zeros = _plateau_ref(ob, name)
    got = est.grid_solve(yz, lab)
    print("plateau %s: zero-cost candidates %d, listed ties %d, flags %d" % (name, zeros, got["ties"], got["flags"]))
    assert got["grid_index"] == flat and got["grid_cost"] == 0.0
    assert tuple(int(v) for v in got["lat"]) == tuple(16 * v for v in _cell(op, flat))
    _assert_downstream(ob, op, yz, lab, got)
    assert got["phase"] == 0 and got["cost_q"] == 0 and got["rounds"] == 5 and got["hops"] == 0
    assert (got["flags"] & border_risk) == 0
    assert bool(got["flags"] & tie_overflow) == (PLATEAUS[name][3] == "overflow")
    assert got["ties"] >= zeros - 1


# ---- E: the summation's domain
@pytest.mark.gpu
@pytest.mark.parametrize("case,div", [(FAR_IN, 16), (FAR_OUT, 16), (FAR_OUT_192, 16), (FAR_OUT_192, 0)],
                         ids=["inside", "outside", "outside_192", "outside_192_div0"])
def test_large_terms_are_summed_exactly(ob, est, case, div):
    """A large huber_delta and points far off the board: the largest terms.  Inside the documented domain of stencil_sweep's
    double sums (delta 5, 8 000 points 0.3-0.9 m off) and outside it (28 800 points 1-2 m off; delta 5: a lane's sum passes 2^53
    in the pattern rounds, delta 50: in the basin check too, whose sums are the reported costs; the wavefront then repeats its
    walk with int64 sums): cost_q and every decision == the oracle's int64 arithmetic, through K7r's
    entry (64- and 192-point strides) and through the solver (256 and 768; above 8192 points from global memory).  The searches
    are cut at FAR_ROUNDS rounds (and two hops): the first rounds are where the points are furthest.  refine_div = 0 keeps the
    start: the basin check there adds exactly the sums that the CPU test above shows a double cannot hold."""
    fields = dict(huber_delta=case["huber_delta"], refine_max_rounds=FAR_ROUNDS, refine_div=div)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab = cp.far_points(case["m"], case["lo"], case["hi"], case["seed"])
    for lat, ph in (([480, 320, 320], 0), ([500, 600, 610], 1)) if div else (([30, 20, 20], 0), ([35, 30, 28], 1)):
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)
    _assert_downstream(ob, op, yz, lab, est.grid_solve(yz, lab))
