"""K7r's sweep -- the fixed-point term on every branch of it, the silence-test trips at every point count around their
multiples, the active-point ring (128 entries per wavefront) at its fills, the move of a round picked by a lane-parallel
argmin -- against the CPU oracle's orc_pattern_refine: lattice point, phase, cost_q, alt_q, rounds and hops, all `==` (the
terms are the oracle's doubles and the sums are integers: no tolerance anywhere).

The constructed inputs come from tests/constructed_points.py; the CPU tests (no marker) check that the inputs built HERE are
what the GPU tests take them for.  Nothing is tuned against the kernels.
"""
import functools

import numpy as np
import pytest

import constructed_clusters as cc
import constructed_points as cp

POSE_B = (0.021, 0.013, -0.022)
POSE_C = (-0.017, 0.021, 0.012)
M_ENTRY = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385)   # 192 threads: 64 points per theta and trip, 192 per basin trip
M_SOLVER = (511, 512, 513, 1023, 1024, 1025)                                              # 768 threads: 256 points per theta and trip
# active points per 64-point chunk, as ONE wavefront meets them (chunk_pattern appends a tail of 17 points, 9 of them active,
# to every list).  The ring holds 128 entries; fewer than 64 stay behind a trip and a trip pushes one chunk, up to 64, so at
# most 127 are live: 63, 64, 64, ... leaves 63 behind its first trip and every later trip pushes 64 onto them -- the bound,
# held for two and for four trips; 62, 64, ... is one short of it; 63, 0, 64, 64 reaches the bound after a chunk that pushed
# nothing; 64, 0, 64, 1 drains exactly and then leaves one point (and the tail's nine) for the last evaluation.
RING_CASES = {
    "bound_twice": [63, 64, 64],
    "bound_four_times": [63, 64, 64, 64, 64],
    "one_short": [62, 64, 64, 64, 64],
    "bound_after_empty": [63, 0, 64, 64],
    "exact_drain": [64, 0, 64, 1],
    "all_active": [64] * 6,
    "none_active": [0] * 6,
}


def _oparams(ob, fields=None):
    p = ob.default_params()
    p.solver = ob.SOLVER_GRID
    return cp.apply_fields(p, fields or {})


def _nparams(fields=None):
    from lidar_camera_calibration_amd import _native as N
    p = N.default_params()
    p.solver = N.SOLVER_GRID
    return cp.apply_fields(p, fields or {})


def _cut_grid(p):
    """the default grid's steps on 9 x 12 x 12 candidates around zero: the same stencils, a short exhaustive search"""
    return dict(n_th=9, th_min=-4 * p.th_step, n_ty=12, ty_min=-6 * p.ty_step, n_tz=12, tz_min=-6 * p.tz_step)


def _i8(lab):
    return lab.astype(np.int8)


def _o_refine(ob, op, yz, lab, lat, ph):
    q, ph, cq, aq, rounds, hops = ob.pattern_refine(yz[:, 0], yz[:, 1], _i8(lab), op, lat, ph)
    return tuple(int(v) for v in q), ph, cq, aq, rounds, hops


def _g_refine(est, yz, lab, lat, ph):
    q, ph, cq, aq, rounds, hops = est.pattern_refine(yz, lab, lat, ph)
    return tuple(int(v) for v in q), ph, cq, aq, rounds, hops


def _assert_solver_downstream(ob, op, est, yz, lab):
    """everything downstream of the 768-thread solver's OWN grid argmin == the oracle's refinement from that start"""
    got = est.grid_solve(yz, lab)
    div = op.refine_div if op.refine_div > 0 else 1
    c = got["grid_index"] >> 1
    start = [div * (c // (op.n_ty * op.n_tz)), div * ((c // op.n_tz) % op.n_ty), div * (c % op.n_tz)]
    want = _o_refine(ob, op, yz, lab, start, got["grid_index"] & 1)
    assert (tuple(int(v) for v in got["lat"]), got["phase"], got["cost_q"], got["alt_cost_q"], got["rounds"], got["hops"]) == want, (got, want)


# ------------------------------------------------------------------------------------------------------------------ inputs
# the dyadic board (6 x 8 squares of 0.25 m, huber_delta = 1/8 square, lattice unit of refine_div = 16: 2^-10 m = 1/256 square;
# theta row 160 is 0.0 exactly): board coordinates of the extra points at t = 0, in squares.  Off the board along i by 1/16
# with j 1/16 inside the outline: res = 1/16 + 1/16 == huber_delta exactly; one lattice unit nearer / further: just below /
# just above it.  Every point once with each label.
_OFF = [(-1 / 16, 1 / 16), (-1 / 16 - 1 / 256, 1 / 16), (-1 / 16 + 1 / 256, 1 / 16),
        (6 + 1 / 16, 8 - 1 / 16), (6 + 1 / 16 + 1 / 256, 8 - 1 / 16), (6 + 1 / 16 - 1 / 256, 8 - 1 / 16),
        (1 / 16, -1 / 16), (3.5, 8 + 1 / 8), (3.5, 8 + 1 / 8 + 1 / 256), (3.5, 8 + 1 / 8 - 1 / 256),   # (i = 3.5: 2.5 squares from either outline -- far above delta)
        (0.0, 0.0), (6.0, 8.0), (0.0, 4.5), (3.0, 8.0), (2.5, 3.5), (2.0, 3.0)]
EDGE_STARTS = [([160, 256, 256], 0), ([160, 256, 256], 1), ([160, 257, 255], 0), ([160, 255, 257], 1), ([160, 240, 272], 0),
               ([160, 272, 240], 1), ([160, 260, 252], 0), ([160, 248, 264], 1)]


@functools.lru_cache(maxsize=None)
def _edge_points():
    """dyadic_points(11) + the outside points of _OFF with both labels -> (yz, lab), read-only"""
    p = cp.apply_fields(type("P", (), {})(), cp.dyadic_params())
    yz, lab = cp.dyadic_points(11)
    i = np.array([v[0] for v in _OFF] * 2)
    j = np.array([v[1] for v in _OFF] * 2)
    yz = np.concatenate([yz, cp.from_board(p, i, j)])
    lab = np.concatenate([lab, np.repeat(np.array([0, 1], np.uint8), len(_OFF))])
    yz.setflags(write=False)
    lab.setflags(write=False)
    return yz, lab


# Wrong-colour points a few lattice units inside a cell border along i, in the middle of the cell along j: a step of the
# first round's stride across that border puts each of them in a cell of its own colour, whatever the step along j -- the
# neighbours beyond the border cost 0 for every db (and, the rotation being small, for more than one dk): a cost tie between
# neighbours of DIFFERENT d2.
_CROSS_CELLS = [(2, 3), (4, 1), (1, 6), (3, 4), (5, 2), (2, 5)]
CROSS_START = ([160, 256, 256], 0)


@functools.lru_cache(maxsize=None)
def _crossing_points():
    p = cp.apply_fields(type("P", (), {})(), cp.dyadic_params())
    ci = np.array([c[0] for c in _CROSS_CELLS], np.float64)
    cj = np.array([c[1] for c in _CROSS_CELLS], np.float64)
    yz = cp.from_board(p, ci + 8 / 256, cj + 0.5)
    lab = (((ci + cj).astype(np.int64) & 1) ^ 1).astype(np.uint8)   # phase 0: the cell's colour is (ci + cj) & 1 -- these carry the other
    yz.setflags(write=False)
    lab.setflags(write=False)
    return yz, lab


def _ring_counts(name, waves_per_theta):
    """chunk counts under which every one of a theta's wavefronts meets RING_CASES[name] (wavefront g takes chunks g, g + waves, ...)"""
    return [c for c in RING_CASES[name] for _ in range(waves_per_theta)]


# ================================================================================================================== CPU tests
def test_edge_points_sit_on_the_branches_of_the_term(ob):
    """At t = 0 the extra points have the board coordinates they were built from, exactly; the set holds exact integers, both
    outlines, exact half cells and, off the board, res == huber_delta exactly and one lattice unit to either side of it.  The
    starts of EDGE_STARTS are within 16 lattice units of t = 0, so the first round's stencils (stride 16, 8, ...) put these
    coordinates under the start or one of its neighbours."""
    op = _oparams(ob, dict(cp.dyadic_params(), refine_div=16))
    yz, lab = _edge_points()
    i, j = cp.board_coords(op, yz, (0.0, 0.0, 0.0))
    n = len(_OFF)
    assert np.array_equal(i[600:600 + n], np.array([v[0] for v in _OFF])) and np.array_equal(j[600:600 + n], np.array([v[1] for v in _OFF]))
    assert np.array_equal(lab[600:600 + n], np.zeros(n)) and np.array_equal(lab[600 + n:], np.ones(n))
    out = np.minimum(np.abs(i), np.abs(i - op.board_w)) + np.minimum(np.abs(j), np.abs(j - op.board_h))
    d = op.huber_delta
    assert d == 0.125
    assert [float(v) for v in out[600:603]] == [d, d + 1 / 256, d - 1 / 256] and [float(v) for v in out[603:606]] == [d, d + 1 / 256, d - 1 / 256]
    unit = (op.ty_step / op.refine_div) / op.grid_length
    assert unit == 1 / 256
    for lat, _ in EDGE_STARTS:
        assert lat[0] == 160 and abs(lat[1] - 256) <= 16 and abs(lat[2] - 256) <= 16
        assert ob.lattice_point(op, lat)[0] == 0.0


def test_crossing_points_tie_neighbours_of_different_distance(ob):
    """From CROSS_START the cheapest of the 26 neighbours cost 0, below the centre, and they include neighbours of different
    d2 -- among them one of d2 == 1, which "nearer first" must take, and one with a lower index e and a larger d2, which "first
    in (dk, da, db) order" alone would take."""
    op = _oparams(ob, dict(cp.dyadic_params(), refine_div=16))
    yz, lab = _crossing_points()
    lat, ph = CROSS_START

    def cost(q):
        return ob.cost_q(ob.lattice_point(op, q), yz[:, 0], yz[:, 1], _i8(lab), op, ph, 1)

    offs = [(dk, da, db) for dk in (-1, 0, 1) for da in (-1, 0, 1) for db in (-1, 0, 1)]
    v = {o: cost([lat[0] + 16 * o[0], lat[1] + 16 * o[1], lat[2] + 16 * o[2]]) for o in offs if o != (0, 0, 0)}
    best = [o for o in offs if o != (0, 0, 0) and v[o] == min(v.values())]
    d2 = [o[0] ** 2 + o[1] ** 2 + o[2] ** 2 for o in best]
    assert min(v.values()) == 0 < cost(lat)
    assert len(set(d2)) >= 2 and min(d2) == 1
    nearest = [o for o, d in zip(best, d2) if d == 1]
    assert len(nearest) == 1 and offs.index(best[0]) < offs.index(nearest[0])   # the first tied neighbour is not the nearest


@pytest.mark.parametrize("name", list(RING_CASES))
def test_ring_patterns_are_what_they_claim(ob, name):
    """chunk_pattern's designated silent points are silent and its active ones are not, under stencil_sweep's own test in fp64,
    for the first round's three thetas from the start the GPU test uses; per 64-point chunk the requested counts, for one
    wavefront per theta and for four."""
    op = _oparams(ob, _cut_grid(_oparams(ob)))
    near = cp.nearest_lattice(op, POSE_C)
    for waves in (1, 4):
        counts = _ring_counts(name, waves)
        yz, lab, active = cp.chunk_pattern(op, counts, 5, POSE_C)
        assert [int(active[64 * c:64 * c + 64].sum()) for c in range(len(counts))] == counts
        assert counts[::waves] == RING_CASES[name] and counts[waves - 1::waves] == RING_CASES[name]
        for lat in (near, [near[0] + 8, near[1] - 8, near[2] + 8]):
            for dk in (-1, 0, 1):
                silent = cp.silent_mask(op, yz, lab, [lat[0] + dk * op.refine_div, lat[1], lat[2]], 0, op.refine_div)
                assert np.array_equal(silent, ~active), (name, waves, lat, dk)


# ================================================================================================================== GPU tests
@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, 28800, _nparams())
    yield e
    e.close()


@pytest.mark.gpu
def test_term_edges_equal_the_oracle(ob, est):
    """The term and the silence test on coordinates exactly on every branch of them (an integer, k + 1/2, 0, W, H,
    res == huber_delta off the board and one lattice unit to either side), both labels, both phases."""
    fields = dict(cp.dyadic_params(), refine_div=16)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab = _edge_points()
    for lat, ph in EDGE_STARTS:
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)


@pytest.mark.gpu
def test_trip_edges_through_the_192_thread_entry(ob, est):
    """A trip of the workgroup is 64 points per theta, the basin check takes 192 per trip: every m around their multiples (and
    around those of 128), from a start near the pose and from one a square off with the colours swapped."""
    est.set_params(_nparams())
    op = _oparams(ob)
    near = cp.nearest_lattice(op, POSE_B)
    hop_y = round(op.grid_length / (op.ty_step / op.refine_div))
    for m in M_ENTRY:
        yz, lab = cp.noisy_board(op, m, 300 + m, POSE_B)
        for lat, ph in (([near[0] + 2, near[1] - 3, near[2] + 1], 0), ([near[0], near[1] + hop_y, near[2]], 1)):
            assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (m, lat, ph)


@pytest.mark.gpu
def test_trip_edges_through_the_768_thread_solver(ob, est):
    """Four wavefronts per theta: a trip of the workgroup is 256 points per theta.  Everything downstream of the
    solver's own grid argmin == the oracle, on the default grid cut to 9 x 12 x 12 candidates (the same steps and stencils)."""
    fields = _cut_grid(_oparams(ob))
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    for m in M_SOLVER:
        yz, lab = cp.noisy_board(op, m, 400 + m, POSE_C)
        _assert_solver_downstream(ob, op, est, yz, lab)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RING_CASES))
def test_ring_fills_through_both_entries(ob, est, name):
    """The active-point ring filled to its bound of 127 live entries, one short of it, drained exactly, with every point active
    and with none: through K7r's entry (one wavefront per theta takes every chunk) and through the solver (four per theta, each
    taking every fourth chunk -- the counts are laid out so that each of them meets the same sequence)."""
    fields = _cut_grid(_oparams(ob))
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    near = cp.nearest_lattice(op, POSE_C)
    yz, lab, _ = cp.chunk_pattern(op, _ring_counts(name, 1), 5, POSE_C)
    for lat in (near, [near[0] + 8, near[1] - 8, near[2] + 8]):
        assert _g_refine(est, yz, lab, lat, 0) == _o_refine(ob, op, yz, lab, lat, 0), (name, lat)
    yz, lab, _ = cp.chunk_pattern(op, _ring_counts(name, 4), 5, POSE_C)
    _assert_solver_downstream(ob, op, est, yz, lab)
    assert _g_refine(est, yz, lab, near, 0) == _o_refine(ob, op, yz, lab, near, 0), name


@pytest.mark.gpu
def test_decision_ties_equal_the_oracle(ob, est):
    """The move of a round under the oracle's rule -- lower cost, then smaller d2, then lower e: neighbours that tie on cost with
    different d2 (the crossing points), with equal d2 and different e (the symmetric dyadic set on its line ty = tz = 0), and
    starts on the first and the last row of the theta table, where the lanes of thetas outside it take no part."""
    fields = dict(cp.dyadic_params(), refine_div=16)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    yz, lab = _crossing_points()
    for lat, ph in (CROSS_START, ([160, 256, 256], 1), ([0, 256, 256], 0), ([320, 256, 256], 0)):
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)
    yz, lab = cp.dyadic_points_symmetric(11)
    for lat, ph in (([96, 256, 256], 0), ([112, 256, 256], 1), ([144, 256, 256], 1), ([212, 256, 256], 0), ([0, 256, 256], 0), ([0, 256, 256], 1),
                    ([320, 256, 256], 0), ([320, 256, 256], 1), ([4, 250, 263], 0), ([317, 263, 250], 1)):
        assert _g_refine(est, yz, lab, lat, ph) == _o_refine(ob, op, yz, lab, lat, ph), (lat, ph)


@pytest.mark.gpu
def test_pipeline_192_thread_kernel_equals_the_768_thread_kernel():
    """One batch of 257 frames (above kSmallBatchFrames = 64: the 192-thread kernel, points staged in LDS), the same frames in
    batches of 64 (at most kSmallBatchFrames: the 768-thread kernel, the last batch a single frame) and in batches of 128 (the
    192-thread kernel again, at another batch size): status, flags, grid_index, iters_a, iters_b, the fixed-point costs and the
    corners are equal frame by frame.  (A record carries cost_q and alt_q as cost_a = cost_q / 2^40 and cost_b = alt_q / 2^40,
    exact images of integers below 2^53.)"""
    from lidar_camera_calibration_amd import LidarCornersBatch, synth
    from lidar_camera_calibration_amd import _native as N
    F = 4 * cc.SMALL_BATCH + 1
    assert F == 257
    clouds, clicks, _, _ = synth.make_batch(F, seed=0xFACE)
    e = LidarCornersBatch(F, clouds.shape[1], _nparams())
    try:
        def fields(res):
            return (np.array([(r.status, r.flags, r.grid_index, r.iters_a, r.iters_b, r.phase) for r in res], np.int64),
                    np.array([(r.cost_a, r.cost_b, r.sel_cost) + tuple(r.theta_t) for r in res], np.float64),
                    np.stack([np.ctypeslib.as_array(r.corners).copy() for r in res]), np.array([r.n_corners for r in res]))

        big = fields(e.extract(clouds, clicks))
        by_size = {size: [fields(e.extract(clouds[a:a + size], clicks[a:a + size])) for a in range(0, F, size)] for size in (cc.SMALL_BATCH, 128)}
    finally:
        e.close()
    assert int((big[0][:, 0] == N.OK).sum()) >= 200   # (the comparison is about refined frames)
    for size, parts in by_size.items():
        for k in range(4):
            np.testing.assert_array_equal(big[k], np.concatenate([p[k] for p in parts]), err_msg="batches of %d, field %d" % (size, k))
