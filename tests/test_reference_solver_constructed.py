"""The reference-trajectory solver -- K7a's two-pass trust-region / subspace-dogleg solves in both launch layouts, staged in LDS and
from global memory, and K7b's phase choice -- on CONSTRUCTED labelled points (tests/constructed_solves.py), where the rest of the
suite feeds it the ~950 points of synthetic frames through a single wavefront (ilcc_get_theta_t) or the whole pipeline.

The CPU tests (no marker) prove that the inputs ARE what the GPU tests take them for: the exact rational cost equals the oracle's
doubles on the dyadic board, every point of an "active" frame has a positive term, every solve case runs the branches it states
(the oracle's trace, oracle/ilcc_oracle.h ORC_TRACE_*) and is STABLE -- iteration counts and trace unchanged and x within 1e-9 from
the six starts moved by +-1e-11, and the oracle's own results reproducible to a tenth of the tolerances when the points are given
in another order (constructed_solves.py says why) -- so that a chain of ~40 accept / reject decisions can be compared across two implementations.
The GPU tests (`gpu` marker) compare with `==` against exact rationals (the sums at every point-count edge, K7b's decisions) and
against orc_reference_solve / orc_get_theta_t at test_gpu_parity.py's tolerances (iterations equal, theta_t to 1e-7, costs to
rel 1e-9 / abs 1e-12); the two launch layouts, a frame alone and among neighbours, staged and unstaged must agree bit for bit.
Nothing here is tuned against the kernels: seeds, poses and cases were picked on the CPU conditions alone.
What the suite cannot see: the double-buffered exchange slot of the workgroup-per-solve layout (`flip`).  A build that never
toggles it passed every test here -- with two wavefronts per SIMD no reader falls a whole evaluation behind the next writer.

Branches of the minimiser the case list reaches (asserted per case and over the list): Gauss-Newton step inside the radius,
subspace boundary step, boundary step on a reused linearisation, step rejected, step accepted with radius growth / unchanged /
halved, the one-dimensional subspace (one point 1e30 m away: a Jacobian of one row, its Gauss-Newton step outside the first
radius); terminations by function tolerance, iteration cap, gradient tolerance (at iteration 0 and later) and parameter tolerance
(a start with |theta| = 1e8).

Branches no input reached (test_no_input_reaches_the_remaining_branches tries: coincident points, one row / column of cells,
Huber deltas down to 1e-300, 100000 iterations, starts far off the board), and why they are believed unreachable with finite
values in the solver's domain:
  * mu escalation / linear-solver failure: the factorised matrix is A + mu D^2 with D^2 = clamp(diag A, 1e-6, 1e32) and mu >= 1e-8.
    By Cauchy-Schwarz every Schur complement is at least ~2 mu times its diagonal entry (1e-8 relative against a rounding error of
    1e-16), and a zero column still has the pivot mu 1e-6 > 0: Cholesky fails only on a non-finite entry.
  * traditional-dogleg fallback: taken when min_on_circle returns a non-finite value, i.e. again only from non-finite input.
  * invalid step (model_cost_change <= 0) and its fifth-in-a-row exit: the regularised Gauss-Newton step and the boundary minimiser
    both decrease the model whenever the gradient is non-zero; the gradient tolerance (1e-10) ends the solve long before g' A^-1 g
    could underflow.
  * minimum radius (1e-32): a step is at most 1e3 x radius long (D >= 1e-3, Jacobi scale <= 1), so the parameter tolerance
    (|step| <= 1e-8 (|x| + 1e-8), i.e. >= 1e-16) ends the solve some fifty halvings earlier.
"""
import functools
import itertools

import numpy as np
import pytest

import constructed_points as cp
import constructed_solves as cs

PASSES = ((0, 1), (1, 1), (0, 0), (1, 0))      # (topleft_white, use_oob) of the single-pass solves
ATOL_X, REL_COST, ABS_COST = 1e-7, 1e-9, 1e-12   # test_gpu_parity.py's tolerances for K7a against the oracle
REC_FIELDS = ("x", "cost_a", "cost_b", "sel", "iters_a", "iters_b", "phase", "valid")
CASE_BY_NAME = {c.name: c for c in cs.CASES}
NO_PLANE = 3


# ------------------------------------------------------------------------------------------------------------------ parameters
def _oparams(ob, fields=None):
    p = ob.default_params()
    p.solver = ob.SOLVER_REFERENCE_LOCAL
    p.phase_mode = 2
    return cp.apply_fields(p, fields or {})


def _nparams(fields=None):
    from lidar_camera_calibration_amd import _native as N
    p = N.default_params()
    p.solver = N.SOLVER_REFERENCE_LOCAL
    p.phase_mode = 2
    return cp.apply_fields(p, fields or {})


def _i8(lab):
    return lab.astype(np.int8)


def _pca_points(yz, lab):
    """labelled points as orc_get_theta_t takes them: (x, y, z, intensity) with the gray zone [50, 150]"""
    return np.concatenate([np.zeros((len(yz), 1), np.float32), yz, np.where(lab[:, None] == 1, 200.0, 0.0).astype(np.float32)], 1)


def _o_single(ob, op, yz, lab, tlw, oob, start):
    ob.trace_reset()
    t, c, it = ob.get_theta_t(_pca_points(yz, lab), [50.0, 150.0], op, tlw, oob, start)
    return dict(x=t, cost=c, iters=it, trace=ob.trace_get())


def _o_double(ob, op, yz, lab, phase, start=(0.0, 0.0, 0.0)):
    ob.trace_reset()
    r = ob.reference_solve(yz[:, 0], yz[:, 1], _i8(lab), op, phase, start)
    r["trace"] = ob.trace_get()
    return r


@functools.lru_cache(maxsize=None)
def _case_ref(ob, name):
    """-> (yz, lab, {(tlw, oob): single-pass solve from the case's start}, [two-pass solve of phase 0, of phase 1 from 0]): the
    oracle's results with their traces, computed once, shared, never modified"""
    case = CASE_BY_NAME[name]
    op = _oparams(ob, case.fields)
    yz, lab = cs.case_points(op, case)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return yz, lab, {k: _o_single(ob, op, yz, lab, k[0], k[1], case.start) for k in PASSES}, [_o_double(ob, op, yz, lab, ph) for ph in (0, 1)]


def _close_costs(a, b, costs):
    return all(abs(a[k] - b[k]) <= max(cs.PERMUTED_COST_REL * abs(b[k]), cs.PERMUTED_COST_ABS) for k in costs)


def _same_walk(a, b, iters):
    return all(a[k] == b[k] for k in iters) and a["trace"] == b["trace"] and float(np.abs(np.asarray(a["x"]) - np.asarray(b["x"])).max()) <= 1e-9


# the exact-sum frames: every count edge, once active under phase 0 and once under phase 1
@functools.lru_cache(maxsize=None)
def _edge_frames():
    """-> [(yz, lab, m, active phase, exact cost of the active phase as a double)], 2 x 17 frames; the other phase costs exactly 0"""
    from types import SimpleNamespace
    p = SimpleNamespace(**cp.dyadic_params())
    out = []
    for ph in (0, 1):
        for m in cs.M_EDGES:
            yz, lab = cs.active_frame(m, 1, ph)
            yz.setflags(write=False)
            lab.setflags(write=False)
            q = cs.exact_cost(p, yz, lab, 0, 0, ph, True)
            assert q == cs.exact_cost(p, yz, lab, 0, 0, ph, False) and cs.exact_cost(p, yz, lab, 0, 0, 1 - ph, True) == 0
            out.append((yz, lab, m, ph, cs.as_exact_double(q)))
    return out


def _edge_batch(n):
    """n frames drawn from _edge_frames() so that the pairs of frames sharing a workgroup change along the batch"""
    frames = _edge_frames()
    rng = np.random.default_rng(17)
    order = list(range(len(frames)))
    while len(order) < n:
        order += [int(v) for v in rng.permutation(len(frames))]
    return [frames[k] for k in order[:n]]


# K7b: exact ties and near ties between the two phases on the dyadic board at max_iterations = 0
def _choice_frames():
    """-> [(name, yz, lab)]: the two phases cost exactly the same (every point twice, once per label; points off the board only;
    no point at all), or differ by one point's term either way"""
    a, la = cs.active_frame(65, 3, 0)
    tie = (np.concatenate([a, a]), np.concatenate([la, 1 - la]))
    extra, le = cs.active_frame(1, 4, 0)
    off = np.array([[-1.0, 0.25], [0.875, -1.5], [2.0, 2.0]], np.float32)
    return [("tie_doubled", tie[0], tie[1]),
            ("tie_plus_one_wrong_in_phase_0", np.concatenate([tie[0], extra]), np.concatenate([tie[1], le])),
            ("tie_plus_one_wrong_in_phase_1", np.concatenate([tie[0], extra]), np.concatenate([tie[1], 1 - le])),
            ("tie_off_board", off, np.array([0, 1, 1], np.uint8)),
            ("tie_empty", np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)),
            ("active_in_phase_0", a, la), ("active_in_phase_1", a, 1 - la)]


# ================================================================================================================== CPU tests
def test_exact_rational_cost_equals_the_oracle_on_the_dyadic_board(ob):
    """exact_cost (fractions.Fraction: residual and Huber's rho, no rounding step) == orc_cost with `==` on dyadic_points(11) --
    points exactly on the outlines, on cell borders, on half cells and on res == delta -- for both phases, with and without the
    out-of-board term, at (0, 0, 0) and at two dyadic translations; it is the cost the solver reports with max_iterations = 0,
    and no permutation of the points changes the double."""
    op = _oparams(ob, dict(cp.dyadic_params(), max_iterations=0))
    yz, lab = cp.dyadic_points(11)
    rng = np.random.default_rng(0)
    for ty, tz in ((0.0, 0.0), (3 / 64, -5 / 128), (-0.25, 7 / 1024)):
        for ph, oob in itertools.product((0, 1), (1, 0)):
            q = cs.exact_cost(op, yz, lab, ty, tz, ph, bool(oob))
            want = cs.as_exact_double(q)
            assert q * 2 ** 20 == int(q * 2 ** 20) and want > 0
            assert ob.cost([0.0, ty, tz], yz[:, 0], yz[:, 1], _i8(lab), op, ph, oob) == want, (ty, tz, ph, oob)
            for _ in range(3):
                k = rng.permutation(len(lab))
                assert ob.cost([0.0, ty, tz], yz[k, 0], yz[k, 1], _i8(lab[k]), op, ph, oob) == want
            got = _o_single(ob, op, yz, lab, ph, oob, (0.0, ty, tz))
            assert (got["cost"], got["iters"], tuple(got["x"])) == (want, 0, (0.0, ty, tz))


def test_active_frames_make_every_point_count(ob):
    """In an active frame every point has the wrong colour for its cell under the frame's phase and lies at least 1/8 square from
    the cell's borders: its term at theta = t = 0 is positive (and exactly representable), the other phase's is 0.  So the exact
    sum changes when any one point is dropped or counted twice -- for every count edge and both phases."""
    op = _oparams(ob, cp.dyadic_params())
    for yz, lab, m, ph, want in _edge_frames():
        assert len(lab) == m <= cs.M_MAX
        i, j = cp.board_coords(op, yz, (0.0, 0.0, 0.0))
        fi, fj = i - np.floor(i), j - np.floor(j)
        assert (i > 0).all() and (i < op.board_w).all() and (j > 0).all() and (j < op.board_h).all()
        assert (np.minimum(fi, 1 - fi) >= 0.125).all() and (np.minimum(fj, 1 - fj) >= 0.125).all()
        terms = [cs.exact_cost(op, yz[k:k + 1], lab[k:k + 1], 0, 0, ph, True) for k in range(m)]
        assert min(terms) >= cs.exact_cost(op, cp.from_board(op, [0.125], [0.125]), [1], 0, 0, 0, True) > 0 and sum(terms) == want
        assert ob.cost([0.0, 0.0, 0.0], yz[:, 0], yz[:, 1], _i8(lab), op, ph, 0) == want
        assert ob.cost([0.0, 0.0, 0.0], yz[:, 0], yz[:, 1], _i8(lab), op, 1 - ph, 1) == 0.0
    assert len(_edge_frames()) == 2 * len(cs.M_EDGES)
    # the 260-frame batch holds every (count, phase) several times and pairs a frame with different neighbours
    batch = _edge_batch(260)
    assert {(f[2], f[3]) for f in batch} == {(f[2], f[3]) for f in _edge_frames()}
    assert len({(batch[k][2], batch[k + 1][2]) for k in range(0, 260, 2)}) > 60
    assert min(sum(1 for f in batch if (f[2], f[3]) == key) for key in {(f[2], f[3]) for f in batch}) >= 7


def test_phase_choice_frames_tie_exactly(ob):
    """The frames of the K7b test cost what their names say under the exact rational cost AND under the oracle's doubles: exact
    ties between the phases, and ties broken by one point's term in either direction."""
    op = _oparams(ob, dict(cp.dyadic_params(), max_iterations=0))
    for name, yz, lab in _choice_frames():
        q = [cs.exact_cost(op, yz, lab, 0, 0, ph, True) for ph in (0, 1)]
        assert [ob.cost([0.0, 0.0, 0.0], yz[:, 0], yz[:, 1], _i8(lab), op, ph, 1) for ph in (0, 1)] == [cs.as_exact_double(v) for v in q]
        if name.startswith("tie_plus_one_wrong_in_phase_") or name.startswith("active_in_phase_"):
            worse = int(name[-1])
            assert q[worse] > q[1 - worse], name
        else:
            assert q[0] == q[1], name
    # the outline frame puts points exactly on every outline and on interior cell borders
    yz, lab = cs.outline_frame(2)
    i, j = cp.board_coords(op, yz, (0.0, 0.0, 0.0))
    assert (i == 0).sum() >= 12 and (i == op.board_w).sum() >= 12 and (j == 0).sum() >= 12 and (j == op.board_h).sum() >= 12
    assert ((i == np.floor(i)) & (i > 0) & (i < op.board_w)).sum() >= 12 and ((j == np.floor(j)) & (j > 0) & (j < op.board_h)).sum() >= 12


@pytest.mark.parametrize("name", [c.name for c in cs.CASES])
def test_solve_case_is_stable_and_runs_what_it_states(ob, name):
    """The stability condition and the trace of one case: each of its six solves (four single passes from the case's start, the
    two-pass solve of each phase from 0) keeps its iteration counts and its whole trace, and x within 1e-9, from the six starts
    moved by +-1e-11; with the points in another order (other rounding of the sums, nothing else) the oracle repeats its own walk,
    x within 1e-9 and the costs within a tenth of the comparison tolerance (constructed_solves.PERMUTATIONS);
    between them the solves reach every branch the case states; none reaches a branch of NEVER_REACHED."""
    case = CASE_BY_NAME[name]
    op = _oparams(ob, case.fields)
    yz, lab, single, double = _case_ref(ob, name)
    assert len(lab) <= cs.M_MAX
    for (tlw, oob), ref in single.items():
        for s in cs.nudged_starts(case.start):
            assert _same_walk(_o_single(ob, op, yz, lab, tlw, oob, s), ref, ("iters",)), (name, tlw, oob, s)
    for ph, ref in enumerate(double):
        for s in cs.nudged_starts((0.0, 0.0, 0.0)):
            assert _same_walk(_o_double(ob, op, yz, lab, ph, s), ref, ("iters_a", "iters_b")), (name, ph, s)
    # the oracle's own error stays inside the tolerances: the same solves with the points in other orders
    rng = np.random.default_rng(len(lab))
    for _ in range(cs.PERMUTATIONS):
        k = rng.permutation(len(lab))
        for (tlw, oob), ref in single.items():
            got = _o_single(ob, op, yz[k], lab[k], tlw, oob, case.start)
            assert _same_walk(got, ref, ("iters",)) and _close_costs(got, ref, ("cost",)), (name, tlw, oob)
        for ph, ref in enumerate(double):
            got = _o_double(ob, op, yz[k], lab[k], ph)
            assert _same_walk(got, ref, ("iters_a", "iters_b")) and _close_costs(got, ref, ("cost_a", "cost_b", "sel")), (name, ph)
    traces = [r["trace"] for r in single.values()] + [r["trace"] for r in double]
    total = {k: sum(t[k] for t in traces) for k in ob.TRACE_NAMES}
    print(name, {k: v for k, v in total.items() if v})
    assert all(total[k] > 0 for k in case.expects), (name, total)
    assert not any(total[k] for k in cs.NEVER_REACHED), (name, total)
    if case.expects[:len(cs.NOISY)] == cs.NOISY and not case.fields and name.startswith("noisy"):
        # what the probe found for EVERY noisy-board solve, not merely for the case as a whole
        assert all(t[k] > 0 for t in traces for k in cs.NOISY), name


def test_case_list_reaches_every_reachable_branch(ob):
    """Over the list: every accept flavour, every termination that can be reached, and the one-dimensional subspace."""
    total = dict.fromkeys(ob.TRACE_NAMES, 0)
    for c in cs.CASES:
        _, _, single, double = _case_ref(ob, c.name)
        for r in list(single.values()) + double:
            for k, v in r["trace"].items():
                total[k] += v
    assert all(total[k] > 0 for k in cs.NOISY + cs.REACHED_SOMEWHERE), total
    assert set(cs.NOISY + cs.REACHED_SOMEWHERE + cs.NEVER_REACHED + ("solves",)) == set(ob.TRACE_NAMES)
    assert len(cs.CASES) <= 64


def test_no_input_reaches_the_remaining_branches(ob):
    """Attempts on the branches of NEVER_REACHED with finite inputs (the module docstring says why each is believed unreachable):
    coincident points, a Jacobian of one row, Huber deltas down to 1e-300, 100000 iterations, starts far off the board, points
    1e30 m away.  Every attempt ends normally and none of those counters moves."""
    rng = np.random.default_rng(9)
    one = cp.from_board(_oparams(ob), [2.3], [3.4])
    noisy = cp.noisy_board(_oparams(ob), 65, 1, cs.POSE)
    attempts = []
    for n in (1, 2, 5):   # coincident points, wrong colour / both colours
        attempts.append(({}, np.repeat(one, n, 0), np.full(n, 0, np.uint8), cs.START))
        attempts.append(({}, np.repeat(one, n, 0), (np.arange(n) & 1).astype(np.uint8), cs.START))
    for d in (1e-6, 1e-9, 1e-10, 3e-11, 1e-100, 1e-300):
        attempts.append((dict(huber_delta=d, max_iterations=100000), noisy[0], noisy[1], cs.START))
    for start in ((0.0, 5.0, 5.0), (3.0, 0.5, -0.5), (0.0, 1e6, 1e6), (1e8, 0.0, 0.0), (0.0, 1e30, -1e30)):
        attempts.append((dict(max_iterations=100000), noisy[0], noisy[1], start))
    for d in (1e3, 1e9, 1e20, 1e30):
        for pts in ([[d, d]], [[-d, 2 * d]], [[d, d], [-d, 2 * d]]):
            attempts.append((dict(max_iterations=1000), np.array(pts, np.float32), np.ones(len(pts), np.uint8), (0.0, 0.0, 0.0)))
    attempts.append((dict(max_iterations=100000), rng.uniform(-3, 3, (300, 2)).astype(np.float32), rng.integers(0, 2, 300).astype(np.uint8), cs.START))
    ob.trace_reset()
    n = 0
    for fields, yz, lab, start in attempts:
        op = _oparams(ob, fields)
        for tlw, oob in PASSES:
            t, c, it = ob.get_theta_t(_pca_points(yz, lab), [50.0, 150.0], op, tlw, oob, start)
            assert np.isfinite(t).all() and np.isfinite(c) and 0 <= it <= op.max_iterations
            n += 1
    tr = ob.trace_get()
    print(n, "attempts:", {k: v for k, v in tr.items() if v})
    assert not any(tr[k] for k in cs.NEVER_REACHED), tr


# ================================================================================================================== GPU tests
N_WAVE = 260      # a batch above kSolveWideMaxFrames (256): one wavefront per solve, four solves per workgroup


@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(cs.FRAMES_MAX, cs.M_MAX, _nparams())
    yield e
    e.close()


def _records(out, f):
    """frame f's two record slots as one comparable tuple (bit patterns of the doubles)"""
    return tuple(out[k][f].tobytes() for k in REC_FIELDS)


def _tile(frames, n):
    return [frames[k % len(frames)] for k in range(n)]


# ---- the entry's refusals
@pytest.mark.gpu
def test_batch_entry_refuses_what_it_cannot_hold(est):
    """more frames than max_frames, more points than the handle holds, no frame, a status list of another length, a handle in
    GRID mode: refused, and the next call works"""
    from lidar_camera_calibration_amd import IlccError, _native as N
    est.set_params(_nparams())
    one = (np.zeros((1, 2), np.float32), np.zeros(1, np.uint8))
    big = (np.zeros((cs.M_MAX, 2), np.float32), np.zeros(cs.M_MAX, np.uint8))
    for frames, status, want in (([one] * (cs.FRAMES_MAX + 1), None, N.CAPACITY), ([big] * cs.FRAMES_MAX + [one], None, N.CAPACITY),
                                 ([], None, N.BAD_ARGUMENT), ([one], [0, 0], N.BAD_ARGUMENT)):
        with pytest.raises(IlccError) as err:
            est.debug_reference_solve(frames, status)
        assert err.value.status == want, (len(frames), err.value)
    p = _nparams()
    p.solver = N.SOLVER_GRID
    est.set_params(p)
    with pytest.raises(IlccError) as err:
        est.debug_reference_solve([one])
    assert err.value.status == N.BAD_ARGUMENT and "REFERENCE_LOCAL" in str(err.value)
    est.set_params(_nparams())
    out = est.debug_reference_solve([one, big])
    assert out["valid"].tolist() == [[1, 1], [1, 1]] and out["lds_points"] == 1024


# ---- exact sums
@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [34, N_WAVE], ids=["workgroup_per_solve", "wavefront_per_solve"])
def test_exact_sums_at_every_count_edge(ob, est, n_frames):
    """max_iterations = 0 on the dyadic board: pass A, pass B and the selection cost are plain sums at x = 0 -- evaluate<true, *>
    (the linearisation of iteration 0) and evaluate<false, *> -- over active frames of every count edge, both phases.  Every sum
    == the exact rational cost, so no layout, staging loop, lane tail or partial-sum slot drops or repeats a point.  The handle's
    staging holds 1024 points: the 1025-point frames run from global memory beside staged ones in the same launch."""
    est.set_params(_nparams(dict(cp.dyadic_params(), max_iterations=0)))
    batch = _edge_batch(n_frames)
    out = est.debug_reference_solve([(f[0], f[1]) for f in batch])
    assert out["lds_points"] == 1024
    for k, (yz, lab, m, ph, want) in enumerate(batch):
        exact = [0.0, 0.0]
        exact[ph] = want
        for slot in (0, 1):
            got = (out["cost_a"][k, slot], out["sel"][k, slot], out["cost_b"][k, slot])
            print(k, m, ph, slot, got, exact[slot])
            assert got == (exact[slot],) * 3, (k, m, ph, slot)
        assert out["iters_a"][k].tolist() == [0, 0] and out["iters_b"][k].tolist() == [0, 0]
        assert out["phase"][k].tolist() == [0, 1] and out["valid"][k].tolist() == [1, 1]
        assert not out["x"][k].any()
        r = out["results"][k]
        assert (r.status, r.phase, r.sel_cost, r.cost_a, r.cost_b) == (0, 1 - ph, 0.0, 0.0, 0.0)   # the phase that costs 0


# ---- trajectories
def _assert_solve(got_x, got_costs, got_iters, want, where):
    assert tuple(got_iters) == (want["iters_a"], want["iters_b"]), (where, got_iters, want)
    assert np.allclose(got_x, want["x"], rtol=0, atol=ATOL_X), (where, got_x, want["x"])
    for g, w in zip(got_costs, (want["cost_a"], want["cost_b"], want["sel"])):
        assert g == pytest.approx(w, rel=REL_COST, abs=ABS_COST), (where, got_costs, want)


@pytest.mark.gpu
def test_trajectories_single_pass_equal_the_oracle(ob, est):
    """Every stable case through ilcc_get_theta_t (one wavefront, global memory) from the case's start, both phases with and
    without the out-of-board term: iterations equal, theta_t within 1e-7, cost within rel 1e-9 / abs 1e-12 of orc_get_theta_t."""
    for case in cs.CASES:
        est.set_params(_nparams(case.fields))
        yz, lab, single, _ = _case_ref(ob, case.name)
        for (tlw, oob), want in single.items():
            t, c, it = est.get_theta_t(yz, lab, tlw, oob, case.start)
            print(case.name, tlw, oob, it, want["iters"], np.abs(t - want["x"]).max(), c, want["cost"])
            assert it == want["iters"], (case.name, tlw, oob, it, want["iters"])
            assert np.allclose(t, want["x"], rtol=0, atol=ATOL_X), (case.name, tlw, oob, t, want["x"])
            assert c == pytest.approx(want["cost"], rel=REL_COST, abs=ABS_COST), (case.name, tlw, oob)


def _field_groups():
    groups = {}
    for c in cs.CASES:
        groups.setdefault(tuple(sorted(c.fields.items())), []).append(c)
    return list(groups.values())


@pytest.mark.gpu
def test_trajectories_two_pass_both_layouts_equal_the_oracle(ob, est):
    """Every stable case through the batch entry -- pass A, pass B, selection cost, both phases from 0 -- once in a batch of at
    most 256 frames (a workgroup per solve, staged in LDS; the 1025-point cases from global memory) and once in 260 frames (a
    wavefront per solve).  Against orc_reference_solve: iterations equal, theta_t within 1e-7, costs within rel 1e-9 / abs 1e-12;
    the two layouts agree bit for bit on every record field; K7b's record is the slot with the lower selection cost (phase 0 on a
    tie), and its coverage is orc_coverage at the returned theta_t."""
    for cases in _field_groups():
        est.set_params(_nparams(cases[0].fields))
        op = _oparams(ob, cases[0].fields)
        refs = [_case_ref(ob, c.name) for c in cases]
        frames = [(r[0], r[1]) for r in refs]
        wide = est.debug_reference_solve(frames)
        wave = est.debug_reference_solve(_tile(frames, N_WAVE))
        assert wide["lds_points"] == wave["lds_points"] == 1024
        for k, (case, (yz, lab, _, double)) in enumerate(zip(cases, refs)):
            for ph in (0, 1):
                got = (wide["x"][k, ph], (wide["cost_a"][k, ph], wide["cost_b"][k, ph], wide["sel"][k, ph]), (wide["iters_a"][k, ph], wide["iters_b"][k, ph]))
                print(case.name, ph, got[2], (double[ph]["iters_a"], double[ph]["iters_b"]), np.abs(got[0] - double[ph]["x"]).max(), got[1])
                assert (wide["phase"][k, ph], wide["valid"][k, ph]) == (ph, 1)
                _assert_solve(*got, double[ph], (case.name, ph))
            for j in range(k, N_WAVE, len(frames)):
                assert _records(wave, j) == _records(wide, k), (case.name, j)
            best = 1 if wide["sel"][k, 1] < wide["sel"][k, 0] else 0
            for out, j in ((wide, k), (wave, k + len(frames) * ((N_WAVE - 1 - k) // len(frames)))):
                r = out["results"][j]
                assert (r.status, r.phase, tuple(r.theta_t), r.cost_a, r.cost_b, r.sel_cost, r.iters_a, r.iters_b) == \
                    (0, best, tuple(out["x"][j, best]), out["cost_a"][j, best], out["cost_b"][j, best], out["sel"][j, best],
                     out["iters_a"][j, best], out["iters_b"][j, best]), (case.name, j)
                assert (r.cells_hit, r.n_oob) == ob.coverage(list(r.theta_t), yz[:, 0], yz[:, 1], op), (case.name, j)


# ---- neighbours in a workgroup
def _neighbour_pool(ob):
    """distinct frames of the batch: 1 point, 1025 points, counts in between, and an empty one (live, no points)"""
    op = _oparams(ob)
    pool = [cp.noisy_board(op, m, 40 + m, cs.POSE) for m in (1, 1025, 64, 1, 257, 1025, 2, 300)]
    pool.append((np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)))
    return pool


@pytest.mark.gpu
@pytest.mark.parametrize("phase_mode", [0, 1, 2])
def test_neighbours_in_a_workgroup_do_not_touch_a_solve(ob, est, phase_mode):
    """261 frames (the last workgroup partly filled; with one phase per frame it holds ONE live wavefront): frames the front end
    failed (status != OK, some with points behind them) and empty frames interleaved with live ones -- so they share a workgroup
    and its staging region -- and frames of 1 point beside frames of 1025.  Every live frame's record slots are bit-identical to
    the same frame solved alone in a batch of one; a failed frame comes back valid = 0 with its result untouched."""
    from lidar_camera_calibration_amd import _native as N
    est.set_params(_nparams(dict(phase_mode=phase_mode)))
    pool = _neighbour_pool(ob)
    n_slots = 2 if phase_mode == 2 else 1
    alone = [est.debug_reference_solve([f]) for f in pool]
    rng = np.random.default_rng(phase_mode)
    pick = [int(v) for v in rng.integers(0, len(pool), cs.FRAMES_MAX)]
    pick[0:8] = [0, 1, 5, 3, 8, 1, 0, 8]          # 1 point beside 1025, an empty frame between live ones
    pick[-1] = 4                                  # the lone frame of the last workgroup is live
    status = np.where(rng.random(cs.FRAMES_MAX) < 0.3, NO_PLANE, 0).astype(np.int32)
    status[[0, 1, 2, 3, 5, 6, cs.FRAMES_MAX - 1]] = 0
    status[[4, 7, 9]] = (0, NO_PLANE, N.BAD_ARGUMENT)
    out = est.debug_reference_solve([pool[k] for k in pick], status)
    assert out["lds_points"] == 1024 and (status != 0).sum() > 40 and (status == 0).sum() > 150
    blank = N.Result()
    for f, k in enumerate(pick):
        r = out["results"][f]
        if status[f] != 0:
            assert out["valid"][f, :n_slots].tolist() == [0] * n_slots, f
            blank.status = int(status[f])
            assert bytes(r) == bytes(blank), f
            continue
        one = alone[k]
        for name in REC_FIELDS:
            assert out[name][f, :n_slots].tobytes() == one[name][0, :n_slots].tobytes(), (f, k, name)
        assert out["valid"][f, :n_slots].tolist() == [1] * n_slots
        assert out["phase"][f, :n_slots].tolist() == ([0, 1] if phase_mode == 2 else [phase_mode])
        assert bytes(r) == bytes(one["results"][0]), (f, k)
        assert r.status == 0
    # a slot the launch does not solve is not written
    if n_slots == 1:
        assert (out["valid"][:, 1] == -1).all()


# ---- staging fallback
@pytest.mark.gpu
def test_staging_fallback_to_global_memory_gives_the_same_records(ob, est):
    """A handle whose staging capacity was reserved above 4096 points: four staged frames no longer fit the workgroup's LDS and the
    wavefront-per-solve launch runs every frame from global memory (capacity 0).  The same 260 frames, one phase per frame (four
    frames per workgroup), give bit-identical records on the fresh handle (staged) and on the reserved one."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    p = _nparams(dict(phase_mode=1))
    est.set_params(p)
    refs = [_case_ref(ob, c.name) for c in _field_groups()[0]]
    frames = _tile([(r[0], r[1]) for r in refs], N_WAVE)
    staged = est.debug_reference_solve(frames)
    other = LidarCornersBatch(cs.FRAMES_MAX, cs.M_MAX, p)
    try:
        other.reserve(4097, 0)
        unstaged = other.debug_reference_solve(frames)
        wide = other.debug_reference_solve(frames[:len(refs)])     # (a workgroup per solve stages at any capacity)
    finally:
        other.close()
    assert staged["lds_points"] == 1024 and unstaged["lds_points"] == 4352 and 9 * 4352 * 4 > 144 * 1024
    for f in range(N_WAVE):
        assert _records(unstaged, f) == _records(staged, f), f
        assert bytes(unstaged["results"][f]) == bytes(staged["results"][f]), f
    for f in range(len(refs)):
        assert _records(wide, f) == _records(staged, f), f
    assert (staged["valid"][:, 0] == 1).all() and (staged["phase"][:, 0] == 1).all()


# ---- K7b
@pytest.mark.gpu
def test_phase_choice_and_coverage_are_exact(ob, est):
    """K7b on the dyadic board at max_iterations = 0 (x = 0, every decision exact): the chosen phase is the one with the lower
    selection cost, an exact tie goes to phase 0 -- frames whose two phases tie exactly by the rational cost, and frames where one
    point's term breaks the tie either way -- and cells_hit / n_oob equal orc_coverage, with points exactly on the outlines
    (outside: the test is strict) and on interior cell borders (the cell is floor's); ILCC_FLAG_LOW_COVERAGE is set exactly where
    fewer than min_cell_coverage of the cells are hit."""
    from lidar_camera_calibration_amd import _native as N
    fields = dict(cp.dyadic_params(), max_iterations=0)
    est.set_params(_nparams(fields))
    op = _oparams(ob, fields)
    lows = set()
    named = _choice_frames() + [("outline", *cs.outline_frame(2)), ("dyadic_points", *cp.dyadic_points(11)),
                                ("dyadic_symmetric", *cp.dyadic_points_symmetric(11))]
    for n_frames in (len(named), N_WAVE):
        out = est.debug_reference_solve(_tile([(yz, lab) for _, yz, lab in named], n_frames))
        for f in range(n_frames):
            name, yz, lab = named[f % len(named)]
            exact = [cs.as_exact_double(cs.exact_cost(op, yz, lab, 0, 0, ph, True)) for ph in (0, 1)] if f < len(named) else out["sel"][f % len(named)].tolist()
            no_oob = [ob.cost([0.0, 0.0, 0.0], yz[:, 0], yz[:, 1], _i8(lab), op, ph, 0) for ph in (0, 1)]
            assert out["sel"][f].tolist() == exact == out["cost_a"][f].tolist() and out["cost_b"][f].tolist() == no_oob, (name, f)
            want = 1 if exact[1] < exact[0] else 0
            if name.startswith("tie_plus_one_wrong_in_phase_") or name.startswith("active_in_phase_"):
                assert want == 1 - int(name[-1])
            elif name.startswith("tie_"):
                assert exact[0] == exact[1] and want == 0
            r = out["results"][f]
            cells, n_oob = ob.coverage([0.0, 0.0, 0.0], yz[:, 0], yz[:, 1], op)
            low = N.FLAG_LOW_COVERAGE if cells < op.min_cell_coverage * op.board_w * op.board_h else 0
            assert (r.status, r.phase, r.sel_cost, r.cost_a, r.cost_b, tuple(r.theta_t), r.iters_a, r.iters_b, r.flags) == \
                (0, want, exact[want], exact[want], no_oob[want], (0.0, 0.0, 0.0), 0, 0, low), (name, f)
            assert (r.cells_hit, r.n_oob) == (cells, n_oob), (name, f)
            lows.add(low)
    assert lows == {0, N.FLAG_LOW_COVERAGE}
