"""The GRID back end's BATCH kernels on constructed labelled frames, through ilcc_debug_grid_solve_batch
(LidarCornersBatch.grid_solve_batch): what production runs on a real batch and no constructed input reached before --

  * K7r at 192 threads with LDS-staged points (refine_frame<true>: one wavefront per theta in the recount, the sweeps, the first-round
    shortcut and the argmin; blockIdx.x indexing the offsets, the counts, the near-tie lists and the partial records), a frame above
    the staging capacity taking refine_frame<false> beside staged ones in the same launch;
  * k6_locate, the fused locate, from 512 frames on, and everything that follows it;
  * the common pre-pass, the full pass and its listed form at F > 1, whose work items span frames;
  * K5w and K7b per frame at non-zero offsets.

The frames are those of test_grid_backend_constructed, test_k7r_sweep_forms and test_grid_pruning_constructed (zero-cost plateaus
of 2, 33 and more than 256 near ties, coordinates on the term's branches, ring fills at the bound of 127, lane sums past 2^53,
tiles that survive by one rounding), grouped by parameter set and laid out by tests/constructed_batches.py: one batch of 65 frames
per group (the first size above kSmallBatchFrames) and, but for the 28 800-point frames, one of 512 (kLocateMinFrames); each on a
fresh handle at its 1 024 staged points and again once the handle is reserved so that every frame that can be staged is.

What it found (fixed in k6_grid_cost.hip, grid_cost_body<..., OVERFLOW = 2>): a frame above the staging capacity whose interior class
does not fit the staged prefix took the full pass's LDS-free form, which adds the points in another order -- the fp32 grid_cost of
the 2 833-, 2 364- and 8 192-point frames came out one ulp apart on the fresh and on the reserved handle (7b788542 / 7a788542).

Every assertion is `==`.  Per OK frame: everything downstream of the batch's own grid argmin == the oracle's refinement from that
start (test_grid_backend_constructed._assert_downstream); the argmin against the oracle's by the rule of the frame's single-frame
test, unchanged; every field == the single-frame ilcc_grid_solve record of the same frame, but `ties` and ILCC_FLAG_TIE_OVERFLOW
(run-dependent: test_grid_pruning_constructed, note (b)); replicas alike; reserved == fresh capacity; 65 == 512 frames.  A frame
with a failed status: valid == 0, the caller's status, nothing else written.  The OK frame without points: the oracle accepts empty
input, so its own record is held against the oracle's too (argmin and refinement).

The CPU tests (no marker) check that the batches are what the GPU tests take them for.
"""
import functools

import numpy as np
import pytest

import constructed_batches as B
import constructed_points as cp
from test_grid_backend_constructed import _CLASS, K_TIE_CAP, PLATEAUS, _assert_downstream, _flags, _i8, _nparams, _oparams, _plateau_ref
from test_grid_pruning_constructed import CASES, _ref
from test_k7r_sweep_forms import RING_CASES, _ring_counts

K_REFINE_THREADS = 192         # kRefineThreads: K7r above kSmallBatchFrames frames


# ================================================================================================================== CPU tests
def test_groups_are_one_per_parameter_set(ob):
    g = B.groups(ob)
    assert tuple(g) == B.GROUP_NAMES
    structs = [bytes(_oparams(ob, gr.fields)) for gr in g.values()]
    assert len(set(structs)) == len(structs)
    for gr in g.values():
        names = [fr.name for fr in gr.frames]
        assert len(set(names)) == len(names) and len(names) >= 1


def test_every_constructed_case_is_in_some_batch(ob):
    """Every constructed labelled frame of the single-frame suites, byte for byte the frame those suites build, under the
    parameter set they run it with."""
    g = B.groups(ob)

    def has(group, yz, lab, fields):
        assert bytes(_oparams(ob, g[group].fields)) == bytes(_oparams(ob, fields)), group
        return any(np.array_equal(fr.yz, np.asarray(yz, np.float32)) and np.array_equal(fr.lab, lab) for fr in g[group].frames)

    import test_grid_backend_constructed as tb
    import test_k7r_sweep_forms as tk
    op = _oparams(ob)
    for name in PLATEAUS:
        assert has("default", *_plateau_ref(ob, name)[:2], {}), name
    for m in tb.M_SOLVE_DEFAULT:
        assert has("default", *cp.noisy_board(op, m, 200 + m, tb.POSE_B), {}), m
    for m in tk.M_ENTRY:
        assert has("default", *cp.noisy_board(op, m, 300 + m, tk.POSE_B), {}), m
    small = tb._small_grid(op)
    for m in tb.M_SOLVE_SMALL:
        assert has("small_grid", *cp.noisy_board(_oparams(ob, small), m, 200 + m, tb.POSE_B), small), m
    cut = tb._cut_grid(op)
    opc = _oparams(ob, cut)
    for m in tk.M_SOLVER:
        assert has("cut", *cp.noisy_board(opc, m, 400 + m, tk.POSE_C), cut), m
        assert has("default", *cp.noisy_board(op, m, 400 + m, tk.POSE_C), {}) == (m >= B.B_EDGE_FROM), m
    for name in RING_CASES:
        assert has("cut", *cp.chunk_pattern(opc, _ring_counts(name, 1), 5, tk.POSE_C)[:2], cut), name
    assert has("cut", *cp.chunk_pattern(opc, cp.chunk_counts(5), 5, tb.POSE_C)[:2], cut)
    dyadic = dict(cp.dyadic_params(), refine_div=16)
    for yz, lab in (tk._edge_points(), tk._crossing_points(), cp.dyadic_points_symmetric(11)):
        assert has("dyadic", yz, lab, dyadic)
    for case, div, group in ((tb.FAR_IN, 16, "far_delta5"), (tb.FAR_OUT, 16, "far_delta5"), (tb.FAR_OUT_192, 16, "far_delta50"),
                             (tb.FAR_OUT_192, 0, "far_delta50_div0")):
        fields = dict(huber_delta=case["huber_delta"], refine_max_rounds=tb.FAR_ROUNDS, refine_div=div)
        assert has(group, *cp.far_points(case["m"], case["lo"], case["hi"], case["seed"]), fields), group
    for name, case in CASES.items():
        r = _ref(ob, name)
        where = [n for n, gr in g.items() if any(fr.rule == ("pruning", name) for fr in gr.frames)]
        assert len(where) == 1 and has(where[0], r.yz, r.lab, dict(case["fields"], grid_prune=1)), name


@pytest.mark.parametrize("name", B.GROUP_NAMES)
def test_batches_are_laid_out_as_documented(ob, name):
    """Offsets, the special slots, which slots are replicas of which frame, and the interleaving: every pass visits every distinct
    frame once, so replica counts differ by at most one; replicas of a frame start at different offsets; with four or more
    distinct frames some frame meets different predecessors."""
    gr = B.groups(ob)[name]
    k = len(gr.frames)
    assert B.batch_sizes(name) == ((B.F_SMALL,) if max(len(fr.lab) for fr in gr.frames) > 8274 else (B.F_SMALL, B.F_LARGE))
    for F in B.batch_sizes(name):
        b = B.compose(gr, F)
        failed, empty = B.special_slots(F)
        assert len(b.frames) == F and failed[0] == 0 and 0 < failed[1] < F - 1 and empty not in failed and 0 < empty < F - 1
        assert b.offsets[0] == 0 and np.array_equal(np.diff(b.offsets.astype(np.int64)), [len(lab) for _, lab in b.frames])
        assert [f for f in range(F) if b.status[f] != B.STATUS_OK] == list(failed)
        assert b.source[empty] == -1 and len(b.frames[empty][1]) == 0 and b.status[empty] == B.STATUS_OK
        assert all(len(b.frames[f][1]) > 0 for f in failed)   # (a failed frame has points a kernel could wrongly work on)
        counts = []
        for src in range(k):
            slots = B.replicas(b, src)
            counts.append(len(slots))
            for f in slots:
                assert b.frames[f][0] is gr.frames[src].yz and b.frames[f][1] is gr.frames[src].lab
            assert len({int(b.offsets[f]) for f in slots}) == len(slots)
        assert sum(counts) == F - 3 and max(counts) - min(counts) <= 1 and min(counts) >= 2
        if k >= 4:
            before = {src: {int(b.source[f - 1]) for f in B.replicas(b, src)} for src in range(k)}
            assert any(len(v) >= 2 for v in before.values())


@pytest.mark.parametrize("name", B.GROUP_NAMES)
def test_frames_on_both_sides_of_the_staging_capacities(ob, name):
    """The fresh handle's 1 024 points split the group's frames into staged ones and global-memory ones -- or the group says why it
    cannot; the reserved handle stages every frame of at most kGridLdsPointsMax points."""
    gr = B.groups(ob)[name]
    sizes = [len(fr.lab) for fr in gr.frames]
    cap = B.reserved_capacity(gr)
    in_lds, in_global = B.staged(gr, B.LDS_FRESH)
    print("group %s: %d distinct frames of %d to %d points; capacity %d stages %d of them, a fresh handle's %d stages %d" %
          (name, len(sizes), min(sizes), max(sizes), cap, B.staged(gr, cap)[0], B.LDS_FRESH, in_lds))
    assert B.LDS_FRESH <= cap <= B.LDS_MAX and cap % 256 == 0
    assert B.staged(gr, cap)[0] == sum(m <= B.LDS_MAX for m in sizes)
    if gr.sides_note is None:
        assert in_lds >= 1 and in_global >= 1
    else:
        assert (in_lds == 0 or in_global == 0) and len(gr.sides_note) > 20
    if name == "small_grid":
        assert sorted(sizes) == [B.LDS_MAX, B.LDS_MAX + 1]


def test_ring_layouts_are_one_wavefront_per_theta(ob):
    """The 192-thread kernel has ONE wavefront per theta, which takes every 64-point chunk: the cut group's ring frames are laid out
    with _ring_counts(name, 1), so that wavefront meets RING_CASES[name] itself (the CPU test of test_k7r_sweep_forms establishes
    that the designated points are the active ones)."""
    import test_k7r_sweep_forms as tk
    gr = B.groups(ob)["cut"]
    opc = _oparams(ob, gr.fields)
    for name, counts in RING_CASES.items():
        assert _ring_counts(name, 1) == counts
        yz, lab, active = cp.chunk_pattern(opc, counts, 5, tk.POSE_C)
        fr = [f for f in gr.frames if f.name == "ring_" + name][0]
        assert np.array_equal(fr.yz, yz) and np.array_equal(fr.lab, lab) and len(lab) == 64 * len(counts) + 17
        assert [int(active[64 * c:64 * c + 64].sum()) for c in range(len(counts))] == counts


def test_which_groups_take_k6_locate(ob):
    """The host's rule, restated (constructed_batches.locate_form; the GPU tests hold the entry's own answer against it): no batch of
    65 frames takes k6_locate; at 512 frames every group does on a fresh handle but the grid of fewer than 8 thetas, which locates
    nothing at all; on the reserved handle the groups reserved at 8 192 points do not (k6_locate's LDS plan grows with the capacity
    and passes kLocateLdsMax above 3 072 points): there the 512-frame batch runs the three launches."""
    got = {}
    for name, gr in B.groups(ob).items():
        p = _oparams(ob, gr.fields)
        assert B.locate_form(p, B.LDS_FRESH, B.F_SMALL) in (0, 1) and B.locate_form(p, B.reserved_capacity(gr), B.F_SMALL) in (0, 1)
        got[name] = (B.locate_form(p, B.reserved_capacity(gr), B.F_LARGE), B.locate_form(p, B.LDS_FRESH, B.F_LARGE))
    print(got)
    want = {name: (2, 2) for name in B.GROUP_NAMES}
    want["prune_C6_none"] = (0, 0)
    want["small_grid"] = want["far_delta5"] = (1, 2)
    assert got == want
    assert B.locate_form(_oparams(ob), 3072, 512) == 2 and B.locate_form(_oparams(ob), 3328, 512) == 1


# ================================================================================================================== GPU tests
@pytest.fixture(scope="module")
def single():
    """the single-frame solver: ilcc_grid_solve on one handle, its parameters set per group"""
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, 28800, _nparams())
    yield e
    e.close()


_single_cache, _run_cache, _excused = {}, {}, set()


def _masked(flags):
    tie_overflow, _ = _flags()
    return int(flags) & ~tie_overflow


def _single_records(ob, single, name):
    """-> per distinct frame (and, last, for the empty frame) ilcc_grid_solve's record without the run-dependent fields"""
    if name not in _single_cache:
        gr = B.groups(ob)[name]
        single.set_params(_nparams(gr.fields))
        out = []
        for yz, lab in [(fr.yz, fr.lab) for fr in gr.frames] + [(np.zeros((0, 2), np.float32), np.zeros(0, np.uint8))]:
            got = single.grid_solve(yz, lab)
            out.append((got["grid_index"], np.float32(got["grid_cost"]).tobytes(), tuple(int(v) for v in got["lat"]), got["phase"], got["cost_q"],
                        got["alt_cost_q"], got["rounds"], got["hops"], _masked(got["flags"])))
        _single_cache[name] = out
    return _single_cache[name]


def _heads_only(got):
    """the records cut down to the part in front of `corners` (the entry copies no corners)"""
    from lidar_camera_calibration_amd import _native as N
    res = got.pop("results")
    got["heads"] = [bytes(res[f])[:N.Result.corners.offset] for f in range(len(got["valid"]))]
    return got


def _run(ob, name, F, reserved, mode=None):
    """one batch of the group -> (Batch, grid_solve_batch's dict).  The two capacities share a handle of the batch's own (a handle for
    512 frames of 8 192 points takes seconds to allocate): the batch runs on it fresh, at its 1 024 points, and again once
    ilcc_reserve has raised the staging to the group's capacity -- the entry itself never grows a capacity, and reports the one it
    ran with."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    key = (name, F, reserved, mode)
    if key not in _run_cache:
        gr = B.groups(ob)[name]
        b = B.compose(gr, F)
        e = LidarCornersBatch(F, int(b.offsets[-1]), _nparams(gr.fields))
        try:
            if mode is not None:
                e.debug_full_pass_launch(*mode)
            _run_cache[(name, F, False, mode)] = (b, _heads_only(e.grid_solve_batch(b.frames, b.status)))
            e.reserve(B.reserved_capacity(gr), 0)
            _run_cache[(name, F, True, mode)] = (b, _heads_only(e.grid_solve_batch(b.frames, b.status)))
        finally:
            e.close()
    return _run_cache[key]


def _single_view(got, f):
    return (int(got["grid_index"][f]), got["grid_cost"][f].tobytes(), tuple(int(v) for v in got["lat"][f]), int(got["phase"][f]),
            int(got["cost_q"][f]), int(got["alt_cost_q"][f]), int(got["rounds"][f]), int(got["hops"][f]), _masked(got["flags"][f]))


def _head(got, f):
    """the frame's result record in front of `corners` as bytes, without grid_ties and ILCC_FLAG_TIE_OVERFLOW"""
    from lidar_camera_calibration_amd import _native as N
    raw = bytearray(got["heads"][f])
    d = N.Result.grid_ties
    raw[d.offset:d.offset + d.size] = bytes(d.size)
    d = N.Result.flags
    raw[d.offset:d.offset + d.size] = np.int32(_masked(got["result_flags"][f])).tobytes()
    return bytes(raw)


def _batch_view(got, f):
    """everything the entry returns for the frame but the run-dependent fields"""
    return _single_view(got, f) + (int(got["valid"][f]), got["x"][f].tobytes(), _head(got, f))


def _dict_at(got, f):
    return dict(grid_index=int(got["grid_index"][f]), lat=got["lat"][f], phase=int(got["phase"][f]), cost_q=int(got["cost_q"][f]),
                alt_cost_q=int(got["alt_cost_q"][f]), rounds=int(got["rounds"][f]), hops=int(got["hops"][f]), flags=int(got["flags"][f]),
                ties=int(got["ties"][f]), grid_cost=float(got["grid_cost"][f]))


@functools.lru_cache(maxsize=None)
def _oracle_argmin(ob, name, frame):
    gr = B.groups(ob)[name]
    fr = gr.frames[frame]
    return ob.grid_search(fr.yz[:, 0], fr.yz[:, 1], _i8(fr.lab), _oparams(ob, gr.fields), 1)[0]


def _check_argmin(ob, name, src, fr, rec):
    """the frame's single-frame rule for the grid argmin, unchanged"""
    tie_overflow, border_risk = _flags()
    if fr.rule is None:
        return
    kind, arg = fr.rule
    if kind == "plateau":          # test_zero_cost_plateaus
        _, _, flat, _, zeros = _plateau_ref(ob, arg)
        assert rec["grid_index"] == flat and rec["grid_cost"] == 0.0, (fr.name, rec, flat)
        assert (rec["phase"], rec["cost_q"], rec["rounds"], rec["hops"]) == (0, 0, 5, 0), (fr.name, rec)
        assert (rec["flags"] & border_risk) == 0
        assert bool(rec["flags"] & tie_overflow) == (PLATEAUS[arg][3] == "overflow"), (fr.name, rec)
        assert rec["ties"] >= zeros - 1, (fr.name, rec, zeros)
        if PLATEAUS[arg][3] != "overflow":
            assert _CLASS[PLATEAUS[arg][3]][0] - 1 <= rec["ties"] <= K_TIE_CAP, (fr.name, rec)
    elif kind == "solve":          # _solve_case
        flat = _oracle_argmin(ob, name, src)
        assert rec["grid_index"] == flat or (rec["flags"] & border_risk), (fr.name, rec, flat)
        if arg and rec["grid_index"] != flat:
            _excused.add((name, fr.name))
        assert len(_excused) <= 1, _excused
    else:                          # test_pruned_solve_matches_the_oracle_and_rejects_only_losers (a)
        assert rec["grid_index"] == _ref(ob, arg).flat and not (rec["flags"] & border_risk), (fr.name, rec)


def _check_run(ob, single, name, F, reserved, mode=None):
    """every per-frame assertion on one batch -> {distinct frame index (-1: the empty frame): its record}"""
    from lidar_camera_calibration_amd import _native as N
    gr = B.groups(ob)[name]
    op = _oparams(ob, gr.fields)
    b, got = _run(ob, name, F, reserved, mode)
    cap = B.reserved_capacity(gr) if reserved else B.LDS_FRESH
    assert got["lds_points"] == cap
    assert got["k7r_threads"] == K_REFINE_THREADS
    assert got["locate"] == B.locate_form(op, cap, F), (got["locate"], cap, F)
    if mode is not None and got["full_pass"] != mode[0]:
        # (a grid without a common pre-pass keeps the (n_th, F) form)
        assert op.n_th < 7 and got["full_pass"] == N.FULL_PASS_GRID
    failed, empty = B.special_slots(F)
    # ---- failed frames: valid == 0, the caller's status, nothing else written (the record slot keeps every bit set, the result its zeros)
    for f in failed:
        assert got["valid"][f] == 0 and got["status"][f] == b.status[f] != N.OK
        assert (got["rounds"][f], got["hops"][f], got["phase"][f], got["flags"][f], got["ties"][f]) == (-1, -1, -1, -1, -1)
        assert got["cost_q"][f] == -1 and got["alt_cost_q"][f] == -1 and got["x"][f].tobytes() == b"\xff" * 24
        assert got["heads"][f][4:] == bytes(len(got["heads"][f]) - 4), f
    # ---- OK frames
    ok = [f for f in range(F) if b.status[f] == N.OK]
    assert (got["valid"][ok] == 1).all(), [f for f in ok if got["valid"][f] != 1]
    assert all(got["status"][f] in (N.OK, N.AMBIGUOUS) for f in ok)
    singles = _single_records(ob, single, name)
    records = {}
    for src in list(range(len(gr.frames))) + [-1]:
        slots = B.replicas(b, src) if src >= 0 else [empty]
        yz, lab = b.frames[slots[0]]
        first = _batch_view(got, slots[0])
        for f in slots[1:]:                                                  # replicas
            assert _batch_view(got, f) == first, (name, src, slots[0], f)
        rec = _dict_at(got, slots[0])
        _assert_downstream(ob, op, yz, lab, rec)                             # the oracle, refinement
        if src >= 0:
            _check_argmin(ob, name, src, gr.frames[src], rec)                # the oracle, argmin
        else:
            e = np.zeros(0, np.float32)
            assert rec["grid_index"] == ob.grid_search(e, e, np.zeros(0, np.int8), op, 1)[0], rec
        assert _single_view(got, slots[0]) == singles[src], (name, src, _single_view(got, slots[0]), singles[src])   # the single frame
        for f in slots:                                                      # (the record and the result agree)
            assert got["result_flags"][f] & ~N.FLAG_LOW_COVERAGE == got["flags"][f] and got["grid_ties"][f] == got["ties"][f]
        records[src] = first
    return records


@pytest.mark.gpu
@pytest.mark.parametrize("name", B.GROUP_NAMES)
def test_batch_of_65_frames(ob, single, name):
    """The first size above kSmallBatchFrames: the 192-thread K7r behind the three locate launches."""
    from lidar_camera_calibration_amd import _native as N
    reserved = _check_run(ob, single, name, B.F_SMALL, True)
    fresh = _check_run(ob, single, name, B.F_SMALL, False)
    assert _run(ob, name, B.F_SMALL, True)[1]["locate"] in (N.LOCATE_NONE, N.LOCATE_LAUNCHES)
    assert reserved == fresh
    gr = B.groups(ob)[name]
    print("group %s, %d frames: %d distinct; staged / global at capacity %d: %s, at %d: %s" %
          (name, B.F_SMALL, len(gr.frames), B.reserved_capacity(gr), B.staged(gr, B.reserved_capacity(gr)), B.LDS_FRESH, B.staged(gr, B.LDS_FRESH)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in B.GROUP_NAMES if B.F_LARGE in B.batch_sizes(n)])
def test_batch_of_512_frames(ob, single, name):
    """kLocateMinFrames: k6_locate wherever the grid and the capacity take it (the entry's own answer, held against the restated
    rule by _check_run); its records per distinct frame equal the 65-frame batch's."""
    reserved = _check_run(ob, single, name, B.F_LARGE, True)
    fresh = _check_run(ob, single, name, B.F_LARGE, False)
    assert reserved == fresh
    assert reserved == _check_run(ob, single, name, B.F_SMALL, True)
    print("group %s, %d frames: located by %s (reserved) / %s (fresh)" %
          (name, B.F_LARGE, _run(ob, name, B.F_LARGE, True)[1]["locate"], _run(ob, name, B.F_LARGE, False)[1]["locate"]))


@pytest.mark.gpu
def test_full_pass_forms_on_the_default_group(ob, single):
    """The forced (n_th, F) form and the forced listed form at G = 1 and G = 7: identical records (work items span frames)."""
    from lidar_camera_calibration_amd import _native as N
    base = _check_run(ob, single, "default", B.F_SMALL, True, (N.FULL_PASS_GRID, 0))
    assert _run(ob, "default", B.F_SMALL, True, (N.FULL_PASS_GRID, 0))[1]["full_pass"] == N.FULL_PASS_GRID
    for g in (1, 7):
        assert _check_run(ob, single, "default", B.F_SMALL, True, (N.FULL_PASS_LISTED, g)) == base, g
        assert _run(ob, "default", B.F_SMALL, True, (N.FULL_PASS_LISTED, g))[1]["full_pass"] == N.FULL_PASS_LISTED
    assert base == _check_run(ob, single, "default", B.F_SMALL, True)
