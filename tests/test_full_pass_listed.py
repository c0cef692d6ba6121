"""The two launch forms of K6's full pass behind the common pre-pass (k6_group_prepass): the (n_th, F) grid, where a (frame, theta)
workgroup whose group left no tile returns on its first instructions, and the LISTED launch (k6_grid_cost_listed, and
k6_grid_cost_listed_rest for the items beyond its workgroups), which starts only the workgroups the pre-pass listed, the pre-pass
having written the records of all the others.  Same body, same sums: every result must be equal bit for bit whatever the form and
whatever the number of workgroups G -- but for the two fields the suite documents as run-dependent (test_grid_pruning_constructed,
note (b)): the count of listed near ties and ILCC_FLAG_TIE_OVERFLOW, which is that count against kTieCap.

G = 1 leaves all items but one to the looping kernel, G = 3 (or 7) splits them, G = n_th x F is one workgroup per record (no second
launch); the rule for G itself is host arithmetic and is tested without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_camera_calibration_amd import _native as N

from test_front_end_launches import _fields
from test_grid_backend_constructed import _nparams
from test_grid_pruning_constructed import CASES, MAX_POINTS, _record, _ref

N_TH = 61          # the default grid
SOLVED = (N.OK, N.AMBIGUOUS)


# ================================================================================================================== the rule (CPU)
def _rule(observed, n_th, n_frames):
    g = C.c_uint32(0)
    form = N.lib().ilcc_debug_full_pass_rule(int(observed), int(n_th), int(n_frames), C.byref(g))
    return form, int(g.value)


def test_rule_for_the_workgroups_of_the_listed_launch():
    """G is never 0 and never above n_th x n_frames; with nothing observed the rule keeps the (n_th, F) grid; G is monotone in the
    observed live count; a count near the whole grid keeps the grid form, a quarter of it takes the listed one with G >= the count."""
    for n_th, n_frames in ((61, 1024), (61, 1), (1, 1), (129, 128), (6, 9), (61, 2), (7, 4096)):
        full = n_th * n_frames
        form, g = _rule(-1, n_th, n_frames)
        assert form == N.FULL_PASS_GRID and 1 <= g <= full
        last = 0
        for observed in sorted({0, 1, 2, 63, 64, 255, 256, 257, full // 8, full // 4, full // 2, (3 * full) // 4, full - 1, full, full + 1, 10 * full}):
            form, g = _rule(observed, n_th, n_frames)
            assert form in (N.FULL_PASS_GRID, N.FULL_PASS_LISTED)
            assert 1 <= g <= full, (n_th, n_frames, observed, g)
            assert g >= last, (n_th, n_frames, observed, g, last)
            assert g >= min(observed, full)
            last = g
            if observed >= full:
                assert form == N.FULL_PASS_GRID and g == full
    form, g = _rule(61 * 1024 // 4, 61, 1024)
    assert form == N.FULL_PASS_LISTED and 61 * 1024 // 4 <= g <= 61 * 1024 // 2
    assert _rule(0, 61, 0)[1] == 1 and _rule(-1, 0, 0) == (N.FULL_PASS_GRID, 1)   # (an empty batch: still one workgroup, never launched listed)


# ================================================================================================================== constructed cases
@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, MAX_POINTS, _nparams())
    yield e
    e.close()


def _prepass(gp):
    return gp["groups"], gp["words"], None if gp["groups"] == 0 else (gp["states"].tobytes(), gp["mask"].tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases_solve_alike_in_every_form(ob, est, name):
    """Cases A-G of tests/constructed_bounds.py (partial tiles, groups of 7 + 7 + 1, a grid with no common pre-pass, 0 to 65
    border-class points, the 512-thread instance, a frame too large for the walk layout) through ilcc_grid_solve with the (n_th, F)
    grid forced, the listed launch forced at G = 1, and at G = 3: every field of the record but `ties` and
    ILCC_FLAG_TIE_OVERFLOW equal, and the group states and masks equal."""
    r = _ref(ob, name)
    est.set_params(_nparams(dict(r.case["fields"], grid_prune=1)))
    runs = []
    try:
        for mode, g in ((N.FULL_PASS_GRID, 0), (N.FULL_PASS_LISTED, 1), (N.FULL_PASS_LISTED, 3)):
            est.debug_full_pass_launch(mode, g)
            got = est.grid_solve(r.yz, r.lab)
            last = est.debug_full_pass_last()
            runs.append((_record(got), _prepass(est.fetch_group_prepass()), last))
    finally:
        est.debug_full_pass_launch(N.FULL_PASS_RULE)
    print("case %s: forms %s, ties-free record %s" % (name, [(x[2]["form"], x[2]["workgroups"]) for x in runs], runs[0][0]))
    assert runs[0][0]["grid_index"] == r.flat
    assert runs[0][2]["form"] == N.FULL_PASS_GRID
    listed_possible = runs[0][1][0] != 0                      # (a grid of fewer than 7 thetas has no common pre-pass: nothing is listed)
    for (rec, gp, last), g in zip(runs[1:], (1, 3)):
        assert rec == runs[0][0] and gp == runs[0][1], (g, rec, runs[0][0])
        assert last["form"] == (N.FULL_PASS_LISTED if listed_possible else N.FULL_PASS_GRID)
        if listed_possible:
            assert last["workgroups"] == min(g, r.op.n_th)


# ================================================================================================================== pipeline batches
def _record_fields(res, f):
    """every field of frame f's record as bytes, but grid_ties, and the flags without ILCC_FLAG_TIE_OVERFLOW"""
    out = _fields(res[f])
    out["flags"] = int(np.frombuffer(out["flags"], np.int32)[0]) & ~N.FLAG_TIE_OVERFLOW
    return out


DEG = np.pi / 180.0
# 3 degree steps over the default +-30: three groups of 7 thetas, 18 degrees from first to last.  Over such a span the images of every
# sampled rim point lie more than half a square apart, the common pre-pass leaves them all out, its bound is 0 and no tile is
# rejected: EVERY group of a searched frame is alive -- the loose case.
COARSE = dict(n_th=21, th_step=3.0 * DEG, th_min=-30.0 * DEG)


def _two_groups(start_deg):
    """14 thetas one degree apart from start_deg on: two groups of 7"""
    return dict(n_th=14, th_min=start_deg * DEG)


def _handle(max_frames, n_points, reserve, fields=None):
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(max_frames, n_points, _nparams(fields))
    if reserve:
        e.reserve(2048, 4096)   # every frame's labelled points staged in LDS from the first batch on
    return e


def _submit(e, clouds, clicks):
    clouds, clicks = np.ascontiguousarray(clouds, np.float32), np.ascontiguousarray(clicks, np.float32)
    return e.submit_host(clouds.ctypes.data, len(clicks), clouds.shape[1], clicks.ctypes.data), (clouds, clicks)


def _run(clouds, clicks, mode, g=0, reserve=True, fields=None):
    """one batch through submit / wait on a fresh handle with the form forced -> (records, what the handle says about the launch)"""
    e = _handle(len(clicks), clouds.shape[1], reserve, fields)
    try:
        e.debug_full_pass_launch(mode, g)
        ticket, keep = _submit(e, clouds, clicks)
        res = e.wait(ticket)
        del keep
        return [_record_fields(res, f) for f in range(len(clicks))], e.debug_full_pass_last(), res
    finally:
        e.close()


def _live_groups(cloud, click, fields=None):
    """the theta groups of the frame that the common pre-pass leaves alive (state != 0), as a one-frame batch runs it"""
    e = _handle(1, len(cloud), True, fields)
    try:
        res = e.extract(cloud[None], click[None])
        gp = e.fetch_group_prepass()
        return int(res[0].status), int((gp["states"] != 0).sum()), int(gp["groups"])
    finally:
        e.close()


@pytest.fixture(scope="module")
def batch15():
    """15 synthetic VLP-16 frames: eight of make_batch at 2 - 3 m (boards of more than 1024 labelled points among them), the six
    fixture poses without range noise or beam footprint, and a copy of the first with its click 100 m from every point"""
    from lidar_camera_calibration_amd import synth
    clouds, clicks, _, _ = synth.make_batch(8, seed=0x11571ED, range_m=(2.0, 3.0))
    board, lidar = synth.Board(), synth.vlp16()
    clean = [synth.make_frame(lidar, board, synth.pose_from_fixture(k), 0xC1EA + k, sigma_r=0.0, footprint=0.0) for k in range(6)]
    clean_clicks = [synth.make_click(synth.pose_from_fixture(k), 0xC1EA + k) for k in range(6)]
    clouds = np.concatenate([clouds, np.stack(clean), clouds[:1]])
    clicks = np.concatenate([clicks, np.stack(clean_clicks), clicks[:1] + np.float32(100.0)]).astype(np.float32)
    return clouds, clicks


def _one_live_group(clouds, clicks):
    """a window of two theta groups in which the common pre-pass leaves a clean frame exactly ONE live group: the window is moved a
    degree at a time until the frame's minimum sits in one group and the other dies -> (fields, frame, what was seen)"""
    seen = []
    for f in (11, 12, 9):                 # clean frames (on the default grid the pre-pass leaves two of them 2 of 9 groups)
        for start in range(-12, 0):
            fields = _two_groups(start)
            st, n, groups = _live_groups(clouds[f], clicks[f], fields)
            seen.append((f, start, st, n))
            if st in SOLVED and groups == 2 and n == 1:
                return fields, f, seen
    return None, None, seen


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["default", "coarse", "two_groups"])
def test_small_batches_equal_in_every_form(batch15, grid):
    """The batch through submit / wait with the (n_th, F) grid and with the listed launch at G = 1, 7, n_th and n_th x F: identical
    records.  It holds a frame that is not ILCC_OK before K6 (its records are the pre-pass's).  On the default grid (61 thetas one
    degree apart) the pre-pass leaves every frame 2 to 4 of its 9 groups; on the coarse one every group is alive; and on a window of
    two groups, placed for it, the batch holds a frame whose groups all die but one."""
    clouds, clicks = batch15
    fields, n_th = None, N_TH
    if grid == "coarse":
        fields, n_th = COARSE, 21
    if grid == "two_groups":
        fields, frame, seen = _one_live_group(clouds, clicks)
        print("(frame, window start in degrees, status, live groups) tried:", seen)
        assert fields is not None, seen
        n_th = 14
    F = len(clicks)
    base, last, res = _run(clouds, clicks, N.FULL_PASS_GRID, fields=fields)
    assert last["form"] == N.FULL_PASS_GRID and last["frames"] == F
    assert res[F - 1].status == N.NO_ROI_POINTS
    solved = sum(res[f].status in SOLVED for f in range(F))
    assert solved >= F - 3
    # the live count the batch reports: per searched frame its live groups' thetas, nothing for the frame that left the chain
    print("grid %s: the batch lists %d of %d workgroups" % (grid, last["live"], n_th * F))
    assert 0 < last["live"] <= n_th * (F - 1)
    assert (last["live"] == n_th * solved) == (grid == "coarse")
    for g in (1, 7, n_th, n_th * F):
        got, last_g, _ = _run(clouds, clicks, N.FULL_PASS_LISTED, g, fields=fields)
        assert last_g["form"] == N.FULL_PASS_LISTED and last_g["workgroups"] == g and last_g["live"] == last["live"]
        assert got == base, g


@pytest.mark.gpu
def test_overflow_form_beside_staged_frames(batch15):
    """The same batch on a handle left at its first staging capacity (1024 points): the frames with more labelled points take the full
    pass's OVERFLOW form beside staged ones in one launch.  Listed (G = 7 and one per record) == the (n_th, F) grid == the batch
    with every frame staged."""
    clouds, clicks = batch15
    F = len(clicks)
    base, _, res = _run(clouds, clicks, N.FULL_PASS_GRID, reserve=False)
    lab = [res[f].n_black + res[f].n_white for f in range(F) if res[f].status in SOLVED]
    print("labelled points per solved frame:", lab)
    assert max(lab) > 1024 and min(lab) <= 1024
    for g in (7, N_TH * F):
        got, last, _ = _run(clouds, clicks, N.FULL_PASS_LISTED, g, reserve=False)
        assert last["form"] == N.FULL_PASS_LISTED
        assert got == base, g
    staged, _, _ = _run(clouds, clicks, N.FULL_PASS_GRID)
    assert staged == base


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["synchronous", "tickets"])
def test_slot_reuse_leaves_nothing_of_the_first_list(batch15, path):
    """ONE slot, on the coarse grid, where the bound the pre-pass tests against is loose and every group of a searched frame is
    alive: a batch of 9 frames lists 9 x n_th items on slot 0; then a batch of 2 frames on the SAME slot -- the same list buffer and
    the same batch words, reset by K1 alone.  The second batch's records and live count equal those of a fresh handle: nothing of
    the first list or count survives.  synchronous: two extract calls (always slot 0).  tickets: submit / wait takes the four slots
    in turn, so three one-frame batches go in between and the 2-frame batch comes round to slot 0."""
    clouds, clicks = batch15
    fresh, fresh_last, _ = _run(clouds[9:11], clicks[9:11], N.FULL_PASS_LISTED, 5, fields=COARSE)
    e = _handle(9, clouds.shape[1], True, COARSE)
    try:
        e.debug_full_pass_launch(N.FULL_PASS_LISTED, 5)
        if path == "synchronous":
            first = e.extract(clouds[:9], clicks[:9])
            live_first = e.debug_full_pass_last()["live"]
            second = e.extract(clouds[9:11], clicks[9:11])
        else:
            t, keep = _submit(e, clouds[:9], clicks[:9])
            assert t[0] == 0
            first = e.wait(t)
            live_first = e.debug_full_pass_last()["live"]
            for k in (1, 2, 3):
                t, keep = _submit(e, clouds[k:k + 1], clicks[k:k + 1])
                assert t[0] == k
                e.wait(t)
            t, keep = _submit(e, clouds[9:11], clicks[9:11])
            assert t[0] == 0                                   # the slot of the 9-frame batch
            second = e.wait(t)
        live_second = e.debug_full_pass_last()
    finally:
        e.close()
    searched = sum(first[f].status in SOLVED for f in range(9))
    print("live workgroups: first batch %d of %d (%d frames searched), second %d of %d" % (live_first, 21 * 9, searched, live_second["live"], 21 * 2))
    assert searched >= 7 and live_first == 21 * searched
    assert live_second["frames"] == 2 and live_second["live"] == fresh_last["live"] <= 21 * 2
    assert [_record_fields(second, f) for f in range(2)] == fresh


def _expected_g(history, n_th, frames):
    """the workgroups the handle's rule gives a batch of `frames` after the completed batches `history` = [(live, frames), ...]
    (at most the last 8): the largest live count per frame, kept in 1/65536 and rounded up both ways, through the rule"""
    rate = max(((live << 16) + n - 1) // n for live, n in history[-8:])
    return _rule((rate * frames + 65535) >> 16, n_th, frames)


@pytest.mark.gpu
def test_two_batches_in_flight_equal_their_solo_runs(batch15):
    """Two batches of different frame counts in flight on one handle, each with its own list and count: each one's records equal
    its solo run.  Then the rule on the same handle: its form and workgroups are what the completed batches' live counts give, the
    history is dropped by ilcc_set_params, and a handle with no completed batch keeps the (n_th, F) grid."""
    clouds, clicks = batch15
    a, b = slice(0, 7), slice(7, 12)
    solo_a, _, _ = _run(clouds[a], clicks[a], N.FULL_PASS_GRID)
    solo_b, _, _ = _run(clouds[b], clicks[b], N.FULL_PASS_GRID)
    e = _handle(7, clouds.shape[1], True)
    try:
        # the rule with no history: both batches are enqueued before either has come back
        ta, keep_a = _submit(e, clouds[a], clicks[a])
        assert e.debug_full_pass_last()["form"] == N.FULL_PASS_GRID
        tb, keep_b = _submit(e, clouds[b], clicks[b])
        assert e.debug_full_pass_last()["form"] == N.FULL_PASS_GRID
        ra, rb = e.wait(ta), e.wait(tb)
        assert [_record_fields(ra, f) for f in range(7)] == solo_a
        assert [_record_fields(rb, f) for f in range(5)] == solo_b
        e.debug_full_pass_launch(N.FULL_PASS_LISTED, 16)
        ta, keep_a = _submit(e, clouds[a], clicks[a])
        tb, keep_b = _submit(e, clouds[b], clicks[b])
        ra = e.wait(ta)
        live_a = e.debug_full_pass_last()["live"]
        rb = e.wait(tb)
        live_b = e.debug_full_pass_last()["live"]
        assert [_record_fields(ra, f) for f in range(7)] == solo_a
        assert [_record_fields(rb, f) for f in range(5)] == solo_b
        # ... and under the rule, which has four completed batches to go by now (two of each)
        history = [(live_a, 7), (live_b, 5), (live_a, 7), (live_b, 5)]
        e.debug_full_pass_launch(N.FULL_PASS_RULE)
        ta, keep_a = _submit(e, clouds[a], clicks[a])
        ra = e.wait(ta)
        last = e.debug_full_pass_last()
        assert [_record_fields(ra, f) for f in range(7)] == solo_a
        assert (last["form"], last["workgroups"]) == _expected_g(history, N_TH, 7)
        print("rule after %s: form %d, %d workgroups for %d live of %d" % (history, last["form"], last["workgroups"], last["live"], N_TH * 7))
        assert last["live"] == live_a <= last["workgroups"] <= N_TH * 7
        e.set_params(_nparams())                               # the history goes with the parameters
        ta, keep_a = _submit(e, clouds[a], clicks[a])
        assert e.debug_full_pass_last()["form"] == N.FULL_PASS_GRID
        ra = e.wait(ta)
        assert [_record_fields(ra, f) for f in range(7)] == solo_a
    finally:
        e.close()


@pytest.mark.gpu
def test_rule_takes_the_listed_form_once_a_batch_has_completed(batch15):
    """A fresh handle under the rule: the first batch has no history and takes the (n_th, F) grid; the same batch again takes the
    listed launch with the workgroups its own live count gives; the records are the same."""
    clouds, clicks = batch15
    F = len(clicks)
    e = _handle(F, clouds.shape[1], True)
    try:
        first = e.extract(clouds, clicks)
        one = e.debug_full_pass_last()
        second = e.extract(clouds, clicks)
        two = e.debug_full_pass_last()
    finally:
        e.close()
    assert one["form"] == N.FULL_PASS_GRID and one["workgroups"] == N_TH * F and one["frames"] == F
    assert (two["form"], two["workgroups"]) == _expected_g([(one["live"], F)], N_TH, F)
    assert two["form"] == N.FULL_PASS_LISTED and two["live"] == one["live"] <= two["workgroups"] < N_TH * F
    assert [_record_fields(second, f) for f in range(F)] == [_record_fields(first, f) for f in range(F)]
