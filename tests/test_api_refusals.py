"""What the handle API refuses (pytest -m gpu): every call goes to the C ABI of libilcc_hip.so through ctypes, because
the Python wrappers intercept some of these cases themselves.

For every refusal: the status returned, a text behind ilcc_last_error, and that the handle still works afterwards --
batches in flight still deliver what the synchronous call delivers on the same input ((status, n_roi, n_cluster,
n_plane) per frame), and the next accepted submit returns the ticket it would have returned had the refused call
never happened.

Two kinds of refusal carry no text of their own and are checked for their status alone: the ilcc_fetch_cloud /
_classes / _labelled / _walk calls (their status is the negated return value), and ilcc_fetch_results before the
handle has completed any batch.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_camera_calibration_amd import synth
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd.sharding import pack_records

pytestmark = pytest.mark.gpu

F = 4
SLOTS = 4
U64P = C.POINTER(C.c_uint64)
U8P = C.POINTER(C.c_uint8)
REC_W = N.RECORD_HEADER + 3 * 35          # the default board: 5 x 7 corners


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _key(res, n):
    return [(res[f].status, res[f].n_roi, res[f].n_cluster, res[f].n_plane) for f in range(n)]


class Handle:
    """One ilcc handle and the ticket its next accepted submit must return."""

    def __init__(self, max_frames, max_points):
        self.L = N.lib()
        p = N.default_params()
        self.h = self.L.ilcc_create(-1, C.byref(p), max_frames, max_points)
        assert self.h, self.L.ilcc_last_error(None)
        self.next = 0

    def close(self):
        self.L.ilcc_destroy(self.h)
        self.h = None

    def err(self):
        return self.L.ilcc_last_error(self.h).decode()

    def refused(self, st, want):
        assert st == want, (st, self.err())
        assert self.err() != ""

    def busy(self, ticket):
        return self.L.ilcc_record_floats(self.h, ticket) != 0

    def submit(self, fn, xyzi, off, n_frames, clicks):
        """(status, ticket) of one of the three submits; xyzi / clicks are addresses"""
        t = C.c_int32(-1)
        st = fn(self.h, xyzi, off.ctypes.data_as(U64P), n_frames, clicks, C.byref(t))
        return st, t.value

    def accepted(self, fn, xyzi, off, n_frames, clicks):
        st, t = self.submit(fn, xyzi, off, n_frames, clicks)
        assert st == N.OK, self.err()
        assert t == self.next
        self.next = (t + 1) % SLOTS
        return t

    def wait(self, ticket, n_frames=F):
        res = (N.Result * n_frames)()
        st = self.L.ilcc_wait(self.h, ticket, res)
        assert st == N.OK, self.err()
        return _key(res, n_frames)

    def wait_by_point(self, ticket, n_frames=F):
        res = (N.Result * n_frames)()
        st = self.L.ilcc_wait_chessboard_by_point(self.h, ticket, 500, res)
        assert st == N.OK, self.err()
        return _key(res, n_frames)


class World:
    pass


@pytest.fixture(scope="module")
def w():
    """the handle of 4 frames, its input on the host and on the device, and what the synchronous calls deliver on it"""
    import torch
    w = World()
    clouds, clicks, gts, _ = synth.make_batch(F, seed=311)
    w.clouds = np.ascontiguousarray(clouds)
    w.clicks = np.ascontiguousarray(clicks)
    w.points = np.ascontiguousarray(gts.mean(axis=1), dtype=np.float32)
    w.n = clouds.shape[1]
    w.off = np.arange(F + 1, dtype=np.uint64) * np.uint64(w.n)
    dev = torch.device("cuda", 0)
    w.d_clouds = torch.from_numpy(w.clouds).to(dev)
    w.d_clicks = torch.from_numpy(w.clicks).to(dev)
    w.d_records = torch.zeros(F * (N.RECORD_HEADER + 3 * N.MAX_CORNERS), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    w.e = Handle(F, F * w.n)
    L, h = w.e.L, w.e.h
    res = (N.Result * F)()
    assert L.ilcc_extract_batch(h, N.fptr(w.clouds), w.off.ctypes.data_as(U64P), F, N.fptr(w.clicks), res) == N.OK
    w.ref = _key(res, F)
    w.ref_rec = pack_records(res, F, 35)          # what ilcc_wait_compact delivers for the same batch
    assert any(k[0] == N.OK for k in w.ref)
    assert L.ilcc_chessboard_by_point_batch(h, N.fptr(w.clouds), w.off.ctypes.data_as(U64P), F, N.fptr(w.points), 500, res) == N.OK
    w.ref_pt = _key(res, F)
    w.host = (L.ilcc_submit_batch, _vp(w.clouds), w.off, F, _vp(w.clicks))
    w.device = (L.ilcc_submit_batch_device, C.c_void_p(w.d_clouds.data_ptr()), w.off, F, C.c_void_p(w.d_clicks.data_ptr()))
    w.by_point = (L.ilcc_submit_chessboard_by_point, _vp(w.clouds), w.off, F, _vp(w.points))
    yield w
    w.e.close()


def _ticket0_in_flight(w):
    """a host batch in flight under ticket 0 (batches that come before it are waited for at once)"""
    while True:
        t = w.e.accepted(*w.host)
        if t == 0:
            return
        assert w.e.wait(t) == w.ref


def test_a_fifth_submit_is_refused_while_four_batches_are_in_flight(w):
    e = w.e
    kinds = [w.host, w.device, w.by_point, w.host]
    tickets = [e.accepted(*k) for k in kinds]
    for k in (w.host, w.device, w.by_point):
        st, _ = e.submit(*k)
        e.refused(st, N.CAPACITY)
    for k, t in zip(kinds, tickets):
        assert e.busy(t)
        if k is w.by_point:
            assert e.wait_by_point(t) == w.ref_pt
        else:
            assert e.wait(t) == w.ref
    assert e.wait(e.accepted(*w.device)) == w.ref


def test_synchronous_and_diagnostic_calls_are_refused_while_ticket_0_is_in_flight(w):
    e, L, h = w.e, w.e.L, w.e.h
    _ticket0_in_flight(w)
    res = (N.Result * F)()
    off = w.off.ctypes.data_as(U64P)
    yz = np.zeros((8, 2), np.float32)
    lab = np.zeros(8, np.uint8)
    labp = lab.ctypes.data_as(U8P)
    theta_t = (C.c_double * 3)(0.0, 0.0, 0.0)
    lat = (C.c_int32 * 3)(0, 0, 0)
    phase = C.c_int32(0)
    calls = [
        lambda: L.ilcc_extract_batch(h, N.fptr(w.clouds), off, F, N.fptr(w.clicks), res),
        lambda: L.ilcc_extract_batch_device(h, C.c_void_p(w.d_clouds.data_ptr()), off, F, C.c_void_p(w.d_clicks.data_ptr()), res),
        lambda: L.ilcc_extract(h, N.fptr(w.clouds), w.n, N.fptr(w.clicks), res),
        lambda: L.ilcc_chessboard_by_point_batch(h, N.fptr(w.clouds), off, F, N.fptr(w.points), 500, res),
        lambda: L.ilcc_grid_cost(h, N.fptr(yz), labp, 8, 1, None, None, None),
        lambda: L.ilcc_get_theta_t(h, N.fptr(yz), labp, 8, 0, 1, theta_t, None, None),
        lambda: L.ilcc_pattern_refine(h, N.fptr(yz), labp, 8, lat, C.byref(phase), None, None, None, None),
        lambda: L.ilcc_debug_reference_solve(h, N.fptr(yz), labp, (C.c_uint64 * 2)(0, 8), (C.c_int32 * 1)(0), 1, (C.c_double * 12)(),
                                             (C.c_int32 * 8)(), res, None),
        lambda: L.ilcc_debug_grid_solve_batch(h, N.fptr(yz), labp, (C.c_uint64 * 2)(0, 8), (C.c_int32 * 1)(0), 1, (C.c_double * 3)(),
                                              (C.c_int64 * 2)(), (C.c_int32 * 6)(), res, None),
    ]
    for call in calls:
        e.refused(call(), N.BAD_ARGUMENT)
        assert e.busy(0)
    assert "ticket 0 is in flight" in e.err()
    assert e.wait(0) == w.ref
    assert e.wait(e.accepted(*w.host)) == w.ref


def test_offsets_are_checked_before_a_slot_is_taken(w):
    e, L, h = w.e, w.e.L, w.e.h
    good = w.off
    not_from_0 = good.copy()
    not_from_0[0] = 1
    decreasing = good.copy()
    decreasing[2] = decreasing[1] - np.uint64(1)
    too_many_points = good.copy()
    too_many_points[F] += np.uint64(1)
    five = np.arange(F + 2, dtype=np.uint64) * np.uint64(16)
    cases = [(good, 0, N.BAD_ARGUMENT), (five, F + 1, N.CAPACITY), (not_from_0, F, N.BAD_ARGUMENT),
             (decreasing, F, N.BAD_ARGUMENT), (too_many_points, F, N.CAPACITY)]
    res = (N.Result * (F + 1))()
    for off, n_frames, want in cases:
        st, _ = e.submit(L.ilcc_submit_batch, _vp(w.clouds), off, n_frames, _vp(w.clicks))
        e.refused(st, want)
        assert not e.busy(e.next)
        st = L.ilcc_extract_batch(h, N.fptr(w.clouds), off.ctypes.data_as(U64P), n_frames, N.fptr(w.clicks), res)
        e.refused(st, want)
        assert not e.busy(0)
    assert e.wait(e.accepted(*w.host)) == w.ref
    assert L.ilcc_extract_batch(h, N.fptr(w.clouds), good.ctypes.data_as(U64P), F, N.fptr(w.clicks), res) == N.OK
    assert _key(res, F) == w.ref


def test_a_batch_too_ragged_for_the_chunk_table_is_refused_and_frees_its_slot(w):
    """max_frames = 8, max_total_points = 8 * 4096: the crop's chunk table holds 8 + 8 + 1 = 17 entries.  One frame of
    3 * 4096 points and seven of 16 need 3 chunks x 8 frames = 24."""
    e = Handle(8, 8 * 4096)
    sizes = [16, 16, 3 * 4096, 16, 16, 16, 16, 16]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    cloud = np.zeros((int(off[-1]), 4), np.float32)
    clicks = np.zeros((8, 3), np.float32)
    st, _ = e.submit(e.L.ilcc_submit_batch, _vp(cloud), off, 8, _vp(clicks))
    e.refused(st, N.CAPACITY)
    assert not e.busy(0)
    one = np.array([0, w.n], dtype=np.uint64)
    t = e.accepted(e.L.ilcc_submit_batch, _vp(w.clouds), one, 1, _vp(w.clicks))
    assert t == 0
    assert e.wait(t, 1) == w.ref[:1]
    e.close()


def test_a_wait_is_refused_for_a_ticket_that_holds_no_batch(w):
    e, L, h = w.e, w.e.L, w.e.h
    res = (N.Result * F)()
    rec = np.zeros(F * REC_W, np.float32)
    d_rec = C.c_void_p(w.d_records.data_ptr())
    t = e.accepted(*w.host)
    idle = (t + 1) % SLOTS
    assert L.ilcc_record_floats(h, idle) == 0 and L.ilcc_record_floats(h, -1) == 0 and L.ilcc_record_floats(h, SLOTS) == 0
    assert L.ilcc_record_floats(h, t) == REC_W
    for bad in (-1, SLOTS, idle):
        e.refused(L.ilcc_wait(h, bad, res), N.BAD_ARGUMENT)
        e.refused(L.ilcc_wait_compact(h, bad, N.fptr(rec), rec.size), N.BAD_ARGUMENT)
        e.refused(L.ilcc_wait_records_device(h, bad, res, d_rec, 35, 0), N.BAD_ARGUMENT)
        e.refused(L.ilcc_wait_chessboard_by_point(h, bad, 500, res), N.BAD_ARGUMENT)
    assert e.busy(t)
    # one float short: refused with both numbers in the text, the batch stays in flight
    e.refused(L.ilcc_wait_compact(h, t, N.fptr(rec), rec.size - 1), N.BAD_ARGUMENT)
    assert str(rec.size) in e.err() and str(rec.size - 1) in e.err()
    assert e.busy(t)
    assert L.ilcc_wait_compact(h, t, N.fptr(rec), rec.size) == N.OK, e.err()
    assert np.array_equal(rec.reshape(F, REC_W).view(np.uint32), w.ref_rec.view(np.uint32))
    assert not e.busy(t)
    # more corners than a record holds: refused, the batch stays in flight
    t = e.accepted(*w.device)
    e.refused(L.ilcc_wait_records_device(h, t, res, d_rec, N.MAX_CORNERS + 1, 0), N.BAD_ARGUMENT)
    assert e.busy(t)
    assert e.wait(t) == w.ref


def test_setters_are_refused_while_a_batch_is_in_flight(w):
    e, L, h = w.e, w.e.L, w.e.h
    p = N.default_params()
    setters = [lambda: L.ilcc_set_params(h, C.byref(p)), lambda: L.ilcc_reserve(h, 1, 1),
               lambda: L.ilcc_set_result_mode(h, N.RESULTS_FULL), lambda: L.ilcc_debug_separate_launches(h, 0)]
    t = e.accepted(*w.host)
    for s in setters:
        e.refused(s(), N.BAD_ARGUMENT)
        assert e.busy(t)
    assert e.wait(t) == w.ref
    for s in setters:
        assert s() == N.OK, e.err()
    assert e.wait(e.accepted(*w.host)) == w.ref


def test_fetches_are_refused_outside_the_last_completed_batch(w):
    L = w.e.L
    res = (N.Result * F)()
    buf = np.zeros((16, 4), np.float32)
    lab = np.zeros(16, np.uint8)
    counts = (C.c_uint32 * 2)()

    def fetches(h, frame):
        return [L.ilcc_fetch_cloud(h, frame, N.CLOUD_ROI, N.fptr(buf), 16), L.ilcc_fetch_classes(h, frame, lab.ctypes.data_as(U8P), 16),
                L.ilcc_fetch_labelled(h, frame, N.fptr(buf), lab.ctypes.data_as(U8P), 16),
                L.ilcc_fetch_walk(h, frame, N.fptr(buf), lab.ctypes.data_as(U8P), 16, counts)]

    fresh = Handle(F, F * w.n)           # before any batch
    assert L.ilcc_fetch_results(fresh.h, 0, 1, res) == N.BAD_ARGUMENT
    assert fetches(fresh.h, 0) == [-N.BAD_ARGUMENT] * 4
    st = L.ilcc_extract_batch(fresh.h, N.fptr(w.clouds), w.off.ctypes.data_as(U64P), F, N.fptr(w.clicks), res)
    assert st == N.OK and _key(res, F) == w.ref
    fresh.close()
    e, h = w.e, w.e.h
    assert L.ilcc_extract_batch(h, N.fptr(w.clouds), w.off.ctypes.data_as(U64P), F, N.fptr(w.clicks), res) == N.OK
    assert fetches(h, F) == [-N.BAD_ARGUMENT] * 4
    assert L.ilcc_fetch_cloud(h, 0, 99, N.fptr(buf), 16) == -N.BAD_ARGUMENT
    e.refused(L.ilcc_fetch_results(h, F - 1, 2, res), N.BAD_ARGUMENT)
    assert all(n >= 0 for n in fetches(h, F - 1))
    assert L.ilcc_fetch_results(h, 0, F, res) == N.OK and _key(res, F) == w.ref
    assert e.wait(e.accepted(*w.host)) == w.ref


def test_the_views_of_the_last_grid_solve_are_refused_while_a_batch_is_in_flight(w):
    """ilcc_debug_group_prepass / ilcc_debug_solve_walk read slot 0's buffers: refused (status and text) while any ticket is in
    flight, the batch undisturbed; afterwards they answer, and the next batch delivers what it always does."""
    e, L, h = w.e, w.e.L, w.e.h
    dims, bound, counts = (C.c_uint32 * 2)(), C.c_uint32(0), (C.c_uint32 * 2)()
    t = e.accepted(*w.host)
    e.refused(L.ilcc_debug_group_prepass(h, None, None, dims, C.byref(bound)), N.BAD_ARGUMENT)
    assert "with a batch in flight" in e.err() and e.busy(t)
    assert L.ilcc_debug_solve_walk(h, None, None, 0, counts) == -N.BAD_ARGUMENT
    assert "with a batch in flight" in e.err() and e.busy(t)
    assert e.wait(t) == w.ref
    assert L.ilcc_debug_group_prepass(h, None, None, None, None) == N.BAD_ARGUMENT        # no place for the sizes
    assert L.ilcc_debug_group_prepass(h, None, None, dims, C.byref(bound)) == N.OK, e.err()
    assert (dims[0], dims[1]) == (9, 4)        # the default grid: 61 thetas in groups of 7, 40 x 40 translations = 100 tiles of 4 x 4
    assert L.ilcc_debug_solve_walk(h, None, None, 0, counts) >= 0
    assert e.wait(e.accepted(*w.host)) == w.ref


def test_grid_solve_batch_refusals_launch_nothing():
    """ilcc_debug_grid_solve_batch refuses null pointers, offsets that do not describe a batch, more frames than max_frames, more
    points than the handle holds and a handle that is not in ILCC_SOLVER_GRID mode -- each with its status and a text, the outputs
    untouched and, on a handle that has run nothing yet, no full pass on record afterwards (ilcc_debug_full_pass_last: form 0);
    then the same handle accepts a good call.  (A busy ticket 0: with the other diagnostic entries above.)"""
    L = N.lib()
    I32P, I64P, F64P, U32P = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    FRAMES, POINTS = 3, 64
    yz = np.zeros((POINTS + 1, 2), np.float32)
    lab = np.zeros(POINTS + 1, np.uint8)
    status = np.zeros(FRAMES + 1, np.int32)
    d = np.full(3 * (FRAMES + 1), -7.0)
    q = np.full(2 * (FRAMES + 1), -7, np.int64)
    i = np.full(6 * (FRAMES + 1), -7, np.int32)
    res = (N.Result * (FRAMES + 1))()
    good = np.array([0, 16, 16, POINTS], np.uint64)

    def call(h, off, n_frames, **null):
        a = dict(yz=N.fptr(yz), lab=lab.ctypes.data_as(U8P), off=None if off is None else off.ctypes.data_as(U64P),
                 status=status.ctypes.data_as(I32P), d=d.ctypes.data_as(F64P), q=q.ctypes.data_as(I64P), i=i.ctypes.data_as(I32P), res=res)
        a.update({k: None for k in null})
        return L.ilcc_debug_grid_solve_batch(h, a["yz"], a["lab"], a["off"], a["status"], n_frames, a["d"], a["q"], a["i"], a["res"], None)

    def last_form(h):
        out = (C.c_uint32 * N.FULL_PASS_LAST_WORDS)()
        assert L.ilcc_debug_full_pass_last(h, out) == N.OK
        return out[0]

    e = Handle(FRAMES, POINTS)      # (the default parameters: ILCC_SOLVER_GRID)
    try:
        assert L.ilcc_debug_grid_solve_batch(None, None, None, None, None, 0, None, None, None, None, None) == N.BAD_ARGUMENT
        four = np.array([0, 16, 16, 32, POINTS], np.uint64)
        too_many_points = np.array([0, 16, 16, POINTS + 1], np.uint64)
        not_from_0 = np.array([1, 16, 16, POINTS], np.uint64)
        decreasing = np.array([0, 16, 15, POINTS], np.uint64)
        cases = [(good, FRAMES, dict(status=1), N.BAD_ARGUMENT), (good, FRAMES, dict(d=1), N.BAD_ARGUMENT), (good, FRAMES, dict(q=1), N.BAD_ARGUMENT),
                 (good, FRAMES, dict(i=1), N.BAD_ARGUMENT), (good, FRAMES, dict(res=1), N.BAD_ARGUMENT), (good, FRAMES, dict(yz=1), N.BAD_ARGUMENT),
                 (good, FRAMES, dict(lab=1), N.BAD_ARGUMENT), (None, FRAMES, {}, N.BAD_ARGUMENT), (good, 0, {}, N.BAD_ARGUMENT),
                 (four, FRAMES + 1, {}, N.CAPACITY), (too_many_points, FRAMES, {}, N.CAPACITY), (not_from_0, FRAMES, {}, N.BAD_ARGUMENT),
                 (decreasing, FRAMES, {}, N.BAD_ARGUMENT)]
        for off, n_frames, null, want in cases:
            e.refused(call(e.h, off, n_frames, **null), want)
            assert not e.busy(0) and last_form(e.h) == 0
        assert (d == -7.0).all() and (q == -7).all() and (i == -7).all() and all(res[f].status == 0 and res[f].grid_index == 0 for f in range(FRAMES + 1))
        assert call(e.h, good, FRAMES) == N.OK, e.err()
        assert last_form(e.h) != 0 and (i[:6 * FRAMES] != -7).all() and (i[6 * FRAMES:] == -7).all()
    finally:
        e.close()
    p = N.default_params()
    p.solver = N.SOLVER_REFERENCE_LOCAL
    h = L.ilcc_create(-1, C.byref(p), FRAMES, POINTS)
    assert h
    try:
        assert call(h, good, FRAMES) == N.BAD_ARGUMENT and b"ILCC_SOLVER_GRID" in L.ilcc_last_error(h)
        assert last_form(h) == 0
    finally:
        L.ilcc_destroy(h)
