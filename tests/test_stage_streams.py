"""A handle's batches share its three streams: each batch runs whole on the next one in turn, a GRID batch's full pass waits
for the previous one's on another stream, and a wait synchronises on the batch's own last event.  With several batches in flight, every one of them must return exactly
what a synchronous call on the same input returns -- which fails if a slot is reused while a stream still reads it, or a wait
returns before the batch's last kernel has run."""

import numpy as np
import pytest

from lidar_camera_calibration_amd import LidarCornersBatch, synth
from lidar_camera_calibration_amd import _native as N

pytestmark = pytest.mark.gpu

F = 512          # frames per GRID batch: enough for the fused k6_locate launch, as in the bench
NPTS = 28800
DEPTH = 4


@pytest.fixture(scope="module")
def inputs():
    """four distinct seeded batches, their synchronous full records and their compact records with one batch in flight"""
    sets = []
    for k in range(4):
        clouds, clicks, _, _ = synth.make_batch(F, seed=0x5EED + 97 * k)
        sets.append((np.ascontiguousarray(clouds), np.ascontiguousarray(clicks)))
    e = LidarCornersBatch(F, NPTS, N.default_params())
    e.reserve(1792, 2560)
    full = [_record_bytes(e.extract(c, k)) for c, k in sets]
    e.close()
    import torch
    dev = torch.device("cuda", 0)
    e = LidarCornersBatch(F, NPTS, N.default_params())
    e.reserve(1792, 2560)
    e.set_result_mode(N.RESULTS_COMPACT)
    compact = []
    for c, k in sets:
        dc, dk = torch.from_numpy(c).to(dev), torch.from_numpy(k).to(dev)
        torch.cuda.synchronize()
        compact.append(e.wait_compact(e.submit_device(dc.data_ptr(), F, NPTS, dk.data_ptr())).tobytes())
    e.close()
    return sets, full, compact


def _record_bytes(rows):
    """the full records' bytes, grid_ties left out: how many candidates the full pass LISTED as near ties depends on how far the
    frame's bound had come down when each tile completed (test_gpu_parity.py says the same); K7r re-ranks them exactly, so
    every other field, the corners among them, is deterministic"""
    out = []
    for r in rows:
        c = N.Result.from_buffer_copy(r)
        c.grid_ties = 0
        out.append(bytes(c))
    return out


def _pipelined_handle():
    e = LidarCornersBatch(F, NPTS, N.default_params())
    e.reserve(1792, 2560)
    e.set_result_mode(N.RESULTS_COMPACT)
    return e


def _submit_mixed(e, sets, d_sets, h_sets, n):
    """batch n: input n mod 4, device inputs for even n, pinned host inputs for odd n"""
    i = n % len(sets)
    if n % 2 == 0:
        dc, dk = d_sets[i]
        return e.submit_device(dc.data_ptr(), F, NPTS, dk.data_ptr()), i
    hc, hk = h_sets[i]
    return e.submit_host(hc.data_ptr(), F, NPTS, hk.data_ptr()), i


def _staged(sets):
    import torch
    dev = torch.device("cuda", 0)
    d_sets = [(torch.from_numpy(c).to(dev), torch.from_numpy(k).to(dev)) for c, k in sets]
    h_sets = [(torch.from_numpy(c).pin_memory(), torch.from_numpy(k).pin_memory()) for c, k in sets]
    torch.cuda.synchronize()
    return d_sets, h_sets


def test_twelve_grid_batches_at_depth_four_equal_the_synchronous_calls(inputs):
    """12 GRID batches, 4 in flight, over 4 inputs, device and pinned-host submits alternating: every batch's compact records
    (ilcc_wait_compact) and full records (ilcc_fetch_results, copied from HBM after the wait) are byte-identical to those of a
    call with nothing else in flight."""
    sets, full, compact = inputs
    d_sets, h_sets = _staged(sets)
    e = _pipelined_handle()
    inflight, done = [], 0

    def check_oldest():
        (ticket, i) = inflight.pop(0)
        got = e.wait_compact(ticket)
        assert got.tobytes() == compact[i], "batch %d (input %d): compact records differ" % (done, i)
        rows = e.fetch_results(0, F)
        assert _record_bytes(rows) == full[i], "batch %d (input %d): full records differ" % (done, i)

    for n in range(12):
        inflight.append(_submit_mixed(e, sets, d_sets, h_sets, n))
        if len(inflight) == DEPTH:
            check_oldest()
            done += 1
    while inflight:
        check_oldest()
        done += 1
    assert done == 12
    e.close()


def test_device_records_of_the_pipeline_equal_the_compact_records(inputs):
    """The same pipeline waited for through ilcc_wait_records_device (the multi-GPU path: K9 packs into caller memory at wait
    time): the device records equal ilcc_wait_compact's of the same input."""
    import torch
    sets, _, compact = inputs
    d_sets, h_sets = _staged(sets)
    e = _pipelined_handle()
    width = len(compact[0]) // (4 * F)
    n_corners = (width - N.RECORD_HEADER) // 3
    bufs = [torch.full((F, width), -1.0, dtype=torch.float32, device="cuda") for _ in range(DEPTH)]
    inflight = []

    def check_oldest(n):
        (ticket, i) = inflight.pop(0)
        buf = bufs[n % DEPTH]
        e.wait(ticket, buf.data_ptr(), n_corners, tag_base=0, want_results=False)
        assert buf.cpu().numpy().tobytes() == compact[i], "batch %d (input %d): device records differ" % (n, i)

    waited = 0
    for n in range(12):
        inflight.append(_submit_mixed(e, sets, d_sets, h_sets, n))
        if len(inflight) == DEPTH:
            check_oldest(waited)
            waited += 1
    while inflight:
        check_oldest(waited)
        waited += 1
    e.close()


def test_grid_batch_and_online_call_in_flight_together():
    """A GRID batch and an online by-point call in flight on one handle, on different streams, in both orders: each returns
    its synchronous result."""
    import torch
    clouds, clicks, _, poses = synth.make_batch(24, seed=0xA11CE)
    clouds = np.ascontiguousarray(clouds)
    pts = np.stack([(p.centre + [0.03, -0.04, 0.02]) for p in poses]).astype(np.float32)
    p = N.default_params()
    e = LidarCornersBatch(24, NPTS, p)
    want_grid = _record_bytes(e.extract(clouds, clicks))
    online = e.chessboard_by_point(clouds, pts)
    assert sum(1 for r in online if r.status == 0) >= 12
    want_online = [bytes(r) for r in online]
    hc, hk, hp = (torch.from_numpy(a).pin_memory() for a in (clouds, np.ascontiguousarray(clicks), pts))
    for grid_first in (True, False):
        if grid_first:
            tg = e.submit_host(hc.data_ptr(), 24, NPTS, hk.data_ptr())
            to = e.submit_chessboard_by_point(hc.data_ptr(), 24, NPTS, hp.data_ptr())
        else:
            to = e.submit_chessboard_by_point(hc.data_ptr(), 24, NPTS, hp.data_ptr())
            tg = e.submit_host(hc.data_ptr(), 24, NPTS, hk.data_ptr())
        first, second = (tg, to) if grid_first else (to, tg)
        for t in (first, second):
            if t is tg:
                assert _record_bytes(e.wait(tg)) == want_grid, grid_first
            else:
                assert [bytes(r) for r in e.wait_chessboard_by_point(to)] == want_online, grid_first
    e.close()


def test_reference_local_four_in_flight_equal_the_synchronous_calls():
    """REFERENCE_LOCAL batches run whole, each on the next of the three streams: four in flight equal four synchronous calls."""
    import torch
    p = N.default_params()
    p.solver = N.SOLVER_REFERENCE_LOCAL
    e = LidarCornersBatch(16, NPTS, p)
    sets = []
    for k in range(4):
        clouds, clicks, _, _ = synth.make_batch(16, seed=0x10CA1 + k)
        sets.append((np.ascontiguousarray(clouds), np.ascontiguousarray(clicks)))
    want = [[bytes(r) for r in e.extract(c, k)] for c, k in sets]
    dev = torch.device("cuda", 0)
    d_sets = [(torch.from_numpy(c).to(dev), torch.from_numpy(k).to(dev)) for c, k in sets]
    torch.cuda.synchronize()
    for rounds in range(2):
        tickets = [e.submit_device(dc.data_ptr(), 16, NPTS, dk.data_ptr()) for dc, dk in d_sets]
        for i, t in enumerate(tickets):
            assert [bytes(r) for r in e.wait(t)] == want[i], (rounds, i)
    e.close()
