"""k6_locate's anchor through ilcc_debug_locate: the record and the bound word it publishes, on constructed labelled frames.

The anchor scores one 4 x 4 tile at three thetas on EVERY labelled point of the frame.  A frame whose walk layout fits the handle's
LDS staging capacity is copied into the workgroup's LDS first and walked there; any other frame is walked through global memory,
several trips' loads in flight.  Both walks add, lane by lane, the same terms in the same order, so record and bound word must be
the same BITS whichever source a frame takes -- that is what lets the full pass behind them compute what it always did.

Frames: default board and grid.  The points are the labelled points of ONE synthetic 64-ring frame (synth), classified by K5w itself
(grid_solve + fetch_solve_walk on the pool: the class of a point depends on the point and the tables alone), so that a constructed
frame's interior-class count is known exactly: frames of M in SIZES with the pool's own mix; two of 1 792 points with the interior
count = 1 and = 3 (mod 4), where the class boundary falls inside a quad of the walk; one without any interior-class point.  A pool
of fewer points than a frame needs is topped up with copies of itself shifted by a millimetre.

What is asserted:
  1. a handle reserved at 2 048 points (every frame staged) and a fresh handle at its 1 024 (M = 1 025 and 1 792 through global
     memory) give the same records and bound words bit for bit, frame by frame; the frames of M <= 1 024 are the control;
  2. the record is a valid bound: its cost agrees with ilcc_grid_cost's volume at its flat index within kTieEps = 2e-5 relative (the
     project's allowance for two fp32 summation orders), is not below the volume's minimum (on these frames the anchor's candidate
     IS the volume's argmin, and its sum is the volume's own or a rounding above it: 0 to 8.8e-8 relative), and the bound word holds
     the cost's bits;
  3. 64 copies of each of 8 distinct frames in one 512-frame call give 64 identical records each.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from lidar_camera_calibration_amd import LidarCornersBatch, synth
from lidar_camera_calibration_amd import _native as N

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 7, 8, 9, 63, 64, 65, 255, 257, 1023, 1024, 1025, 1792)
BIG = 1792
TIE_EPS = 2e-5          # kTieEps
CAP_POINTS = 2048       # points per frame the handles hold
U8P, U32P, U64P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _params():
    p = N.default_params()
    p.solver = N.SOLVER_GRID
    return p


@functools.lru_cache(maxsize=None)
def _pool():
    """(interior-class points, their labels, border-class points, their labels) of one synthetic frame, as K5w classifies them"""
    lidar, board = synth.hdl64(), synth.Board()
    clouds, clicks, _, _ = synth.make_batch(2, lidar, board, seed=0xC0FFEE, range_m=(2.0, 2.4))
    est = LidarCornersBatch(2, lidar.n_points, _params(), device=0)
    res = est.extract(clouds, clicks)
    sets = [est.fetch_labelled(f) for f in range(2) if res[f].status == N.OK]
    assert sets, "no synthetic frame passed the front end"
    yz, lab = max(sets, key=lambda s: len(s[1]))
    yz, lab = yz.copy(), lab.copy()
    k = 1
    while len(lab) < 2 * BIG:   # top up with shifted copies
        yz = np.concatenate([yz, yz + np.float32(1e-3 * k)])
        lab = np.concatenate([lab, lab])
        k += 1
    yz, lab = yz[:8192], lab[:8192]
    est.grid_solve(yz, lab)
    wyz, wlab, n_in, _ = est.fetch_solve_walk()
    est.close()
    assert len(wlab) == len(lab)
    print("pool: %d labelled points, %d interior class" % (len(lab), n_in))
    assert n_in >= BIG // 2 + 4 and len(lab) - n_in >= BIG // 2, "the pool cannot fill the constructed frames"
    return wyz[:n_in].copy(), wlab[:n_in].copy(), wyz[n_in:].copy(), wlab[n_in:].copy()


def _spread(n_have, n_want):
    """n_want indices spread evenly over n_have"""
    return (np.arange(n_want, dtype=np.int64) * n_have) // max(n_want, 1)


def _frame(n_interior, n_border):
    iyz, ilab, byz, blab = _pool()
    a, b = _spread(len(ilab), n_interior), _spread(len(blab), n_border)
    yz = np.concatenate([iyz[a], byz[b]])
    lab = np.concatenate([ilab[a], blab[b]])
    # (interleaved: the frame's own order must not be the layout's)
    order = np.argsort((np.arange(len(lab), dtype=np.int64) * 7919) % max(len(lab), 1), kind="stable")
    return np.ascontiguousarray(yz[order], np.float32), np.ascontiguousarray(lab[order], np.uint8)


@functools.lru_cache(maxsize=None)
def _frames():
    """the 16 frames of the first call, then the frame without interior-class points; with each its interior-class count"""
    iyz, ilab, byz, blab = _pool()
    share = len(ilab) / float(len(ilab) + len(blab))
    out = []
    for m in SIZES:
        n_in = min(int(round(share * m)), m)
        out.append((_frame(n_in, m - n_in), n_in))
    half = (BIG // 2) & ~3
    for r in (1, 3):
        out.append((_frame(half + r, BIG - half - r), half + r))
    out.append((_frame(0, min(len(blab), 600)), 0))
    return out


def _locate(est, frames):
    counts = [len(lab) for _, lab in frames]
    offsets = np.zeros(len(frames) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    yz = np.ascontiguousarray(np.concatenate([a for a, _ in frames]), dtype=np.float32)
    lab = np.ascontiguousarray(np.concatenate([b for _, b in frames]), dtype=np.uint8)
    rec = np.zeros((len(frames), 4), dtype=np.uint32)
    bound = np.zeros(len(frames), dtype=np.uint32)
    st = est._lib.ilcc_debug_locate(est._h, N.fptr(yz), lab.ctypes.data_as(U8P), offsets.ctypes.data_as(U64P), len(frames),
                                    rec.ctypes.data_as(U32P), bound.ctypes.data_as(U32P))
    assert st == N.OK, est._err()
    return rec, bound


@pytest.fixture(scope="module")
def staged_run():
    """every frame walked from LDS: a handle reserved at 2 048 points.  -> (handle, records, bound words) of the 16 + 1 frames"""
    est = LidarCornersBatch(512, CAP_POINTS, _params(), device=0)
    est.reserve(CAP_POINTS, 0)
    frames = [f for f, _ in _frames()]
    r16, b16 = _locate(est, frames[:16])
    r1, b1 = _locate(est, frames[16:])
    yield est, np.concatenate([r16, r1]), np.concatenate([b16, b1])
    est.close()


def test_interior_counts_are_what_the_frames_were_built_for(staged_run):
    est, _, _ = staged_run
    for k in (14, 15, 16):
        (yz, lab), n_in = _frames()[k]
        est.grid_solve(yz, lab)
        _, wlab, got, _ = est.fetch_solve_walk()
        assert (len(wlab), got) == (len(lab), n_in)
    assert _frames()[14][1] % 4 == 1 and _frames()[15][1] % 4 == 3 and _frames()[16][1] == 0


def test_staged_and_global_walks_give_the_same_record(staged_run):
    _, rec_a, bound_a = staged_run
    est = LidarCornersBatch(32, CAP_POINTS, _params(), device=0)   # fresh: 1 024 points staged, M = 1 025 and 1 792 from global memory
    frames = [f for f, _ in _frames()]
    r16, b16 = _locate(est, frames[:16])
    r1, b1 = _locate(est, frames[16:])
    est.close()
    rec_b, bound_b = np.concatenate([r16, r1]), np.concatenate([b16, b1])
    for k, ((_, lab), n_in) in enumerate(_frames()):
        print("frame %2d: M %4d interior %4d  staged %s / %08x   capacity 1024 %s / %08x" %
              (k, len(lab), n_in, rec_a[k], bound_a[k], rec_b[k], bound_b[k]))
    assert (rec_a[:, 2] != 0xFFFFFFFF).all(), "a frame without a record"
    assert np.array_equal(rec_a, rec_b) and np.array_equal(bound_a, bound_b)


def test_the_record_is_a_valid_bound(staged_run):
    est, rec, bound = staged_run
    for k, ((yz, lab), _) in enumerate(_frames()):
        _, _, vol = est.grid_cost(yz, lab, want_volume=True)
        cost = float(rec[k, 0:1].view(np.float32)[0])
        flat, vmin = int(rec[k, 2]), float(vol.min())
        at = float(vol[flat])
        print("frame %2d: M %4d cost %.9g volume[flat] %.9g (rel %.2e) volume min %.9g (cost / min - 1 = %.2e)" %
              (k, len(lab), cost, at, abs(cost - at) / max(at, 1e-30), vmin, cost / max(vmin, 1e-30) - 1.0))
        assert abs(cost - at) <= TIE_EPS * at
        assert cost >= vmin
        assert bound[k] == rec[k, 0]
        p = est.params
        ab = int(rec[k, 3])
        assert (flat >> 1) % (p.n_ty * p.n_tz) == (ab >> 16) * p.n_tz + (ab & 0xFFFF)


def test_identical_frames_give_identical_records(staged_run):
    est, rec, bound = staged_run
    pick = [8, 9, 10, 11, 12, 13, 14, 7]   # M = 255, 257, 1 023, 1 024, 1 025, 1 792, 1 792 (interior = 1 mod 4), 65
    frames = [_frames()[k][0] for k in pick]
    r, b = _locate(est, frames * 64)
    r, b = r.reshape(64, 8, 4), b.reshape(64, 8)
    assert (r == r[0]).all() and (b == b[0]).all()
    # ... and the ones the 16-frame call gave
    assert np.array_equal(r[0], rec[pick]) and np.array_equal(b[0], bound[pick])


def test_refusals():
    (yz, lab), _ = _frames()[6]
    off2 = np.array([0, len(lab)], dtype=np.uint64)
    rec, bound = np.zeros(4 * 4, np.uint32), np.zeros(4, np.uint32)
    args = lambda off, n: (N.fptr(yz), lab.ctypes.data_as(U8P), off.ctypes.data_as(U64P), n, rec.ctypes.data_as(U32P), bound.ctypes.data_as(U32P))
    est = LidarCornersBatch(2, CAP_POINTS, _params(), device=0)
    assert est._lib.ilcc_debug_locate(est._h, *args(off2, 1)) == N.OK
    off4 = np.array([0, 0, 0, 0, len(lab)], dtype=np.uint64)
    assert est._lib.ilcc_debug_locate(est._h, *args(off4, 4)) == N.CAPACITY      # more frames than max_frames
    assert est._lib.ilcc_debug_locate(est._h, *args(off2, 1)[:4], None, bound.ctypes.data_as(U32P)) == N.BAD_ARGUMENT
    est.close()
    p = _params()
    p.solver = N.SOLVER_REFERENCE_LOCAL
    est = LidarCornersBatch(2, CAP_POINTS, p, device=0)
    assert est._lib.ilcc_debug_locate(est._h, *args(off2, 1)) == N.BAD_ARGUMENT   # not a GRID handle
    est.close()
