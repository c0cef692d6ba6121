"""Corners from every scan of a bag on the GPU (include/ilcc_sequence.h; pytest -m gpu): K0b against the numpy unpack and
against K0 message by message, byte for byte, and the chain bag -> per-scan records -> fused corners against
ilcc_extract_batch, the restated fusion (tests/sequence_ref.py) and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import rosbag_writer as W
import sequence_cases as K
import sequence_ref as R
from lidar_camera_calibration_amd import LidarCornersBatch, ingest, sequence, synth
from lidar_camera_calibration_amd import _native as N

pytestmark = pytest.mark.gpu

F32 = W.FLOAT32
GUARD = 64


def _msg(rng, n, step, fields, **kw):
    """n points of random bytes (every bit pattern, NaNs included) in the given layout"""
    raw = rng.integers(0, 256, (n, step), dtype=np.uint8)
    return W.pointcloud2(raw, fields, step, **kw)


XYZI16 = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1)]
VELO = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 16, F32, 1), ("ring", 20, W.UINT16, 1)]


def _mixed_batch():
    """-> [(message, alignment of its data[] inside the blob)]: every layout class, every path, the tile borders"""
    rng = np.random.Generator(np.random.Philox(key=0xB0B))
    return [
        (_msg(rng, 0, 32, VELO), 16),                                                      # empty, first
        (_msg(rng, 1, 16, XYZI16), 16),                                                    # tiled 16
        (_msg(rng, 1023, 32, VELO), 16),                                                   # tiled 32, one short of a tile
        (_msg(rng, 1024, 48, [("intensity", 44, F32, 1), ("z", 0, F32, 1), ("y", 20, F32, 1), ("x", 24, F32, 1)]), 16),   # tiled 48, one tile
        (_msg(rng, 1025, 64, [("x", 60, F32, 1), ("y", 32, F32, 1), ("z", 4, F32, 1), ("intensity", 8, F32, 1)]), 16),    # tiled 64, a tile and a point
        (_msg(rng, 2049, 32, VELO), 16),                                                   # tiled 32, three tiles
        (_msg(rng, 0, 20, VELO[:4]), 16),                                                  # empty in the middle
        (_msg(rng, 1025, 20, [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 16, F32, 1)]), 16),     # generic: step 20
        (_msg(rng, 2049, 80, [("x", 72, F32, 1), ("y", 4, F32, 1), ("z", 40, F32, 1), ("intensity", 76, F32, 1)]), 16),   # generic: step 80
        (_msg(rng, 300, 32, [("x", 2, F32, 1), ("y", 6, F32, 1), ("z", 10, F32, 1), ("intensity", 17, F32, 1)]), 16),     # generic: odd field offsets
        (_msg(rng, 1024, 16, XYZI16[:3]), 16),                                             # tiled 16, intensity absent
        (_msg(rng, 4 * 257, 32, VELO, height=4, row_pad=8), 16),                           # generic: padded rows
        (_msg(rng, 2 * 600, 32, VELO, height=2), 16),                                      # tiled 32: packed rows
        (_msg(rng, 1030, 32, VELO), 4),                                                    # generic: source not 16-byte aligned
        (_msg(rng, 0, 16, XYZI16), 16),                                                    # empty, last
    ]


class Device:
    """a blob, its layouts, and two guarded outputs in device memory"""

    def __init__(self, batch, spare_points=0):
        import torch
        self.torch = torch
        self.layouts = [ingest.parse_pointcloud2(m) for m, _ in batch]
        self.src, at, parts = [], 0, []
        for (m, align), lay in zip(batch, self.layouts):
            at = (at + 15) // 16 * 16 + (align % 16)
            self.src.append(at)
            parts.append((at, m[lay.data_offset:lay.data_offset + lay.data_bytes]))
            at += lay.data_bytes
        blob = np.full(max(at, 16), 0x5A, np.uint8)
        for o, d in parts:
            blob[o:o + len(d)] = np.frombuffer(d, np.uint8)
        self.blob_bytes = at
        self.d_blob = torch.from_numpy(blob).cuda()
        self.want = np.concatenate([R.unpack(m) for m, _ in batch]) if batch else np.zeros((0, 4), np.float32)
        self.points = len(self.want)
        self.cap = self.points + spare_points
        self.out = torch.full((16 * self.cap + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
        self.out_k0 = torch.full((16 * self.cap + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def host(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    def untouched(self):
        return bool((self.host(self.out) == 0xCD).all())


def _check_batch(batch, want_launches, plan=None):
    """plan: the caller's own (left open); without one, a plan of exactly the batch's size"""
    d = Device(batch)
    own = plan is None
    plan = sequence.UnpackPlan(max(1, len(batch))) if own else plan
    offsets = sequence.unpack_batch_device(d.d_blob.data_ptr(), d.blob_bytes, d.layouts, d.src, d.out.data_ptr(), d.cap, plan)
    assert plan.launches == want_launches
    assert list(offsets) == list(np.concatenate([[0], np.cumsum([lay.n_points for lay in d.layouts])]))
    got = d.host(d.out)
    assert got[:16 * d.points].tobytes() == d.want.tobytes()                 # the numpy unpack, byte for byte
    assert (got[16 * d.points:] == 0xCD).all()                                # nothing behind the last point
    for lay, src, off in zip(d.layouts, d.src, offsets):                      # K0, message by message
        ingest.unpack_device(d.d_blob.data_ptr() + src, lay, d.out_k0.data_ptr() + 16 * int(off))
    assert d.host(d.out_k0).tobytes() == got.tobytes()
    # the plan serves the next call: the same batch again into the same buffer
    d.out.fill_(0xCD)
    sequence.unpack_batch_device(d.d_blob.data_ptr(), d.blob_bytes, d.layouts, d.src, d.out.data_ptr(), d.cap, plan)
    assert d.host(d.out).tobytes() == got.tobytes()
    if own:
        plan.close()
    return d


def test_k0b_equals_numpy_and_k0_on_a_batch_of_every_layout():
    d = _check_batch(_mixed_batch(), 5)                                       # four tiled classes and the generic one: five launches for 15 messages
    assert d.points == 1 + 1023 + 1024 + 1025 + 2049 + 1025 + 2049 + 300 + 1024 + 1028 + 1200 + 1030


def test_k0b_on_one_message_and_on_empty_messages():
    rng = np.random.Generator(np.random.Philox(key=7))
    _check_batch([(_msg(rng, 1500, 32, VELO), 16)], 1)
    _check_batch([(_msg(rng, 0, 32, VELO), 16), (_msg(rng, 0, 20, VELO[:4]), 16), (_msg(rng, 0, 16, XYZI16), 4)], 0)


@pytest.mark.parametrize("name", list(K.UNPACK_BATCHES))
def test_k0b_on_batches_of_hundreds_of_messages(name):
    """Every kernel with 1, 2, 3, 256 and 257 entries over the batches; what each batch is, tests/test_sequence_cpu.py holds against
    the restated entry table.  The plan is of exactly the batch's size; batch a's is a multiple of 32 messages, so its entries
    start right behind the UnpackArgs, the others' behind padding."""
    batch = K.unpack_batch(name)
    d = _check_batch(batch, len(K.UNPACK_BATCHES[name]))                      # one launch per populated class
    assert d.d_blob.data_ptr() % 16 == 0                                      # a message's layout class depends on it
    assert d.points == K.unpack_table(batch)[1][-1]


def test_k0b_plan_larger_than_the_batch_then_a_small_batch_on_it():
    """Nothing of the larger table shows through the smaller one: 15 messages after 690-odd on the same plan."""
    big = K.unpack_batch("e")
    plan = sequence.UnpackPlan(len(big) + 37)
    _check_batch(big, 5, plan)
    _check_batch(_mixed_batch(), 5, plan)
    _check_batch(K.unpack_batch("f"), 4, plan)
    plan.close()


def test_k0b_refusals_launch_nothing_and_leave_the_output_untouched():
    batch = _mixed_batch()[:6]
    d = Device(batch, spare_points=8)
    plan = sequence.UnpackPlan(len(batch))
    offsets_before = np.full(len(batch) + 1, 77, np.uint64)

    def call(layouts=d.layouts, blob_bytes=d.blob_bytes, cap=d.cap, n=len(batch)):
        arr = (ingest.Layout * n)(*layouts[:n])
        src = np.asarray(d.src[:n], np.uint64)
        offs = offsets_before.copy()
        st = sequence.lib().ilcc_pointcloud2_unpack_batch_device(C.c_void_p(d.d_blob.data_ptr()), blob_bytes, arr, src.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                 n, C.c_void_p(d.out.data_ptr()), cap, offs.ctypes.data_as(C.POINTER(C.c_uint64)), plan._p, None)
        return st, N.lib().ilcc_last_error(None).decode(), offs

    big = [ingest.Layout.from_buffer_copy(lay) for lay in d.layouts]
    big[4].is_bigendian = 1
    for kwargs, status, text in (({"layouts": big}, N.BAD_ARGUMENT, "big-endian PointCloud2 is not supported"),
                                 ({"blob_bytes": d.blob_bytes - 1}, N.BAD_ARGUMENT, "runs past the blob"),
                                 ({"cap": d.points - 1}, N.CAPACITY, "more points than the output holds")):
        st, err, offs = call(**kwargs)
        assert st == status and text in err, (st, err)
        assert (offs == 77).all() and plan.launches == 0 and d.untouched()
    plan2 = sequence.UnpackPlan(len(batch) - 1)
    keep, plan = plan, plan2
    st, err, _ = call()
    assert st == N.BAD_ARGUMENT and "more messages than the plan holds" in err and d.untouched()
    plan = keep
    st, _, offs = call()                                                      # and the very same call, unrefused, works
    assert st == N.OK and offs[-1] == d.points and plan.launches == 4
    assert d.host(d.out)[:16 * d.points].tobytes() == d.want.tobytes()
    plan.close()
    plan2.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------
# bag index of the twelve scans (an empty cloud sits at 4, the ground-and-wall scan at 13)
BAG_INDEX = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]
SKIP = ("grid_ties", "corners")


def _same_record(got, want, where):
    for name, _ in N.Result._fields_:
        if name in SKIP:
            continue
        a, b = getattr(got, name), getattr(want, name)
        a, b = (list(a), list(b)) if hasattr(a, "__len__") else (a, b)
        assert a == b or (a != a and b != b), (where, name, a, b)
    assert got.corners_array().tobytes() == want.corners_array().tobytes(), where


def _accepted(r, n_corners):
    return r.status == N.OK and not (r.flags & N.FLAG_LOW_COVERAGE) and r.n_corners == n_corners


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the bag, its clouds, the click, a 16-frame handle, ilcc_extract_batch's records and the chain's result on it"""
    path = str(tmp_path_factory.mktemp("sequence") / "pose0.bag")
    clouds = K.write_sequence_bag(path)
    _, click, pose, board = K.sequence(0)
    est = LidarCornersBatch(16, max(len(c) for c in clouds))
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    want = est.extract(np.concatenate(clouds), np.tile(click, (len(clouds), 1)), offsets)
    res, scans = sequence.bag_corners_all_scans(est, path, K.TOPIC, click)
    yield dict(path=path, clouds=clouds, click=click, pose=pose, board=board, est=est, want=want, res=res, scans=scans)
    est.close()


def test_chain_records_equal_extract_batch_and_the_fusion_equals_its_restatement(chain):
    res, scans, board = chain["res"], chain["scans"], chain["board"]
    assert res.status == N.OK and res.n_scans == len(scans) == 14 and res.n_batches == 1
    assert list(res.click) == list(chain["click"])
    for k, sc in enumerate(scans):
        _same_record(sc.result, chain["want"][k], k)
        stamp = (100 + k // 10, (k % 10) * 100000000)                       # the writer gives a scan's header and its record the same time
        assert (sc.message, (sc.stamp_sec, sc.stamp_nsec), (sc.time_sec, sc.time_nsec)) == (k, stamp, stamp)
        assert bool(sc.accepted) == _accepted(sc.result, board.n_corners)
    assert scans[4].result.status != N.OK and scans[4].result.n_points == 0 and scans[13].result.status != N.OK
    a, b = board.w - 1, board.h - 1
    corners = np.stack([np.ctypeslib.as_array(sc.result.corners)[:3 * a * b].reshape(-1, 3) for sc in scans])
    want = R.fuse(corners, [sc.accepted for sc in scans], a, b, board.g / 2)
    assert (res.status, res.n_ok, res.n_used, res.ref_scan, res.n_corners) == (want.status, want.n_ok, want.n_used, want.ref_scan, want.n_corners)
    assert res.corners_array().tobytes() == want.corners.tobytes()           # bit for bit
    assert res.spread_max == want.spread_max and abs(res.spread_rms - want.spread_rms) <= 1e-12 * want.spread_rms
    assert [bool(sc.used) for sc in scans] == list(want.used)
    assert np.allclose([sc.distance for sc in scans], want.dist, rtol=1e-15, atol=0)


@pytest.mark.parametrize("solver", [N.SOLVER_GRID, N.SOLVER_REFERENCE_LOCAL])
def test_chain_uses_the_scans_the_oracle_uses_and_lands_on_its_fused_corners(chain, golden_dir, solver):
    """Both solver modes, each against the oracle in the same mode (as smoke() compares them).  The library's default is the grid
    solver; the oracle's default is the reference's local solve, and K.ORACLE_USED lists what that gives: it leaves out scan 1, which
    the local solve puts one square off and flags LOW_COVERAGE.  The grid solver places scan 1 correctly, on the GPU and in the oracle."""
    board = chain["board"]
    if solver == N.SOLVER_GRID:
        res, scans = chain["res"], chain["scans"]
    else:
        params = N.default_params()
        params.solver = solver
        est = LidarCornersBatch(16, max(len(c) for c in chain["clouds"]), params)
        res, scans = sequence.bag_corners_all_scans(est, chain["path"], K.TOPIC, chain["click"])
        est.close()
    corners, accepted = K.golden_oracle_sequence(golden_dir, solver)         # the oracle's corners of the twelve scans, computed once
    oracle = R.fuse(corners, accepted, board.w - 1, board.h - 1, board.g / 2)
    assert res.status == oracle.status == N.OK
    oracle_used = [BAG_INDEX[s] for s in np.flatnonzero(oracle.used)]
    if solver == N.SOLVER_REFERENCE_LOCAL:
        assert oracle_used == [BAG_INDEX[s] for s in K.ORACLE_USED[0]]
    else:
        assert oracle_used == [BAG_INDEX[s] for s in range(K.N_SCANS) if s not in K.SHIFTED]
    assert [k for k, sc in enumerate(scans) if sc.used] == oracle_used
    assert [k for k, sc in enumerate(scans) if sc.accepted] == [BAG_INDEX[s] for s in np.flatnonzero(accepted)]
    dev = synth.corner_error(res.corners_array(), oracle.corners, board)
    print("solver %d: fused GPU vs fused oracle %.3g m" % (solver, dev))
    assert dev < 1e-3                                                         # smoke()'s GPU-to-oracle bar


@pytest.mark.parametrize("mode", [sequence.SEED_AUTO, sequence.SEED_AUTO_PLANAR])
def test_chain_finds_its_own_seed(chain, mode):
    """ilcc_extract_auto accepts scan 0 of this sequence (rank 0; its board is the shifted one, so the seed sits a square from the
    other scans' board centre, well inside the ROI): its seed becomes the click of every scan, and the same scans are used."""
    from lidar_camera_calibration_amd import seed
    fn = seed.extract_auto if mode == sequence.SEED_AUTO else seed.extract_auto_planar
    first, seeds, ranks = fn(chain["est"], chain["clouds"][0])
    assert first[0].status == N.OK and ranks[0] == 0
    res, scans = sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, None, seed_mode=mode)
    assert res.status == N.OK and list(res.click) == list(seeds[0])
    assert [sc.used for sc in scans] == [sc.used for sc in chain["scans"]]
    assert [sc.accepted for sc in scans] == [sc.accepted for sc in chain["scans"]]
    assert synth.corner_error(res.corners_array(), chain["res"].corners_array(), chain["board"]) < 1e-3
    _same_record(scans[0].result, first[0], "scan 0 with its own seed")


def test_chain_first_and_stride_select_the_scans(chain):
    sp = sequence.default_sequence_params()
    sp.first, sp.stride = 2, 3
    res, scans = sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, chain["click"], sp=sp)
    assert [sc.message for sc in scans] == [2, 5, 8, 11] and res.n_scans == 4
    for sc in scans:
        _same_record(sc.result, chain["scans"][sc.message].result, sc.message)
    sp.max_scans = 2
    res, scans = sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, chain["click"], sp=sp)
    assert [sc.message for sc in scans] == [2, 5]
    sp.first = 14
    with pytest.raises(sequence.SequenceError) as e:
        sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, chain["click"], sp=sp)
    assert e.value.status == N.BAD_ARGUMENT


def _same_result(res, scans, chain):
    ref = chain["res"]
    assert (res.status, res.n_scans, res.n_ok, res.n_used, res.ref_scan, res.n_corners, res.spread_rms, res.spread_max) == \
        (ref.status, ref.n_scans, ref.n_ok, ref.n_used, ref.ref_scan, ref.n_corners, ref.spread_rms, ref.spread_max)
    assert res.corners_array().tobytes() == ref.corners_array().tobytes()
    for k, sc in enumerate(scans):
        _same_record(sc.result, chain["scans"][k].result, k)
        assert (sc.used, sc.accepted, sc.distance) == (chain["scans"][k].used, chain["scans"][k].accepted, chain["scans"][k].distance)


def test_chain_in_four_batches_gives_the_identical_result(chain):
    small = LidarCornersBatch(4, max(len(c) for c in chain["clouds"]))
    res, scans = sequence.bag_corners_all_scans(small, chain["path"], K.TOPIC, chain["click"])
    assert res.n_batches == 4                                                 # 14 scans, four frames per batch
    _same_result(res, scans, chain)
    small.close()
    # ... and so does a staging budget of two scans' bytes (seven batches of the 16-frame handle)
    sp = sequence.default_sequence_params()
    sp.staging_bytes = 2 * 32 * max(len(c) for c in chain["clouds"])
    res, scans = sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, chain["click"], sp=sp)
    assert res.n_batches >= 7
    _same_result(res, scans, chain)
    # a handle that cannot hold one scan
    tiny = LidarCornersBatch(4, 1000)
    with pytest.raises(sequence.SequenceError) as e:
        sequence.bag_corners_all_scans(tiny, chain["path"], K.TOPIC, chain["click"])
    assert e.value.status == N.CAPACITY
    tiny.close()


def test_chain_refuses_a_missing_click_and_an_unknown_mode(chain):
    for click, mode in ((None, sequence.SEED_CLICK), (chain["click"], 7)):
        with pytest.raises(sequence.SequenceError) as e:
            sequence.bag_corners_all_scans(chain["est"], chain["path"], K.TOPIC, click, seed_mode=mode)
        assert e.value.status == N.BAD_ARGUMENT
