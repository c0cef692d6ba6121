"""K15 on the GPU (pytest -m gpu): the integer component records of ilcc_debug_seed_components against the numpy restatement
(tests/seed_ref.py) -- keys, counts and all nine int64 moments, exactly -- on clouds constructed for every path of the kernels;
the host refusals; and the closed loop seeds -> ordinary pipeline -> accepted corners on 32 config-2 and 2 config-5 frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seed_cases as K   # noqa: E402
import seed_ref as R     # noqa: E402
from lidar_camera_calibration_amd import LidarCornersBatch, LidarCornersEst, synth   # noqa: E402
from lidar_camera_calibration_amd import _native as N   # noqa: E402
from lidar_camera_calibration_amd import seed as S      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_corners")
POINTS = 1 << 20


@pytest.fixture(scope="module")
def est():
    e = LidarCornersBatch(8, POINTS // 8, N.default_params())
    yield e
    e.close()


def native(sp: R.SeedParams, params=None) -> S.SeedParams:
    out = S.default_seed_params(params if params is not None else N.default_params())
    for name in ("cell", "range", "cluster_min", "max_components", "max_seeds", "board_w", "board_h", "grid_length", "max_rms",
                 "size_lo", "size_hi", "max_oob_share"):
        setattr(out, name, getattr(sp, name))
    return out


def check_records(est, cloud, sp, offsets=None, frame=0, frame_cloud=None, scratch=None):
    """the GPU's records of `frame` equal the restatement's, word for word"""
    st, got = S.debug_components(est, cloud, offsets, frame, native(sp), scratch)
    assert st == N.OK, est._err()
    want = R.components(frame_cloud if frame_cloud is not None else cloud, sp, R.grid(sp, POINTS))
    assert got.tolist() == want
    return want


def test_defaults_mirror_the_restatement():
    sp, ref = S.default_seed_params(N.default_params()), R.SeedParams()
    for name in ("cell", "range", "cluster_min", "max_components", "max_seeds", "board_w", "board_h", "grid_length", "max_rms",
                 "size_lo", "size_hi", "max_oob_share"):
        assert getattr(sp, name) == getattr(ref, name), name
    assert (S.RECORD_WORDS, S.GRID_MAX, S.TABLE_MIN) == (R.RECORD_WORDS, R.GRID_MAX, R.TABLE_MIN)


@pytest.mark.parametrize("step", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, 1, 1), (1, -1, 1), (-1, -1, -1)])
def test_adjacent_plates_join_and_plates_a_cell_apart_do_not(est, step):
    sp = K.small_params()
    assert [r[1] for r in check_records(est, K.two_plates(step, 1), sp)] == [50]
    assert [r[1] for r in check_records(est, K.two_plates(step, 2), sp)] == [25, 25]


def test_cell_borders_and_the_range_limit(est):
    recs = check_records(est, K.borders(), K.small_params())
    kept = sum(r[1] for r in recs)
    assert 0 < kept < len(K.borders())                      # the points one quantum beyond the range are dropped
    g = K.G
    for q, n in ((g.range_q, 1), (g.range_q + 1, 0)):
        for sign in (1, -1):
            got = check_records(est, K.cloud_of([[sign * q, 0, 0], [0, sign * q, 0], [0, 0, sign * q]]), K.small_params())
            assert sum(r[1] for r in got) == 3 * n


def test_negative_coordinates_on_every_axis(est):
    cloud = K.random_box(700, 1, -1.0, 1.0)
    assert (cloud[:, :3] < 0).any(0).all()
    check_records(est, cloud, K.small_params())
    check_records(est, K.random_box(900, 2, -3.0, -0.2), K.small_params())


def test_non_finite_coordinates_are_dropped(est):
    cloud = K.non_finite()
    recs = check_records(est, cloud, K.small_params())
    assert sum(r[1] for r in recs) == 40


def test_frames_of_0_1_63_64_65_257_points_in_one_batch(est):
    points, offsets, frames = K.ragged_batch()
    for f, frame in enumerate(frames):
        recs = check_records(est, points, K.small_params(), offsets, f, frame)
        assert sum(r[1] for r in recs) == len(frame)


def test_all_points_in_one_cell(est):
    recs = check_records(est, K.one_cell(), K.small_params())
    assert len(recs) == 1 and recs[0][1] == 500


def test_131072_identical_points_at_the_range_limit(est):
    recs = check_records(est, K.range_limit(), K.small_params())
    q = K.G.range_q
    assert recs == [[recs[0][0], 131072, 131072 * q, -131072 * q, 131072 * q, 131072 * q * q, -131072 * q * q, 131072 * q * q,
                     131072 * q * q, -131072 * q * q, 131072 * q * q]]


def test_300_cells_whose_keys_collide_in_the_hash(est):
    recs = check_records(est, K.colliding(300), K.small_params())
    assert sum(r[1] for r in recs) == 300


def test_snake_of_600_cells_in_descending_key_order(est):
    recs = check_records(est, K.snake(), K.small_params())
    assert len(recs) == 1 and recs[0][1] == 600


def test_slab_of_20_x_20_x_2_cells(est):
    recs = check_records(est, K.slab(), K.small_params())
    assert len(recs) == 1 and recs[0][1] == 1600


def test_one_frame_over_capacity_leaves_the_others_intact(est):
    sp = K.small_params(cluster_min=3, max_components=8)
    over, fits, other = K.isolated(9), K.isolated(8), K.one_cell(300)
    sizes = [len(other), len(over), len(fits)]
    points = np.concatenate([other, over, fits])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    st, got = S.debug_components(est, points, offsets, 1, native(sp))
    assert st == N.CAPACITY and len(got) == 0
    assert len(check_records(est, points, sp, offsets, 0, other)) == 1
    assert len(check_records(est, points, sp, offsets, 2, fits)) == 8
    seeds = S.propose_seeds(est, points, offsets, native(sp))
    assert seeds[1] is None and seeds[0] is not None and seeds[2] is not None


def test_scratch_of_0xff_and_then_dirty(est):
    import torch
    sp = K.small_params()
    a, b = K.slab(), K.random_box(700, 1, -1.0, 1.0)
    need = max(S.scratch_bytes(1, len(a), native(sp)), S.scratch_bytes(1, len(b), native(sp)))
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert scratch.data_ptr() % 256 == 0
    check_records(est, a, sp, scratch=scratch.data_ptr())
    check_records(est, b, sp, scratch=scratch.data_ptr())      # dirty from the first call
    check_records(est, a, sp, scratch=scratch.data_ptr())


# ---- hundreds of frames in one batch, and a frame above 1024 x 256 points

MANY_SP = K.small_params(max_components=K.MANY_MAX_COMPONENTS)
_restated_seeds = {}


@pytest.fixture(scope="module")
def est_many():
    e = LidarCornersBatch(1024, POINTS // 1024, N.default_params())      # 1024 frames of the same 2^20 points in all: R.grid(sp, POINTS) as above
    yield e
    e.close()


def _assert_seeds_are_the_restatement_s(got, picks):
    """frame by frame: no frame over capacity, the restatement's seeds in its order (computed once per distinct cloud)"""
    assert len(got) == len(picks)
    for f, (pick, seeds) in enumerate(zip(picks, got)):
        if pick not in _restated_seeds:
            recs = R.components(K.many_members(pick[0])[pick[1]], MANY_SP, R.grid(MANY_SP, POINTS))
            _restated_seeds[pick] = [(s.key, s.n, tuple(float(v) for v in s.centroid)) for s in R.finish(recs, MANY_SP)]
        assert seeds is not None, f
        assert [(s.key, s.n, tuple(s.centroid_array().tolist())) for s in seeds] == _restated_seeds[pick], f


def test_600_frames_in_one_batch(est_many):
    points, offsets, picks = K.many_frames()
    got = S.propose_seeds(est_many, points, offsets, native(MANY_SP))
    _assert_seeds_are_the_restatement_s(got, picks)
    assert sum(len(s) == 1 for s in got) >= 20 and len({s[0].key for s in got if s}) == 3        # the frames that hold a board-sized plate
    for f, size in K.MANY_CHECKED.items():
        frame = points[int(offsets[f]):int(offsets[f + 1])]
        recs = check_records(est_many, points, MANY_SP, offsets, f, frame)
        assert sum(r[1] for r in recs) == len(frame) == size


def test_600_frames_with_scratch_of_0xff_and_then_dirty(est_many):
    """the counters of all 600 frames are reset by k15_clear alone: a frame whose record counter kept 0xFFFFFFFF, or the count of the
    call before, would be over capacity or hold other records"""
    import torch
    points, offsets, picks = K.many_frames()
    nsp = native(MANY_SP)
    scratch = torch.full((S.scratch_bytes(len(picks), len(points), nsp),), 0xFF, dtype=torch.uint8, device="cuda")
    d_points = torch.from_numpy(points).cuda()
    torch.cuda.synchronize()
    assert scratch.data_ptr() % 256 == 0
    for _ in range(2):                                         # 0xFF everywhere, then dirty from the calls before
        _assert_seeds_are_the_restatement_s(S.propose_seeds_device(est_many, d_points.data_ptr(), offsets, nsp, scratch.data_ptr()), picks)
        for f in (599, 256):
            check_records(est_many, points, MANY_SP, offsets, f, points[int(offsets[f]):int(offsets[f + 1])], scratch=scratch.data_ptr())


def test_a_frame_of_262144_and_257_points_beside_one_of_65(est_many):
    """gridDim.x is capped at 1024 blocks of 256: the large frame's lanes take a second point in k15_insert and k15_moments, and
    the last trip of k15_moments is one full block and one block of a single point, whose other lanes still exchange values"""
    big, dropped = K.big_frame()
    small = K.random_box(65, 165, -0.6, 0.6)
    assert len(big) == 1024 * 256 + 257
    points = np.concatenate([big, small])
    offsets = np.array([0, len(big), len(big) + len(small)], np.uint64)
    recs = check_records(est_many, points, K.small_params(), offsets, 0, big)
    assert len(recs) == 2 and sum(r[1] for r in recs) == len(big) - dropped
    recs = check_records(est_many, points, K.small_params(), offsets, 1, small)
    assert sum(r[1] for r in recs) == len(small)


def test_host_refusals_leave_the_outputs_untouched(est):
    import torch
    L = S.lib()
    sp = native(R.SeedParams())
    cloud = K.random_box(100, 4)
    d_cloud = torch.from_numpy(cloud).cuda()
    scratch = torch.zeros(S.scratch_bytes(1, 100, sp) + 256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off = np.array([0, 100], np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    seeds = (S.Seed * sp.max_seeds)()
    C.memset(seeds, 0x5A, C.sizeof(seeds))
    counts = np.full(1, 0x5A5A5A5A, np.int32)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int32))
    before = bytes(seeds)

    def call(h=est._h, x=d_cloud.data_ptr(), o=offp, n=1, p=C.byref(sp), s=scratch.data_ptr(), out=seeds, cnt=cp):
        return L.ilcc_propose_seeds_device(h, x, o, n, p, s, out, cnt, None)

    assert call(h=None) == N.BAD_ARGUMENT
    assert call(x=None) == N.BAD_ARGUMENT
    assert call(o=None) == N.BAD_ARGUMENT
    assert call(n=0) == N.BAD_ARGUMENT
    assert call(p=None) == N.BAD_ARGUMENT
    assert call(s=None) == N.BAD_ARGUMENT
    assert call(out=None) == N.BAD_ARGUMENT
    assert call(cnt=None) == N.BAD_ARGUMENT
    assert call(s=scratch.data_ptr() + 4) == N.BAD_ARGUMENT and "aligned" in est._err()
    assert call(n=9, o=np.arange(10, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))) == N.CAPACITY     # more frames than the handle's
    big = np.array([0, POINTS + 1], np.uint64)
    assert call(o=big.ctypes.data_as(C.POINTER(C.c_uint64))) == N.CAPACITY
    for field, value in (("cell", 0.01), ("cell", 0.0), ("range", -1.0), ("range", 1e9), ("cluster_min", 0), ("max_components", 0), ("max_seeds", 0)):
        bad = native(R.SeedParams())
        setattr(bad, field, value)
        assert call(p=C.byref(bad)) == N.BAD_ARGUMENT, field
    assert bytes(seeds) == before and counts[0] == 0x5A5A5A5A
    # the host-buffer entries refuse the same way
    res = (N.Result * 1)()
    seed3, rank = np.full(3, 7.0, np.float32), np.full(1, 77, np.int32)
    bad = native(R.SeedParams(cell=0.01))
    assert L.ilcc_extract_auto_batch(est._h, N.fptr(cloud), offp, 1, C.byref(bad), res, N.fptr(seed3), rank.ctypes.data_as(C.POINTER(C.c_int32))) == N.BAD_ARGUMENT
    assert L.ilcc_extract_auto_batch(est._h, None, offp, 1, C.byref(sp), res, N.fptr(seed3), rank.ctypes.data_as(C.POINTER(C.c_int32))) == N.BAD_ARGUMENT
    assert bytes(res[0]) == bytes(C.sizeof(N.Result)) and seed3.tolist() == [7.0] * 3 and rank[0] == 77
    assert call() == N.OK and counts[0] == 0                  # and the same arguments, all valid, run


# ---- the closed loop

def _record_bytes(r):
    """A full record's bytes, grid_ties left out: how many candidates K6's full pass LISTED as near ties depends on how far the
    frame's bound had come when each completed -- on timing -- so two runs of ilcc_extract itself differ in that field (the
    project's other record comparisons leave it out likewise); every other byte is compared."""
    c = N.Result.from_buffer_copy(bytes(r))
    c.grid_ties = 0
    return bytes(c)


def _close_the_loop(e, clouds, gts, board, committed, sp_ref):
    sp = native(sp_ref, e.params)
    n = len(committed)
    seeds = S.propose_seeds(e, clouds[:n], None, sp)
    for (f, key, centroid), got in zip(committed, seeds):
        want = R.propose(clouds[f], sp_ref, R.grid(sp_ref, n * clouds.shape[1] * sp_ref.max_seeds))
        assert [(s.key, tuple(float(v) for v in s.centroid)) for s in want] == [(key, centroid)]
        assert [(s.key, tuple(s.centroid_array().tolist())) for s in got] == [(key, centroid)], f        # same keys and order, centroids equal as float32
        assert [s.n for s in got] == [s.n for s in want]
    res, out_seed, rank = S.extract_auto(e, clouds[:n], None, sp)
    accepted = 0
    for (f, key, centroid) in committed:
        assert out_seed[f].tolist() == list(centroid)
        ref = e.extract(clouds[f][None], out_seed[f][None])[0]
        want = bytearray(_record_bytes(ref))
        if rank[f] < 0:                                        # the best-ranked candidate's record under another status
            assert res[f].status == N.BOARD_NOT_FOUND
            want[0:4] = np.int32(N.BOARD_NOT_FOUND).tobytes()
        assert _record_bytes(res[f]) == bytes(want), f         # byte for byte what extract returns with click = out_seed
        ok = ref.status == N.OK and not (ref.flags & N.FLAG_LOW_COVERAGE) and ref.n_oob <= sp.max_oob_share * (ref.n_black + ref.n_white)
        assert rank[f] == (0 if ok else -1), f                 # the restatement ranks the board first on every one of these frames
        if ok:
            accepted += 1
            assert synth.corner_error(res[f].corners_array(), gts[f], board) < 0.02, f
    return accepted


def test_closed_loop_on_32_config2_frames():
    clouds, _, gts, _ = K.config2(32)
    e = LidarCornersBatch(32 * 4, 28800, N.default_params())
    try:
        accepted = _close_the_loop(e, clouds, gts, synth.Board(), K.CLOSED_LOOP_2, R.SeedParams())
    finally:
        e.close()
    # the CPU oracle accepts 29 of these 32 frames from these seeds (all but 5, 6 and 21: profiles/r09_seed_recall_cpu.json's run); one
    # frame of slack for a grid argmin that the fp32 ranking places differently (FLAGS_FP32_ONLY)
    assert accepted >= 28


def test_closed_loop_on_2_config5_frames():
    clouds, _, gts, _ = K.config5(2)
    p = N.default_params()
    p.board_w, p.board_h, p.grid_length = 9, 12, 0.10
    p.n_th, p.n_ty, p.n_tz = 129, 129, 129
    p.th_min, p.th_step = -16.0 * np.pi / 180.0, 0.25 * np.pi / 180.0
    p.ty_min = p.tz_min = -0.10
    p.ty_step = p.tz_step = 0.10 / 64
    e = LidarCornersBatch(2 * 4, 131072, p)
    e.reserve(6400, 20000)     # the staging capacities of a warmed handle from the first batch on (ilcc_reserve), as the bench does
    try:
        _close_the_loop(e, clouds, gts, K.BOARD5, K.CLOSED_LOOP_5, K.params5())
    finally:
        e.close()


def test_scene_without_a_board_is_board_not_found(est):
    cloud = K.no_board_frame()
    assert S.propose_seeds(est, cloud)[0] == []
    res, seed, rank = S.extract_auto(est, cloud)
    assert res[0].status == N.BOARD_NOT_FOUND and rank[0] == -1 and res[0].n_points == len(cloud) and res[0].n_corners == 0
    m = LidarCornersEst(max_frames=4, max_points_per_frame=30000)
    try:
        found, _ = m.find_board(cloud)
        assert not found
        found, seed = m.find_board(K.config2(32)[0][0])
        corners = []
        assert found and seed.tolist() == list(K.CLOSED_LOOP_2[0][2]) and m.EuclideanCluster() and m.get_corners(corners) and len(corners) == 35
    finally:
        m.close()


def test_cli_auto_writes_the_file_the_printed_seed_writes(tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_corners"
    raw = tmp_path / "frame.bin"
    K.config2(32)[0][0].tofile(raw)
    out_auto, out_click = tmp_path / "auto.txt", tmp_path / "click.txt"
    r = subprocess.run([CLI, "--cloud", str(raw), "--auto", "--out", str(out_auto)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    seed = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("seed ")]
    assert len(seed) == 1 and [float(np.float32(float(v))) for v in seed[0]] == list(K.CLOSED_LOOP_2[0][2])
    r = subprocess.run([CLI, "--cloud", str(raw), "--click", *seed[0], "--out", str(out_click)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out_auto.read_bytes() == out_click.read_bytes() and len(out_auto.read_bytes()) > 0
    r = subprocess.run([CLI, "--cloud", str(raw), "--auto", "--click", "1", "2", "3", "--out", str(out_auto)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2                                   # one of the two, not both
