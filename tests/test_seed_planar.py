"""Planar seeds (K15p) on the GPU (pytest -m gpu): the integer records of ilcc_debug_seed_planar_components against the numpy
restatement (tests/seed_planar_ref.py), exactly, on clouds constructed for every path of the classify launch and of the
core-aware union and pack; the host refusals; and scenes in which the chessboard stands on or in the floor or on a pole, where
the ordinary proposer finds nothing and extract_auto_planar must return what ilcc_extract returns for the seed it names."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seed_planar_cases as K   # noqa: E402
import seed_planar_ref as P     # noqa: E402
import seed_ref as R            # noqa: E402
from lidar_camera_calibration_amd import LidarCornersBatch   # noqa: E402
from lidar_camera_calibration_amd import _native as N         # noqa: E402
from lidar_camera_calibration_amd import seed as S            # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_corners")
POINTS = 1 << 20
SP = K.small_params()
NAMES = ("cell", "range", "cluster_min", "max_components", "max_seeds", "board_w", "board_h", "grid_length", "max_rms", "size_lo",
         "size_hi", "max_oob_share")


@pytest.fixture(scope="module")
def est():
    e = LidarCornersBatch(8, POINTS // 8, N.default_params())
    yield e
    e.close()


def native(sp: R.SeedParams, pp: P.PlanarParams = K.PP, params=None):
    out, npp = S.default_seed_planar_params(params if params is not None else N.default_params())
    for name in NAMES:
        setattr(out, name, getattr(sp, name))
    npp.planar_rms, npp.min_spread, npp.own_rms = pp.planar_rms, pp.min_spread, pp.own_rms
    return out, npp


def check_records(est, cloud, sp=SP, offsets=None, frame=0, frame_cloud=None, scratch=None, points=POINTS):
    """the GPU's planar records of `frame` equal the restatement's, word for word"""
    nsp, npp = native(sp)
    st, got = S.debug_planar_components(est, cloud, offsets, frame, nsp, npp, scratch)
    assert st == N.OK, est._err()
    want = P.components(frame_cloud if frame_cloud is not None else cloud, sp, K.PP, R.grid(sp, points))
    assert got.tolist() == want
    return want


def test_planar_defaults_mirror_the_restatement():
    sp, pp = S.default_seed_planar_params(N.default_params())
    ref, plain = P.default_params(), S.default_seed_params(N.default_params())
    for name in NAMES:
        assert getattr(sp, name) == getattr(ref, name), name
        assert name == "max_rms" or getattr(sp, name) == getattr(plain, name), name
    assert (pp.planar_rms, pp.min_spread, pp.own_rms) == (K.PP.planar_rms, K.PP.min_spread, K.PP.own_rms)
    assert S.planar_scratch_bytes(3, 1000, sp) >= S.scratch_bytes(3, 1000, sp) + 1000


def test_dense_plate(est):
    recs = check_records(est, K.dense_plate())
    assert [r[1] for r in recs] == [len(K.dense_plate())]


@pytest.mark.parametrize("normals", [(2, 0), (1, 0), (2, 1)])
@pytest.mark.parametrize("origin", [(-4, 3, -2), (-9, -8, -7)])
def test_ell_in_three_orientations(est, normals, origin):
    cloud = K.ell(*normals, origin=origin)
    assert (cloud[:, :3] < 0).any()
    recs = check_records(est, cloud)
    assert len(recs) == 2 and sum(r[1] for r in recs) < len(cloud)
    st, plain = S.debug_components(est, cloud, None, 0, native(SP)[0])
    assert st == N.OK and plain[:, 1].tolist() == [len(cloud)]


def test_line_and_slabs(est):
    assert check_records(est, K.line()) == []
    assert [r[1] for r in check_records(est, K.slab(0.5))] == [len(K.slab(0.5))]
    assert check_records(est, K.slab(2.0)) == []


def test_plate_with_a_hanging_line(est):
    recs = check_records(est, K.plate_with_line())
    assert len(recs) == 1 and len(K.plate_with_line()) - 240 <= recs[0][1] < len(K.plate_with_line())


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_blocks_that_reach_outside_the_grid_do_not_wrap(est, axis):
    cloud = K.edge_plates(axis)
    assert [r[1] for r in check_records(est, cloud, K.EDGE_SP)] == [len(cloud) // 2] * 2


def test_ragged_batch_of_0_1_63_64_65_257_points(est):
    points, offsets, frames = K.ragged_batch()
    for f, frame in enumerate(frames):
        check_records(est, points, SP, offsets, f, frame)
    # and frames that have core cells beside frames that have none
    parts = [K.dense_plate(), np.zeros((0, 4), np.float32), K.line(), K.ell()]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    for f, frame in enumerate(parts):
        check_records(est, np.concatenate(parts), SP, offsets, f, frame)


def test_all_points_in_one_cell_are_not_core(est):
    assert check_records(est, K.one_cell()) == []


def test_cells_whose_keys_collide_in_the_hash(est):
    check_records(est, K.colliding(300))
    both = np.concatenate([K.colliding(300), K.dense_plate()])
    assert sum(r[1] for r in check_records(est, both)) >= len(K.dense_plate())


def test_non_finite_points_are_dropped(est):
    recs = check_records(est, K.non_finite())
    assert max(r[1] for r in recs) >= len(K.dense_plate())


def test_order_of_the_points_decides_nothing(est):
    cloud = K.ell()
    want = check_records(est, cloud)
    for seed in (1, 2, 3):
        assert check_records(est, cloud[np.random.default_rng(seed).permutation(len(cloud))]) == want


def test_scratch_of_0xff_then_dirty_and_shared_with_the_ordinary_path(est):
    import torch
    a, b = K.ell(), K.plate_with_line()
    nsp = native(SP)[0]
    need = max(S.planar_scratch_bytes(1, len(a), nsp), S.planar_scratch_bytes(1, len(b), nsp))
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert scratch.data_ptr() % 256 == 0
    check_records(est, a, scratch=scratch.data_ptr())
    check_records(est, b, scratch=scratch.data_ptr())          # dirty from the first call
    # planar, ordinary, planar on one buffer: the flag array leaks into neither
    st, plain = S.debug_components(est, a, None, 0, nsp, scratch.data_ptr())
    assert st == N.OK and plain.tolist() == R.components(a, SP, R.grid(SP, POINTS))
    check_records(est, a, scratch=scratch.data_ptr())
    st, plain = S.debug_components(est, b, None, 0, nsp, scratch.data_ptr())
    assert st == N.OK and plain.tolist() == R.components(b, SP, R.grid(SP, POINTS))


# ---- hundreds of frames in one batch, and a frame above 1024 x 256 points (the planar twins of tests/test_seed.py's)

MANY_SP = K.small_params(max_components=K.K.MANY_MAX_COMPONENTS)
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
            recs = P.components(K.many_members(pick[0])[pick[1]], MANY_SP, K.PP, R.grid(MANY_SP, POINTS))
            _restated_seeds[pick] = [(s.key, s.n, tuple(float(v) for v in s.centroid)) for s in R.finish(recs, MANY_SP)]
        assert seeds is not None, f
        assert [(s.key, s.n, tuple(s.centroid_array().tolist())) for s in seeds] == _restated_seeds[pick], f


def test_600_frames_in_one_batch(est_many):
    points, offsets, picks = K.many_frames()
    got = S.propose_seeds_planar(est_many, points, offsets, *native(MANY_SP))
    _assert_seeds_are_the_restatement_s(got, picks)
    assert sum(len(s) == 1 for s in got) >= 10 and len({s[0].key for s in got if s}) == 2        # the frames that hold a board-sized plate
    for f, size in K.K.MANY_CHECKED.items():
        frame = points[int(offsets[f]):int(offsets[f + 1])]
        assert len(frame) == size
        check_records(est_many, points, MANY_SP, offsets, f, frame)


def test_600_frames_with_scratch_of_0xff_and_then_dirty(est_many):
    import torch
    points, offsets, picks = K.many_frames()
    nsp, npp = native(MANY_SP)
    scratch = torch.full((S.planar_scratch_bytes(len(picks), len(points), nsp),), 0xFF, dtype=torch.uint8, device="cuda")
    d_points = torch.from_numpy(points).cuda()
    torch.cuda.synchronize()
    assert scratch.data_ptr() % 256 == 0
    for _ in range(2):                                         # 0xFF everywhere, then dirty from the calls before
        _assert_seeds_are_the_restatement_s(S.propose_seeds_planar_device(est_many, d_points.data_ptr(), offsets, nsp, npp, scratch.data_ptr()), picks)
        for f in (599, 256):
            check_records(est_many, points, MANY_SP, offsets, f, points[int(offsets[f]):int(offsets[f + 1])], scratch=scratch.data_ptr())


def test_a_frame_of_262144_and_257_points_beside_one_of_65(est_many):
    """the large frame's lanes take a second point in k15_insert and k15_moments; its sheet is one core component, its box none"""
    big, _ = K.K.big_frame()
    small = K.many_members(65)[5]
    assert len(big) == 1024 * 256 + 257 and len(small) == 65
    points = np.concatenate([big, small])
    offsets = np.array([0, len(big), len(big) + len(small)], np.uint64)
    recs = check_records(est_many, points, SP, offsets, 0, big)
    assert len(recs) == 1 and recs[0][1] > 200_000
    check_records(est_many, points, SP, offsets, 1, small)


def test_one_frame_over_capacity_leaves_the_others_intact(est):
    sp = K.small_params(cluster_min=3, max_components=8)
    over, fits, other = K.isolated_plates(9), K.isolated_plates(8), K.dense_plate()
    parts = [other, over, fits]
    points = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    nsp, npp = native(sp)
    st, got = S.debug_planar_components(est, points, offsets, 1, nsp, npp)
    assert st == N.CAPACITY and len(got) == 0
    assert len(check_records(est, points, sp, offsets, 0, other)) == 1
    assert len(check_records(est, points, sp, offsets, 2, fits)) == 8
    seeds = S.propose_seeds_planar(est, points, offsets, nsp, npp)
    assert seeds[1] is None and seeds[0] is not None and seeds[2] is not None


def test_host_refusals_leave_the_outputs_untouched(est):
    import torch
    L = S.lib()
    sp, pp = native(P.default_params())
    n_big = 104858                                             # cell 10 m: cq 10240, and 104858 x 2 x 10240 >= 2^31 > 104857 x 2 x 10240
    cloud = K.random_box(n_big, 4)
    d_cloud = torch.from_numpy(cloud).cuda()
    wide = native(P.default_params(cell=10.0))[0]
    scratch = torch.zeros(S.planar_scratch_bytes(1, n_big, sp) + 256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off = np.array([0, 100], np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    seeds = (S.Seed * sp.max_seeds)()
    C.memset(seeds, 0x5A, C.sizeof(seeds))
    counts = np.full(1, 0x5A5A5A5A, np.int32)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int32))
    before = bytes(seeds)

    def call(h=est._h, x=d_cloud.data_ptr(), o=offp, n=1, p=C.byref(sp), q=C.byref(pp), s=scratch.data_ptr(), out=seeds, cnt=cp):
        return L.ilcc_propose_seeds_planar_device(h, x, o, n, p, q, s, out, cnt, None)

    assert call(h=None) == N.BAD_ARGUMENT
    for name in ("x", "o", "p", "q", "s", "out", "cnt"):
        assert call(**{name: None}) == N.BAD_ARGUMENT, name
    assert call(n=0) == N.BAD_ARGUMENT
    assert call(s=scratch.data_ptr() + 4) == N.BAD_ARGUMENT and "aligned" in est._err()
    assert call(n=9, o=np.arange(10, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))) == N.CAPACITY
    big = np.array([0, POINTS + 1], np.uint64)
    assert call(o=big.ctypes.data_as(C.POINTER(C.c_uint64))) == N.CAPACITY
    for field, value in (("cell", 0.01), ("cell", 0.0), ("range", -1.0), ("cluster_min", 0), ("max_components", 0), ("max_seeds", 0)):
        bad = native(P.default_params())[0]
        setattr(bad, field, value)
        assert call(p=C.byref(bad)) == N.BAD_ARGUMENT, field
    for field in ("planar_rms", "min_spread", "own_rms"):
        for value in (0.0, -0.01, float("nan")):
            bad = native(P.default_params())[1]
            setattr(bad, field, value)
            assert call(q=C.byref(bad)) == N.BAD_ARGUMENT, field
    # the frame-size bound: n 2 cq < 2^31
    over = np.array([0, n_big], np.uint64)
    assert call(o=over.ctypes.data_as(C.POINTER(C.c_uint64)), p=C.byref(wide)) == N.BAD_ARGUMENT and "2^31" in est._err()
    assert bytes(seeds) == before and counts[0] == 0x5A5A5A5A
    # the host-buffer entries refuse the same way
    res = (N.Result * 1)()
    seed3, rank = np.full(3, 7.0, np.float32), np.full(1, 77, np.int32)
    rp = rank.ctypes.data_as(C.POINTER(C.c_int32))
    bad = native(P.default_params())[1]
    bad.own_rms = 0.0
    assert L.ilcc_extract_auto_planar_batch(est._h, N.fptr(cloud), offp, 1, C.byref(sp), C.byref(bad), res, N.fptr(seed3), rp) == N.BAD_ARGUMENT
    assert L.ilcc_extract_auto_planar_batch(est._h, N.fptr(cloud), offp, 1, C.byref(sp), None, res, N.fptr(seed3), rp) == N.BAD_ARGUMENT
    assert L.ilcc_extract_auto_planar_batch(est._h, N.fptr(cloud), over.ctypes.data_as(C.POINTER(C.c_uint64)), 1, C.byref(wide), C.byref(pp), res,
                                            N.fptr(seed3), rp) == N.BAD_ARGUMENT
    assert bytes(res[0]) == bytes(C.sizeof(N.Result)) and seed3.tolist() == [7.0] * 3 and rank[0] == 77
    # one point fewer is within the bound, and the same arguments, all valid, run
    under = np.array([0, n_big - 1], np.uint64)
    assert call(o=under.ctypes.data_as(C.POINTER(C.c_uint64)), p=C.byref(wide)) == N.OK and counts[0] == 0
    counts[0] = 0x5A5A5A5A
    assert call() == N.OK and counts[0] == 0


# ---- scenes

def _record_bytes(r):
    """a full record's bytes, grid_ties left out (it depends on timing in any call: tests/test_seed.py::_record_bytes)"""
    c = N.Result.from_buffer_copy(bytes(r))
    c.grid_ties = 0
    return bytes(c)


def _scenes(e, frames, lidar):
    """frames: [(scene, frame)].  Records equal the restatement's; extract_auto_planar accepts the first seed and returns what
    extract returns for it; the ordinary extract_auto finds no board."""
    clouds = np.stack([K.scene_cached(scene, f, lidar)[0] for scene, f in frames])
    sp_ref, pp_ref = K.seed_params(lidar)
    sp, pp = native(sp_ref, pp_ref, e.params)
    n, per = len(frames), clouds.shape[1]
    g = R.grid(sp_ref, n * per * sp_ref.max_seeds)
    seeds = S.propose_seeds_planar(e, clouds, None, sp, pp)
    for k in range(n):
        st, got = S.debug_planar_components(e, clouds, None, k, sp, pp)
        assert st == N.OK, e._err()
        want = P.components(clouds[k], sp_ref, pp_ref, g)
        assert got.tolist() == want, frames[k]
        ranked = R.finish(want, sp_ref)
        assert [(s.key, s.n, s.centroid_array().tolist()) for s in seeds[k]] == [(s.key, s.n, s.centroid.tolist()) for s in ranked], frames[k]
    res, out_seed, rank = S.extract_auto_planar(e, clouds, None, sp, pp)
    for k in range(n):
        assert rank[k] == 0 and res[k].status == N.OK, frames[k]                   # chosen so: condition (b)
        assert out_seed[k].tolist() == seeds[k][0].centroid_array().tolist()
        ref = e.extract(clouds[k][None], out_seed[k][None])[0]
        assert _record_bytes(res[k]) == _record_bytes(ref), frames[k]              # byte for byte what extract returns with click = out_seed
        pose = K.scene_cached(frames[k][0], frames[k][1], lidar)[1]
        assert np.linalg.norm(out_seed[k] - pose.centre) < 0.3
    plain, _, plain_rank = S.extract_auto(e, clouds, None, S.default_seed_params(e.params))
    for k in range(n):
        assert plain[k].status == N.BOARD_NOT_FOUND and plain_rank[k] == -1, frames[k]          # condition (c)


@pytest.fixture(scope="module")
def est_scenes():
    e = LidarCornersBatch(8 * 4, 28800, N.default_params())
    yield e
    e.close()


def test_eight_frames_with_the_floor_5_cm_below_the_board(est_scenes):
    _scenes(est_scenes, [("floor5", f) for f in K.FLOOR5_FRAMES], "vlp16")


def test_eight_frames_with_the_board_2_cm_in_the_floor(est_scenes):
    _scenes(est_scenes, [("in2", f) for f in K.IN2_FRAMES], "vlp16")


def test_two_frames_with_the_board_on_a_pole(est_scenes):
    _scenes(est_scenes, [("pole", f) for f in K.POLE_FRAMES], "vlp16")


def test_two_hdl64_frames():
    p = N.default_params()
    p.board_w, p.board_h, p.grid_length = 9, 12, 0.10
    p.n_th, p.n_ty, p.n_tz = 129, 129, 129
    p.th_min, p.th_step = -16.0 * np.pi / 180.0, 0.25 * np.pi / 180.0
    p.ty_min = p.tz_min = -0.10
    p.ty_step = p.tz_step = 0.10 / 64
    e = LidarCornersBatch(4, 131072, p)
    e.reserve(6400, 20000)
    try:
        for scene, f in K.HDL64_FRAMES:
            _scenes(e, [(scene, f)], "hdl64")
    finally:
        e.close()


def test_cli_auto_planar_writes_the_file_the_printed_seed_writes(tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_corners"
    raw = tmp_path / "frame.bin"
    K.scene_cached("floor5", K.FLOOR5_FRAMES[0])[0].tofile(raw)
    out_auto, out_click = tmp_path / "auto.txt", tmp_path / "click.txt"
    r = subprocess.run([CLI, "--cloud", str(raw), "--auto", "--out", str(out_auto)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "no chessboard found" in r.stdout       # the ordinary proposer does not find this board
    r = subprocess.run([CLI, "--cloud", str(raw), "--auto-planar", "--out", str(out_auto)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    seed = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("seed ")]
    want = P.propose(K.scene_cached("floor5", K.FLOOR5_FRAMES[0])[0], *K.seed_params(), R.grid(R.SeedParams(), 4 * 28801))
    assert len(seed) == 1 and [np.float32(float(v)) for v in seed[0]] == want[0].centroid.tolist()
    r = subprocess.run([CLI, "--cloud", str(raw), "--click", *seed[0], "--out", str(out_click)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out_auto.read_bytes() == out_click.read_bytes() and len(out_auto.read_bytes()) > 0
    r = subprocess.run([CLI, "--cloud", str(raw), "--auto", "--auto-planar", "--out", str(out_auto)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2                                   # one way of finding the seed, not two
