"""Structure recovery of a batch of corner lists on the GPU (K18, include/ilcc_image_structure.h) against the host code
(ilcc_chessboard_from_corners, ilcc_chessboard_seed_board): the constructed cases of structure_cases.py in one batch, every seed's
board and energy before the overlap rule, the independence of an image from its batch, real corners from K10b, and both bag chains
with structure="gpu" against structure="host".

Streams: the entry takes host memory and is synchronous on return, so the late-producer scheme of tests/stream_contract.py has
nothing to bite on here -- there is no device input that a delayed side stream could still be writing, and no device output that a
consumer could read too early.  Instead the entry runs on a non-default stream, and two plans run on two streams from two threads
at once."""
import ctypes as C
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

import image_sequence_cases as K
import image_sequence_ref as R
import structure_cases as S
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import image_sequence as IS
from lidar_camera_calibration_amd import jpeg_sequence as JS
from lidar_camera_calibration_amd import jpeg_write
from lidar_camera_calibration_amd.image_corners import CORNER_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
BOARD = (7, 5)

_host = {}


def host(corners, board, key=None):
    """(status, index matrix or None) of ilcc_chessboard_from_corners on the list alone; computed once per key"""
    if key is None or key not in _host:
        try:
            got = (N.OK, IC.chessboard_from_corners(corners, board))
        except IC.BoardNotFound as e:
            got = (e.status, None)
        if key is None:
            return got
        _host[key] = got
    return _host[key]


def host_case(name):
    c = S.case(name)
    st, idx = host(c.corners, c.board, key=name)
    assert st == c.status, "case %s: the host gives %d, the case table says %d" % (name, st, c.status)
    if c.shape is not None:
        assert idx.shape == c.shape
    return st, idx


def assert_equals_host(status, boards, m, want):
    st, idx = want
    assert status[m] == st, (m, status[m], st)
    if st == N.OK:
        assert boards[m].shape == idx.shape and np.array_equal(boards[m], idx), m
    else:
        assert boards[m] is None


def by_board(names):
    groups = {}
    for n in names:
        groups.setdefault(S.case(n).board, []).append(n)
    return groups


# ---- one batch of all cases ----------------------------------------------------------------------------------------------------

def test_every_case_in_one_batch_per_board_equals_the_host():
    groups = by_board(S.BATCH_CASES)
    assert len(groups) == 3
    with IS.StructurePlan(16, 2048) as plan:
        for board, names in groups.items():
            status, boards = IS.chessboards_from_corners_batch([S.case(n).corners for n in names], board, plan=plan)
            for m, n in enumerate(names):
                assert_equals_host(status, boards, m, host_case(n))
            assert plan.fallbacks == 0, (board, names)       # J (1 235 corners) and M (exactly 256 cells) among them
            assert plan.launches == 2


def test_a_board_above_the_capacity_falls_back_to_the_host():
    names = ["A", "W", "B"]
    with IS.StructurePlan(3, 512) as plan:
        status, boards = IS.chessboards_from_corners_batch([S.case(n).corners for n in names], BOARD, plan=plan)
        for m, n in enumerate(names):
            assert_equals_host(status, boards, m, host_case(n))
        assert 1 <= plan.fallbacks <= 1 and status[1] == N.BOARD_NOT_FOUND
        with pytest.raises(IS.ImageSequenceError) as e:      # a recomputed image has no device boards
            IS.seed_board(plan=plan, image=1, seed=0)
        assert e.value.status == N.CAPACITY


def test_lists_the_device_does_not_take_fall_back():
    """more corners than ILCC_STRUCTURE_MAX_CORNERS, and a non-finite coordinate: marked on the host, the host's answer"""
    a = S.case("A").corners
    rng = np.random.default_rng(5)
    many = S.scan_order(a, S.strays(rng, IS.STRUCTURE_MAX_CORNERS + 1 - len(a), (4000, 3000), S.MID, 400))
    assert len(many) == IS.STRUCTURE_MAX_CORNERS + 1
    nan = a.copy()
    nan["v"][len(nan) - 1] = np.nan
    with IS.StructurePlan(3, len(many)) as plan:
        status, boards = IS.chessboards_from_corners_batch([many[:40], nan, a], BOARD, plan=plan)
        assert plan.fallbacks == 1
        for m, c in enumerate([many[:40], nan, a]):
            assert_equals_host(status, boards, m, host(c, BOARD))
        # exactly ILCC_STRUCTURE_MAX_CORNERS stay on the device (all 64 KB of LDS, every bit of the used words), one more does not
        full = many[:-1]
        status, boards = IS.chessboards_from_corners_batch([a, many, full], BOARD, plan=plan)
        assert plan.fallbacks == 1
        assert_equals_host(status, boards, 0, host_case("A"))
        assert_equals_host(status, boards, 1, host(many, BOARD))
        assert_equals_host(status, boards, 2, host(full, BOARD))
        assert status[2] == N.OK
        IS.seed_board(plan=plan, image=2, seed=len(full) - 1)          # on the device: it has a stage output
        with pytest.raises(IS.ImageSequenceError):
            IS.seed_board(plan=plan, image=1, seed=0)


# ---- stage parity --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C", "H", "K", "N"])
def test_every_seed_grows_the_host_board_with_the_host_energy(name):
    c = S.case(name)
    with IS.StructurePlan(1, len(c.corners)) as plan:
        IS.chessboards_from_corners_batch([c.corners], c.board, plan=plan)
        assert plan.fallbacks == 0
        grown = 0
        for seed in range(len(c.corners)):
            want, want_e = IS.seed_board(c.corners, seed)
            got, got_e = IS.seed_board(plan=plan, image=0, seed=seed)
            assert (got is None) == (want is None), seed
            if want is not None:
                grown += 1
                assert got.shape == want.shape and np.array_equal(got, want), seed
            assert struct.pack("<d", got_e) == struct.pack("<d", want_e), (seed, got_e, want_e)
        assert grown >= 9       # the comparison must not pass on seeds without boards


# ---- batch independence --------------------------------------------------------------------------------------------------------

def test_an_image_does_not_depend_on_its_batch_or_the_capacity():
    b = S.case("B").corners
    want = host_case("B")
    fillers = ["A", "C", "I", "K", "L", "E", "F", "Z"]
    rng = np.random.default_rng(40)
    with IS.StructurePlan(40, 4096) as plan:
        status, boards = IS.chessboards_from_corners_batch([b], BOARD, plan=plan)
        assert_equals_host(status, boards, 0, want)
        alone, launches, allocations = boards[0], plan.launches, plan.allocations
        for at in (0, 17, 39):
            names = [fillers[k] for k in rng.integers(0, len(fillers), 40)]
            lists = [S.case(n).corners for n in names]
            lists[at] = b
            for capacity in (len(b), len(b) + 1, 4096):
                status, boards = IS.chessboards_from_corners_batch(lists, BOARD, plan=plan, capacity=capacity)
                assert status[at] == N.OK and np.array_equal(boards[at], alone), (at, capacity)
                assert plan.launches == launches and plan.allocations == allocations and plan.fallbacks == 0
            for m in (0, 16, 38, 39):      # and the neighbours are their own hosts' too
                if m != at:
                    assert_equals_host(status, boards, m, host_case(names[m]))
        # a later, smaller call on the same plan: nothing of the 40 images' scratch leaks into it
        for n in ("I", "E", "Z", "K"):
            status, boards = IS.chessboards_from_corners_batch([S.case(n).corners], BOARD, plan=plan)
            assert_equals_host(status, boards, 0, host_case(n))
        status, boards = IS.chessboards_from_corners_batch([], BOARD, plan=plan)
        assert len(status) == 0 and plan.launches == 0 and plan.allocations == allocations


def test_refusals_that_need_a_plan_leave_the_outputs_untouched():
    a = S.case("A").corners
    table = np.zeros((2, 40), CORNER_DTYPE)
    table[0, :35] = table[1, :35] = a
    i32p = C.POINTER(C.c_int32)
    with IS.StructurePlan(2, 40) as plan:
        def call(counts, n=2, capacity=40, p=plan, board=BOARD):
            cnt = np.array(counts, np.int32)
            out = [np.full(2, 77, np.int32) for _ in range(3)] + [np.full(2 * 35, 77, np.int32)]
            st = IS.lib().ilcc_chessboards_from_corners_batch(table.ctypes.data_as(C.c_void_p), capacity, cnt.ctypes.data_as(i32p), n, board[0], board[1],
                                                              *[o.ctypes.data_as(i32p) for o in out], p._p if p else None, None)
            return st, all((o == 77).all() for o in out)
        assert call([35, 35]) == (N.OK, False)
        assert call([35, 35], capacity=34) == (N.BAD_ARGUMENT, True)       # capacity below an image's count
        assert call([35, -1]) == (N.BAD_ARGUMENT, True)
        assert call([35, 35, 35], n=3) == (N.BAD_ARGUMENT, True)           # more images than the plan's
        assert call([35, 35], board=(2, 5)) == (N.BAD_ARGUMENT, True)
        assert call([35, 35], board=(16, 17)) == (N.BAD_ARGUMENT, True)
        assert call([35, 35], p=None) == (N.BAD_ARGUMENT, True)
        launches = plan.launches
        assert launches == 2
    with IS.StructurePlan(2, 34) as small:
        assert call([35, 35], p=small) == (N.BAD_ARGUMENT, True)           # more corners than the plan's


# ---- real corners --------------------------------------------------------------------------------------------------------------

def test_corners_of_the_golden_crops_and_the_rendered_frames():
    lists = []
    for i in range(1, 7):
        crop = np.load(os.path.join(GOLD, "pointgrey%d_crop.npz" % i))["image"]
        lists += IS.find_corners_batch([np.ascontiguousarray(crop)])
    frames = [im for im, _ in K.chain_images()]
    lists += IS.find_corners_batch(frames)
    assert len(lists) == 15 and min(len(c) for c in lists) >= 9
    with IS.StructurePlan(len(lists), max(len(c) for c in lists)) as plan:
        status, boards = IS.chessboards_from_corners_batch(lists, BOARD, plan=plan)
        print("corners per list %s, fallbacks %d" % ([len(c) for c in lists], plan.fallbacks))
        for m, c in enumerate(lists):
            assert_equals_host(status, boards, m, host(c, BOARD))
        assert plan.fallbacks == 0
    assert status[6 + K.CHAIN_OCCLUDED] == N.BOARD_NOT_FOUND and (status == N.OK).sum() >= 8


# ---- the chains ----------------------------------------------------------------------------------------------------------------

def _same_but_recovery_ms(a, b):
    (out_a, rec_a), (out_b, rec_b) = a, b
    assert [bytes(r) for r in rec_a] == [bytes(r) for r in rec_b]
    ra, rb = IS.ImageSequenceResult.from_buffer_copy(out_a), IS.ImageSequenceResult.from_buffer_copy(out_b)
    ra.host_recovery_ms = rb.host_recovery_ms = 0.0
    assert bytes(ra) == bytes(rb)
    assert out_a.host_recovery_ms > 0 and out_b.host_recovery_ms > 0


@pytest.fixture(scope="module")
def chain_bags(tmp_path_factory):
    d = tmp_path_factory.mktemp("image_structure")
    grays = [im for im, _ in K.chain_images()]
    import jpeg_ref
    jpgs = [jpeg_write.encode(g, 95, "420") for g in grays]
    msgs = [jpeg_ref.compressed_image_msg(j, "jpeg", seq=k, stamp=(100 + k, 7 * k)) for k, j in enumerate(jpgs)]
    return (K.write_bag(d / "nine.bag", K.chain_messages(), per_chunk=4),
            K.write_bag(d / "nine_jpeg.bag", msgs, per_chunk=4, conn=("sensor_msgs/CompressedImage", jpeg_ref.COMPRESSED_IMAGE_MD5)), d)


def test_both_chains_give_the_host_route_records(chain_bags):
    raw, compressed, _ = chain_bags
    want = IS.bag_corners_all_images(raw, K.TOPIC, None, BOARD, structure="host")
    assert want[0].status == N.OK and want[0].n_ok == 8 and want[1][K.CHAIN_OCCLUDED].status == N.BOARD_NOT_FOUND
    _same_but_recovery_ms(IS.bag_corners_all_images(raw, K.TOPIC, None, BOARD, structure="gpu"), want)
    _same_but_recovery_ms(IS.bag_corners_all_images(raw, K.TOPIC, None, BOARD), want)                     # the default is the host route
    # three batches: the plan serves them all
    split = IS.bag_corners_all_images(raw, K.TOPIC, None, BOARD, device_bytes=3 * R.device_bytes_per_image(*K.CHAIN_SIZE), structure="gpu")
    assert split[0].n_batches == 3 and [bytes(r) for r in split[1]] == [bytes(r) for r in want[1]]
    want = JS.bag_corners_all_compressed_images(compressed, K.TOPIC, None, BOARD, structure="host")
    assert want[0].status == N.OK and want[0].n_ok >= 5
    _same_but_recovery_ms(JS.bag_corners_all_compressed_images(compressed, K.TOPIC, None, BOARD, structure="gpu"), want)
    _same_but_recovery_ms(JS.bag_corners_all_compressed_images(compressed, K.TOPIC, None, BOARD, structure="gpu", huffman="gpu"), want)


def test_cli_structure_gpu_writes_the_same_files(tmp_path, chain_bags):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    yaml_path = tmp_path / "cam.yaml"
    yaml_path.write_text(K.yaml_text(K.chain_camera()))
    files = {}
    for bag in chain_bags[:2]:
        for route in ("host", "gpu"):
            out, report = tmp_path / ("fused_%s.txt" % route), tmp_path / ("report_%s.txt" % route)
            r = subprocess.run([CLI, "--bag", bag, "--topic", K.TOPIC, "--yaml", str(yaml_path), "--out", str(out), "--all-images", "--report", str(report),
                                "--structure", route], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            files[route] = (out.read_bytes(), report.read_bytes(), r.stdout.replace(str(out), "OUT"))
        assert files["host"] == files["gpu"] and len(files["gpu"][1].split(b"\n")) == 10


# ---- streams -------------------------------------------------------------------------------------------------------------------

def test_a_side_stream_and_two_plans_on_two_threads():
    import torch
    names = ["B", "A", "K", "C", "J"]
    lists = [S.case(n).corners for n in names]
    want = [host_case(n) for n in names]
    side = torch.cuda.Stream()
    with IS.StructurePlan(len(lists), 2048) as plan:
        status, boards = IS.chessboards_from_corners_batch(lists, BOARD, plan=plan, stream=side)
        for m in range(len(names)):
            assert_equals_host(status, boards, m, want[m])
    results, errors = {}, []

    def run(tag, order):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with IS.StructurePlan(len(lists), 2048) as p:
                for _ in range(3):
                    results[tag] = IS.chessboards_from_corners_batch([lists[k] for k in order], BOARD, plan=p, stream=stream)
        except Exception as e:      # noqa: BLE001 -- reported below, on the main thread
            errors.append((tag, repr(e)))

    orders = {"a": [0, 1, 2, 3, 4], "b": [4, 3, 2, 1, 0]}
    threads = [threading.Thread(target=run, args=(tag, order)) for tag, order in orders.items()]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for tag, order in orders.items():
        status, boards = results[tag]
        for m, k in enumerate(order):
            assert_equals_host(status, boards, m, want[k])
