"""Camera corners from every image of a bag, on the GPU (include/ilcc_image_sequence.h): K10b against the single-image entry byte
for byte (mixed batches, seams, pitches, capacity, refusals, the plan's counters, the candidate order), and the chain
bag -> fused board against K11 + ilcc_find_chessboard_device image by image and against the restated fusion."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import image_sequence_cases as K
import image_sequence_ref as R
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import image_sequence as IS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
BOARD = (7, 5)

_single = {}


def single(img):
    """(corners, 1-based candidates in scan order) of ilcc_image_corners_device on the image alone; computed once per image"""
    key = (img.shape, hashlib.sha1(np.ascontiguousarray(img).tobytes()).hexdigest())
    if key not in _single:
        corners, st = IC.find_corners(np.ascontiguousarray(img), stages=True)
        assert st["n_candidates"] == len(st["candidates"])
        _single[key] = (corners, st["candidates"])
    return _single[key]


def laid_out(images, stride=None, gap=0, fill=0xFF):
    """the images in ONE device buffer, rows `stride` apart, images stride * h + gap apart, everything between filled with `fill`;
    -> the [n, h, w] view K10b is given"""
    import torch
    n, (h, w) = len(images), images[0].shape
    stride = stride or w
    pitch = stride * h + gap
    buf = np.full(n * pitch + 64, fill, np.uint8)
    for m, im in enumerate(images):
        rows = buf[m * pitch:m * pitch + stride * h].reshape(h, stride)
        rows[:, :w] = im
    t = torch.from_numpy(buf).cuda()
    return t.as_strided((n, h, w), (pitch, stride, 1))


def assert_batch_equals_single(images, plan=None, **layout):
    got = IS.find_corners_batch(laid_out(images, **layout), plan=plan)
    assert len(got) == len(images)
    for m, im in enumerate(images):
        want, _ = single(im)
        assert len(got[m]) == len(want), (m, len(got[m]), len(want))
        assert got[m].tobytes() == want.tobytes(), "image %d differs from the single entry" % m
    return got


# ---- K10b against the single entry --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.BATCHES))
def test_mixed_batches_equal_the_single_entry(name):
    images = K.mixed_batch(K.BATCHES[name])
    with IS.CornerPlan(len(images), K.W0, K.H0) as plan:
        assert_batch_equals_single(images, plan=plan)
        cand, off = plan.candidates(len(images))
        assert plan.launches <= 8
        counts = np.diff(off.astype(np.int64))
        for m, n in enumerate(K.BATCHES[name]):
            assert counts[m] == len(single(images[m])[1])
            if n == "constant":
                assert counts[m] == 0
            if n.startswith("noise"):
                assert counts[m] > 256          # out of 1 008 slots: maxima on both sides of the 64- and the 256-slot seams
                ids = [R.block_id(u, v, K.H0) for _, u, v in cand[off[m]:off[m + 1]]]
                assert len({i // 256 for i in ids}) == 4 and len({i // 64 for i in ids}) == 16
        if name == "constant_only":
            assert off[-1] == 0 and plan.launches == 7      # no refine launch
        else:
            assert plan.launches == 8


@pytest.mark.parametrize("size", [(161, 131), (35, 41)])
def test_images_back_to_back_do_not_read_their_neighbours(size):
    """image_pitch == stride * height: 161 = 10 x 16 + 1 and 131 = 8 x 16 + 3 leave both tile residues, 35 x 41 is barely above
    the smallest; the scan blocks of 161 x 131 end 1 and 3 pixels before the margin.  A halo or a scan block that read the
    neighbouring image would see other content than the zero padding the single entry sees."""
    images = K.seam_batch(*size)
    assert_batch_equals_single(images)
    assert sum(len(single(im)[0]) for im in images) > 0


def test_pitch_gap_and_padded_rows():
    images = K.mixed_batch(["board", "noise", "squares"])
    assert_batch_equals_single(images, gap=1000)                 # the gap is 0xFF
    assert_batch_equals_single(images, stride=K.W0 + 1)
    assert_batch_equals_single(images, stride=K.W0 + 13, gap=7)


def test_tie_heavy_fixture_in_a_batch():
    images = K.mixed_batch(["tie_heavy", "board", "tie_heavy"])
    got = assert_batch_equals_single(images)
    assert len(got[0]) >= 35 and got[0].tobytes() == got[2].tobytes()


def _raw_call(t, n, w, h, stride, pitch, corners, capacity, counts, plan, ptr=None):
    import torch
    return IS.lib().ilcc_image_corners_batch_device(C.c_void_p(t.data_ptr() if ptr is None else ptr), pitch, n, w, h, stride,
                                                    corners.ctypes.data_as(C.c_void_p) if corners is not None else None, capacity,
                                                    counts.ctypes.data_as(C.POINTER(C.c_int32)) if counts is not None else None,
                                                    plan._p if plan is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_capacity_contract_per_image():
    names = ["board", "constant", "noise", "range3"]
    images = K.mixed_batch(names)
    want = [single(im)[0] for im in images]
    sizes = [len(w) for w in want]
    cap = (min(n for n in sizes if n) + max(sizes)) // 2                # some images fit, some do not, one has no corner at all
    assert min(n for n in sizes if n) <= cap < max(sizes) and sizes[1] == 0
    t = laid_out(images)
    out = np.zeros((len(images), cap), IC.CORNER_DTYPE)
    out.view(np.uint8)[:] = 0xEE
    counts = np.full(len(images), -1, np.int32)
    with IS.CornerPlan(len(images), K.W0, K.H0) as plan:
        st = _raw_call(t, len(images), K.W0, K.H0, K.W0, K.W0 * K.H0, out, cap, counts, plan)
        fullest = max(m for m, w in enumerate(want) if len(w) > cap)
        assert st == N.CAPACITY and "image %d" % fullest in IS._last_error()
        assert list(counts) == [len(w) for w in want]                         # the full count, also above capacity
        for m, w in enumerate(want):
            k = min(len(w), cap)
            assert out[m, :k].tobytes() == w[:k].tobytes()
            assert (out[m, k:].view(np.uint8) == 0xEE).all()                  # nothing written behind an image's corners
        # capacity 0 with a null array: the counts alone
        counts[:] = -1
        assert _raw_call(t, len(images), K.W0, K.H0, K.W0, K.W0 * K.H0, None, 0, counts, plan) == N.CAPACITY
        assert list(counts) == [len(w) for w in want]


def test_refusals_leave_the_outputs_untouched():
    import torch
    images = K.mixed_batch(["board", "noise"])
    t = laid_out(images)
    w, h = K.W0, K.H0
    out = np.zeros((2, 16), IC.CORNER_DTYPE)
    out.view(np.uint8)[:] = 0xEE
    counts = np.full(2, -7, np.int32)
    with IS.CornerPlan(2, w, h) as plan, IS.CornerPlan(1, 64, 64) as small:
        before = plan.allocations
        calls = {
            "null images": dict(ptr=0),
            "null corners": dict(corners=None),
            "null counts": dict(counts=None),
            "null plan": dict(plan=None),
            "too many images": dict(n=3),
            "image larger than the plan's": dict(plan=small, n=1),
            "narrow": dict(w=33, stride=33, pitch=33 * h),
            "low": dict(h=33, pitch=w * 33),
            "stride below width": dict(stride=w - 1),
            "pitch below stride * height": dict(pitch=w * h - 1),
            "negative capacity": dict(capacity=-1),
        }
        for what, kw in calls.items():
            a = dict(n=2, w=w, h=h, stride=w, pitch=w * h, corners=out, capacity=16, counts=counts, plan=plan)
            a.update(kw)
            st = _raw_call(t, a["n"], a["w"], a["h"], a["stride"], a["pitch"], a["corners"], a["capacity"], a["counts"], a["plan"], ptr=a.get("ptr"))
            assert st == N.BAD_ARGUMENT, what
            assert (out.view(np.uint8) == 0xEE).all() and (counts == -7).all(), what
        # no image is no error, and nothing is launched
        assert _raw_call(t, 0, w, h, w, w * h, out, 16, counts, plan) == N.OK
        assert plan.launches == 0 and (counts == -7).all() and plan.allocations == before
    assert IS.lib().ilcc_image_corner_plan_create(0, 64, 64) is None
    assert IS.lib().ilcc_image_corner_plan_create(2, 33, 64) is None
    assert IS.lib().ilcc_image_corner_plan_create(2, 64, 33) is None
    torch.cuda.synchronize()


def test_plan_runs_twice_counts_launches_and_allocates_once():
    nine = K.mixed_batch(K.BATCHES["n9"])
    with IS.CornerPlan(9, K.W0, K.H0) as plan:
        created = plan.allocations
        assert created == 4                    # scratch, the page-locked counts, the records on both sides
        first = assert_batch_equals_single(nine, plan=plan)
        assert plan.launches == 8
        after_first = plan.allocations           # the record buffer may have grown once
        second = assert_batch_equals_single(nine, plan=plan)
        assert plan.allocations == after_first and plan.launches == 8
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        assert_batch_equals_single(nine[:1], plan=plan)           # one image on the same plan: the same number of launches
        assert plan.launches == 8 and plan.allocations == after_first
        # a smaller image than the plan's
        assert_batch_equals_single(K.seam_batch(35, 41), plan=plan)
        assert plan.allocations == after_first


def test_candidate_order_equals_the_restatement():
    names = K.BATCHES["n9"]
    images = K.mixed_batch(names)
    with IS.CornerPlan(9, K.W0, K.H0) as plan:
        IS.find_corners_batch(laid_out(images), plan=plan)
        cand, off = plan.candidates(9)
    rng = np.random.default_rng(3)
    shuffled = [single(im)[1][rng.permutation(len(single(im)[1]))] for im in images]     # the restatement sorts: any order in
    want, want_off = R.compact(shuffled, K.H0)
    assert list(off) == list(want_off) and cand.tobytes() == want.tobytes()
    keys = [(m, R.block_id(u, v, K.H0)) for m, u, v in cand]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # ... which is the single entry's own (scan) order, image by image
    for m, im in enumerate(images):
        assert np.array_equal(cand[off[m]:off[m + 1], 1:], single(im)[1])


# ---- hundreds of images: the tiles of k10b_offsets and its carry ----------------------------------------------------------------

def _check_many(images, plan):
    """corners, candidate offsets and the candidate list itself against the single entry, image by image"""
    n, (h, w) = len(images), images[0].shape
    assert_batch_equals_single(images, plan=plan)
    assert plan.launches <= 8
    cand, off = plan.candidates(n)
    alone = [single(im)[1] for im in images]
    assert list(off) == list(np.concatenate([[0], np.cumsum([len(c) for c in alone])]))
    want = np.concatenate([np.column_stack([np.full(len(c), m), c]) for m, c in enumerate(alone)] + [np.zeros((0, 3))]).astype(np.int32)
    assert cand.tobytes() == want.tobytes()                  # the single entry's own (scan) order, image by image
    keys = [(m, R.block_id(u, v, h)) for m, u, v in cand]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    return off


@pytest.mark.parametrize("name", list(K.MANY_BATCHES))
def test_hundreds_of_images_equal_the_single_entry(name):
    """256 chunk counts to a tile of k10b_offsets: one tile exactly, a second of one chunk, three, a seam inside an image and between
    two, a tile without a candidate.  What each batch is, tests/test_image_sequence_cpu.py holds against the restated chunk counts."""
    cpi, names = K.MANY_BATCHES[name]
    for member, im in K.many_images(K.MANY_SIDES[cpi]).items():
        assert (len(single(im)[1]) > 0) == (member in K.WITH_CANDIDATES), member
    images = K.many_batch(name)
    with IS.CornerPlan(len(images), K.MANY_SIDES[cpi], K.MANY_SIDES[cpi]) as plan:
        off = _check_many(images, plan)
        assert (np.diff(off.astype(np.int64)) > 0).tolist() == [n in K.WITH_CANDIDATES for n in names]
        assert plan.launches == 8


def test_a_large_batch_and_then_a_smaller_one_of_smaller_images_on_one_plan():
    """counts[], cand_offsets[] and the min / max words of 86 images of 108 x 108 (258 chunks) lie under the 40 images of 34 x 34
    that follow them on the same plan, and under the three constant ones after those"""
    side = K.MANY_SIDES[3]
    with IS.CornerPlan(86, side, side) as plan:
        _check_many(K.many_batch("cpi3_n86"), plan)
        small = K.many_batch("cpi1_n600")[100:140]
        _check_many(small, plan)
        off = _check_many([K.many_images(K.MANY_SIDES[1])["constant_a"]] * 3, plan)
        assert off[-1] == 0 and plan.launches == 7
        _check_many(K.many_batch("cpi2_n129")[:86], plan)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

def _alone(raw, encoding, camera=None):
    """K11 + ilcc_find_chessboard_device on one image: (status, board or None)"""
    mono = CI.to_mono8(raw, encoding, camera)
    try:
        return N.OK, IC.find_chessboard(mono, BOARD)
    except IC.BoardNotFound as e:
        return e.status, None


def _assert_records_equal_alone(records, raws, encoding, camera=None, messages=None):
    messages = messages if messages is not None else list(range(len(raws)))
    assert [r.message for r in records] == messages
    for r, k in zip(records, messages):
        st, board = _alone(raws[k], encoding, camera)
        assert r.status == st, k
        if st == N.OK:
            assert (r.rows, r.cols) == board.shape[:2] and r.board().tobytes() == board.tobytes(), k
        else:
            assert (r.rows, r.cols, r.accepted, r.used) == (0, 0, 0, 0) and r.distance == -1
        assert (r.stamp_sec, r.stamp_nsec, r.time_sec, r.time_nsec) == (100 + k, 7 * k, 50 + k, 0)


def _assert_fusion_is_the_restatement(out, records, gate_px=0.0):
    want = R.fuse([r.board() for r in records], [r.status == N.OK for r in records], BOARD[0], BOARD[1], gate_px)
    assert (out.status, out.n_images, out.n_ok, out.n_used, out.ref_image, out.rows, out.cols) == \
        (want.status, want.n_images, want.n_ok, want.n_used, want.ref_image, want.rows, want.cols)
    assert (out.gate, out.spread_rms, out.spread_max) == (want.gate, want.spread_rms, want.spread_max)
    assert out.board().tobytes() == np.ascontiguousarray(want.xy).tobytes()
    assert [bool(r.used) for r in records] == list(want.used) and [r.distance for r in records] == list(want.dist)
    assert [bool(r.accepted) for r in records] == [r.status == N.OK for r in records]


@pytest.fixture(scope="module")
def chain_bag(tmp_path_factory):
    d = tmp_path_factory.mktemp("image_sequence")
    return K.write_bag(d / "nine.bag", K.chain_messages(), per_chunk=4), d


@pytest.fixture(scope="module")
def chain_result(chain_bag):
    return IS.bag_corners_all_images(chain_bag[0], K.TOPIC, None, BOARD)


def test_chain_on_nine_images(chain_bag, chain_result):
    """render_board((480, 400), square=36, theta=0.2, seed=k) for k = 0 .. 8; image 3 is shifted by one square along the board's
    long axis, image 6 has the corner [2][3] occluded.  cbdetect_ref.find_corners holds all 35 true corners of each of the other
    seven (seeds 0, 1, 2, 4, 5, 7, 8) within 0.5 px in its own list (checked on the CPU when this test was written)."""
    out, records = chain_result
    raws = [im for im, _ in K.chain_images()]
    _assert_records_equal_alone(records, raws, "mono8")
    # record 0 is ilcc_bag_find_chessboard
    assert records[0].board().tobytes() == CI.bag_find_chessboard(chain_bag[0], K.TOPIC, None, BOARD).tobytes()
    assert out.status == N.OK and out.n_images == 9 and out.n_batches == 1
    assert records[K.CHAIN_OCCLUDED].status == N.BOARD_NOT_FOUND and not records[K.CHAIN_OCCLUDED].accepted
    assert [k for k, r in enumerate(records) if r.accepted and not r.used] == [K.CHAIN_SHIFTED]      # the gate drops exactly the shifted image
    assert (out.n_ok, out.n_used) == (8, 7)
    assert abs(records[K.CHAIN_SHIFTED].distance - K.CHAIN_SQUARE) < 0.5 and abs(out.gate - K.CHAIN_SQUARE / 2) < 0.5
    _assert_fusion_is_the_restatement(out, records)
    truth = K.chain_images()[0][1]
    d = np.linalg.norm(out.board().reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    print("fused board vs truth: %.4f px; spread rms %.4f max %.4f px; host recovery %.2f ms" % (d.min(0).max(), out.spread_rms, out.spread_max,
                                                                                                  out.host_recovery_ms))
    assert d.min(0).max() < 0.25 and d.min(1).max() < 0.25


def _summary(out, records):
    return ((out.status, out.n_images, out.n_ok, out.n_used, out.ref_image, out.rows, out.cols, out.gate, out.spread_rms, out.spread_max,
             out.board().tobytes()), [bytes(r) for r in records])


def test_chain_in_one_two_three_and_nine_batches(chain_bag, chain_result):
    msgs = K.chain_messages()
    one = R._up(len(msgs[0]))
    per = R.device_bytes_per_image(*K.CHAIN_SIZE)
    seen = []
    for staging, device in ((0, 0), (5 * one, 0), (0, 3 * per), (one, 0), (0, per), (4 * one, 2 * per)):
        out, records = IS.bag_corners_all_images(chain_bag[0], K.TOPIC, None, BOARD, staging_bytes=staging, device_bytes=device)
        want = R.cut([len(m) for m in msgs], per, staging, device)
        assert out.n_batches == len(want) - 1
        assert _summary(out, records) == _summary(*chain_result), (staging, device)
        seen.append(out.n_batches)
    assert seen == [1, 2, 3, 9, 9, 5]


@pytest.mark.parametrize("first,stride,max_images", [(1, 2, 0), (2, 3, 2), (8, 1, 0)])
def test_chain_selection(chain_bag, first, stride, max_images):
    raws = [im for im, _ in K.chain_images()]
    sel = R.select(9, first, stride, max_images)
    out, records = IS.bag_corners_all_images(chain_bag[0], K.TOPIC, None, BOARD, first=first, stride=stride, max_images=max_images,
                                             raise_on_failure=False)
    assert out.n_images == len(sel)
    _assert_records_equal_alone(records, raws, "mono8", messages=sel)
    _assert_fusion_is_the_restatement(out, records)


@pytest.mark.parametrize("encoding", ["bayer_rggb8", "bgr8"])
def test_chain_on_bayer_and_colour_topics_with_a_camera(tmp_path, encoding):
    cam = K.chain_camera()
    ncam = CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width, cam.height)
    grays = [im for im, _ in K.chain_images()][:3]
    raws = [K.encode(g, encoding) for g in grays]
    path = K.write_bag(tmp_path / "t.bag", K.chain_messages(encoding, grays), per_chunk=2)
    out, records = IS.bag_corners_all_images(path, K.TOPIC, ncam, BOARD, raise_on_failure=False)
    _assert_records_equal_alone(records, raws, encoding, ncam)
    _assert_fusion_is_the_restatement(out, records)
    if encoding == "bgr8":                      # gray in every channel converts back to itself: the boards are found
        assert out.status == N.OK and out.n_used == 3
    if records[0].status == N.OK:
        assert CI.bag_find_chessboard(path, K.TOPIC, ncam, BOARD).tobytes() == records[0].board().tobytes()


def test_chain_refusals(tmp_path, chain_bag):
    msgs = K.chain_messages()[:3]

    def refused(path, status, *words, **kw):
        with pytest.raises(IS.ImageSequenceError) as e:
            IS.bag_corners_all_images(path, K.TOPIC, kw.pop("camera", None), kw.pop("board", BOARD), **kw)
        assert e.value.status == status, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    import jpeg_ref
    compressed = K.write_bag(tmp_path / "c.bag", [jpeg_ref.compressed_image_msg(b"\xff\xd8\xff\xd9")], conn=("sensor_msgs/CompressedImage", jpeg_ref.COMPRESSED_IMAGE_MD5))
    refused(compressed, N.BAD_ARGUMENT, "carries only sensor_msgs/CompressedImage")
    small = K.CR.image_msg(np.zeros((300, 480), np.uint8), "mono8")
    refused(K.write_bag(tmp_path / "size.bag", msgs[:2] + [small]), N.BAD_ARGUMENT, "message 2", "differs from the first selected image's")
    colour = K.CR.image_msg(K.encode(K.chain_images()[0][0], "rgb8"), "rgb8")
    refused(K.write_bag(tmp_path / "enc.bag", msgs[:1] + [colour]), N.BAD_ARGUMENT, "message 1", "encoding")
    cam = K.chain_camera()
    other = CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width + 1, cam.height)
    refused(chain_bag[0], N.BAD_ARGUMENT, "camera's width / height", camera=other)
    tiny = K.CR.image_msg(np.zeros((33, 64), np.uint8), "mono8")
    refused(K.write_bag(tmp_path / "tiny.bag", [tiny]), N.BAD_ARGUMENT, "smaller than 34 px")
    refused(chain_bag[0], N.CAPACITY, "above staging_bytes or device_bytes", staging_bytes=1000)
    refused(chain_bag[0], N.CAPACITY, "above staging_bytes or device_bytes", device_bytes=1000)
    refused(chain_bag[0], N.BAD_ARGUMENT, "select no message", first=9)
    refused(chain_bag[0], N.BAD_ARGUMENT, "board", board=(2, 5))
    # per_image_out too small: the number needed, nothing run
    L = IS.lib()
    sp = IS.default_params()
    out = IS.ImageSequenceResult()
    buf = (IS.ImageRecord * 4)()
    st = L.ilcc_bag_corners_all_images(0, chain_bag[0].encode(), K.TOPIC.encode(), None, 7, 5, C.byref(sp), C.byref(out), buf, 4)
    assert (st, out.status, out.n_images, out.n_batches) == (N.CAPACITY, N.CAPACITY, 9, 0) and not any(bytes(buf))
    assert L.ilcc_bag_corners_all_images(0, chain_bag[0].encode(), K.TOPIC.encode(), None, 7, 5, None, C.byref(out), buf, 4) == N.BAD_ARGUMENT
    assert L.ilcc_bag_corners_all_images(0, chain_bag[0].encode(), K.TOPIC.encode(), None, 7, 5, C.byref(sp), C.byref(out), None, 4) == N.BAD_ARGUMENT


def test_moving_board_is_ambiguous(tmp_path):
    """three images, the board one and a half squares further in each: only the middle one lies within half a square of the median"""
    c, s = np.cos(K.CHAIN_THETA), np.sin(K.CHAIN_THETA)
    images = [K.render_board(K.CHAIN_SIZE, square=K.CHAIN_SQUARE, theta=K.CHAIN_THETA, seed=k,
                             centre=(240 + (k - 1) * 1.5 * K.CHAIN_SQUARE * c, 200 + (k - 1) * 1.5 * K.CHAIN_SQUARE * s))[0] for k in range(3)]
    path = K.write_bag(tmp_path / "moving.bag", K.chain_messages("mono8", images))
    with pytest.raises(IC.BoardNotFound) as e:
        IS.bag_corners_all_images(path, K.TOPIC, None, BOARD)
    assert e.value.status == N.AMBIGUOUS
    out, records = IS.bag_corners_all_images(path, K.TOPIC, None, BOARD, raise_on_failure=False)
    assert (out.status, out.n_ok, out.n_used) == (N.AMBIGUOUS, 3, 1) and not out.board().size
    _assert_fusion_is_the_restatement(out, records)


# ---- the program -------------------------------------------------------------------------------------------------------------------

def test_cli_all_images_and_the_old_invocation(tmp_path, chain_bag):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    cam = K.chain_camera()
    ncam = CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width, cam.height)
    yaml_path = tmp_path / "cam.yaml"
    yaml_path.write_text(K.yaml_text(cam))
    base = [CLI, "--bag", chain_bag[0], "--topic", K.TOPIC, "--yaml", str(yaml_path)]
    # the old invocation: the first image alone, the file it has always written
    old = tmp_path / "first.txt"
    r = subprocess.run(base + ["--out", str(old)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = tmp_path / "first_want.txt"
    IC.save_cam_corners(str(want), CI.bag_find_chessboard(chain_bag[0], K.TOPIC, ncam, BOARD))
    assert old.read_bytes() == want.read_bytes() and "all images" not in r.stdout
    # every image
    fused, report = tmp_path / "fused.txt", tmp_path / "report.txt"
    r = subprocess.run(base + ["--out", str(fused), "--all-images", "--report", str(report)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out, records = IS.bag_corners_all_images(chain_bag[0], K.TOPIC, ncam, BOARD)
    IC.save_cam_corners(str(want), out.board())
    assert fused.read_bytes() == want.read_bytes() and fused.read_bytes() != old.read_bytes()
    lines = report.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 10
    for k, rec in enumerate(records):
        assert lines[k] == "image %d message %d stamp %d.%09d status %d accepted %d used %d distance_px %.3f" % (
            k, rec.message, rec.stamp_sec, rec.stamp_nsec, rec.status, rec.accepted, rec.used, rec.distance if rec.distance >= 0 else -1.0)
    assert "all images: status 0 images 9 accepted %d used %d batches 1" % (out.n_ok, out.n_used) in r.stdout
    # a selection and a gate of one's own
    r = subprocess.run(base + ["--out", str(fused), "--all-images", "--first", "1", "--stride", "2", "--max-images", "3", "--gate", "2.5"],
                       capture_output=True, text=True, timeout=300)
    out, _ = IS.bag_corners_all_images(chain_bag[0], K.TOPIC, ncam, BOARD, first=1, stride=2, max_images=3, gate_px=2.5, raise_on_failure=False)
    assert "images 3" in r.stdout and "gate_px 2.500" in r.stdout and r.returncode == (0 if out.status == N.OK else 4)
    # refused with a usage text
    for extra in (["--all-images", "--jpg-out", str(tmp_path / "x.jpg")], ["--all-images", "--pgm", str(tmp_path / "x.pgm")], ["--first", "2"]):
        r = subprocess.run(base + ["--out", str(fused)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "usage:" in r.stderr and "--all-images" in r.stderr
    r = subprocess.run([CLI, "--jpg", "x.jpg", "--out", str(fused), "--all-images"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr
