"""JPEG reading on the GPU (include/ilcc_jpeg.h): the host decoder through the C-ABI, K13 (csrc/k13_jpeg.hip) from
constructed coefficients and from files, byte for byte against the numpy restatement (tests/jpeg_ref.py) and the recorded
libjpeg results (tests/golden/jpeg/expected.json); the reference's own six frames through the detector to the
calibration; and the bag entries on sensor_msgs/CompressedImage topics against the step-by-step route."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import camera_image_ref
import jpeg_cases as J
import jpeg_ref as R
import rosbag_writer as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import calib
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
CAM = (1061.37439737547, 980.706836288949, 1061.02435228316, 601.685030610243)   # fx cx fy cy, pointgrey.yaml
IMG = (camera_image_ref.IMAGE_TYPE, camera_image_ref.IMAGE_MD5)
CIMG = ("sensor_msgs/CompressedImage", R.COMPRESSED_IMAGE_MD5)
PC2 = ("sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5)
FILL = 0xAB


# ------------------------------------------------------------------------------------------ CPU: interface

def test_exports_match_header():
    hdr = open(os.path.join(ROOT, "include", "ilcc_jpeg.h")).read()
    declared = re.findall(r"^(?:int32_t|uint64_t) (ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(jpeg.JPEG_EXPORTS)
    L = jpeg.lib()
    for s in jpeg.JPEG_EXPORTS:
        assert hasattr(L, s), s
    assert (C.sizeof(jpeg.Component), C.sizeof(jpeg.Info), C.sizeof(jpeg.CompressedImageLayout)) == (40, 664, 160)


def test_not_here_lines_are_gone():
    for header in ("ilcc_camera_image.h", "ilcc_image_corners.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "JPEG / " not in text and "CompressedImage decoding" not in text, header


# ------------------------------------------------------------------------------------------ GPU: host decoder through the C-ABI

def _same_info(info, want):
    assert (info.width, info.height, info.n_components, info.restart_interval, info.coef_count, info.scan_offset) == \
        (want.width, want.height, want.n_components, want.restart_interval, want.coef_count, want.scan_offset)
    for c, w in zip(info.comp, want.comps):
        assert (c.h, c.v, c.quant_index, c.dc_table, c.ac_table, c.blocks_w, c.blocks_h, c.coef_offset) == \
            (w.h, w.v, w.tq, w.td, w.ta, w.blocks_w, w.blocks_h, w.offset)
    used = sorted({w.tq for w in want.comps})
    assert np.array_equal(info.quant_array()[used], want.quant[used])


@pytest.mark.gpu
def test_coefficients_equal_the_restatement():
    for name in J.small_fixtures() + ["pointgrey1.jpg"]:
        want_info, want, _ = J.restated(name)
        info = jpeg.parse(J.data(name))
        _same_info(info, want_info)
        assert np.array_equal(jpeg.entropy_decode(J.data(name), info), want), name
    info = jpeg.parse(J.data(J.COLOUR))
    short = np.zeros(info.coef_count - 1, np.int16)
    arr, n = jpeg._bytes_arg(J.data(J.COLOUR))
    assert jpeg.lib().ilcc_jpeg_entropy_decode(arr, n, C.byref(info), short.ctypes.data_as(C.c_void_p), short.size) == N.CAPACITY
    assert not short.any()
    info.comp[0].blocks_w += 1                                   # an info that is not these bytes' is refused, not trusted
    big = np.zeros(info.coef_count + 4096, np.int16)
    assert jpeg.lib().ilcc_jpeg_entropy_decode(arr, n, C.byref(info), big.ctypes.data_as(C.c_void_p), big.size) == N.BAD_ARGUMENT


@pytest.mark.gpu
def test_compressed_image_parse():
    jpg = J.data(J.GRAY)
    msg = R.compressed_image_msg(jpg, "mono8; jpeg compressed ", seq=9, stamp=(5, 6), frame_id="pointgrey")
    lay = jpeg.parse_compressed_image(msg)
    assert (lay.seq, lay.stamp_sec, lay.stamp_nsec, lay.frame_id, lay.format) == (9, 5, 6, b"pointgrey", b"mono8; jpeg compressed ")
    assert msg[lay.data_offset:lay.data_offset + lay.data_bytes] == jpg
    assert jpeg.parse_compressed_image(R.compressed_image_msg(jpg, "jpg")).data_bytes == len(jpg)
    for bad, words in ((R.compressed_image_msg(jpg, "png"), "'png'"), (R.compressed_image_msg(jpg, "bgr8; png compressed bgr8"), "png compressed"),
                       (R.compressed_image_msg(b"", "jpeg"), "empty"), (msg[:-1], "runs past"), (msg[:20], "truncated"), (b"", "truncated"),
                       (msg[:12] + b"\xf0\xff\xff\xff" + msg[16:], "truncated")):
        with pytest.raises(CI.CameraImageError) as e:
            jpeg.parse_compressed_image(bad)
        assert e.value.status == N.BAD_ARGUMENT and words in str(e.value), words


# ------------------------------------------------------------------------------------------ GPU: K13 from constructed coefficients

def _k13(width, height, sampling, quant, coef):
    """K13's pixels and the restatement's for the same constructed coefficients."""
    info = jpeg.make_info(width, height, sampling, quant)
    rinfo = R.make_info(width, height, jpeg.SAMPLINGS.get(sampling, sampling), quant)
    assert info.coef_count == rinfo.coef_count == coef.size
    return jpeg.idct(info, coef).cpu().numpy(), R.pixels(rinfo, coef)


@pytest.mark.gpu
def test_k13_single_coefficients():
    """Only coefficient k set, each of the 64, both signs, an amplitude that clamps and one that does not: a slip in the
    transposes or in the row / column order of the passes moves the pattern."""
    coef = J.single_coefficient_blocks()
    got, want = _k13(256 * 8, 8, None, np.full(64, 8), coef)
    assert want[:, :128 * 8].min() > 0 and want[:, :128 * 8].max() < 255              # amplitude 4: nothing clamps
    assert want[:, 128 * 8:].min() == 0 and want[:, 128 * 8:].max() == 255            # amplitude 120: both ends clamp
    bad = np.argwhere((got != want).any(0).reshape(256, 8).any(1)).ravel()
    assert bad.size == 0, "blocks (k + 64 * case) that differ: %s" % bad[:16]
    blocks = want.reshape(8, 256, 8).transpose(1, 0, 2)                               # k is row-major: k = 1 varies along x, k = 8 along y
    assert (blocks[1] == blocks[1][:1]).all() and (blocks[8] == blocks[8][:, :1]).all() and not np.array_equal(blocks[1], blocks[8])


@pytest.mark.gpu
def test_k13_dc_only_and_all_64():
    for dc in (-1024, -3, 0, 5, 1016):
        coef = np.zeros(64, np.int16)
        coef[0] = dc
        got, want = _k13(8, 8, None, np.ones(64), coef)
        assert np.array_equal(got, want) and (want == want[0, 0]).all(), dc
    rng = np.random.default_rng(3)
    coef = rng.integers(-40, 41, 64 * 6).astype(np.int16)
    got, want = _k13(48, 8, None, np.full(64, 3), coef)
    assert np.array_equal(got, want) and len(np.unique(want)) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("quant", sorted(J.QUANTS))
def test_k13_block_grids_one_component(quant):
    q = J.QUANTS[quant]
    for k, (bw, bh, w, h) in enumerate(J.GRIDS):
        coef = J.grid_coefficients(bw * bh * 64, 10 + k, max(1, 1000 // int(q.max())))
        got, want = _k13(w, h, None, q, coef)
        assert got.shape == want.shape == (h, w) and np.array_equal(got, want), (bw, bh, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", ["444", "422", "420"])
def test_k13_block_grids_three_components(sampling):
    hs, vs = jpeg.SAMPLINGS[sampling]
    sizes = [(1, 1), (3, 3), (4, 4), (5, 3), (7, 7), (9, 7), (15, 1), (1, 15), (17, 9), (257, 9), (263, 15), (249, 17), (255, 23), (511, 33),
             (513, 31)]                                          # odd chroma sizes, chroma width 1, 2 and 3, both sides of the store tiles
    for k, (w, h) in enumerate(sizes):
        for quant in sorted(J.QUANTS):
            q = J.QUANTS[quant]
            rinfo = R.make_info(w, h, (hs, vs), np.stack([q, q[::-1]]))
            coef = J.grid_coefficients(rinfo.coef_count, 100 + k, max(1, 1000 // int(q.max())))
            got, want = _k13(w, h, sampling, np.stack([q, q[::-1]]), coef)
            assert got.shape == want.shape == (h, w, 3) and np.array_equal(got, want), (sampling, w, h, quant)


@pytest.mark.gpu
def test_k13_refuses_before_any_launch():
    import torch
    info = jpeg.make_info(17, 9, "420", np.ones((2, 64)))
    coef = torch.zeros(info.coef_count, dtype=torch.int16, device="cuda")
    out = torch.full((9, 17 * 3), FILL, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(jpeg.scratch_bytes(info), dtype=torch.uint8, device="cuda")

    def call(info=info, coef=coef.data_ptr(), dst=out.data_ptr(), stride=51, scr=scratch.data_ptr(), scr_bytes=scratch.numel()):
        return jpeg.lib().ilcc_jpeg_idct_device(C.byref(info), C.c_void_p(coef), C.c_void_p(dst), stride, C.c_void_p(scr), scr_bytes, None)

    forged = jpeg.make_info(17, 9, "420", np.ones((2, 64)))
    forged.comp[1].blocks_w += 1
    moved = jpeg.make_info(17, 9, "420", np.ones((2, 64)))
    moved.comp[2].coef_offset += 64
    wide = jpeg.make_info(17, 9, "420", np.ones((2, 64)))
    wide.width = 33
    assert jpeg.scratch_bytes(forged) == 0
    for st in (call(info=forged), call(info=moved), call(info=wide), call(coef=0), call(dst=0), call(stride=50), call(coef=coef.data_ptr() + 2),
               call(scr=0), call(scr_bytes=scratch.numel() - 1)):
        assert st == N.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert (out == FILL).all()
    assert call() == N.OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy().reshape(9, 17, 3) == R.pixels(R.make_info(17, 9, (2, 2), np.ones((2, 64))), np.zeros(info.coef_count, np.int16))).all()
    with pytest.raises(CI.CameraImageError):
        jpeg.make_info(17, 9, (1, 2))
    with pytest.raises(CI.CameraImageError):
        jpeg.make_info(0, 9)


# ------------------------------------------------------------------------------------------ GPU: pixels of files

@pytest.mark.gpu
def test_decode_every_fixture():
    for name in J.small_fixtures():
        got = jpeg.decode(J.data(name)).cpu().numpy()
        assert np.array_equal(got, J.restated(name)[2]), name
        assert J.sha256(got) == J.expected()[name]["sha256"], name


def _decode_into(jpg, buffer, offset, stride, cap):
    w, h, enc = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    arr, n = jpeg._bytes_arg(jpg)
    st = jpeg.lib().ilcc_jpeg_decode_device(arr, n, C.c_void_p(buffer.data_ptr() + offset), stride, cap, C.byref(w), C.byref(h), C.byref(enc),
                                            None)
    return st, w.value, h.value, enc.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise_257x9_gray_q95_r0.jpg", "noise_257x9_444_q95_r2.jpg", "noise_255x9_422_q50_r0.jpg",
                                  "noise_257x9_420_q95_r0.jpg", "noise_17x33_420_q50_r2.jpg", "noise_4x3_420_q95_r0.jpg"])
def test_decode_strides_and_offsets_write_only_the_rows(name):
    import torch
    _, _, want = J.restated(name)
    h, w = want.shape[:2]
    row = want.reshape(h, -1).shape[1]                           # bpp * w
    for extra in (0, 1, 13):
        for offset in range(4):
            stride = row + extra
            buf = torch.full((offset + h * stride + 8,), FILL, dtype=torch.uint8, device="cuda")
            st, gw, gh, enc = _decode_into(J.data(name), buf, offset, stride, (h - 1) * stride + row)
            assert (st, gw, gh, CI.ENCODINGS[enc]) == (N.OK, w, h, "mono8" if want.ndim == 2 else "bgr8")
            flat = buf.cpu().numpy()
            body = flat[offset:offset + h * stride].reshape(h, stride)
            assert np.array_equal(body[:, :row], want.reshape(h, row)), (extra, offset)
            assert (body[:, row:] == FILL).all() and (flat[:offset] == FILL).all() and (flat[offset + h * stride:] == FILL).all(), (extra, offset)


@pytest.mark.gpu
def test_decode_capacity_and_refusals_leave_the_destination_untouched():
    import torch
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    jpg = J.data(J.COLOUR)                                        # 17 x 33, three components
    st, w, h, enc = _decode_into(jpg, buf, 0, 51, 32 * 51 + 50)   # one byte short
    assert (st, w, h, CI.ENCODINGS[enc]) == (N.CAPACITY, 17, 33, "bgr8")
    st, w, h, _ = _decode_into(jpg, buf, 0, 50, 1 << 16)          # a stride shorter than a row
    assert (st, w, h) == (N.BAD_ARGUMENT, 17, 33)
    for name, (bad, _, words) in J.refusals().items():
        st, _, _, _ = _decode_into(bad, buf, 0, 1024, 1 << 16)
        assert st == N.BAD_ARGUMENT, name
        text = N.lib().ilcc_last_error(None).decode()
        assert words in text and text.startswith("jpeg: "), (name, text)
    torch.cuda.synchronize()
    assert (buf == FILL).all()
    assert _decode_into(jpg, buf, 0, 51, 32 * 51 + 51)[0] == N.OK


# ------------------------------------------------------------------------------------------ GPU: the reference's files

@pytest.fixture(scope="module")
def detected(tmp_path_factory):
    """pointgrey<i>.txt as ilcc_jpeg_find_chessboard + ilcc_save_cam_corners write them from the reference's jpgs (once)."""
    out = tmp_path_factory.mktemp("detected")
    for i in range(1, 7):
        board = jpeg.find_chessboard(os.path.join(J.HERE, "pointgrey%d.jpg" % i), None, (7, 5))
        assert board.shape[:2] in ((7, 5), (5, 7)), i
        IC.save_cam_corners(str(out / ("pointgrey%d.txt" % i)), board)
    return out


@pytest.mark.gpu
def test_reference_images_decode_to_the_recorded_pixels():
    for name in J.reference_images():
        got = jpeg.decode(J.data(name))
        assert tuple(got.shape) == (1200, 1920) and J.sha256(got.cpu().numpy()) == J.expected()[name]["sha256"], name


@pytest.mark.gpu
def test_reference_images_give_the_reference_detector_output(detected):
    """The MATLAB step on the reference's own files: every corner within 0.5 px of pointgrey<i>.txt, RMS <= 0.2 px."""
    rows = []
    for i in range(1, 7):
        got = calib.check_order_cam(calib.read_cam_corners(str(detected / ("pointgrey%d.txt" % i)), 35))
        want = calib.check_order_cam(calib.read_cam_corners(os.path.join(GOLD, "pointgrey%d.txt" % i), 35))
        assert got.shape == want.shape == (35, 2)
        d = np.linalg.norm(got - want, axis=1)
        rows.append((i, d.max(), math.sqrt((d ** 2).mean())))
    print("\n".join("pointgrey%d.jpg: max %.4f px, rms %.4f px" % r for r in rows))
    for i, mx, rms in rows:
        assert mx <= 0.5 and rms <= 0.2, (i, mx, rms)


@pytest.mark.gpu
def test_reference_images_calibrate_to_the_shipped_extrinsic(detected, tmp_path):
    for i in range(1, 7):
        shutil.copy(detected / ("pointgrey%d.txt" % i), tmp_path / ("pointgrey%d.txt" % i))
        shutil.copy(os.path.join(GOLD, "pointgrey_lidar_%d.txt" % i), tmp_path / ("pointgrey_lidar_%d.txt" % i))
    T, err = calib.calib_lidar_cam(str(tmp_path), "pointgrey", 6, CAM)
    ref = calib.extrinsic_read(os.path.join(GOLD, "pointgrey.bin"))
    c = (np.trace(T[:3, :3].T @ ref[:3, :3]) - 1) / 2
    rot = math.degrees(math.acos(min(1.0, max(-1.0, c))))
    dt = np.linalg.norm(T[:3, 3] - ref[:3, 3])
    print("extrinsic vs pointgrey.bin: %.4f deg, %.2f mm, reprojection %.3f px" % (rot, dt * 1e3, err))
    assert rot < 0.1 and dt < 5e-3


@pytest.mark.gpu
def test_cli_jpg_output_is_the_library_s(detected, tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    out = tmp_path / "cli.txt"
    r = subprocess.run([CLI, "--jpg", os.path.join(J.HERE, "pointgrey3.jpg"), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == (detected / "pointgrey3.txt").read_bytes()
    # with the yaml the file is undistorted first and the board comes from the yaml: the step-by-step route gives the same file
    cam = CI.read_camera_yaml(os.path.join(GOLD, "pointgrey.yaml"))
    board = jpeg.find_chessboard(os.path.join(J.HERE, "pointgrey3.jpg"), cam, (7, 5))
    steps = IC.find_chessboard(CI.to_mono8(jpeg.decode(J.data("pointgrey3.jpg")), "mono8", cam), (7, 5))
    assert board.tobytes() == steps.tobytes()
    IC.save_cam_corners(str(tmp_path / "lib.txt"), board)
    r = subprocess.run([CLI, "--jpg", os.path.join(J.HERE, "pointgrey3.jpg"), "--yaml", os.path.join(GOLD, "pointgrey.yaml"), "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == (tmp_path / "lib.txt").read_bytes()
    r = subprocess.run([CLI, "--jpg", str(tmp_path / "missing.jpg"), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "can not open" in r.stderr
    r = subprocess.run([CLI, "--jpg", os.path.join(J.HERE, "pointgrey3.jpg"), "--topic", "/x", "--out", str(out)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2


# ------------------------------------------------------------------------------------------ GPU: CompressedImage topics in bags

def _bag(path, messages, compression="none"):
    bag = W.BagWriter(str(path), compression)
    bag.add_chunk(messages)
    bag.write()
    return str(path)


def _cloud_msg(pts):
    a, fields, step = W.velodyne_points(np.asarray(pts, np.float32))
    return W.pointcloud2(a, fields, step)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise_50x35_gray_q95_r2.jpg", "noise_50x35_420_q95_r0.jpg", "ramp_33x17_422_q50_r2.jpg"])
def test_bag_first_image_from_a_compressed_topic(tmp_path, name):
    jpg = J.data(name)
    later = R.compressed_image_msg(J.data("noise_31x16_gray_q50_r0.jpg"), "jpeg", seq=2)
    path = _bag(tmp_path / "c.bag", [("/velodyne_points", *PC2, (1, 0), _cloud_msg(np.zeros((4, 4)))),
                                     ("/camera/image_raw/compressed", *CIMG, (2, 0), later),
                                     ("/camera/image_raw/compressed", *CIMG, (1, 5), R.compressed_image_msg(jpg, "bgr8; jpeg compressed bgr8", seq=1))],
                "bz2")
    decoded = jpeg.decode(jpg)
    enc = "mono8" if decoded.dim() == 2 else "bgr8"
    h, w = decoded.shape[:2]
    assert np.array_equal(CI.bag_first_image(path, "/camera/image_raw/compressed"), CI.to_mono8(decoded, enc).cpu().numpy())
    cam = CI.CameraModel.make(0.8 * w, 0.48 * w, 0.9 * h, 0.52 * h, (-0.30, 0.10, 0.002, -0.0015, 0.05), w, h)
    assert np.array_equal(CI.bag_first_image(path, "/camera/image_raw/compressed", cam), CI.to_mono8(decoded, enc, cam).cpu().numpy())
    small = np.zeros(10, np.uint8)
    gw, gh = C.c_int32(0), C.c_int32(0)
    st = CI.lib().ilcc_bag_first_image(0, path.encode(), b"/camera/image_raw/compressed", None, small.ctypes.data_as(C.c_void_p), small.size,
                                       C.byref(gw), C.byref(gh))
    assert st == N.CAPACITY and (gw.value, gh.value) == (w, h) and not small.any()


@pytest.mark.gpu
def test_bag_topic_with_both_types_takes_the_image_and_refuses_other_formats(tmp_path):
    px = np.random.default_rng(5).integers(0, 256, (6, 9), dtype=np.uint8)
    image = camera_image_ref.image_msg(px, "mono8", seq=3)
    comp = R.compressed_image_msg(J.data(J.GRAY), "jpeg", seq=1)
    path = _bag(tmp_path / "both.bag", [("/camera/image_raw", *CIMG, (1, 0), comp), ("/camera/image_raw", *IMG, (2, 0), image)])
    assert np.array_equal(CI.bag_first_image(path, "/camera/image_raw"), px)        # the later Image wins over the earlier CompressedImage
    path = _bag(tmp_path / "png.bag", [("/camera/image_raw", *CIMG, (1, 0), R.compressed_image_msg(J.data(J.GRAY), "mono8; png compressed "))])
    with pytest.raises(CI.CameraImageError) as e:
        CI.bag_first_image(path, "/camera/image_raw")
    assert e.value.status == N.BAD_ARGUMENT and "png compressed" in str(e.value)
    path = _bag(tmp_path / "bad.bag", [("/camera/image_raw", *CIMG, (1, 0), R.compressed_image_msg(J.refusals()["progressive"][0], "jpeg"))])
    with pytest.raises(CI.CameraImageError) as e:
        CI.bag_find_chessboard(path, "/camera/image_raw", None)
    assert e.value.status == N.BAD_ARGUMENT and "progressive" in str(e.value)
    with pytest.raises(CI.CameraImageError) as e:
        CI.bag_first_image(path, "/camera/other")
    assert e.value.status == N.BAD_ARGUMENT and "no message of that type on topic" in str(e.value)


@pytest.mark.gpu
def test_bag_find_chessboard_from_a_compressed_topic(tmp_path):
    jpg = J.data("board_480x400_gray_q90.jpg")
    path = _bag(tmp_path / "board.bag", [("/camera/image_raw/compressed", *CIMG, (1, 0), R.compressed_image_msg(jpg, "mono8; jpeg compressed "))], "lz4")
    cam = CI.CameraModel.make(400.0, 236.0, 390.0, 204.0, (-0.05, 0.01, 0.0005, -0.0004, 0.0), 480, 400)
    for camera in (None, cam):
        one = CI.bag_find_chessboard(path, "/camera/image_raw/compressed", camera, (7, 5))
        two = IC.find_chessboard(CI.to_mono8(jpeg.decode(jpg), "mono8", camera), (7, 5))
        assert one.shape[:2] in ((7, 5), (5, 7)) and one.tobytes() == two.tobytes()
    jpg_path = tmp_path / "board.jpg"
    jpg_path.write_bytes(jpg)
    assert jpeg.find_chessboard(str(jpg_path), None, (7, 5)).tobytes() == CI.bag_find_chessboard(path, "/camera/image_raw/compressed", None).tobytes()


@pytest.mark.gpu
def test_bag_pcd2image_from_a_compressed_topic(tmp_path):
    import torch
    import test_overlay as TO
    from lidar_camera_calibration_amd import overlay as OV
    from lidar_camera_calibration_amd import project
    jpg = J.data("board_320x240_420_q90.jpg")
    cam = TO.small_camera()
    ncam = TO.native(cam)
    pts = TO.scene(5000, 4)
    path = _bag(tmp_path / "pcd.bag", [("/camera/image_raw/compressed", *CIMG, (1, 0), R.compressed_image_msg(jpg, "bgr8; jpeg compressed bgr8")),
                                       ("/velodyne_points", *PC2, (1, 0), _cloud_msg(pts))], "bz2")
    T = TO.extrinsic()
    one, n_drawn = OV.bag_pcd2image(path, "/camera/image_raw/compressed", "/velodyne_points", ncam, T, distance_valid=TO.DISTANCE)
    image = CI.to_bgr8(jpeg.decode(jpg), "bgr8", ncam)
    d_hits, m = TO._hits_on_gpu(pts, cam)
    scratch = torch.empty(project.draw_hits_scratch_bytes(320, 240), dtype=torch.uint8, device="cuda")
    project.draw_hits_device(image.data_ptr(), 320, 240, 960, d_hits.data_ptr(), m, scratch.data_ptr())
    assert n_drawn == m > 100 and np.array_equal(one, image.cpu().numpy())
