"""Camera images (include/ilcc_camera_image.h): the intrinsics reader, the sensor_msgs/Image parser and
the bag reader on Image topics are host code (CPU tests); conversion to mono8 and undistortion are one
HIP kernel, K11 (gpu tests), held byte for byte against the numpy restatement in camera_image_ref.py.
The CPU tests also guard the restatement itself: that its cases exercise what the GPU cases are taken to
exercise (taps outside the source, negative codes, every edge), and that undistortion followed by the
corner detector's restatement reaches the bar the GPU closed loop is held to."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import camera_image_ref as R
import cbdetect_ref
import rosbag_writer as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
IMG = (R.IMAGE_TYPE, R.IMAGE_MD5)
PC2 = ("sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5)

D_ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
D_BARREL = (-0.30, 0.10, 0.002, -0.0015, 0.05)
D_PINCUSHION = (0.35, 0.2, -0.01, 0.02, 0.0)
D_TANGENTIAL = (0.0, 0.0, 0.03, -0.02, 0.0)
D_K3_ONLY = (0.0, 0.0, 0.0, 0.0, 0.4)
D_HUGE = (1e8, 0.0, 0.0, 0.0, 0.0)      # codes beyond 2^30 away from the centre: the outside rule
LENSES = {"zero": D_ZERO, "barrel": D_BARREL, "pincushion": D_PINCUSHION, "tangential": D_TANGENTIAL, "k3": D_K3_ONLY,
          "huge": D_HUGE}


def cam_for(w, h, d):
    """The 37 x 29 camera (fx, cx, fy, cy = 30, 17.6, 29, 14.3) scaled to w x h."""
    return R.camera(30.0 / 37 * w, 17.6 / 37 * w, 29.0 / 29 * h, 14.3 / 29 * h, d, w, h)


def native(cam):
    return CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width, cam.height)


def noise_image(w, h, encoding, seed=1):
    shape = (h, w) if encoding == "mono8" else (h, w, R.BPP[encoding])
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------ CPU: interface

def test_exports_match_header():
    hdr = open(os.path.join(ROOT, "include", "ilcc_camera_image.h")).read()
    declared = re.findall(r"^int32_t (ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(CI.CAMERA_IMAGE_EXPORTS)
    L = CI.lib()
    for s in CI.CAMERA_IMAGE_EXPORTS:
        assert hasattr(L, s), s
    assert C.sizeof(CI.CameraModel) == 9 * 8 + 2 * 4
    assert C.sizeof(CI.ImageLayout) == 8 * 4 + 2 * 8 + 64
    assert CI.IMAGE_MD5 == R.IMAGE_MD5 and CI.ENCODINGS == R.ENCODINGS
    # the other headers keep their lists: nothing of this one leaked into them
    for name in ("ilcc_image_corners.h", "ilcc_ingest.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(ilcc_\w+)\s*\(", other)) & set(CI.CAMERA_IMAGE_EXPORTS)


def _yaml(K=None, d=None, d_shape=None, size=(1920, 1200), with_K=True, extra=""):
    K = K if K is not None else [1061.37439737547, 0, 980.706836288949, 0, 1061.02435228316, 601.685030610243, 0, 0, 1]
    d = d if d is not None else [-0.149007007770170, 0.0729485326193990, 0.000257753168848673, -0.000207183134328829, 0]
    rows, cols = d_shape if d_shape else (len(d), 1)
    out = "%YAML:1.0\n\n"
    if with_K:
        out += "K: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [%s]\n" % ", ".join(repr(float(v)) for v in K)
    # the data of d runs over two lines, as cv::FileStorage breaks long rows
    vals = [repr(float(v)) for v in d]
    out += "d: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s,\n       %s ]\n" % (
        rows, cols, ", ".join(vals[:2]), ", ".join(vals[2:]))
    out += "\nCamera.width: %d\nCamera.height: %d\n\ngrid_length: 0.15\ncorner_in_x: 7\ncorner_in_y: 5\n%s" % (size[0], size[1], extra)
    return out


def test_read_camera_yaml_golden():
    cam = CI.read_camera_yaml(os.path.join(GOLD, "pointgrey.yaml"))
    assert (cam.fx, cam.cx, cam.fy, cam.cy) == (1061.37439737547, 980.706836288949, 1061.02435228316, 601.685030610243)
    assert tuple(cam.d) == (-0.149007007770170, 0.0729485326193990, 0.000257753168848673, -0.000207183134328829, 0.0)
    assert (cam.width, cam.height) == (1920, 1200)


def test_read_camera_yaml_variants(tmp_path):
    p = tmp_path / "cam.yaml"
    p.write_text(_yaml(d=[-0.2, 0.05, 1e-3, -2e-3]))                       # four entries: k3 = 0
    cam = CI.read_camera_yaml(str(p))
    assert tuple(cam.d) == (-0.2, 0.05, 1e-3, -2e-3, 0.0)
    p.write_text(_yaml(d=[-0.2, 0.05, 1e-3, -2e-3, 0.125], d_shape=(1, 5), size=(640, 480)))   # a row vector
    cam = CI.read_camera_yaml(str(p))
    assert tuple(cam.d) == (-0.2, 0.05, 1e-3, -2e-3, 0.125) and (cam.width, cam.height) == (640, 480)
    assert (cam.fx, cam.fy) == (1061.37439737547, 1061.02435228316)
    refused = {
        "skew": _yaml(K=[1000, 0.5, 960, 0, 1000, 600, 0, 0, 1]),
        "last row": _yaml(K=[1000, 0, 960, 0, 1000, 600, 0, 0, 2]),
        "missing K": _yaml(with_K=False),
        "six coefficients": _yaml(d=[0.1, 0.1, 0, 0, 0.1, 0.2]),
        "d is 2 x 2": _yaml(d=[0.1, 0.1, 0, 0], d_shape=(2, 2)),
        "no size": _yaml().replace("Camera.width", "Camera_width"),
    }
    for what, text in refused.items():
        p.write_text(text)
        with pytest.raises(CI.CameraImageError) as e:
            CI.read_camera_yaml(str(p))
        assert e.value.status == N.BAD_ARGUMENT, what
    assert "skew" in _raises(lambda: (p.write_text(refused["skew"]), CI.read_camera_yaml(str(p))))
    with pytest.raises(CI.CameraImageError) as e:
        CI.read_camera_yaml(str(tmp_path / "missing.yaml"))
    assert e.value.status == N.IO_ERROR and "can not open" in str(e.value)


def _raises(fn):
    with pytest.raises(CI.CameraImageError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("encoding", R.ENCODINGS)
def test_parse_image_round_trip(encoding):
    px = noise_image(7, 5, encoding)
    row = 7 * R.BPP[encoding]
    for step in (row, row + 1, row + 13):
        msg = R.image_msg(px, encoding, step=step, seq=9, stamp=(12, 34), frame_id="pointgrey")
        lay = CI.parse_image(msg)
        assert (lay.height, lay.width, lay.step, lay.encoding_name) == (5, 7, step, encoding)
        assert (lay.seq, lay.stamp_sec, lay.stamp_nsec, lay.frame_id, lay.is_bigendian) == (9, 12, 34, b"pointgrey", 0)
        assert lay.data_bytes == step * 5 and lay.data_offset + lay.data_bytes == len(msg)
        data = np.frombuffer(msg, np.uint8, lay.data_bytes, lay.data_offset).reshape(5, step)
        assert (data[:, :row].reshape(px.shape) == px).all()


def test_parse_image_refusals():
    px = noise_image(7, 5, "mono8")
    for enc in ("mono16", "bayer_rggb8"):
        msg = R.image_msg(px, enc)
        assert enc in _raises(lambda: CI.parse_image(msg))
    good = R.image_msg(noise_image(7, 5, "bgr8"), "bgr8")
    assert CI.parse_image(good).width == 7
    for cut in (0, 3, 11, 20, 30, 40, len(good) - 1):          # truncated anywhere, the last data byte included
        with pytest.raises(CI.CameraImageError) as e:
            CI.parse_image(good[:cut])
        assert e.value.status == N.BAD_ARGUMENT, cut
    lay = CI.parse_image(good)
    at = lay.data_offset - 4
    for forged_len in (0xFFFFFFFF, lay.data_bytes + 1):       # data[] asks for more than the message holds
        forged = good[:at] + struct.pack("<I", forged_len) + good[at + 4:]
        assert "runs past" in _raises(lambda: CI.parse_image(forged))
    short = good[:at] + struct.pack("<I", lay.data_bytes - 1) + good[at + 4:-1]   # consistent, but less than step * height
    assert "shorter than step" in _raises(lambda: CI.parse_image(short))
    frame_at = 12                                             # frame_id's length prefix
    forged = good[:frame_at] + struct.pack("<I", 0xFFFFFFF0) + good[frame_at + 4:]
    assert "truncated" in _raises(lambda: CI.parse_image(forged))
    assert "step" in _raises(lambda: CI.parse_image(R.image_msg(noise_image(7, 5, "bgr8"), "bgr8", step=20,
                                                                 data=bytes(20 * 5))))
    assert "empty" in _raises(lambda: CI.parse_image(R.image_msg(px, "mono8", height=0)))
    # sizes whose product wraps 32 bits are still refused: step * height is taken in 64 bits
    assert "shorter than step" in _raises(lambda: CI.parse_image(
        R.image_msg(px, "mono8", height=0x10000, width=7, step=0x10000, data=bytes(64))))


# ------------------------------------------------------------------------------------------ CPU: Image topics in bags

def _cloud_msg(n, seed):
    a, fields, step = W.velodyne_points(np.random.default_rng(seed).normal(0, 5, (n, 4)).astype(np.float32))
    return W.pointcloud2(a, fields, step)


@pytest.mark.parametrize("compression", ["none", "bz2", "lz4"])
def test_bag_with_cloud_and_image_topics(tmp_path, compression):
    image = R.image_msg(noise_image(9, 6, "rgb8"), "rgb8", seq=4)
    cloud = _cloud_msg(40, 1)
    bag = W.BagWriter(str(tmp_path / "t.bag"), compression)
    bag.add_chunk([("/velodyne_points", *PC2, (10, 0), cloud), ("/camera/image_raw", *IMG, (10, 5), image)])
    bag.write()
    path = str(tmp_path / "t.bag")
    assert ingest.bag_first_message(path, "/camera/image_raw", R.IMAGE_MD5) == image
    assert ingest.bag_first_message(path, "/velodyne_points") == cloud
    lay = CI.parse_image(ingest.bag_first_message(path, "/camera/image_raw", R.IMAGE_MD5))
    assert (lay.width, lay.height, lay.encoding_name, lay.seq) == (9, 6, "rgb8", 4)


def test_bag_image_on_a_connection_with_another_md5(tmp_path):
    image = R.image_msg(noise_image(9, 6, "mono8"), "mono8")
    bag = W.BagWriter(str(tmp_path / "t.bag"))
    bag.add_chunk([("/camera/image_raw", R.IMAGE_TYPE, "0" * 32, (1, 0), image), ("/velodyne_points", *PC2, (1, 0), _cloud_msg(5, 1))])
    bag.write()
    with pytest.raises(ingest.IngestError) as e:
        ingest.bag_first_message(str(tmp_path / "t.bag"), "/camera/image_raw", R.IMAGE_MD5)
    assert e.value.status == N.BAD_ARGUMENT and "no message of that type on topic" in str(e.value)


def test_bag_first_image_in_time_order_sits_in_the_second_chunk(tmp_path):
    first, later = R.image_msg(noise_image(9, 6, "mono8", 2), "mono8", seq=1), R.image_msg(noise_image(9, 6, "mono8", 3), "mono8", seq=2)
    bag = W.BagWriter(str(tmp_path / "t.bag"), "bz2")
    bag.add_chunk([("/camera/image_raw", *IMG, (50, 0), later), ("/velodyne_points", *PC2, (2, 0), _cloud_msg(5, 1))])
    bag.add_chunk([("/camera/image_raw", *IMG, (49, 999999999), first)])
    bag.write()
    assert ingest.bag_first_message(str(tmp_path / "t.bag"), "/camera/image_raw", R.IMAGE_MD5) == first


# ------------------------------------------------------------------------------------------ CPU: guards on the restatement

def _tap_census(cam):
    iu, iv = R.undistort_map(cam)
    inside = R.taps_inside(iu, iv, cam.width, cam.height)
    n_out = 4 - inside.sum(0)
    x0, y0, _ = R.tap_positions(iu, iv)
    two = n_out == 2
    edges = dict(left=int((two & (x0 == -1)).sum()), right=int((two & (x0 == cam.width - 1)).sum()),
                 top=int((two & (y0 == -1)).sum()), bottom=int((two & (y0 == cam.height - 1)).sum()))
    return iu, iv, [int((n_out == k).sum()) for k in range(5)], edges


def test_restatement_identity_lens():
    for w, h in ((37, 29), (130, 67), (5, 3), (1, 1)):
        cam = cam_for(w, h, D_ZERO)
        iu, iv = R.undistort_map(cam)
        assert (iu == 32 * np.arange(w)[None, :]).all() and (iv == 32 * np.arange(h)[:, None]).all()
        for enc in R.ENCODINGS:
            src = noise_image(w, h, enc)
            assert (R.undistort(src, enc, cam) == R.to_mono8(src, enc)).all()


def test_restatement_gray_formula():
    assert R.to_mono8(np.array([[[255, 255, 255]]], np.uint8), "bgr8")[0, 0] == 255
    assert R.to_mono8(np.array([[[255, 0, 0, 7]]], np.uint8), "bgra8")[0, 0] == (1868 * 255 + 8192) >> 14    # B first, alpha ignored
    assert R.to_mono8(np.array([[[255, 0, 0, 7]]], np.uint8), "rgba8")[0, 0] == (4899 * 255 + 8192) >> 14
    src = noise_image(6, 4, "rgb8")
    assert (R.to_mono8(src, "rgb8") == R.to_mono8(src[..., ::-1], "bgr8")).all()


def test_restatement_pincushion_counts_37x29():
    cam = R.camera(30, 17.6, 29, 14.3, D_PINCUSHION, 37, 29)
    iu, iv, counts, edges = _tap_census(cam)
    assert counts == [793, 0, 80, 3, 197]            # inside, -, two taps out, three, fully outside
    assert edges == dict(left=20, right=17, top=26, bottom=17)
    assert (iu < 0).any() and (iv < 0).any()
    # a pixel whose taps straddle the border is not 0 on noise: the per-tap rule shows
    out = R.remap(noise_image(37, 29, "mono8", 1), iu, iv)
    inside = R.taps_inside(iu, iv, 37, 29)
    assert (out[(4 - inside.sum(0)) == 4] == 0).all() and (out[(4 - inside.sum(0)) == 2] != 0).sum() > 60


@pytest.mark.parametrize("w,h", [(37, 29), (130, 67)])
def test_restatement_pincushion_reaches_every_edge(w, h):
    iu, iv, counts, edges = _tap_census(cam_for(w, h, D_PINCUSHION))
    assert counts[2] > 0 and counts[3] > 0 and counts[4] > 0 and counts[1] == 0
    assert all(v > 0 for v in edges.values()), edges
    assert (iu < 0).any() and (iv < 0).any()


def test_restatement_barrel_stays_inside_and_huge_falls_outside():
    assert _tap_census(R.camera(30, 17.6, 29, 14.3, D_BARREL, 37, 29))[2] == [1073, 0, 0, 0, 0]
    iu, iv = R.undistort_map(cam_for(130, 67, D_HUGE))
    gone = iu == R.OUTSIDE
    assert gone.any() and not gone.all() and ((iv == R.OUTSIDE) == gone).all()
    assert (R.remap(np.full((67, 130), 200, np.uint8), iu, iv)[gone] == 0).all()


# fx = fy = 1, cx = cy = 0, p2 = -1/64: 32 u = 32 j - (3 j^2 + i^2) / 2 and 32 v = 32 i - i j, every step exact in fp64, so the
# codes of pixels with j + i odd sit on exact ties
TIE_CAM = R.camera(1.0, 0.0, 1.0, 0.0, (0.0, 0.0, 0.0, -1.0 / 64, 0.0), 8, 3)


def test_restatement_rounds_half_to_even_and_floors_negative_codes():
    iu, iv = R.undistort_map(TIE_CAM)
    assert iu[0].tolist() == [0, 30, 58, 82, 104, 122, 138, 150]        # 30.5, 82.5, 122.5, 150.5 go to the even code
    j, i = np.meshgrid(np.arange(8), np.arange(3))
    exact2 = 64 * j - (3 * j * j + i * i)                               # 64 u, an integer
    ties = exact2 % 2 == 1
    assert ties.sum() == 12 and (iu[ties] % 2 == 0).all() and (np.abs(2 * iu - exact2)[ties] == 1).all()
    assert (2 * iu == exact2)[~ties].all() and (iv == 32 * i - i * j).all()
    assert (np.floor(exact2 / 2 + 0.5).astype(np.int64) != iu)[ties].any()   # rounding half up would differ
    iu = np.array([[-1, -32, -33, 31]], np.int32)
    x0, _, _ = R.tap_positions(iu, np.zeros_like(iu))
    assert x0.tolist() == [[-1, -1, -2, 0]]
    assert np.rint(np.array([0.5, 1.5, 2.5, -0.5, -1.5])).tolist() == [0.0, 2.0, 2.0, -0.0, -2.0]


# ------------------------------------------------------------------------------------------ the closed loop

LOOP_CAM = R.camera(200, 161.3, 199, 118.6, (-0.30, 0.10, 0.002, -0.0015, 0.0), 320, 240)
LOOP_BOARD = dict(board=(7, 5), square=30.0, theta=0.2, centre=(175, 125), persp=(1e-4, -8e-5), seed=0)


@functools.lru_cache(maxsize=None)
def loop_case():
    """The distorted frame, the true pinhole corners, and the restatement's undistorted frame (computed once)."""
    raw, truth = R.render_board((320, 240), cam=LOOP_CAM, **LOOP_BOARD)
    flat = R.undistort(raw, "mono8", LOOP_CAM)
    raw.setflags(write=False)
    flat.setflags(write=False)
    return raw, truth, flat


def _nearest(found_uv, truth):
    d = np.linalg.norm(found_uv.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    return d.min(0)


def _detected(img):
    return cbdetect_ref.find_corners(np.asarray(img))["p"]


def test_closed_loop_on_the_cpu():
    """Restatement undistort + cbdetect_ref.find_corners: the bar of the GPU closed loop (0.25 px, the bar of
    test_synthetic_boards) is reachable by the reference alone, and not without undistortion.
    Measured: 0.055 px max / 0.032 RMS after undistortion (0.050 / 0.025 for the same board rendered without a
    lens), 11.9 px on the raw distorted frame."""
    raw, truth, flat = loop_case()
    moved = np.linalg.norm(np.stack(R.distort_points(LOOP_CAM, truth[..., 0], truth[..., 1]), -1) - truth, axis=-1)
    print("the lens moves the board's corners by %.2f .. %.2f px" % (moved.min(), moved.max()))
    assert moved.max() > 10
    err = _nearest(_detected(flat), truth)
    print("undistorted: max %.3f px, rms %.3f px over %d corners" % (err.max(), math_rms(err), err.size))
    assert err.size == 35 and err.max() < 0.25
    err_raw = _nearest(_detected(raw), truth)
    print("raw distorted frame: max %.2f px" % err_raw.max())
    assert err_raw.max() > 5


def math_rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


# ------------------------------------------------------------------------------------------ GPU helpers

def _pitched_source(px, pitch, offset):
    """The pixels as a view of a noise-filled flat device buffer: rows `pitch` bytes apart, first byte at `offset`."""
    import torch
    h, w = px.shape[:2]
    bpp = 1 if px.ndim == 2 else px.shape[2]
    host = np.random.default_rng(99).integers(0, 256, offset + h * pitch + 8, dtype=np.uint8)
    for r in range(h):
        host[offset + r * pitch: offset + r * pitch + w * bpp] = px[r].reshape(-1)
    return torch.from_numpy(host).cuda()


def _run_k11(px, encoding, cam, pitch, src_off, dst_stride, dst_off):
    """ilcc_image_to_mono8_device on a pitched source into a pitched destination pre-filled with 0xA5; returns the
    image and whether every byte outside it still holds 0xA5."""
    import torch
    h, w = px.shape[:2]
    src = _pitched_source(px, pitch, src_off)
    dst = torch.full((dst_off + h * dst_stride + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    st = CI.lib().ilcc_image_to_mono8_device(C.c_void_p(src.data_ptr() + src_off), w, h, pitch, R.ENCODINGS.index(encoding),
                                             C.byref(native(cam)) if cam is not None else None,
                                             C.c_void_p(dst.data_ptr() + dst_off), dst_stride, None)
    assert st == N.OK, N.lib().ilcc_last_error(None)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    body = flat[dst_off: dst_off + h * dst_stride].reshape(h, dst_stride)
    untouched = (flat[:dst_off] == 0xA5).all() and (flat[dst_off + h * dst_stride:] == 0xA5).all() and (body[:, w:] == 0xA5).all()
    return body[:, :w].copy(), bool(untouched)


def _layouts(w, bpp):
    """(source pitch, source offset, destination stride, destination offset): every pitch and stride kind, offsets 0 .. 3"""
    row = w * bpp
    aligned = (row + 255) // 256 * 256
    return [(row + 1, 1, w + 1, 0), (row + 13, 2, w + 13, 1), (aligned, 3, w + 1, 2), (row + 13, 1, w + 13, 3), (aligned, 0, w + 13, 0)]


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 29), (64, 8), (130, 67), (260, 3), (3, 260), (1027, 5)])
def test_map_equals_restatement(w, h):
    for name, d in LENSES.items():
        cam = cam_for(w, h, d)
        iu, iv = CI.undistort_map(native(cam))
        ru, rv = R.undistort_map(cam)
        assert iu.shape == (h, w) and (iu.cpu().numpy() == ru).all() and (iv.cpu().numpy() == rv).all(), name
    if (w, h) == (130, 67):
        assert (R.undistort_map(cam_for(w, h, D_HUGE))[0] == R.OUTSIDE).any()


@pytest.mark.gpu
def test_exact_ties_round_to_even():
    iu, iv = CI.undistort_map(native(TIE_CAM))
    ru, rv = R.undistort_map(TIE_CAM)
    assert (iu.cpu().numpy() == ru).all() and (iv.cpu().numpy() == rv).all()
    px = noise_image(8, 3, "mono8")
    assert (CI.to_mono8(px, "mono8", native(TIE_CAM)).cpu().numpy() == R.undistort(px, "mono8", TIE_CAM)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", R.ENCODINGS)
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 29), (130, 67)])
def test_pixels_equal_restatement(w, h, encoding):
    px = noise_image(w, h, encoding, seed=w + h)
    for name in ("pincushion", "barrel", "huge"):
        cam = cam_for(w, h, LENSES[name])
        want = R.undistort(px, encoding, cam)
        for pitch, soff, stride, doff in _layouts(w, R.BPP[encoding]):
            got, untouched = _run_k11(px, encoding, cam, pitch, soff, stride, doff)
            assert (got == want).all(), (name, pitch, soff, stride, doff, int((got != want).sum()))
            assert untouched, (name, pitch, soff, stride, doff)


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", R.ENCODINGS)
def test_conversion_only_equals_restatement(encoding):
    for w in (1, 3, 4, 5, 67):
        for h in (1, 7):
            px = noise_image(w, h, encoding, seed=10 * w + h)
            want = R.to_mono8(px, encoding)
            for pitch, soff, stride, doff in _layouts(w, R.BPP[encoding]):
                got, untouched = _run_k11(px, encoding, None, pitch, soff, stride, doff)
                assert (got == want).all() and untouched, (w, h, pitch, soff, stride, doff)
            assert (CI.to_mono8(px, encoding).cpu().numpy() == want).all()      # the packed route of the mirror


@pytest.mark.gpu
def test_mirror_reads_a_pitched_device_view_in_place():
    import torch
    px = noise_image(37, 29, "bgr8")
    cam = cam_for(37, 29, D_PINCUSHION)
    frame = torch.zeros((29, 50, 3), dtype=torch.uint8, device="cuda")
    frame[:, 5:42] = torch.from_numpy(px).cuda()
    assert (CI.to_mono8(frame[:, 5:42], "bgr8", native(cam)).cpu().numpy() == R.undistort(px, "bgr8", cam)).all()
    with pytest.raises(ValueError):
        CI.to_mono8(px, "mono8")
    with pytest.raises(ValueError):
        CI.to_mono8(px, "mono16")


@pytest.mark.gpu
def test_closed_loop():
    raw, truth, flat = loop_case()
    got = CI.to_mono8(np.array(raw), "mono8", native(LOOP_CAM))      # a writable copy: the shared frame stays as it is
    assert (got.cpu().numpy() == flat).all()
    b = IC.find_chessboard(got, (7, 5))
    assert b.shape[:2] in ((7, 5), (5, 7))
    d = np.linalg.norm(b.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    a, bmax = d.min(0).max(), d.min(1).max()
    print("closed loop: %.3f px / %.3f px" % (a, bmax))
    assert a < 0.25 and bmax < 0.25, (a, bmax)
    # control: without undistortion the board is lost or off by pixels
    try:
        c = IC.find_chessboard(np.array(raw), (7, 5))
    except IC.BoardNotFound:
        return
    d = np.linalg.norm(c.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    assert d.min(0).max() > 5


@pytest.mark.gpu
def test_from_a_bag_three_routes_one_file(tmp_path):
    raw, truth, flat = loop_case()
    bgr = np.repeat(np.array(raw)[:, :, None], 3, axis=2)
    bag_path, yaml_path = str(tmp_path / "cam.bag"), str(tmp_path / "cam.yaml")
    bag = W.BagWriter(bag_path, "bz2")
    bag.add_chunk([("/velodyne_points", *PC2, (1, 0), _cloud_msg(64, 3)),
                   ("/camera/image_raw", *IMG, (1, 10), R.image_msg(bgr, "bgr8", step=320 * 3 + 4))])
    bag.write()
    c = LOOP_CAM
    open(yaml_path, "w").write(_yaml(K=[c.fx, 0, c.cx, 0, c.fy, c.cy, 0, 0, 1], d=list(c.d), size=(320, 240)))
    cam = CI.read_camera_yaml(yaml_path)
    assert (cam.fx, cam.cx, cam.fy, cam.cy, tuple(cam.d)) == (c.fx, c.cx, c.fy, c.cy, c.d)

    image = CI.bag_first_image(bag_path, "/camera/image_raw", cam)
    assert image.shape == (240, 320) and (image == flat).all()      # gray replicated into B, G, R converts back to itself
    assert (CI.bag_first_image(bag_path, "/camera/image_raw") == np.array(raw)).all()
    files = [tmp_path / ("route%d.txt" % k) for k in range(3)]
    IC.save_cam_corners(str(files[0]), CI.bag_find_chessboard(bag_path, "/camera/image_raw", cam, (7, 5)))
    IC.save_cam_corners(str(files[1]), IC.find_chessboard(image, (7, 5)))
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    pgm = tmp_path / "undistorted.pgm"
    r = subprocess.run([CLI, "--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", yaml_path, "--out", str(files[2]),
                        "--pgm", str(pgm)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    blobs = [f.read_bytes() for f in files]
    assert blobs[0] == blobs[1] == blobs[2] and blobs[0].count(b"\n") in (10, 14)
    header = b"P5\n320 240\n255\n"
    payload = pgm.read_bytes()
    assert payload.startswith(header) and payload[len(header):] == image.tobytes()

    # ILCC_CAPACITY still reports the sizes
    w, h = C.c_int32(0), C.c_int32(0)
    small = np.zeros(100, np.uint8)
    st = CI.lib().ilcc_bag_first_image(0, bag_path.encode(), b"/camera/image_raw", C.byref(cam), small.ctypes.data_as(C.c_void_p),
                                       small.size, C.byref(w), C.byref(h))
    assert st == N.CAPACITY and (w.value, h.value) == (320, 240) and not small.any()
    # a camera of another size is refused; so is a topic without images
    other = CI.CameraModel.make(c.fx, c.cx, c.fy, c.cy, c.d, 640, 480)
    with pytest.raises(CI.CameraImageError) as e:
        CI.bag_first_image(bag_path, "/camera/image_raw", other)
    assert e.value.status == N.BAD_ARGUMENT
    with pytest.raises(CI.CameraImageError) as e:
        CI.bag_find_chessboard(bag_path, "/velodyne_points", cam)
    assert e.value.status == N.BAD_ARGUMENT and "no message of that type on topic" in str(e.value)
    r = subprocess.run([CLI, "--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", str(tmp_path / "missing.yaml"),
                        "--out", str(tmp_path / "x.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "can not open" in r.stderr and not (tmp_path / "x.txt").exists()


@pytest.mark.gpu
def test_input_checks():
    import torch
    L = CI.lib()
    src = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 * 80,), 0xA5, dtype=torch.uint8, device="cuda")
    cam = native(cam_for(64, 64, D_BARREL))
    sp, dp = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    MONO, BGR = 0, 1

    def call(s=sp, w=64, h=64, step=64, enc=MONO, camera=C.byref(cam), d=dp, stride=64):
        return L.ilcc_image_to_mono8_device(s, w, h, step, enc, camera, d, stride, None)

    other = native(cam_for(64, 63, D_BARREL))
    cases = [dict(s=None), dict(d=None), dict(w=0), dict(h=0), dict(w=-3), dict(step=63), dict(enc=BGR, step=64 * 3 - 1),
             dict(stride=63), dict(camera=C.byref(other)), dict(enc=5), dict(enc=-1),
             dict(d=sp), dict(d=C.c_void_p(src.data_ptr() + 64 * 63)),               # in place; the last source row
             dict(s=C.c_void_p(dst.data_ptr() + 63), h=1, camera=None)]             # the source starts on the destination's last byte
    for kw in cases:
        N.lib().ilcc_last_error(None)
        assert call(**kw) == N.BAD_ARGUMENT, kw
        assert N.lib().ilcc_last_error(None).decode(), kw
    iu = torch.full((64 * 64,), 7, dtype=torch.int32, device="cuda")
    ip = C.c_void_p(iu.data_ptr())
    assert L.ilcc_undistort_map_device(None, ip, ip, None) == N.BAD_ARGUMENT
    assert L.ilcc_undistort_map_device(C.byref(cam), None, ip, None) == N.BAD_ARGUMENT
    assert L.ilcc_undistort_map_device(C.byref(cam), ip, None, None) == N.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert (dst == 0xA5).all() and (iu == 7).all() and not src.any()       # nothing was launched
    # the same arguments, valid: adjacent ranges do not overlap
    assert call(d=C.c_void_p(dst.data_ptr()), stride=80) == N.OK
    torch.cuda.synchronize()
    assert (dst.view(64, 80)[:, :64] == 0).all() and (dst.view(64, 80)[:, 64:] == 0xA5).all()
