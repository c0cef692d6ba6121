"""Bayer frames on the GPU (include/ilcc_camera_image.h): K11 and K11c demosaic bayer_rggb8 / bggr8 / gbrg8 / grbg8 sources
tap by tap (csrc/bayer_tap.h) in their one launch, held byte for byte against the numpy restatement tests/bayer_ref.py
-- conversion only and through the lens, at every pitch and base offset, with noise in every padding -- and the bag
entries and both programs take a Bayer topic the way they take any other."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bayer_ref as B
import camera_image_ref as R
import overlay_ref as O
import rosbag_writer as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import overlay as OV
from test_bayer_cpu import colour_loop_case
from test_camera_image import CLI, D_BARREL, D_PINCUSHION, D_ZERO, LOOP_CAM, _tap_census, _yaml, cam_for, native
from test_overlay import DISTANCE, _cloud_msg, _hits_on_gpu, extrinsic, scene

pytestmark = pytest.mark.gpu

IMG = (R.IMAGE_TYPE, R.IMAGE_MD5)
PC2 = ("sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5)
FILL = 0xA5
# every residue of the 4-pixel quad, rows of one quad, rows with a 1 .. 3 pixel tail, more than one workgroup both ways
SIZES = [(3, 3), (4, 3), (5, 4), (37, 29), (64, 8), (130, 67), (260, 3), (3, 260), (1027, 5)]
LENSES = {"identity": D_ZERO, "pincushion": D_PINCUSHION, "barrel": D_BARREL}


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def case(encoding, w, h, lens, channels):
    """(raw frame, the restatement's image): computed once per case, shared read-only."""
    raw = noise(w, h, seed=w + 7 * h)
    cam = None if lens is None else cam_for(w, h, LENSES[lens])
    want = B.to_mono8(raw, encoding, cam) if channels == 1 else B.to_bgr8(raw, encoding, cam)
    raw.setflags(write=False)
    want.setflags(write=False)
    return raw, want


def layouts(w, channels):
    """(source pitch, source offset, destination stride, destination offset): pitches w + 1, w + 13 and a multiple of 256,
    strides beyond the row, every base offset 0 .. 3 on both sides."""
    aligned = (w + 255) // 256 * 256
    row = w * channels
    return [(w + 1, 1, row + 1, 0), (w + 13, 2, row + 13, 1), (aligned, 3, row + 1, 2), (w + 13, 1, row + 13, 3), (aligned, 0, row + 13, 0),
            (w + 1, 0, row + 3, 2)]


def run(raw, encoding, cam, channels, pitch, src_off, dst_stride, dst_off):
    """One K11 / K11c call on a pitched source whose padding is noise, into a pitched destination pre-filled with FILL:
    the image, and whether every byte outside it still holds FILL."""
    import torch
    h, w = raw.shape
    host = np.random.default_rng(99).integers(0, 256, src_off + h * pitch + 8, dtype=np.uint8)
    for r in range(h):
        host[src_off + r * pitch: src_off + r * pitch + w] = raw[r]
    src = torch.from_numpy(host).cuda()
    dst = torch.full((dst_off + h * dst_stride + 8,), FILL, dtype=torch.uint8, device="cuda")
    entry = CI.lib().ilcc_image_to_mono8_device if channels == 1 else CI.lib().ilcc_image_to_bgr8_device
    st = entry(C.c_void_p(src.data_ptr() + src_off), w, h, pitch, CI.encoding_code(encoding), C.byref(native(cam)) if cam is not None else None,
               C.c_void_p(dst.data_ptr() + dst_off), dst_stride, None)
    assert st == N.OK, N.lib().ilcc_last_error(None)
    torch.cuda.synchronize()
    flat = dst.cpu().numpy()
    body = flat[dst_off: dst_off + h * dst_stride].reshape(h, dst_stride)
    n = w * channels
    untouched = (flat[:dst_off] == FILL).all() and (flat[dst_off + h * dst_stride:] == FILL).all() and (body[:, n:] == FILL).all()
    return body[:, :n].reshape((h, w) if channels == 1 else (h, w, 3)).copy(), bool(untouched)


def check_every_layout(encoding, w, h, lens, channels, which=slice(None)):
    raw, want = case(encoding, w, h, lens, channels)
    cam = None if lens is None else cam_for(w, h, LENSES[lens])
    for lay in layouts(w, channels)[which]:
        got, untouched = run(raw, encoding, cam, channels, *lay)
        assert (got == want).all(), (lens, lay, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert untouched, (lens, lay)


def test_layouts_cover_every_offset_and_pitch_kind():
    for channels in (1, 3):
        ls = layouts(130, channels)
        assert {l[1] for l in ls} == {l[3] for l in ls} == {0, 1, 2, 3}
        assert {l[0] for l in ls} == {131, 143, 256} and all(l[2] > 130 * channels for l in ls)


@pytest.mark.parametrize("encoding", B.PATTERNS)
@pytest.mark.parametrize("w,h", SIZES)
def test_conversion_only_equals_restatement(w, h, encoding):
    for channels in (1, 3):
        check_every_layout(encoding, w, h, None, channels)
    raw = np.array(case(encoding, w, h, None, 1)[0])                            # the packed route of the mirror
    assert (CI.to_mono8(raw, encoding).cpu().numpy() == case(encoding, w, h, None, 1)[1]).all()
    assert (CI.to_bgr8(raw, encoding).cpu().numpy() == case(encoding, w, h, None, 3)[1]).all()


@pytest.mark.parametrize("encoding", B.PATTERNS)
@pytest.mark.parametrize("w,h,lens", [(37, 29, "identity"), (130, 67, "identity"), (37, 29, "pincushion"), (130, 67, "pincushion"),
                                      (130, 67, "barrel")])
def test_through_the_lens_equals_restatement(w, h, lens, encoding):
    if lens == "pincushion":                                                     # taps outside all four edges, negative codes
        iu, iv, counts, edges = _tap_census(cam_for(w, h, D_PINCUSHION))
        assert counts[2] > 0 and counts[3] > 0 and counts[4] > 0 and all(v > 0 for v in edges.values()) and (iu < 0).any() and (iv < 0).any()
    for channels in (1, 3):
        if lens == "identity":
            assert (case(encoding, w, h, lens, channels)[1] == case(encoding, w, h, None, channels)[1]).all()
        check_every_layout(encoding, w, h, lens, channels)


def test_small_frames_through_the_lens():
    """3 x 3 .. 5 x 4 with a camera: every tap's window hangs over the frame's last column or row."""
    for encoding in B.PATTERNS:
        for w, h in ((3, 3), (4, 3), (5, 4), (3, 260)):
            for lens in ("pincushion", "barrel"):
                for channels in (1, 3):
                    check_every_layout(encoding, w, h, lens, channels, slice(0, 3))


def test_mirror_shapes():
    raw = noise(37, 29, 3)
    for bad in (np.zeros((29, 37, 3), np.uint8), np.zeros((29, 37, 1, 1), np.uint8), raw.astype(np.int16)):
        with pytest.raises(ValueError):
            CI.to_mono8(bad, "bayer_rggb8")
    with pytest.raises(ValueError):
        CI.to_bgr8(raw, "bayer_rggb16")
    with pytest.raises(CI.CameraImageError) as e:
        CI.to_mono8(noise(2, 5, 1), "bayer_rggb8")
    assert e.value.status == N.BAD_ARGUMENT and "3 x 3" in str(e.value)
    import torch
    frame = torch.zeros((29, 50), dtype=torch.uint8, device="cuda")           # a pitched device view is read in place
    frame[:, 5:42] = torch.from_numpy(raw).cuda()
    cam = cam_for(37, 29, D_PINCUSHION)
    assert (CI.to_mono8(frame[:, 5:42], "bayer_gbrg8", native(cam)).cpu().numpy() == B.to_mono8(raw, "bayer_gbrg8", cam)).all()


def test_refusals_launch_nothing():
    import torch
    L = CI.lib()
    src = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 * 64 * 3 + 64,), FILL, dtype=torch.uint8, device="cuda")
    sp, dp = src.data_ptr(), dst.data_ptr()
    RGGB = 16
    for entry, channels in ((L.ilcc_image_to_mono8_device, 1), (L.ilcc_image_to_bgr8_device, 3)):
        def call(s=sp, w=64, h=16, step=64, enc=RGGB, d=dp, stride=64 * channels):
            return entry(C.c_void_p(s), w, h, step, enc, None, C.c_void_p(d), stride, None)

        cases = [dict(w=2, h=5), dict(w=5, h=2), dict(step=63), dict(enc=5), dict(enc=15), dict(enc=20), dict(enc=17, w=2),
                 dict(d=sp), dict(d=sp + 64 * 15 + 63),                         # in place; on the source's last byte
                 dict(s=dp + 64 * channels * 16 - 1)]                            # the source starts on the destination's last byte
        for kw in cases:
            N.lib().ilcc_last_error(None)
            assert call(**kw) == N.BAD_ARGUMENT, kw
            assert N.lib().ilcc_last_error(None).decode(), kw
        torch.cuda.synchronize()
        assert (dst == FILL).all() and not src.any()
        for enc in (16, 17, 18, 19):                                            # the same arguments, valid
            assert call(enc=enc) == N.OK
        torch.cuda.synchronize()
        assert (dst[:64 * channels * 16] == 0).all() and (dst[64 * channels * 16:] == FILL).all()
        dst.fill_(FILL)
    # K14 keeps refusing anything but mono8 / bgr8
    from lidar_camera_calibration_amd import jpeg_write as JW
    info = JW.write_info(64, 16, None, 90, 0)
    coef = torch.zeros(info.coef_count, dtype=torch.int16, device="cuda")
    for enc, want in ((RGGB, N.BAD_ARGUMENT), (19, N.BAD_ARGUMENT), (0, N.OK)):
        assert JW.lib().ilcc_jpeg_fdct_device(C.byref(info), C.c_void_p(sp), 64, enc, C.c_void_p(coef.data_ptr()), None, 0, None) == want
        assert want == N.OK or "encoding" in N.lib().ilcc_last_error(None).decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ from a bag

@pytest.mark.parametrize("encoding", ["bayer_rggb8", "bayer_grbg8"])
def test_from_a_bag_of_a_bayer_topic(tmp_path, encoding):
    scene_bgr, truth = colour_loop_case()
    raw = B.mosaic(scene_bgr, encoding)
    pts = scene(20000, 4)
    bag_path, yaml_path = str(tmp_path / "cam.bag"), str(tmp_path / "cam.yaml")
    bag = W.BagWriter(bag_path, "bz2")
    bag.add_chunk([("/velodyne_points", *PC2, (1, 0), _cloud_msg(pts)),
                   ("/camera/image_raw", *IMG, (1, 10), R.image_msg(raw, encoding, step=320 + 4))])
    bag.write()
    c = LOOP_CAM
    open(yaml_path, "w").write(_yaml(K=[c.fx, 0, c.cx, 0, c.fy, c.cy, 0, 0, 1], d=list(c.d), size=(320, 240)))
    cam = CI.read_camera_yaml(yaml_path)

    flat = B.to_mono8(raw, encoding, LOOP_CAM)
    image = CI.bag_first_image(bag_path, "/camera/image_raw", cam)
    assert image.shape == (240, 320) and (image == flat).all()
    assert (CI.bag_first_image(bag_path, "/camera/image_raw") == B.to_mono8(raw, encoding)).all()

    files = [tmp_path / ("route%d.txt" % k) for k in range(3)]
    corners = CI.bag_find_chessboard(bag_path, "/camera/image_raw", cam, (7, 5))
    IC.save_cam_corners(str(files[0]), corners)
    IC.save_cam_corners(str(files[1]), IC.find_chessboard(image, (7, 5)))
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    r = subprocess.run([CLI, "--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", yaml_path, "--out", str(files[2])],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    blobs = [f.read_bytes() for f in files]
    assert blobs[0] == blobs[1] == blobs[2] and blobs[0].count(b"\n") in (10, 14)
    d = np.linalg.norm(corners.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    print("%s from the bag: %.3f px / %.3f px" % (encoding, d.min(0).max(), d.min(1).max()))
    assert d.min(0).max() < 0.25 and d.min(1).max() < 0.25                       # the bar of the mono8 loop

    # pcd2image on the same topic: the restated colour image, undistorted and drawn on by overlay_ref
    T = extrinsic()
    got, n_drawn = OV.bag_pcd2image(bag_path, "/camera/image_raw", "/velodyne_points", cam, T, distance_valid=DISTANCE)
    d_hits, m = _hits_on_gpu(pts, LOOP_CAM)
    hits = d_hits.cpu().numpy().view(O.HIT_DTYPE).reshape(-1)[:m]
    colour = O.undistort_bgr8(B.demosaic(raw, encoding), "bgr8", LOOP_CAM)
    assert (colour == B.to_bgr8(raw, encoding, LOOP_CAM)).all()
    assert n_drawn == m > 100 and (got == O.draw_hits(colour, hits)).all()
