"""JPEG writing on the GPU (include/ilcc_jpeg_write.h): K14's coefficients (csrc/k14_jpeg_write.hip) over the case grid and
on constructed blocks against the numpy restatement (tests/jpeg_write_ref.py), the files of ilcc_jpeg_encode_device against
the recorded libjpeg results (tests/golden/jpeg_write/expected.json), pitched sources and guarded outputs, the refusals,
the reference's own frame written again, and the bag chain bag -> <camera><i>.jpg -> corners through the library, the
programs and the step-by-step route."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_ref as R
import jpeg_write_cases as K
import jpeg_write_ref as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import jpeg
from lidar_camera_calibration_amd import jpeg_write as JW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
PCD2IMAGE = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_pcd2image")
FILL = 0xAB
MONO8, BGR8 = 0, 1


def _info_of(name):
    _, w, h, mode, q, r = K.cases()[name]
    return JW.write_info(w, h, None if mode == "gray" else mode, q, r)


def _same_info(info, want):
    assert (info.width, info.height, info.n_components, info.restart_interval, info.coef_count, info.scan_offset) == \
        (want.width, want.height, want.n_components, want.restart_interval, want.coef_count, 0)
    for c, w in zip(info.comp, want.comps):
        assert (c.h, c.v, c.quant_index, c.dc_table, c.ac_table, c.blocks_w, c.blocks_h, c.coef_offset) == \
            (w.h, w.v, w.tq, w.td, w.ta, w.blocks_w, w.blocks_h, w.offset)
    assert np.array_equal(info.quant_array()[:2], want.quant[:2]) and not info.quant_array()[2:].any()


# ------------------------------------------------------------------------------------------ GPU: K14's coefficients

@pytest.mark.gpu
def test_k14_coefficients_equal_the_restatement_over_the_case_grid():
    """The whole buffer, dummy blocks included, for every size, mode, quality and source."""
    import torch
    bad = []
    for name in K.cases():
        want_info, want, _ = K.restated(name)
        info = _info_of(name)
        _same_info(info, want_info)
        got = JW.fdct(info, torch.from_numpy(np.array(K.source(name))).cuda()).cpu().numpy()
        if not np.array_equal(got, want):
            bad.append((name, np.flatnonzero(got != want)[:4].tolist()))
    assert not bad, "%d cases differ, first: %s" % (len(bad), bad[:6])


def _gray_blocks(blocks):
    """(n, 8, 8) uint8 blocks side by side: an (8, 8 n) image."""
    return np.ascontiguousarray(np.asarray(blocks, np.uint8).transpose(1, 0, 2).reshape(8, -1))


def _k14_gray(image, quality):
    info = JW.write_info(image.shape[1], image.shape[0], None, quality)
    rinfo = W.make_info(image.shape[1], image.shape[0], None, quality)
    return JW.fdct(info, image).cpu().numpy().reshape(-1, 64), W.coefficients(rinfo, image).reshape(-1, 64), rinfo


@pytest.mark.gpu
def test_k14_constant_and_single_pixel_blocks():
    """Constants 0, 128, 255 and one bright pixel at each of the 64 positions (on black and, dark, on white): a slip in the
    transposes or in the row / column order of the passes moves the pattern."""
    blocks = [np.full((8, 8), v) for v in (0, 128, 255)]
    for base, pixel in ((0, 255), (255, 0)):
        for k in range(64):
            b = np.full(64, base)
            b[k] = pixel
            blocks.append(b.reshape(8, 8))
    for quality in (100, 95, 50):
        got, want, _ = _k14_gray(_gray_blocks(blocks), quality)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, "quality %d: blocks that differ: %s" % (quality, bad[:16])
    got, want, _ = _k14_gray(_gray_blocks(blocks), 100)              # every divisor 8: the DCT itself
    assert (want[0] == [-1024] + [0] * 63).all() and not want[1].any() and (want[2] == [1016] + [0] * 63).all()
    assert not np.array_equal(want[3 + 1], want[3 + 8]) and want[3 + 1][8] == want[3 + 8][1] != 0   # pixel (0, 1) against pixel (1, 0)


@pytest.mark.gpu
def test_k14_quantiser_rounds_as_libjpeg_at_both_signs():
    """DC = sum(sample - 128) exactly, so a block can be built for any DC: one below, at and one above every rounding point
    d k + d / 2 of the quantiser that fits 8-bit samples, both signs, for the divisors 8 (quality 100), 16, 128 and 2040
    (quality 1: the table clamped at 255)."""
    for quality, d in ((100, 8), (95, 16), (50, 128), (1, 2040)):
        targets = []
        for k in (0, 1, 2, 3):
            for delta in (-1, 0, 1):
                c = d * k + d // 2 + delta
                targets += [c, -c]
        targets = [c for c in targets if -8192 <= c <= 8128]
        blocks = []
        for c in targets:
            b = np.full(64, 128 + c // 64)
            b[:c % 64] += 1
            assert b.sum() - 8192 == c and b.min() >= 0 and b.max() <= 255
            blocks.append(b.reshape(8, 8))
        got, want, rinfo = _k14_gray(_gray_blocks(blocks), quality)
        assert rinfo.quant[0][0] * 8 == d
        dc = [int(np.sign(c)) * ((abs(c) + d // 2) // d) for c in targets]
        assert want[:, 0].tolist() == dc                             # the restatement is the formula
        assert {abs(v) for v in dc} >= {0, 1, 2, 3}
        assert np.array_equal(got, want), quality


# ------------------------------------------------------------------------------------------ GPU: the files

@pytest.mark.gpu
def test_encode_hashes_to_the_recorded_files():
    import torch
    bad = []
    for name, (_, w, h, mode, q, r) in K.cases().items():
        data = JW.encode(torch.from_numpy(np.array(K.source(name))).cuda(), q, "420" if mode == "gray" else mode, r)
        if (len(data), K.sha256(data)) != (K.expected()[name]["bytes"], K.expected()[name]["sha256"]):
            bad.append(name)
    assert not bad, "%d files differ from libjpeg's, first: %s" % (len(bad), bad[:8])
    for name in K.committed_files():                                 # and the files kept for a segment-by-segment diff
        assert K.sha256(open(os.path.join(K.HERE, name), "rb").read()) == K.expected()[name[:-4]]["sha256"]


@pytest.mark.gpu
def test_entropy_encode_through_the_c_abi():
    for name in ("noise_17x33_420_q95_r2", "noise_257x9_gray_q1_r0", "checker_40x24_422_q100_r0"):
        info, coef, data = K.restated(name)
        mine = _info_of(name)
        assert JW.entropy_encode(mine, np.array(coef)) == data
        assert len(data) <= JW.file_bound(mine)
        back = jpeg.entropy_decode(data)
        assert np.array_equal(back, coef)


@pytest.mark.gpu
def test_round_trip_through_k13():
    """jpeg.decode(encode(px)) is the restated decode of the same bytes: every size and mode at quality 95."""
    import torch
    for name, (kind, w, h, mode, q, r) in K.cases().items():
        if (kind, q, r) != ("noise", 95, 0):
            continue
        data = JW.encode(torch.from_numpy(np.array(K.source(name))).cuda(), q, "420" if mode == "gray" else mode, r)
        assert np.array_equal(jpeg.decode(data).cpu().numpy(), R.decode(data)), name


# ------------------------------------------------------------------------------------------ GPU: source layout, guards, refusals

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise_257x9_gray_q95_r0", "noise_263x15_444_q50_r0", "noise_255x9_422_q95_r2", "noise_17x33_420_q95_r0",
                                  "noise_7x5_420_q50_r0"])
def test_pitched_sources_and_guarded_outputs(name):
    """Source pitches bpp w + 1, + 13 and a multiple of 256 at base offsets 0 .. 3 give the contiguous result; the bytes
    around the coefficient buffer and around the output file stay 0xAB."""
    import torch
    info, want, data = K.restated(name)
    mine = _info_of(name)
    px = np.array(K.source(name))
    h, w = px.shape[:2]
    row = px.reshape(h, -1).shape[1]
    _, _, _, mode, q, r = K.cases()[name]
    hs, vs = W.SAMPLINGS[mode] or (1, 1)
    enc = MONO8 if px.ndim == 2 else BGR8
    for stride in (row + 1, row + 13, -(-row // 256) * 256):
        for offset in range(4):
            src = torch.full((offset + h * stride,), 0x5C, dtype=torch.uint8, device="cuda")
            body = src[offset:].view(h, stride)
            body[:, :row] = torch.from_numpy(px.reshape(h, row)).cuda()
            # the source's own padding must not matter: another fill, the same result
            guard = torch.full((64 + 2 * info.coef_count + 64,), FILL, dtype=torch.uint8, device="cuda")
            assert guard.data_ptr() % 16 == 0
            scratch = torch.empty(max(JW.fdct_scratch_bytes(mine), 16), dtype=torch.uint8, device="cuda")
            st = JW.lib().ilcc_jpeg_fdct_device(C.byref(mine), C.c_void_p(src.data_ptr() + offset), stride, enc, C.c_void_p(guard.data_ptr() + 64),
                                                C.c_void_p(scratch.data_ptr()), scratch.numel(), None)
            assert st == N.OK, N.lib().ilcc_last_error(None)
            flat = guard.cpu().numpy()
            assert (flat[:64] == FILL).all() and (flat[-64:] == FILL).all(), (stride, offset)
            assert np.array_equal(flat[64:-64].view(np.int16), want), (stride, offset)
            out = np.full(32 + len(data) + 32, FILL, np.uint8)
            n = C.c_uint64(0)
            st = JW.lib().ilcc_jpeg_encode_device(C.c_void_p(src.data_ptr() + offset), stride, w, h, enc, q, hs, vs, r,
                                                  C.c_void_p(out.ctypes.data + 32), len(data), C.byref(n), None)
            assert (st, n.value) == (N.OK, len(data)) and out[32:-32].tobytes() == data, (stride, offset)
            assert (out[:32] == FILL).all() and (out[-32:] == FILL).all()
            view = body[:, :row] if px.ndim == 2 else torch.as_strided(src, (h, w, 3), (stride, 3, 1), offset)
            assert JW.encode(view, q, mode if px.ndim == 3 else "420", r) == data      # the Python entry reads the view in place


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    import torch
    L = JW.lib()
    src = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    coef = torch.full((1 << 15,), FILL, dtype=torch.uint8, device="cuda")
    scratch = torch.full((1 << 15,), FILL, dtype=torch.uint8, device="cuda")
    out = np.full(1 << 16, FILL, np.uint8)
    n = C.c_uint64(77)
    sp, cp, xp, op = (C.c_void_p(src.data_ptr()), C.c_void_p(coef.data_ptr()), C.c_void_p(scratch.data_ptr()), C.c_void_p(out.ctypes.data))

    # ilcc_jpeg_write_info
    info = jpeg.Info()
    for args in ((0, 8, 1, 1, 1), (8, 0, 1, 1, 1), (65536, 8, 1, 1, 1), (8, 65536, 3, 2, 2), (8, 8, 2, 1, 1), (8, 8, 4, 1, 1), (8, 8, 0, 1, 1),
                 (8, 8, 3, 1, 2), (8, 8, 3, 4, 1), (8, 8, 3, 2, 4), (8, 8, 3, 0, 0)):
        assert L.ilcc_jpeg_write_info(*args, 95, 0, C.byref(info)) == N.BAD_ARGUMENT, args
    assert L.ilcc_jpeg_write_info(8, 8, 1, 1, 1, 95, -1, C.byref(info)) == N.BAD_ARGUMENT
    assert L.ilcc_jpeg_write_info(8, 8, 1, 1, 1, 95, 0, None) == N.BAD_ARGUMENT
    assert bytes(info) == bytes(jpeg.Info())                        # a refusal writes nothing
    assert L.ilcc_jpeg_write_info(65535, 65535, 3, 2, 2, 95, 65535, C.byref(info)) == N.OK
    assert L.ilcc_jpeg_write_info(8, 8, 1, 7, 9, 95, 0, C.byref(info)) == N.OK and (info.comp[0].h, info.comp[0].v) == (1, 1)
    assert np.array_equal(JW.write_info(8, 8, None, 0).quant_array(), JW.write_info(8, 8, None, 1).quant_array())      # clamped to 1 .. 100
    assert np.array_equal(JW.write_info(8, 8, None, 1000).quant_array(), JW.write_info(8, 8, None, 100).quant_array())

    # ilcc_jpeg_fdct_device
    gray, colour = JW.write_info(64, 64, None), JW.write_info(64, 64, "420")
    moved = JW.write_info(64, 64, "420")
    moved.comp[1].coef_offset += 64
    grown = JW.write_info(64, 64, None)
    grown.comp[0].blocks_w += 1
    zero_q = JW.write_info(64, 64, None)
    zero_q.quant[0][5] = 0
    wide_q = JW.write_info(64, 64, None)
    wide_q.quant[0][63] = 256

    def fdct(i=colour, s=sp, stride=192, enc=BGR8, c=cp, x=xp, xb=1 << 15):
        return L.ilcc_jpeg_fdct_device(C.byref(i) if i is not None else None, s, stride, enc, c, x, xb, None)

    cases = [dict(i=None), dict(s=None), dict(c=None), dict(x=None), dict(i=moved), dict(i=grown, enc=MONO8), dict(i=zero_q, enc=MONO8),
             dict(i=wide_q, enc=MONO8), dict(stride=191), dict(i=gray, enc=MONO8, stride=63), dict(enc=MONO8), dict(i=gray, enc=BGR8),
             dict(enc=2), dict(enc=-1), dict(c=C.c_void_p(coef.data_ptr() + 2)), dict(c=C.c_void_p(coef.data_ptr() + 8)),
             dict(x=C.c_void_p(scratch.data_ptr() + 4)), dict(xb=JW.fdct_scratch_bytes(colour) - 1), dict(xb=0)]
    for kw in cases:
        N.lib().ilcc_last_error(None)
        assert fdct(**kw) == N.BAD_ARGUMENT, kw
        assert N.lib().ilcc_last_error(None).decode().startswith("ilcc_jpeg_fdct_device: "), kw
    assert JW.fdct_scratch_bytes(gray) == 0 and JW.fdct_scratch_bytes(moved) == 0 and JW.file_bound(moved) == 0

    # ilcc_jpeg_encode_device
    def encode(s=sp, stride=192, w=64, h=64, enc=BGR8, q=95, hs=2, vs=2, r=0, o=op, cap=1 << 16, nb=C.byref(n)):
        return L.ilcc_jpeg_encode_device(s, stride, w, h, enc, q, hs, vs, r, o, cap, nb, None)

    for kw in (dict(s=None), dict(o=None), dict(nb=None), dict(stride=191), dict(w=0), dict(h=65536), dict(enc=2), dict(hs=1, vs=2), dict(r=-1)):
        assert encode(**kw) == N.BAD_ARGUMENT, kw
    assert n.value == 0
    whole = JW.encode(src.view(64, 64, 3))
    assert encode(cap=len(whole) - 1) == N.CAPACITY and n.value == 0
    torch.cuda.synchronize()
    assert (coef == FILL).all() and (scratch == FILL).all() and not src.any()
    out[:len(whole)] = FILL                                          # what a too small cap had written up to it is unspecified
    assert (out == FILL).all()
    assert encode(cap=len(whole)) == N.OK and n.value == len(whole) and out[:len(whole)].tobytes() == whole

    # ilcc_jpeg_entropy_encode: libjpeg's limits, with the cause in the last-error text
    info = JW.write_info(8, 8, None)
    for k, value, words in ((0, 2048, "DC difference outside 11 bits"), (0, -2048, "DC difference"), (5, 1024, "AC value outside 10 bits"),
                            (63, -1024, "AC value")):
        c = np.zeros(64, np.int16)
        c[k] = value
        with pytest.raises(CI.CameraImageError) as e:
            JW.entropy_encode(info, c)
        assert e.value.status == N.BAD_ARGUMENT and words in str(e.value)
    with pytest.raises(CI.CameraImageError) as e:
        JW.entropy_encode(moved, np.zeros(moved.coef_count, np.int16))
    assert e.value.status == N.BAD_ARGUMENT


@pytest.mark.gpu
def test_save_writes_the_file_imwrite_writes(tmp_path):
    for name in ("noise_33x17_gray_q95_r0", "noise_33x17_420_q95_r0", "noise_263x15_420_q50_r0"):
        _, _, data = K.restated(name)
        path = tmp_path / (name + ".jpg")
        JW.save(str(path), np.array(K.source(name)), K.cases()[name][4])
        assert path.read_bytes() == data
    padded = np.full((17, 40), FILL, np.uint8)                       # a host view with a row pitch
    padded[:, :33] = K.source("noise_33x17_gray_q95_r0")
    st = JW.lib().ilcc_jpeg_write_file(0, str(tmp_path / "pitched.jpg").encode(), padded.ctypes.data_as(C.c_void_p), 40, 33, 17, MONO8, 95)
    assert st == N.OK and (tmp_path / "pitched.jpg").read_bytes() == K.restated("noise_33x17_gray_q95_r0")[2]
    with pytest.raises(CI.CameraImageError) as e:
        JW.save(str(tmp_path / "no" / "such" / "folder.jpg"), np.zeros((8, 8), np.uint8))
    assert e.value.status == N.IO_ERROR and "can not write" in str(e.value)


# ------------------------------------------------------------------------------------------ GPU: the reference's frame

@pytest.mark.gpu
def test_reference_frame_written_again(tmp_path):
    """encode(decode(pointgrey1.jpg), 95) is the file libjpeg writes for those pixels (a generation: not the shipped file), and
    the detector finds on it what it finds on the restatement's bytes."""
    frame = jpeg.decode(J.data("pointgrey1.jpg"))
    data = JW.encode(frame, 95)
    want = K.expected()["pointgrey1_reencoded_q95"]
    assert (len(data), K.sha256(data)) == (want["bytes"], want["sha256"]) and data != J.data("pointgrey1.jpg")
    restated = W.encode(J.restated("pointgrey1.jpg")[2], 95)
    assert K.sha256(restated) == want["sha256"]
    (tmp_path / "gpu.jpg").write_bytes(data)
    (tmp_path / "restated.jpg").write_bytes(restated)
    one = jpeg.find_chessboard(str(tmp_path / "gpu.jpg"), None, (7, 5))
    two = jpeg.find_chessboard(str(tmp_path / "restated.jpg"), None, (7, 5))
    assert one.shape[:2] in ((7, 5), (5, 7)) and one.tobytes() == two.tobytes()


# ------------------------------------------------------------------------------------------ GPU: the bag chain

@pytest.mark.gpu
def test_from_a_bag_three_routes_one_jpg_and_its_corners(tmp_path):
    import rosbag_writer as B
    import test_camera_image as TC
    raw, truth, flat = TC.loop_case()
    bag_path, yaml_path = str(tmp_path / "cam.bag"), str(tmp_path / "cam.yaml")
    bag = B.BagWriter(bag_path, "bz2")
    bag.add_chunk([("/camera/image_raw", *TC.IMG, (1, 10), TC.R.image_msg(np.array(raw), "mono8", step=320 + 4))])
    bag.write()
    c = TC.LOOP_CAM
    open(yaml_path, "w").write(TC._yaml(K=[c.fx, 0, c.cx, 0, c.fy, c.cy, 0, 0, 1], d=list(c.d), size=(320, 240)))
    cam = CI.read_camera_yaml(yaml_path)

    files = [tmp_path / ("route%d.jpg" % k) for k in range(4)]
    JW.bag_save_jpeg(bag_path, "/camera/image_raw", cam, str(files[0]))
    image = CI.bag_first_image(bag_path, "/camera/image_raw", cam)
    assert (image == flat).all()
    files[1].write_bytes(JW.encode(image, 95))
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    r = subprocess.run([CLI, "--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", yaml_path, "--jpg-out", str(files[2])],
                       capture_output=True, text=True, timeout=300)                  # get_image_corners_bag alone: no --out
    assert r.returncode == 0 and "image 320 x 240 -> " in r.stdout, r.stdout + r.stderr
    bag_txt, jpg_txt = tmp_path / "bag.txt", tmp_path / "jpg.txt"
    r = subprocess.run([CLI, "--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", yaml_path, "--out", str(bag_txt), "--jpg-out", str(files[3]),
                        "--quality", "95"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "image 320 x 240 board" in r.stdout, r.stdout + r.stderr
    blobs = [f.read_bytes() for f in files]
    assert blobs[0] == blobs[1] == blobs[2] == blobs[3] == W.encode(flat, 95)
    low = tmp_path / "q50.jpg"
    JW.bag_save_jpeg(bag_path, "/camera/image_raw", cam, str(low), quality=50)
    assert low.read_bytes() == W.encode(flat, 50)

    # the loop closes: the written file, read back by the --jpg route, gives the board the bag route finds.  The file is
    # lossy (quality 95): the corners agree as the reader's test holds the reference's own jpgs to its detector output
    r = subprocess.run([CLI, "--jpg", str(files[0]), "--out", str(jpg_txt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    from lidar_camera_calibration_amd import calib
    got, want = (calib.check_order_cam(calib.read_cam_corners(str(p), 35)) for p in (jpg_txt, bag_txt))
    d = np.linalg.norm(got - want, axis=1)
    print("bag route against --jpg route: max %.4f px" % d.max())
    assert got.shape == want.shape == (35, 2) and d.max() <= 0.5

    # refusals: bag mode only, and --out is needed unless --jpg-out is there
    for args in (["--jpg", str(files[0]), "--out", str(jpg_txt), "--jpg-out", str(tmp_path / "x.jpg")],
                 ["--bag", bag_path, "--topic", "/camera/image_raw", "--yaml", yaml_path]):
        r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--jpg-out" in r.stderr, args
    assert not (tmp_path / "x.jpg").exists()
    with pytest.raises(CI.CameraImageError) as e:
        JW.bag_save_jpeg(bag_path, "/camera/other", cam, str(tmp_path / "x.jpg"))
    assert e.value.status == N.BAD_ARGUMENT and "no message of that type on topic" in str(e.value) and not (tmp_path / "x.jpg").exists()


@pytest.mark.gpu
def test_pcd2image_jpg_out_is_the_picture_of_its_ppm(tmp_path):
    import shutil

    import rosbag_writer as B
    import test_overlay as TO
    cam, frame, pts, _ = TO.chain_case()
    bag_path, yaml_path, pose_path = str(tmp_path / "a.bag"), str(tmp_path / "cam.yaml"), str(tmp_path / "pose.bin")
    bag = B.BagWriter(bag_path, "none")
    bag.add_chunk([("/velodyne_points", *TO.PC2, (1, 0), TO._cloud_msg(pts)),
                   ("/camera/image_raw", *TO.IMG, (1, 10), TO.R.image_msg(np.array(frame), "bgr8", seq=1))])
    bag.write()
    open(yaml_path, "w").write(TO._yaml_text(cam))
    shutil.copy(os.path.join(TO.GOLD, "pointgrey.bin"), pose_path)
    ppm, jpg = tmp_path / "out.ppm", tmp_path / "out.jpg"
    base = [PCD2IMAGE, "--bag", bag_path, "--image-topic", "/camera/image_raw", "--lidar-topic", "/velodyne_points", "--yaml", yaml_path,
            "--extrinsic", pose_path, "--out", str(ppm), "--distance-valid", str(TO.DISTANCE)]
    r = subprocess.run(base + ["--jpg-out", str(jpg), "--quality", "90"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "points drawn -> " in r.stdout and "quality 90 -> " in r.stdout, r.stdout + r.stderr
    picture = np.ascontiguousarray(TO.O.read_ppm(str(ppm))[..., ::-1])           # R, G, B in the file -> B, G, R
    want = W.encode(picture, 90, (2, 2))
    assert jpg.read_bytes() == want
    assert np.array_equal(jpeg.decode(jpg.read_bytes()).cpu().numpy(), R.decode(want))
