"""The JPEG batch writer on the GPU (include/ilcc_jpeg_write_sequence.h): K14b against K14, K17 byte for byte against
ilcc_jpeg_entropy_encode on the same coefficients, and the chain against ilcc_bag_save_jpeg message by message.  Every K17 case
runs with a coef_pitch that leaves slack behind every image and an output buffer filled with a sentinel that must survive
wherever K17 has nothing to write.  No tolerance anywhere; the expected bytes are never K17's own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import image_sequence_cases as IK
import jpeg_cases as J
import jpeg_ref as R
import jpeg_write_cases as K
import jpeg_write_ref as W
import stream_contract as SC
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from lidar_camera_calibration_amd import image_sequence as IS
from lidar_camera_calibration_amd import jpeg
from lidar_camera_calibration_amd import jpeg_huffman as JH
from lidar_camera_calibration_amd import jpeg_write
from lidar_camera_calibration_amd import jpeg_write_sequence as S
from lidar_camera_calibration_amd.camera_image import CameraImageError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
SLACK = 72                      # int16 behind every image's coefficients
GUARD = 256                     # bytes behind out_cap
FILL = 0xA5
MODES = {"gray": None, "444": "444", "422": "422", "420": "420"}


@pytest.fixture(scope="module", autouse=True)
def torch_stream_rotation():
    """torch hands out the 32 side streams of its pool in rotation, and which of them share a hardware queue is settled when the pool is
    made.  Tests later in the session pair consecutive draws (the controls of test_stream_contract.py need their two streams on
    different queues), so the delayed-stream cases of this module leave the rotation where they found it: a whole turn at the start
    tells the order, and at the end the pool is turned on to the same place."""
    import torch
    ring = [torch.cuda.Stream().cuda_stream for _ in range(32)]
    yield
    if len(set(ring)) == 32:
        for _ in range(32):
            if torch.cuda.Stream().cuda_stream == ring[-1]:
                break


def up16(x):
    return -(-x // 16) * 16


def host_scan(info, coef):
    """ilcc_jpeg_entropy_encode's bytes between the SOS header and EOI, None where it refuses"""
    try:
        data = jpeg_write.entropy_encode(info, coef)
    except CameraImageError:
        return None
    head = S.write_headers(info)
    assert data.startswith(head) and data.endswith(S.EOI)
    return data[len(head):-2]


def expected_rows(want):
    rows, at = [], 0
    for w in want:
        rows.append((at, 0 if w is None else len(w)))
        at += up16(0 if w is None else len(w))
    return rows, (rows[-1][0] + rows[-1][1] if rows else 0)


def run_and_compare(info, coefs, tag, want=None, out_cap=None):
    """K17 on the batch: status 0, the host's bytes and the host's placement where the host accepts and the image fits; a status and
    no bytes otherwise; every byte of the output that belongs to no placed image still the sentinel -> rows"""
    want = [host_scan(info, c) for c in coefs] if want is None else want
    count = int(info.coef_count)
    arr = np.full((len(coefs), count + SLACK), 0x5A5A, np.int16)
    for m, c in enumerate(coefs):
        arr[m, :count] = c
    rows_want, need = expected_rows(want)
    out_cap = need + 48 if out_cap is None else out_cap
    scans, rows, out = S.encode_batch(info, arr, out_cap, guard=GUARD, fill=FILL)
    untouched = np.ones(len(out), bool)
    full = False
    for m, w in enumerate(want):
        off, size = rows_want[m]
        full = full or (w is not None and off + size > out_cap)
        if w is None:
            assert rows[m]["status"] & (S.DC_RANGE | S.AC_RANGE) and rows[m]["bytes"] == 0, (tag, m, rows[m])
        elif full:
            assert rows[m]["status"] == S.CAPACITY and rows[m]["bytes"] == 0, (tag, m, rows[m])
        else:
            assert rows[m]["status"] == 0, (tag, m, hex(int(rows[m]["status"])))
            assert (int(rows[m]["offset"]), int(rows[m]["bytes"])) == (off, size), (tag, m, rows[m], off, size)
            assert scans[m] == w, (tag, m, sum(a != b for a, b in zip(scans[m], w)), len(w))
            untouched[off:off + size] = False
        if full:
            assert rows[m]["status"] & S.CAPACITY, (tag, m)
    assert (out[untouched] == FILL).all(), (tag, "bytes outside the placed scans were written to", int((out[untouched] != FILL).sum()))
    return rows


# ---- K14b against K14 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (9, 9), (17, 33), (257, 9)])
def test_k14b_equals_k14_image_by_image(size, mode):
    import torch
    w, h = size
    info = jpeg_write.write_info(w, h, MODES[mode], 90, 0)
    bpp, count, n = (1 if mode == "gray" else 3), int(info.coef_count), 5
    rng = np.random.default_rng(w * 1000 + h)
    images = [rng.integers(0, 256, (h, w) if bpp == 1 else (h, w, 3), dtype=np.uint8) for _ in range(n)]
    image_bytes = w * h * bpp
    pitch = image_bytes + 13                                   # slack behind every image, and odd addresses
    flat = np.full(n * pitch, 0xC3, np.uint8)
    for m, im in enumerate(images):
        flat[m * pitch:m * pitch + image_bytes] = im.reshape(-1)
    out = torch.full((n, count + SLACK), 0x5A5A, dtype=torch.int16, device="cuda")
    d_flat = torch.from_numpy(flat).cuda()
    got = S.fdct_batch(info, d_flat, coef_pitch=count + SLACK, out=out, image_pitch=pitch)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(d_flat.cpu().numpy(), flat)
    for m, im in enumerate(images):
        alone = jpeg_write.fdct(info, im).cpu().numpy()
        assert got[m, :count].tobytes() == alone.tobytes(), (size, mode, m, int((got[m, :count] != alone).sum()))
        assert (got[m, count:] == 0x5A5A).all(), (size, mode, m)


def test_k14b_refuses_before_any_launch():
    import torch
    info = jpeg_write.write_info(17, 33, "420", 90, 0)
    count = int(info.coef_count)
    px = torch.zeros(2 * 17 * 33 * 3, dtype=torch.uint8, device="cuda")
    coef = torch.full((2, count), 77, dtype=torch.int16, device="cuda")
    scratch = torch.zeros(S.fdct_batch_scratch_bytes(info, 2), dtype=torch.uint8, device="cuda")
    bgr8, mono8 = CI.ENCODINGS.index("bgr8"), CI.ENCODINGS.index("mono8")
    kw = dict(layout=C.pointer(info), d_src=px.data_ptr(), image_pitch=17 * 33 * 3, src_stride=51, encoding=bgr8, d_coef=coef.data_ptr(), coef_pitch=count,
              d_scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), n_images=2, reserved=0, hip_stream=0)
    bad = jpeg_write.write_info(17, 33, "420", 90, 0)
    bad.comp[1].blocks_w += 1
    cases = [({"d_src": 0}, "null"), ({"d_coef": 0}, "null"), ({"layout": C.pointer(bad)}, "ilcc_jpeg_layout"), ({"encoding": mono8}, "encoding"),
             ({"n_images": 65536}, "65535"), ({"src_stride": 50}, "src_stride"), ({"image_pitch": 17 * 33 * 3 - 1}, "image_pitch"),
             ({"coef_pitch": count - 8}, "coef_pitch"), ({"coef_pitch": count + 4}, "coef_pitch"), ({"d_coef": coef.data_ptr() + 8}, "d_coef"),
             ({"d_scratch": 0}, "d_scratch"), ({"d_scratch": scratch.data_ptr() + 4}, "d_scratch"), ({"scratch_bytes": scratch.numel() - 1}, "scratch_bytes")]
    for change, word in cases:
        job = S.FdctBatchJob(**dict(kw, **change))
        assert S.lib().ilcc_jpeg_fdct_batch_device(C.byref(job)) == N.BAD_ARGUMENT, change
        assert word in N.lib().ilcc_last_error(None).decode(), (change, N.lib().ilcc_last_error(None).decode())
    assert S.lib().ilcc_jpeg_fdct_batch_device(None) == N.BAD_ARGUMENT
    assert S.lib().ilcc_jpeg_fdct_batch_device(C.byref(S.FdctBatchJob(**dict(kw, n_images=0)))) == N.OK
    torch.cuda.synchronize()
    assert (coef == 77).all().item()                           # nothing was launched by any of them


# ---- K17 against the host encoder --------------------------------------------------------------------------------------------------

def test_k17_on_every_case_of_the_writers_grid_in_batches_by_geometry():
    """q1 / q50 / q95 / q100 of the noise, and without restarts the ramp and the checker: one batch per (size, mode, restart).  1 x 1
    gray is one block whose whole scan sits in one word with the padding; 257 x 9 and 15 x 17 in 4:2:0 have dummy blocks right of
    and below the real ones"""
    groups = {}
    for name, (kind, w, h, mode, q, r) in K.cases().items():
        groups.setdefault((w, h, mode, r), []).append(name)
    assert len(groups) == 14 * 4 * 2 and min(len(g) for g in groups.values()) >= 4
    for (w, h, mode, r), names in sorted(groups.items()):
        info = jpeg_write.write_info(w, h, W.SAMPLINGS[mode], 95, r)
        run_and_compare(info, [K.restated(n)[1] for n in names], (w, h, mode, r))


@pytest.mark.parametrize("case", [(136, 136, None, 1), (136, 136, None, 2), (136, 136, None, 3), (80, 112, "420", 1), (80, 112, "420", 2),
                                  (80, 112, "420", 3), (40, 24, "422", 1), (80, 40, "444", 3)])
def test_restart_intervals_that_wrap_the_marker_and_do_not_divide_the_mcus(case):
    w, h, mode, interval = case
    info = jpeg_write.write_info(w, h, mode, 75, interval)
    c0 = info.comp[0]
    mcus = (c0.blocks_w // c0.h) * (c0.blocks_h // c0.v)
    segments = -(-mcus // interval)
    assert segments >= 9 and (interval != 3 or mcus % 3) and ((w, h, interval) != (136, 136, 1) or segments > 256)
    rng = np.random.default_rng(w + h + interval)
    coefs = []
    for k in range(3):
        b = np.zeros((int(info.coef_count) // 64, 64), np.int64)
        b[:, 0] = rng.integers(-200, 201, len(b))
        b[:, 1:8] = rng.integers(-30, 31, (len(b), 7)) * (k + 1)
        coefs.append(b.reshape(-1).astype(np.int16))
    want = [host_scan(info, c) for c in coefs]
    assert all(b"\xff\xd7" in x and x.count(b"\xff\xd0") >= (2 if segments > 9 else 1) for x in want)    # RST7, then RST0 again: the counter wrapped
    run_and_compare(info, coefs, case, want=want)


def _scan_order(info):
    """per component: the offsets of its blocks in the order the scan holds them, and the MCU each lies in"""
    c0 = info.comp[0]
    mcus_w, mcus_h = c0.blocks_w // c0.h, c0.blocks_h // c0.v
    out = []
    for c in range(info.n_components):
        k = info.comp[c]
        out.append([(int(k.coef_offset) + ((my * k.v + dy) * k.blocks_w + mx * k.h + dx) * 64, my * mcus_w + mx)
                    for my in range(mcus_h) for mx in range(mcus_w) for dy in range(k.v) for dx in range(k.h)])
    return out


PATTERNS = ["all-zero blocks", "every AC nonzero at size 10", "ZRL chains ending at coefficient 63", "coefficients 2^s - 1", "all ones",
            "DC swings of 2047"]


def _pattern(info, what, seed):
    rng = np.random.default_rng(seed)
    n = int(info.coef_count) // 64
    b = np.zeros((n, 64), np.int64)
    if what == "all-zero blocks":                              # 6 bits a gray block, 4 a chroma block: many blocks share one word
        pass
    elif what == "every AC nonzero at size 10":                # 1658 bits a block: interior words owned by one block
        b[:, 1:] = rng.integers(512, 1024, (n, 63)) * rng.choice([-1, 1], (n, 63))
        b[:, 0] = rng.integers(-30, 31, n)
    elif what == "ZRL chains ending at coefficient 63":       # three ZRL and a run of 14; three ZRL and a run of 0 at 49; 48 alone
        b[0::3, 63] = rng.integers(1, 1024, len(b[0::3])) * rng.choice([-1, 1], len(b[0::3]))
        b[1::3, R.ZIGZAG[49]] = 5
        b[1::3, 63] = -1
        b[2::3, R.ZIGZAG[48]] = -700
        b[2::3, R.ZIGZAG[16]] = 1
    elif what == "coefficients 2^s - 1":                       # extra bits all 1: runs of 1-bits, 0xFF bytes, stuffing
        b[:, 1:] = (1 << rng.integers(1, 11, (n, 63))) - 1
        b[:, 0] = rng.integers(0, 2, n) * 1023
    elif what == "all ones":                                   # 1023 everywhere: more stuffed bytes in front of a chunk than the chunk holds
        b[:, 1:] = 1023
    elif what == "DC swings of 2047":                          # differences of +-2047 from 0 at every restart
        b[:, 1] = rng.integers(-3, 4, n)
    else:
        raise KeyError(what)
    coef = b.reshape(-1)
    if what == "DC swings of 2047":
        interval = info.restart_interval or (1 << 30)
        for blocks in _scan_order(info):
            v, step, segment = 0, 2047, -1
            for at, mcu in blocks:
                if mcu // interval != segment:
                    segment = mcu // interval
                    v, step = 0, 2047 if segment % 2 == 0 else -2047
                if abs(v + step) > 32767:
                    step = -step
                v += step
                coef[at] = v
    return coef.astype(np.int16)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", [(64, 64), (17, 33)])
def test_constructed_coefficients(size, mode):
    for interval in (0, 1, 2, 7):
        info = jpeg_write.write_info(size[0], size[1], MODES[mode], 90, interval)
        coefs = [_pattern(info, what, 100 * interval + k) for k, what in enumerate(PATTERNS)]
        want = [host_scan(info, c) for c in coefs]
        assert all(x is not None for x in want)
        ones = want[PATTERNS.index("all ones")]
        assert ones.count(b"\xff\x00") * 8 > len(ones)
        assert size != (64, 64) or ones.count(b"\xff\x00") > 4096     # more stuffed bytes in front of the last chunks than a chunk holds
        run_and_compare(info, coefs, (size, mode, interval), want=want)


def test_padding_that_completes_an_ff_and_an_ff_as_the_last_data_byte_before_rstn():
    """gray blocks whose 1-bits run into the segment's end: with the padding the last byte is 0xFF (stuffed) right in front of RSTn"""
    info = jpeg_write.write_info(64, 8, None, 90, 1)
    hits = 0
    coefs = []
    for tail in range(1, 11):
        b = np.zeros((8, 64), np.int64)
        b[:, 1:4] = (1 << tail) - 1
        b[:, 63] = 1023
        coefs.append(b.reshape(-1).astype(np.int16))
    want = [host_scan(info, c) for c in coefs]
    hits = sum(x.count(b"\xff\x00\xff\xd0") + x.count(b"\xff\x00\xff\xd3") for x in want)
    assert hits >= 2, hits
    run_and_compare(info, coefs, "ff before rst", want=want)


def test_a_refused_image_in_the_middle_of_a_batch_of_three():
    for mode in (None, "420"):
        info = jpeg_write.write_info(40, 24, mode, 90, 2)
        good = [_pattern(info, "coefficients 2^s - 1", s) for s in (1, 2)]
        for at, value, bit, words in ((int(info.comp[0].coef_offset) + 64 * 2, 2048, S.DC_RANGE, "DC difference"), (64 * 3 + 17, -1024, S.AC_RANGE, "AC value"),
                                      (int(info.comp[info.n_components - 1].coef_offset) + 64 + 5, 1024, S.AC_RANGE, "AC value")):
            bad = np.zeros(int(info.coef_count), np.int16)
            bad[at] = value
            with pytest.raises(CameraImageError) as e:
                jpeg_write.entropy_encode(info, bad)
            assert words in str(e.value)
            rows = run_and_compare(info, [good[0], bad, good[1]], (mode, at, value))
            assert int(rows[1]["status"]) == bit and int(rows[0]["status"]) == 0 and int(rows[2]["status"]) == 0
            alone = run_and_compare(info, [good[0], good[1]], "without it")
            assert (int(rows[2]["offset"]), int(rows[2]["bytes"])) == (int(alone[1]["offset"]), int(alone[1]["bytes"]))


def test_capacity_exact_and_one_byte_less():
    info = jpeg_write.write_info(33, 17, "420", 90, 2)
    coefs = [_pattern(info, what, 5) for what in ("coefficients 2^s - 1", "all-zero blocks", "every AC nonzero at size 10")]
    want = [host_scan(info, c) for c in coefs]
    _, need = expected_rows(want)
    rows = run_and_compare(info, coefs, "exact", want=want, out_cap=need)
    assert not rows["status"].any()
    rows = run_and_compare(info, coefs, "one less", want=want, out_cap=need - 1)
    assert rows["status"].tolist() == [0, 0, S.CAPACITY]
    first = len(want[0])
    rows = run_and_compare(info, coefs, "the first alone", want=want, out_cap=first)
    assert rows["status"].tolist() == [0, S.CAPACITY, S.CAPACITY]
    rows = run_and_compare(info, coefs, "none", want=want, out_cap=first - 1)
    assert rows["status"].tolist() == [S.CAPACITY] * 3
    run_and_compare(info, coefs, "no room at all", want=want, out_cap=0)
    bad = np.zeros(int(info.coef_count), np.int16)
    bad[0] = -2048
    rows = run_and_compare(info, [coefs[0], coefs[2], bad, coefs[1]], "refused behind the full one", out_cap=first + 20)
    assert rows["status"].tolist() == [0, S.CAPACITY, S.CAPACITY | S.DC_RANGE, S.CAPACITY]


def test_more_blocks_than_one_tile_of_any_scan():
    rng = np.random.default_rng(640)
    px = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    info = jpeg_write.write_info(640, 480, None, 95, 0)
    coef = jpeg_write.fdct(info, px).cpu().numpy()
    assert int(info.coef_count) // 64 == 4800
    other = jpeg_write.fdct(info, rng.integers(64, 192, (480, 640), dtype=np.uint8)).cpu().numpy()
    run_and_compare(info, [coef, other], "640 x 480 noise")
    info = jpeg_write.write_info(640, 480, None, 95, 25)       # 192 segments of 25 blocks: segments that straddle tiles
    run_and_compare(info, [coef], "640 x 480 noise, restarts")


def test_the_reference_frames_as_one_batch_of_six():
    names = J.reference_images()
    coefs = [jpeg.entropy_decode(J.data(n)) for n in names]
    assert len(coefs) == 6
    info = jpeg_write.write_info(1920, 1200, None, 95, 0)
    assert int(info.coef_count) == coefs[0].size
    rows = run_and_compare(info, coefs, "pointgrey")
    assert rows["bytes"].min() > 100000


def test_round_trip_through_k16():
    info = jpeg_write.write_info(50, 35, "420", 90, 3)
    coefs = [_pattern(info, what, 9) for what in PATTERNS[:5]]
    scans, rows, _ = S.encode_batch(info, np.stack(coefs))
    assert not rows["status"].any()
    files = [S.file_of(info, s) for s in scans]
    back, status = JH.decode_batch(files)
    assert not status.any()
    for m, c in enumerate(coefs):
        assert back[m, :c.size].tobytes() == c.tobytes(), m


def test_k17_refuses_before_any_launch():
    import torch
    info = jpeg_write.write_info(17, 33, "420", 90, 2)
    count = int(info.coef_count)
    coef = torch.zeros((2, count), dtype=torch.int16, device="cuda")
    out = torch.full((4096,), 77, dtype=torch.uint8, device="cuda")
    rows = torch.full((32,), 77, dtype=torch.uint8, device="cuda")
    need = S.huffman_encode_scratch_bytes(info, 2, 4096)
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    kw = dict(layout=C.pointer(info), d_coef=coef.data_ptr(), coef_pitch=count, d_out=out.data_ptr(), out_cap=4096, d_rows=rows.data_ptr(),
              d_scratch=scratch.data_ptr(), scratch_bytes=need, n_images=2, reserved=0, hip_stream=0)
    bad = jpeg_write.write_info(17, 33, "420", 90, 2)
    bad.comp[1].blocks_w += 1
    tables = jpeg_write.write_info(17, 33, "420", 90, 2)
    tables.comp[2].ac_table = 2
    interval = jpeg_write.write_info(17, 33, "420", 90, 2)
    interval.restart_interval = 65536
    cases = [({"d_coef": 0}, "null"), ({"d_out": 0}, "null"), ({"d_rows": 0}, "null"), ({"d_scratch": 0}, "null"), ({"layout": C.pointer(bad)}, "ilcc_jpeg_layout"),
             ({"layout": C.pointer(tables)}, "table index"), ({"layout": C.pointer(interval)}, "restart interval"), ({"n_images": 65536}, "65535"),
             ({"coef_pitch": count - 8}, "coef_pitch"), ({"coef_pitch": count + 4}, "coef_pitch"), ({"d_coef": coef.data_ptr() + 8}, "d_coef"),
             ({"d_out": out.data_ptr() + 8}, "d_out"), ({"d_rows": rows.data_ptr() + 4}, "d_rows"), ({"d_scratch": scratch.data_ptr() + 128}, "d_scratch"),
             ({"scratch_bytes": need - 1}, "scratch_bytes"), ({"out_cap": 1 << 40}, "out_cap")]
    for change, word in cases:
        job = S.EncodeJob(**dict(kw, **change))
        assert S.lib().ilcc_jpeg_huffman_encode_batch_device(C.byref(job)) == N.BAD_ARGUMENT, change
        assert word in N.lib().ilcc_last_error(None).decode(), (change, N.lib().ilcc_last_error(None).decode())
    assert S.lib().ilcc_jpeg_huffman_encode_batch_device(None) == N.BAD_ARGUMENT
    assert S.lib().ilcc_jpeg_huffman_encode_batch_device(C.byref(S.EncodeJob(**dict(kw, n_images=0)))) == N.OK
    torch.cuda.synchronize()
    assert (out == 77).all().item() and (rows == 77).all().item()       # nothing was launched by any of them
    assert S.lib().ilcc_jpeg_huffman_encode_batch_device(C.byref(S.EncodeJob(**kw))) == N.OK
    torch.cuda.synchronize()
    got = rows.cpu().numpy().view(S.ROW_DTYPE)
    assert got["status"].tolist() == [0, 0] and got["offset"].tolist() == [0, up16(int(got["bytes"][0]))]


# ---- the stream contract ------------------------------------------------------------------------------------------------------

def _k17_stream_case(name, seed):
    """two images of dense coefficients with restart interval 7; the decoy: two others of the same shape.  Host arguments: the job and
    the layout, both scribbled over once the entry has returned."""
    info = jpeg_write.write_info(64, 48, "420", 90, 7)
    count = int(info.coef_count)
    out_cap = 2 * 19200                                       # just above what two such images take: most of the buffer is scan

    def batch(s):
        coefs = [_pattern(info, "every AC nonzero at size 10", s + k) for k in range(2)]
        scans = [host_scan(info, c) for c in coefs]
        out = np.full(out_cap, SC.SENTINEL, np.uint8)
        rows = np.zeros(2, S.ROW_DTYPE)
        at = 0
        assert up16(len(scans[0])) + len(scans[1]) <= out_cap < 3 * len(scans[0])
        for m, sc in enumerate(scans):
            out[at:at + len(sc)] = np.frombuffer(sc, np.uint8)
            rows[m] = (at, len(sc), 0)
            at += up16(len(sc))
        return np.stack(coefs), out, rows

    (real, want_out, want_rows), (decoy, decoy_out, decoy_rows) = batch(seed), batch(seed + 50)
    scratch = S.huffman_encode_scratch_bytes(info, 2, out_cap)
    bufs = [SC.Buf("coef", real, decoy), SC.Buf("out", nbytes=out_cap, out=True), SC.Buf("rows", nbytes=32, out=True), SC.Buf("scratch", nbytes=scratch, scratch=True)]
    host_args = {}

    def call(p, stream):
        host_args["layout"] = jpeg_write.write_info(64, 48, "420", 90, 7)
        host_args["job"] = S.EncodeJob(C.pointer(host_args["layout"]), p["coef"], count, p["out"], out_cap, p["rows"], p["scratch"], scratch, 2, 0, stream)
        return S.lib().ilcc_jpeg_huffman_encode_batch_device(C.byref(host_args["job"]))

    def scribble():
        C.memset(C.byref(host_args["job"]), 0, C.sizeof(S.EncodeJob))
        C.memset(C.byref(host_args["layout"]), 0xFF, C.sizeof(jpeg.Info))

    return SC.Case(name, bufs, call, {"out": want_out, "rows": want_rows}, {"out": decoy_out, "rows": decoy_rows}, scribble=scribble, host_want=N.OK)


def test_k17_on_a_delayed_side_stream():
    SC.check_entry(_k17_stream_case("ilcc_jpeg_huffman_encode_batch_device", 1))


def test_two_k17_calls_with_separate_scratch_on_two_delayed_streams():
    cases = [_k17_stream_case("ilcc_jpeg_huffman_encode_batch_device two in flight %d" % k, 10 + k) for k in range(2)]
    for case, (got, ret) in zip(cases, SC.in_flight_together(cases)):
        SC.same(case, got, case.want, "the host encoder (two in flight)")
        assert ret == N.OK


@pytest.mark.parametrize("mode", ["gray", "420"])
def test_k14b_on_a_delayed_side_stream(mode):
    w, h, n = 64, 48, 2
    bpp = 1 if mode == "gray" else 3
    info = jpeg_write.write_info(w, h, MODES[mode], 100, 0)
    count = int(info.coef_count)
    ref = W.make_info(w, h, W.SAMPLINGS[mode], 100, 0)
    rng = np.random.default_rng(3)

    def batch():
        px = rng.integers(0, 256, (n, h, w) if bpp == 1 else (n, h, w, 3), dtype=np.uint8)
        return px, np.stack([W.coefficients(ref, p) for p in px])

    (real, want), (decoy, want_decoy) = batch(), batch()
    scratch = max(S.fdct_batch_scratch_bytes(info, n), 16)
    bufs = [SC.Buf("px", real, decoy), SC.Buf("coef", nbytes=2 * n * count, out=True), SC.Buf("scratch", nbytes=scratch, scratch=True)]
    host_args = {}

    def call(p, stream):
        host_args["layout"] = jpeg_write.write_info(w, h, MODES[mode], 100, 0)
        host_args["job"] = S.FdctBatchJob(C.pointer(host_args["layout"]), p["px"], w * h * bpp, w * bpp, CI.ENCODINGS.index("mono8" if bpp == 1 else "bgr8"),
                                          p["coef"], count, p["scratch"], scratch, n, 0, stream)
        return S.lib().ilcc_jpeg_fdct_batch_device(C.byref(host_args["job"]))

    def scribble():
        C.memset(C.byref(host_args["job"]), 0, C.sizeof(S.FdctBatchJob))
        C.memset(C.byref(host_args["layout"]), 0xFF, C.sizeof(jpeg.Info))

    SC.check_entry(SC.Case("ilcc_jpeg_fdct_batch_device " + mode, bufs, call, {"coef": want}, {"coef": want_decoy}, scribble=scribble, host_want=N.OK))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

SMALL = (64, 48)
COMPRESSED = ("sensor_msgs/CompressedImage", R.COMPRESSED_IMAGE_MD5)


def small_images():
    rng = np.random.default_rng(64)
    y, x = np.mgrid[0:SMALL[1], 0:SMALL[0]]
    out = []
    for k in range(8):
        im = ((x * (k + 1) + y * 3) % 256).astype(np.uint8)
        im[8:40, 8 + 2 * k:40 + 2 * k] = rng.integers(0, 256, (32, 32), dtype=np.uint8)
        out.append(im)
    return out


def small_camera():
    cam = IK.CR.camera(70.0, 31.5, 68.0, 23.25, (-0.06, 0.02, 0.0005, -0.0004, 0.0), *SMALL)
    return CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width, cam.height)


def _messages(kind):
    if kind == "raw":
        return [IK.CR.image_msg(im, "mono8", seq=k, stamp=(100 + k, 7 * k)) for k, im in enumerate(small_images())], IK.IMG
    return [R.compressed_image_msg(W.encode(IK.encode(im, "bgr8"), 90, (2, 2)), "jpeg", seq=k, stamp=(100 + k, 7 * k)) for k, im in enumerate(small_images())], COMPRESSED


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """per kind: the bag of 8 messages, and for every message what ilcc_bag_save_jpeg writes for a bag that holds it alone"""
    d = tmp_path_factory.mktemp("jpeg_write_sequence")
    out = {}
    for kind in ("raw", "compressed"):
        msgs, conn = _messages(kind)
        bag = IK.write_bag(d / (kind + ".bag"), msgs, per_chunk=3, conn=conn)
        alone = []
        for k, msg in enumerate(msgs):
            one = IK.write_bag(d / ("%s_%d.bag" % (kind, k)), [msg], conn=conn)
            path = d / ("%s_%d.jpg" % (kind, k))
            jpeg_write.bag_save_jpeg(one, IK.TOPIC, small_camera(), str(path), 90)
            alone.append(path.read_bytes())
        assert len(set(alone)) == 8
        out[kind] = (bag, alone, [len(m) for m in msgs])
    return out, d


def _files(prefix, messages=range(8)):
    return [open("%s%06d.jpg" % (prefix, k), "rb").read() for k in messages]


@pytest.mark.parametrize("kind", ["raw", "compressed"])
def test_chain_writes_what_bag_save_jpeg_writes_for_every_message(chain, kind):
    (bag, alone, lengths), d = chain[0][kind], chain[1]
    cam = small_camera()
    prefix = str(d / (kind + "_gpu_"))
    out, records = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90)
    assert (out.status, out.n_images, out.n_batches, out.n_host_encoded) == (N.OK, 8, 1, 0)
    assert _files(prefix) == alone
    assert [(r.message, r.stamp_sec, r.stamp_nsec, r.time_sec, r.route, r.file_bytes) for r in records] == \
        [(k, 100 + k, 7 * k, 50 + k, 0, len(alone[k])) for k in range(8)]
    assert out.file_bytes == sum(len(a) for a in alone) and out.d2h_bytes < out.file_bytes + 8 * 16
    # route 1: the same files, the coefficients travel
    prefix = str(d / (kind + "_host_"))
    host, records = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, huffman="host")
    assert _files(prefix) == alone and host.n_host_encoded == 8 and all(r.route == 1 for r in records)
    assert host.d2h_bytes == 8 * 2 * int(jpeg_write.write_info(64, 48, None, 90, 0).coef_count) > out.d2h_bytes
    # budgets that force three batches, by either budget
    device = S.sequence_bytes(*SMALL)
    if kind == "raw":
        staged = [-(-n // 256) * 256 for n in lengths]
        three = next(b for b in range(max(staged), sum(staged), 256) if len(IS.sequence_cut(lengths, device, b, 0)) - 1 == 3)
        prefix = str(d / "raw_staged3_")
        got, _ = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, staging_bytes=three)
        assert got.n_batches == 3 and _files(prefix) == alone
        prefix = str(d / "raw_device3_")
        got, _ = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, device_bytes=3 * device)
        assert got.n_batches == 3 and _files(prefix) == alone
    else:
        prefix = str(d / "compressed_staged3_")
        one = -(-2 * int(jpeg.parse(W.encode(IK.encode(small_images()[0], "bgr8"), 90, (2, 2))).coef_count) // 256) * 256 + 512
        got, _ = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, staging_bytes=3 * one)
        assert got.n_batches == 3 and _files(prefix) == alone
    # too little room per image: K17 flags the images that do not fit, the host encoder finishes them, the files are the same
    smallest = min(len(a) for a in alone)
    prefix = str(d / (kind + "_fallback_"))
    got, records = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, out_bytes_per_image=smallest // 2)
    assert _files(prefix) == alone and 0 < got.n_host_encoded <= 8 and got.n_host_encoded == sum(r.route for r in records)
    # a selection, and no camera
    prefix = str(d / (kind + "_sel_"))
    got, records = S.bag_save_jpeg_all(bag, IK.TOPIC, cam, prefix, 90, first=1, stride=3)
    assert [r.message for r in records] == [1, 4, 7] and _files(prefix, (1, 4, 7)) == [alone[k] for k in (1, 4, 7)]
    assert not os.path.exists(prefix + "000000.jpg")
    prefix = str(d / (kind + "_nocam_"))
    S.bag_save_jpeg_all(bag, IK.TOPIC, None, prefix, 90, max_images=2)
    one = str(d / (kind + "_nocam_one.jpg"))
    jpeg_write.bag_save_jpeg(bag, IK.TOPIC, None, one, 90)
    assert _files(prefix, (0,))[0] == open(one, "rb").read() != alone[0]


def test_chain_refusals(chain, tmp_path):
    (bag, _, _), _ = chain[0]["raw"], chain[1]
    for kw, status, word in (({"huffman": 2}, N.BAD_ARGUMENT, "route"), ({"first": 8}, N.BAD_ARGUMENT, "select no message"),
                             ({"device_bytes": 1000}, N.CAPACITY, "above staging_bytes or device_bytes")):
        with pytest.raises(S.JpegWriteSequenceError) as e:
            S.bag_save_jpeg_all(bag, IK.TOPIC, None, str(tmp_path / "x_"), 90, **kw)
        assert e.value.status == status and word in str(e.value), (kw, str(e.value))
    other = IK.CR.image_msg(np.zeros((40, 64), np.uint8), "mono8")
    mixed = IK.write_bag(tmp_path / "mixed.bag", _messages("raw")[0][:2] + [other])
    with pytest.raises(S.JpegWriteSequenceError) as e:
        S.bag_save_jpeg_all(mixed, IK.TOPIC, None, str(tmp_path / "m_"), 90)
    assert e.value.status == N.BAD_ARGUMENT and "message 2" in str(e.value) and "differs from the first selected image's" in str(e.value)
    with pytest.raises(S.JpegWriteSequenceError) as e:
        S.bag_save_jpeg_all(bag, IK.TOPIC, None, str(tmp_path / "no_such_dir" / "y_"), 90)
    assert e.value.status == N.IO_ERROR and "can not write" in str(e.value)


def test_cli_writes_the_same_files(chain, tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    (bag, alone, _), _ = chain[0]["raw"], chain[1]
    cam = IK.CR.camera(70.0, 31.5, 68.0, 23.25, (-0.06, 0.02, 0.0005, -0.0004, 0.0), *SMALL)
    yaml_path = tmp_path / "cam.yaml"
    yaml_path.write_text(IK.yaml_text(cam))
    base = [CLI, "--bag", bag, "--topic", IK.TOPIC, "--yaml", str(yaml_path)]
    for route in ("gpu", "host", None):
        prefix = str(tmp_path / ("cli_%s_" % route))
        r = subprocess.run(base + ["--all-images", "--jpg-out-all", prefix, "--quality", "90"] + (["--huffman", route] if route else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "all images: 8 files" in r.stdout, r.stdout + r.stderr
        assert ("host_encoded 8" in r.stdout) == (route == "host"), r.stdout
        assert _files(prefix) == alone
    r = subprocess.run(base + ["--jpg-out-all", str(tmp_path / "x_")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr and "--jpg-out-all" in r.stderr
