"""K16 on the GPU (include/ilcc_jpeg_huffman.h): the Huffman scans of a batch decoded on the device, byte for byte against
ilcc_jpeg_entropy_decode on the same bytes.  Every case runs at S = 256 and at the default, with a coef_pitch that leaves slack behind
every image, filled with a sentinel that must survive.  No tolerance anywhere; the expected value is never K16's own."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_huffman_ref as H
import jpeg_ref as R
import jpeg_write_ref as W
import stream_contract as SC
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import jpeg
from lidar_camera_calibration_amd import jpeg_huffman as JH
from lidar_camera_calibration_amd import jpeg_sequence as JS
from lidar_camera_calibration_amd import jpeg_write
from lidar_camera_calibration_amd.camera_image import CameraImageError

pytestmark = pytest.mark.gpu

BITS = [256, 0]                 # 0: the default
SLACK = 72                      # int16 behind every image's coefficients
SENTINEL = 0x5A5A
CORRUPT_SCANS = ["a code in no table", "four ZRL", "a run of 15 at coefficient 49", "DC sum above 32767", "DC sum below -32768", "cut inside the scan"]
MODES = {"gray": None, "444": "444", "422": "422", "420": "420"}


def host(jpg):
    """ilcc_jpeg_entropy_decode's coefficients, None where it refuses"""
    try:
        return jpeg.entropy_decode(jpg)
    except CameraImageError:
        return None


def run_and_compare(jpgs, bits, tag, want=None, counters=False):
    """K16 on the batch: status 0 and the host's coefficients where the host accepts, a status where it refuses; the sentinel behind
    every image untouched.  -> (statuses, counters)"""
    want = [host(j) for j in jpgs] if want is None else want
    count = int(jpeg.parse(jpgs[0]).coef_count)
    coef, status, stats = JH.decode_batch(jpgs, bits, coef_pitch=count + SLACK, fill=SENTINEL, with_counters=True)
    assert coef.shape == (len(jpgs), count + SLACK)
    for m, w in enumerate(want):
        assert (coef[m, count:] == SENTINEL).all(), (tag, m, "the int16 behind the image were written to")
        if w is None:
            assert status[m] != 0, (tag, m, "the host refuses this scan")
        else:
            assert status[m] == 0, (tag, m, hex(int(status[m])))
            assert coef[m, :count].tobytes() == w.tobytes(), (tag, m, int((coef[m, :count] != w).sum()))
    return status, stats


def _geometry(name):
    e = J.expected()[name]
    return e["width"], e["height"], name.split("_")[2]


@pytest.mark.parametrize("bits", BITS)
def test_all_small_fixtures_in_batches_by_geometry(bits):
    """q50 / q95 / q100 carry different tables, r0 / r2 different segment tables: both differ inside a batch"""
    groups = {}
    for name in J.small_fixtures():
        groups.setdefault(_geometry(name), []).append(name)
    assert len(groups) > 40 and max(len(g) for g in groups.values()) >= 4
    for key, names in sorted(groups.items()):
        run_and_compare([J.data(n) for n in names], bits, key, want=[jpeg.entropy_decode(J.data(n)) for n in names])


@pytest.mark.parametrize("bits", BITS)
def test_full_frames_as_one_batch_of_six(bits):
    """1920 x 1200 gray, one segment each, 373 KB: six chunks at S = 2048 and 46 at S = 256, and a real frame settles at once"""
    names = J.reference_images()
    _, stats = run_and_compare([J.data(n) for n in names], bits, "pointgrey", want=[jpeg.entropy_decode(J.data(n)) for n in names])
    assert (stats[:, 1] >= (40 if bits == 256 else 5)).all(), stats
    print("pointgrey: S = %d: subsequences, chunks, rounds, most rounds of a chunk\n%s" % (bits or JH.DEFAULT_BITS, stats))
    assert (stats[:, 3] < 32).all(), stats                    # rounds of the slowest chunk: nowhere near the bound of 255


@pytest.mark.parametrize("bits", BITS)
def test_inputs_that_never_synchronise_reach_the_bound_on_the_gpu(bits):
    """flat images (one short pattern repeated: a decoder that starts out of phase stays out of phase) and the checker fixtures at
    q100: the rounds the kernel counts are the restatement's, and for the flat images the bound, (subsequences of the chunk) - 1.  A
    synchroniser that stopped after a fixed small number of rounds would fail here."""
    S = bits or JH.DEFAULT_BITS
    flat = [(W.encode(np.full((480, 640), 128, np.uint8), 90, None), True), (W.encode(np.full((240, 320, 3), 200, np.uint8), 90, (2, 2)), True)]
    for jpg, at_bound in flat + [(J.data("checker_40x24_420_q100.jpg"), False), (J.data("checker_40x24_gray_q100.jpg"), False)]:
        _, stats = run_and_compare([jpg], bits, "never synchronises")
        restated = H.decode_file(jpg, S)[3]
        assert len(restated) == 1 and (int(stats[0, 0]), int(stats[0, 1]), int(stats[0, 3])) == (restated[0][1], 1, restated[0][2]), (stats, restated)
        subs, rounds = restated[0][1:]
        assert subs >= 5 and (rounds == subs - 1 if at_bound else rounds >= subs // 2), restated


# ---- constructed coefficients through the host encoder -----------------------------------------------------------------------

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


def _pattern(info, what, seed):
    rng = np.random.default_rng(seed)
    n = int(info.coef_count) // 64
    b = np.zeros((n, 64), np.int64)
    if what == "all-zero blocks":                              # 6 bits a gray block: the decoder never synchronises
        pass
    elif what == "every AC nonzero at size 10":                # 26 bits a coefficient: a block spans several subsequences
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
    elif what == "DC swings of 2047":                          # sums that come near +-32767, from 0 at every restart
        b[:, 1] = rng.integers(-3, 4, n)
    else:
        raise KeyError(what)
    coef = b.reshape(-1)
    if what == "DC swings of 2047":
        interval = info.restart_interval or (1 << 30)
        for blocks in _scan_order(info):
            v, step, segment = 0, 2047, -1
            for at, mcu in blocks:
                if mcu // interval != segment:                 # the predictor starts from 0 again
                    segment = mcu // interval
                    v, step = 0, 2047 if segment % 2 == 0 else -2047
                if abs(v + step) > 32767:
                    step = -step
                v += step
                coef[at] = v
    return coef.astype(np.int16)


PATTERNS = ["all-zero blocks", "every AC nonzero at size 10", "ZRL chains ending at coefficient 63", "coefficients 2^s - 1", "DC swings of 2047"]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", [(64, 64), (17, 33)])
def test_constructed_coefficients(size, mode, bits):
    """one batch per geometry: every pattern at restart intervals 0, 1, 2 and 7 -- the restart interval and with it the segment table
    differ inside the batch"""
    jpgs, want, tags = [], [], []
    for interval in (0, 1, 2, 7):
        info = jpeg_write.write_info(size[0], size[1], MODES[mode], 90, interval)
        for k, what in enumerate(PATTERNS):
            coef = _pattern(info, what, 100 * interval + k)
            jpgs.append(jpeg_write.entropy_encode(info, coef))
            want.append(coef)
            tags.append((what, interval))
    for j, w in zip(jpgs, want):                               # the encoder's own round trip, so that `want` is the host decoder's
        assert np.array_equal(jpeg.entropy_decode(j), w)
    status, stats = run_and_compare(jpgs, bits, (size, mode, tags), want=want)
    dense = tags.index(("every AC nonzero at size 10", 0))
    if size == (64, 64) and bits == 256:
        # a block of 63 coefficients of some 26 bits is six subsequences of 256 bits long: more subsequences than blocks, so some complete none
        assert int(stats[dense, 0]) > int(jpeg_write.write_info(64, 64, MODES[mode], 90, 0).coef_count) // 64, stats[dense]
    if size == (64, 64) and mode == "444" and bits == 256:
        assert int(stats[dense, 1]) >= 3, stats[dense]          # one segment of at least three chunks: the chunk carry


@pytest.mark.parametrize("bits", BITS)
def test_a_single_segment_of_three_chunks_and_an_image_of_one_mcu(bits):
    info = jpeg_write.write_info(256, 64, None, 90, 0)
    coef = _pattern(info, "every AC nonzero at size 10", 7)
    _, stats = run_and_compare([jpeg_write.entropy_encode(info, coef)], bits, "chunk carry", want=[coef])
    assert int(stats[0, 1]) == -(-int(stats[0, 0]) // 256) and int(stats[0, 1]) >= (3 if bits == 256 else 1), stats
    for w, h, mode in ((8, 8, None), (16, 16, "420"), (16, 8, "422"), (1, 1, "444")):
        info = jpeg_write.write_info(w, h, mode, 90, 0)
        assert info.comp[0].blocks_w == info.comp[0].h and info.comp[0].blocks_h == info.comp[0].v
        jpgs, want = [], []
        for k, what in enumerate(PATTERNS):
            want.append(_pattern(info, what, k))
            jpgs.append(jpeg_write.entropy_encode(info, want[-1]))
        run_and_compare(jpgs, bits, ("one MCU", w, h, mode), want=want)


def _with_segment_lengths(jpg, lengths):
    """the file (restart interval 1) with segment k padded with bytes the decoder never reaches to lengths[k % len] unstuffed bytes"""
    info = R.parse(jpg)
    segs, end = R._split_scan(jpg, info.scan_offset)
    out = jpg[:info.scan_offset]
    for k, (buf, rst) in enumerate(segs):
        target = lengths[k % len(lengths)]
        assert len(buf) <= target, (len(buf), target)
        buf = buf + bytes((37 * i + k) & 0x7F for i in range(target - len(buf)))
        out += buf.replace(b"\xff", b"\xff\x00") + (b"" if rst is None else bytes([0xFF, 0xD0 + rst]))
    return out + jpg[end:]


@pytest.mark.parametrize("bits", BITS)
def test_segments_of_one_byte_less_than_a_subsequence_exactly_one_and_one_byte_more(bits):
    """S / 8 - 1, S / 8 and S / 8 + 1 bytes: one subsequence, one that is full, and a second one of 8 bits"""
    S = bits or JH.DEFAULT_BITS
    for mode in (None, "420"):
        info = jpeg_write.write_info(17, 33, mode, 90, 1)
        rng = np.random.default_rng(S)
        b = np.zeros((int(info.coef_count) // 64, 64), np.int16)
        b[:, 0] = rng.integers(-8, 9, len(b))
        b[:, 1] = rng.integers(-1, 2, len(b))
        coef = b.reshape(-1)
        jpg = _with_segment_lengths(jpeg_write.entropy_encode(info, coef), [S // 8 - 1, S // 8, S // 8 + 1])
        rows = JH.scan_prepare(jpg)[1]
        assert sorted(set(rows[:, 1].tolist())) == [S // 8 - 1, S // 8, S // 8 + 1]
        _, stats = run_and_compare([jpg, jpg], bits, ("segment lengths", mode), want=[coef, coef])
        n = len(rows)
        assert int(stats[0, 0]) == sum(-(-8 * int(c) // S) for c in rows[:, 1]) and int(stats[0, 1]) == n


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _neighbours(jpg):
    """two intact fixtures of the file's geometry"""
    info = jpeg.parse(jpg)
    mode = "gray" if info.n_components == 1 else {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[(info.comp[0].h, info.comp[0].v)]
    names = [n for n in J.small_fixtures() if _geometry(n) == (info.width, info.height, mode)]
    assert len(names) >= 2
    return J.data(names[0]), J.data(names[-1])


@pytest.mark.parametrize("bits", BITS)
def test_a_corrupt_scan_in_the_middle_of_a_batch_of_three(bits):
    cases = {name: J.refusals()[name][0] for name in CORRUPT_SCANS}
    many = J.data(J.MANY_BLOCKS)
    cases["a gray scan cut at 40 bytes"] = many[:R.parse(many).scan_offset + 40]
    for name, bad in cases.items():
        assert host(bad) is None, name
        a, b = _neighbours(bad)
        status, _ = run_and_compare([a, bad, b], bits, name)
        assert status[1] != 0 and status[0] == 0 and status[2] == 0, (name, status)
    bit = {"a code in no table": JH.NO_CODE, "four ZRL": JH.RUN_PAST_63, "DC sum above 32767": JH.DC_RANGE, "cut inside the scan": JH.ENDS_EARLY}
    for name, want in bit.items():
        a, b = _neighbours(cases[name])
        assert int(run_and_compare([a, cases[name], b], bits, name)[0][1]) & want, name
    # a valid scan with garbage bits behind its last block: the host never reads them, K16 must not report them
    for name in (J.MANY_BLOCKS, J.COLOUR, "noise_50x35_444_q95_r2.jpg"):
        jpg = J.data(name)
        eoi = jpg.rindex(b"\xff\xd9")
        garbage = bytes(np.random.default_rng(5).integers(0, 255, 300, dtype=np.uint8))
        longer = jpg[:eoi] + garbage + jpg[eoi:]
        assert np.array_equal(host(longer), host(jpg))
        a, b = _neighbours(jpg)
        status, _ = run_and_compare([a, longer, b], bits, ("garbage behind", name))
        assert not status.any()


def _device_job(jpgs, pitch_slack=8):
    import torch
    infos = [jpeg.parse(j) for j in jpgs]
    b = JH.Batch([JH.scan_prepare(j, i) for j, i in zip(jpgs, infos)])
    pitch = int(infos[0].coef_count) + pitch_slack
    t = {k: torch.from_numpy(v).cuda() for k, v in (("scans", b.scans), ("tables", b.tables), ("segments", b.segments), ("images", b.images))}
    t["coef"] = torch.zeros((b.n, pitch), dtype=torch.int16, device="cuda")
    t["status"] = torch.zeros(b.n, dtype=torch.int32, device="cuda")
    t["scratch"] = torch.zeros(max(JH.scratch_bytes(b.n), 16), dtype=torch.uint8, device="cuda")
    kw = dict(layout=infos[0], d_scans=t["scans"].data_ptr(), scans_bytes=b.scans_bytes, d_tables=t["tables"].data_ptr(), d_segments=t["segments"].data_ptr(),
              n_segments=b.n_segments, d_images=t["images"].data_ptr(), n_images=b.n, max_segments=b.max_segments, d_coef=t["coef"].data_ptr(),
              coef_pitch=pitch, d_status=t["status"].data_ptr(), d_scratch=t["scratch"].data_ptr(), scratch_nbytes=t["scratch"].numel())
    return kw, t


def test_k16_refuses_before_any_launch():
    import torch
    jpgs = [J.data("noise_17x33_420_q50_r2.jpg"), J.data("noise_17x33_420_q95_r0.jpg")]
    kw, t = _device_job(jpgs)
    JH.huffman_batch(**kw)
    torch.cuda.synchronize()
    good = t["coef"].clone()
    assert not t["status"].any().item() and np.array_equal(good[0, :-8].cpu().numpy(), jpeg.entropy_decode(jpgs[0]))
    t["coef"].fill_(77)
    bad_layout = jpeg.parse(jpgs[0])
    bad_layout.comp[1].blocks_w += 1
    cases = [({"d_scans": 0}, "null"), ({"d_tables": 0}, "null"), ({"d_segments": 0}, "null"), ({"d_images": 0}, "null"), ({"d_coef": 0}, "null"),
             ({"d_status": 0}, "null"), ({"d_scratch": 0}, "null"), ({"layout": bad_layout}, "ilcc_jpeg_layout"),
             ({"n_images": 65536}, "65535"), ({"coef_pitch": kw["coef_pitch"] - 16}, "coef_pitch"), ({"coef_pitch": kw["coef_pitch"] + 4}, "coef_pitch"),
             ({"d_coef": kw["d_coef"] + 8}, "d_coef"), ({"d_tables": kw["d_tables"] + 8}, "d_tables"), ({"d_segments": kw["d_segments"] + 8}, "d_segments"),
             ({"d_images": kw["d_images"] + 4}, "d_images"), ({"d_status": kw["d_status"] + 2}, "d_status"), ({"d_scratch": kw["d_scratch"] + 8}, "d_scratch"),
             ({"scratch_nbytes": 31}, "scratch_bytes"), ({"max_segments": 0}, "max_segments"), ({"max_segments": kw["n_segments"] + 1}, "max_segments")]
    cases += [({"subsequence_bits": s}, "subsequence_bits") for s in (1, 128, 255, 768, 4096, 1 << 31)]
    for change, word in cases:
        with pytest.raises(CameraImageError) as e:
            JH.huffman_batch(**dict(kw, **change))
        assert e.value.status == N.BAD_ARGUMENT, change
        assert word in N.lib().ilcc_last_error(None).decode(), (change, N.lib().ilcc_last_error(None).decode())
    assert JH.lib().ilcc_jpeg_huffman_batch_device(None) == N.BAD_ARGUMENT
    JH.huffman_batch(**dict(kw, n_images=0, max_segments=0))       # nothing to do: ILCC_OK, no launch
    torch.cuda.synchronize()
    assert (t["coef"] == 77).all().item()                          # nothing was launched by any of them
    for s in JH.SUBSEQUENCE_BITS:
        JH.huffman_batch(**dict(kw, subsequence_bits=s))
        torch.cuda.synchronize()
        assert torch.equal(t["coef"][:, :-8], good[:, :-8]) and (t["coef"][:, -8:] == 77).all().item(), s


@pytest.mark.parametrize("names", [["noise_50x35_gray_q50_r0.jpg", "ramp_50x35_gray_q95_r2.jpg", "noise_50x35_gray_q95_r0.jpg"],
                                   ["noise_33x17_420_q50_r2.jpg", "ramp_33x17_420_q95_r0.jpg"]])
def test_k16_then_k13b_gives_the_restated_pixels(names):
    import torch
    jpgs = [J.data(n) for n in names]
    layout = jpeg.parse(jpgs[0])
    coef, status = JH.decode_batch(jpgs)
    assert not status.any()
    quants = np.stack([JS.quant_rows(jpeg.parse(j)) for j in jpgs])
    px = JS.idct_batch(layout, quants, torch.from_numpy(coef).cuda()).cpu().numpy()
    for m, n in enumerate(names):
        assert np.array_equal(px[m], J.restated(n)[2]), n


# ---- the stream contract ------------------------------------------------------------------------------------------------------

def _stream_case(name, seed, bits):
    """two images of dense coefficients (nearly every output byte depends on the input) with restart interval 7; the decoy: two
    others of the same shape.  Host arguments: the job and the layout, both scribbled over once the entry has returned."""
    info = jpeg_write.write_info(64, 48, "420", 90, 7)
    count = int(info.coef_count)

    def batch(s):
        want = [_pattern(info, "every AC nonzero at size 10", s + k) for k in range(2)]
        return JH.Batch([JH.scan_prepare(jpeg_write.entropy_encode(info, w)) for w in want]), want

    (real, want), (decoy, want_decoy) = batch(seed), batch(seed + 50)
    n_scans = max(len(real.scans), len(decoy.scans))
    assert real.n_segments == decoy.n_segments and real.max_segments == decoy.max_segments

    def padded(b):
        return np.concatenate([b.scans, np.zeros(n_scans - len(b.scans), np.uint8)])

    pitch = count + 8
    bufs = [SC.Buf("scans", padded(real), padded(decoy)), SC.Buf("tables", real.tables, decoy.tables), SC.Buf("segments", real.segments, decoy.segments),
            SC.Buf("images", real.images, decoy.images), SC.Buf("coef", nbytes=2 * 2 * pitch, out=True), SC.Buf("status", nbytes=8, out=True),
            SC.Buf("scratch", nbytes=64, scratch=True)]

    def expected(coefs):
        out = np.full((2, pitch), SC.SENTINEL | (SC.SENTINEL << 8), np.uint16).view(np.int16)
        for m in range(2):
            out[m, :count] = coefs[m]
        return out

    host_args = {}

    def call(p, stream):
        host_args["layout"] = jpeg_write.write_info(64, 48, "420", 90, 7)
        host_args["job"] = JH.Job(C.pointer(host_args["layout"]), p["scans"], n_scans, p["tables"], p["segments"], p["images"], p["coef"], pitch, p["status"],
                                  p["scratch"], 64, 2, real.n_segments, real.max_segments, bits, stream)
        return JH.lib().ilcc_jpeg_huffman_batch_device(C.byref(host_args["job"]))

    def scribble():
        C.memset(C.byref(host_args["job"]), 0, C.sizeof(JH.Job))
        C.memset(C.byref(host_args["layout"]), 0xFF, C.sizeof(jpeg.Info))

    return SC.Case(name, bufs, call, {"coef": expected(want), "status": np.zeros(2, np.uint32)},
                   {"coef": expected(want_decoy), "status": np.zeros(2, np.uint32)}, scribble=scribble, host_want=N.OK)


@pytest.mark.parametrize("bits", BITS)
def test_k16_on_a_delayed_side_stream(bits):
    SC.check_entry(_stream_case("ilcc_jpeg_huffman_batch_device S=%d" % bits, 1, bits))


def test_two_k16_calls_with_separate_scratch_on_two_delayed_streams():
    cases = [_stream_case("ilcc_jpeg_huffman_batch_device two in flight %d" % k, 10 + k, 256 if k else 0) for k in range(2)]
    for case, (got, ret) in zip(cases, SC.in_flight_together(cases)):
        SC.same(case, got, case.want, "the restatement (two in flight)")
        assert ret == N.OK


# ---- the chain: route 1 (K16) against route 0 (the host pool) -----------------------------------------------------------------------

import os                                                            # noqa: E402
import subprocess                                                    # noqa: E402

import image_sequence_cases as K                                     # noqa: E402
from lidar_camera_calibration_amd import camera_image as CI          # noqa: E402
from lidar_camera_calibration_amd import image_corners as IC         # noqa: E402
from lidar_camera_calibration_amd import image_sequence as IS        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")
BOARD = (7, 5)
COMPRESSED = ("sensor_msgs/CompressedImage", R.COMPRESSED_IMAGE_MD5)
_jpgs = {}


def chain_jpgs(mode, quality=95):
    """the nine chain images of tests/test_jpeg_sequence.py as JPEG files by the project's writer, gray or bgr8 4:2:0"""
    if (mode, quality) not in _jpgs:
        grays = [im for im, _ in K.chain_images()]
        _jpgs[(mode, quality)] = [jpeg_write.encode(g if mode == "gray" else K.encode(g, "bgr8"), quality, "420") for g in grays]
    return _jpgs[(mode, quality)]


def _bag(path, jpgs, per_chunk=4):
    msgs = [R.compressed_image_msg(j, "jpeg", seq=k, stamp=(100 + k, 7 * k)) for k, j in enumerate(jpgs)]
    return K.write_bag(path, msgs, per_chunk=per_chunk, conn=COMPRESSED)


def _summary(out, records):
    return ((out.status, out.n_images, out.n_ok, out.n_used, out.ref_image, out.rows, out.cols, out.gate, out.spread_rms, out.spread_max,
             out.board().tobytes()), [bytes(r) for r in records])


@pytest.fixture(scope="module")
def bags(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_huffman")
    return {mode: _bag(d / ("nine_%s.bag" % mode), chain_jpgs(mode)) for mode in ("gray", "420")}


def _route_staged(jpgs):
    out = []
    for j in jpgs:
        info = jpeg.parse(j)
        msg = R.compressed_image_msg(j, "jpeg", seq=0, stamp=(0, 0))
        out.append(JH.sequence_bytes(info, len(j), JH.scan_bound(info, len(j))[1]))
        assert len(msg) > len(j)
    return out


@pytest.mark.parametrize("mode", ["gray", "420"])
def test_chain_route_1_equals_route_0_field_for_field(bags, mode):
    jpgs, bag = chain_jpgs(mode), bags[mode]
    base = JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD)
    assert base[0].status == N.OK and base[0].n_images == 9 and sum(r.status == N.OK for r in base[1]) >= 5
    got = JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, huffman="gpu")
    assert got[0].n_batches == 1 and _summary(*got) == _summary(*base)
    cam = K.chain_camera()
    cam = CI.CameraModel.make(cam.fx, cam.cx, cam.fy, cam.cy, cam.d, cam.width, cam.height)
    assert _summary(*JS.bag_corners_all_compressed_images(bag, K.TOPIC, cam, BOARD, raise_on_failure=False, huffman="gpu")) == \
        _summary(*JS.bag_corners_all_compressed_images(bag, K.TOPIC, cam, BOARD, raise_on_failure=False))
    # a budget that forces three batches, by either budget; neither the cut nor the threads change a byte
    sizes = _route_staged(jpgs)
    staged, device = [s for s, _ in sizes], max(d for _, d in sizes)
    three = next(b for b in range(max(staged), sum(staged), 256) if len(IS.sequence_cut(staged, device, b, 0)) - 1 == 3)
    for staging, budget, threads in ((three, 0, 1), (0, 3 * device, 4)):
        out, records = JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, staging_bytes=staging, device_bytes=budget, decode_threads=threads,
                                                            huffman="gpu")
        assert out.n_batches == len(IS.sequence_cut(staged, device, staging, budget)) - 1 == 3, (staging, budget, out.n_batches)
        assert _summary(out, records) == _summary(*base), (staging, budget)
    # what the copy moves: the files, not the coefficients
    assert sum(staged) < 9 * JS.sequence_bytes(jpeg.parse(jpgs[0]))[0]
    with pytest.raises(IS.ImageSequenceError) as e:
        JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, huffman=2)
    assert e.value.status == N.BAD_ARGUMENT and "reserved0" in str(e.value)


def test_chain_route_1_with_one_image_of_another_quality_and_restart_intervals(tmp_path):
    jpgs = list(chain_jpgs("420")[:4])
    jpgs[1] = chain_jpgs("420", 80)[1]
    g = K.encode(K.chain_images()[2][0], "bgr8")
    jpgs[2] = jpeg_write.encode(g, 95, "420", restart_interval=5)      # message 2 brings 100s of segments, its neighbours one each
    assert len(JH.scan_prepare(jpgs[2])[1]) > 100 and len(JH.scan_prepare(jpgs[0])[1]) == 1
    bag = _bag(tmp_path / "mixed.bag", jpgs, per_chunk=2)
    base = JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, raise_on_failure=False)
    assert any(r.status == N.OK for r in base[1])
    assert _summary(*JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, raise_on_failure=False, huffman="gpu")) == _summary(*base)


def test_chain_route_1_ends_on_a_corrupt_scan_as_route_0_does(tmp_path, bags):
    gray = chain_jpgs("gray")
    cut = gray[2][:jpeg.parse(gray[2]).scan_offset + 40]
    no_code = gray[2][:jpeg.parse(gray[2]).scan_offset] + b"\xff\x00" * 400 + b"\xff\xd9"
    r1 = jpeg_write.encode(K.chain_images()[2][0], 95, "420", restart_interval=9)
    at = r1.index(b"\xff\xd1", jpeg.parse(r1).scan_offset)
    out_of_order = r1[:at + 1] + b"\xd3" + r1[at + 2:]
    for name, bad, words in (("cut", cut, "ends early"), ("no_code", no_code, "in no table"), ("rst", out_of_order, "restart marker")):
        bag = _bag(tmp_path / (name + ".bag"), gray[:2] + [bad] + gray[3:5], per_chunk=2)
        texts = []
        for route in ("host", "gpu"):
            with pytest.raises(IS.ImageSequenceError) as e:
                JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, huffman=route)
            texts.append((e.value.status, str(e.value)))
        assert texts[0] == texts[1] and texts[0][0] == N.BAD_ARGUMENT and "message 2" in texts[0][1] and words in texts[0][1], (name, texts)
    # two bad images of different kinds in one batch: the lowest one is named, whichever stage finds it
    for name, bad in (("bits_then_rst", {1: no_code, 3: out_of_order}), ("rst_then_bits", {1: out_of_order, 3: no_code}), ("bits_twice", {1: cut, 3: no_code})):
        bag = _bag(tmp_path / (name + ".bag"), [bad.get(k, gray[k]) for k in range(5)], per_chunk=2)
        texts = []
        for route in ("host", "gpu"):
            with pytest.raises(IS.ImageSequenceError) as e:
                JS.bag_corners_all_compressed_images(bag, K.TOPIC, None, BOARD, huffman=route)
            texts.append((e.value.status, str(e.value)))
        assert texts[0] == texts[1] and "message 1" in texts[0][1], (name, texts)
    out, _ = JS.bag_corners_all_compressed_images(bags["gray"], K.TOPIC, None, BOARD, max_images=2, huffman="gpu")
    assert out.status == N.OK                                  # the process is as good as before


def test_cli_with_huffman_gpu_writes_the_same_file(tmp_path, bags):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    yaml_path = tmp_path / "cam.yaml"
    yaml_path.write_text(K.yaml_text(K.chain_camera()))
    base = [CLI, "--bag", bags["gray"], "--topic", K.TOPIC, "--yaml", str(yaml_path)]
    files = {}
    for route in ("host", "gpu"):
        fused, report = tmp_path / ("fused_%s.txt" % route), tmp_path / ("report_%s.txt" % route)
        r = subprocess.run(base + ["--out", str(fused), "--all-images", "--report", str(report), "--huffman", route], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "all images: status 0 images 9" in r.stdout, r.stdout + r.stderr
        files[route] = (fused.read_bytes(), report.read_bytes())
    assert files["host"] == files["gpu"] and len(files["gpu"][0]) > 100
    r = subprocess.run(base + ["--out", str(tmp_path / "x.txt"), "--huffman", "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr and "--huffman need it" in r.stderr
    r = subprocess.run(base + ["--out", str(tmp_path / "x.txt"), "--all-images", "--huffman", "fast"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--huffman" in r.stderr
