"""Bayer frames (include/ilcc_camera_image.h), the part that needs no GPU: the numpy restatement tests/bayer_ref.py is
written twice and the two are held against each other; hand-computed answers pin its roundings; the parser takes the
four names through ilcc_image_parse_any only; csrc/bayer_tap.h -- the code K11 runs per tap -- reproduces the restatement
as a stand-alone program under AddressSanitizer and UBSan; and the restatement alone closes the loop from a colour
scene behind a colour filter array to the chessboard's corners."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bayer_ref as B
import camera_image_ref as R
import cbdetect_ref
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import camera_image as CI
from test_camera_image import LOOP_BOARD, LOOP_CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(3, 3), (4, 3), (3, 4), (5, 4), (6, 5), (37, 29), (130, 67)]


def noise(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def distinct(w, h):
    """Raw values that differ between any two pixels close to each other (w, h <= 16 here: all differ)."""
    return ((np.arange(h)[:, None] * 16 + np.arange(w)[None, :]) * 37 % 251).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the two statements agree

@pytest.mark.parametrize("encoding", B.PATTERNS)
@pytest.mark.parametrize("w,h", SIZES)
def test_positional_rules_equal_the_scanning_loop(encoding, w, h):
    for raw in (noise(w, h, seed=w + 3 * h), np.full((h, w), 255, np.uint8)):
        colour, gray = B.demosaic(raw, encoding), B.demosaic(raw, encoding, gray=True)
        assert colour.shape == (h, w, 3) and gray.shape == (h, w) and colour.dtype == gray.dtype == np.uint8
        assert colour.tobytes() == B.demosaic_scan(raw, encoding).tobytes()
        assert gray.tobytes() == B.demosaic_scan(raw, encoding, gray=True).tobytes()


def test_names_codes_and_site_colours():
    assert B.BAYER_ENCODINGS == CI.BAYER_ENCODINGS == {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19}
    assert [CI.encoding_code(n) for n in R.ENCODINGS + B.PATTERNS] == [0, 1, 2, 3, 4, 16, 17, 18, 19]
    with pytest.raises(ValueError):
        CI.encoding_code("mono16")
    assert CI.ENCODINGS == R.ENCODINGS                                  # the five-tuple stays what callers index
    assert B.site_colours("bayer_rggb8", 3, 3).tolist() == [list("rgr"), list("gbg"), list("rgr")]
    assert B.site_colours("bayer_bggr8", 2, 2).tolist() == [list("bg"), list("gr")]
    assert B.site_colours("bayer_grbg8", 2, 2).tolist() == [list("gr"), list("bg")]
    assert B.site_colours("bayer_gbrg8", 2, 2).tolist() == [list("gb"), list("rg")]
    for small in ((2, 5), (5, 2)):
        for fn in (B.demosaic, B.demosaic_scan):
            with pytest.raises(ValueError):
                fn(noise(*small), "bayer_rggb8")


# ------------------------------------------------------------------------------------------ a uniform colour

@pytest.mark.parametrize("encoding", B.PATTERNS)
def test_uniform_colour_comes_back_exactly(encoding):
    rng = np.random.default_rng(5)
    colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)] + [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(20)]
    for w, h in ((3, 3), (4, 5), (9, 6)):
        for r, g, b in colours:
            scene = np.empty((h, w, 3), np.uint8)
            scene[...] = (b, g, r)
            raw = B.mosaic(scene, encoding)
            assert (B.demosaic(raw, encoding) == scene).all(), (r, g, b)               # borders included
            want = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14                       # K11's gray of that colour
            assert (B.demosaic(raw, encoding, gray=True) == want).all(), (r, g, b)
            assert (R.to_mono8(scene, "bgr8") == want).all()


# ------------------------------------------------------------------------------------------ hand-computed answers

def _everywhere(raw, encoding):
    """A 3 x 3 frame has one interior pixel, which the border rule repeats: its B, G, R and Y."""
    colour, gray = B.demosaic(np.array(raw, np.uint8), encoding), B.demosaic(np.array(raw, np.uint8), encoding, gray=True)
    assert (colour == colour[1, 1]).all() and (gray == gray[1, 1]).all()
    return tuple(int(v) for v in colour[1, 1]), int(gray[1, 1])


def test_known_answers_3x3():
    # rggb: the centre is a B site.  cross 0 + 1 + 0 + 0 = 1 -> (1 + 2) >> 2 = 0; diagonals 0 + 1 + 1 + 0 = 2 -> (2 + 2) >> 2 = 1
    # Y = (4 * 1868 * 9 + 9617 * 1 + 4899 * 2 + 32768) >> 16 = 119431 >> 16 = 1
    assert _everywhere([[0, 0, 1], [0, 9, 1], [1, 0, 0]], "bayer_rggb8") == ((9, 0, 1), 1)
    # the same bytes as bggr: the centre is an R site, the diagonals are blue
    assert _everywhere([[0, 0, 1], [0, 9, 1], [1, 0, 0]], "bayer_bggr8") == ((1, 0, 9), (4 * 4899 * 9 + 9617 * 1 + 1868 * 2 + 32768) >> 16)
    # grbg: the centre is a G site of a "B G" row.  B = (0 + 1 + 1) >> 1 = 1 (the pair (0, 1) rounds up), R = (2 + 3 + 1) >> 1 = 3
    # Y = (2 * 9617 * 7 + 1868 * 1 + 4899 * 5 + 16384) >> 15 = 177385 >> 15 = 5
    assert _everywhere([[5, 2, 5], [0, 7, 1], [5, 3, 5]], "bayer_grbg8") == ((1, 7, 3), 5)
    # gbrg: the same site in an "R G" row: the horizontal pair is red, the vertical one blue
    assert _everywhere([[5, 2, 5], [0, 7, 1], [5, 3, 5]], "bayer_gbrg8") == ((3, 7, 1), (2 * 9617 * 7 + 4899 * 1 + 1868 * 5 + 16384) >> 15)
    # gray at its rounding boundaries.  B site: 4 * 1868 * 143 + 4899 * 16 + 32768 = 1179648 = 18 * 65536 exactly -> 18
    assert _everywhere([[4, 0, 4], [0, 143, 0], [4, 0, 4]], "bayer_rggb8") == ((143, 0, 4), 18)
    # ... and 4 * 1868 * 246 + 9617 * 22 + 4899 * 3 + 32768 = 2097151 = 32 * 65536 - 1 -> 31
    assert _everywhere([[1, 5, 1], [6, 246, 5], [1, 6, 0]], "bayer_rggb8") == ((246, 6, 1), 31)
    # G site: 2 * 9617 * 142 + 1868 * 0 + 4899 * 1 + 16384 = 2752511 = 84 * 32768 - 1 -> 83; the gray of its B,G,R = (0, 142, 1)
    # would be (4899 + 9617 * 142 + 8192) >> 14 = 84: gray is made from the raw sums
    assert _everywhere([[9, 1, 9], [0, 142, 0], [9, 0, 9]], "bayer_grbg8") == ((0, 142, 1), 83)
    assert int(R.to_mono8(np.array([[[0, 142, 1]]], np.uint8), "bgr8")[0, 0]) == 84


def test_known_answers_4x4():
    raw = np.array([[1, 2, 4, 8], [16, 32, 64, 128], [3, 5, 7, 9], [11, 13, 17, 19]], np.uint8)
    # rggb interior: (1,1) B site: B 32, G (16+64+2+5+2)>>2 = 22, R (1+4+3+7+2)>>2 = 4
    #                (2,1) G site of a "G B" row: G 64, B (32+128+1)>>1 = 80, R (4+7+1)>>1 = 6
    #                (1,2) G site of an "R G" row: G 5, R (3+7+1)>>1 = 5, B (32+13+1)>>1 = 23
    #                (2,2) R site: R 7, G (5+9+64+17+2)>>2 = 24, B (32+128+13+19+2)>>2 = 48
    inner = np.array([[[32, 22, 4], [80, 64, 6]], [[23, 5, 5], [48, 24, 7]]], np.uint8)
    # Y: (4*1868*32 + 9617*87 + 4899*15 + 32768) >> 16 = 1182036 >> 16 = 18;  (2*9617*64 + 1868*160 + 4899*11 + 16384) >> 15 = 48
    #    (2*9617*5 + 4899*10 + 1868*45 + 16384) >> 15 = 245604 >> 15 = 7;      (4*4899*7 + 9617*95 + 1868*192 + 32768) >> 16 = 22
    inner_y = np.array([[18, 48], [7, 22]], np.uint8)
    pick = [0, 0, 1, 1]                                                        # clamp(0..3, 1, 2) - 1
    assert (B.demosaic(raw, "bayer_rggb8") == inner[pick][:, pick]).all()
    assert (B.demosaic(raw, "bayer_rggb8", gray=True) == inner_y[pick][:, pick]).all()


# ------------------------------------------------------------------------------------------ relations between the patterns

@pytest.mark.parametrize("w,h", [(6, 5), (37, 29)])
def test_pattern_relations_on_interior_pixels(w, h):
    S = noise(w, h, seed=7)
    rggb, rggb_y = B.demosaic(S, "bayer_rggb8"), B.demosaic(S, "bayer_rggb8", gray=True)
    assert (B.demosaic(S, "bayer_bggr8") == rggb[..., ::-1]).all()             # red and blue change places
    # grbg on S without its first column is rggb on S, one column on: interior pixels of the shorter frame
    grbg, grbg_y = B.demosaic(S[:, 1:], "bayer_grbg8"), B.demosaic(S[:, 1:], "bayer_grbg8", gray=True)
    assert (grbg[1:-1, 1:-1] == rggb[1:-1, 2:-1]).all() and (grbg_y[1:-1, 1:-1] == rggb_y[1:-1, 2:-1]).all()
    gbrg, gbrg_y = B.demosaic(S[1:], "bayer_gbrg8"), B.demosaic(S[1:], "bayer_gbrg8", gray=True)
    assert (gbrg[1:-1, 1:-1] == rggb[2:-1, 1:-1]).all() and (gbrg_y[1:-1, 1:-1] == rggb_y[2:-1, 1:-1]).all()
    # gray is not the gray of the demosaiced colour: the roundings differ somewhere on noise, never by more than a level
    twice = R.to_mono8(rggb, "bgr8").astype(int)
    assert np.abs(twice - rggb_y).max() <= 1 and ((twice != rggb_y).any() or w * h < 100)     # 6 x 5 has 12 interior pixels


@pytest.mark.parametrize("encoding", B.PATTERNS)
def test_border_repeats_its_inner_neighbour(encoding):
    for w, h in ((3, 3), (4, 3), (7, 6), (16, 9)):
        raw = distinct(w, h)
        for out in (B.demosaic(raw, encoding), B.demosaic(raw, encoding, gray=True)):
            assert (out[0] == out[1]).all() and (out[-1] == out[-2]).all()                 # corners included
            assert (out[:, 0] == out[:, 1]).all() and (out[:, -1] == out[:, -2]).all()
        if w > 4 and h > 4:
            assert (B.demosaic(raw, encoding)[1] != B.demosaic(raw, encoding)[2]).any()   # not a constant image


# ------------------------------------------------------------------------------------------ the parser

def _raises(fn):
    with pytest.raises(CI.CameraImageError) as e:
        fn()
    assert e.value.status == N.BAD_ARGUMENT
    return str(e.value)


@pytest.mark.parametrize("encoding", R.ENCODINGS + B.PATTERNS)
def test_parse_image_any_round_trip(encoding):
    bpp = CI.BYTES_PER_PIXEL[encoding]
    px = np.random.default_rng(2).integers(0, 256, (5, 7) if bpp == 1 else (5, 7, bpp), dtype=np.uint8)
    row = 7 * bpp
    for step in (row, row + 1, row + 13):
        msg = R.image_msg(px, encoding, step=step, seq=9, stamp=(12, 34), frame_id="pointgrey")
        lay = CI.parse_image_any(msg)
        assert (lay.height, lay.width, lay.step, lay.encoding_name, lay.encoding) == (5, 7, step, encoding, CI.encoding_code(encoding))
        assert (lay.seq, lay.stamp_sec, lay.stamp_nsec, lay.frame_id, lay.is_bigendian) == (9, 12, 34, b"pointgrey", 0)
        assert lay.data_bytes == step * 5 and lay.data_offset + lay.data_bytes == len(msg)
        data = np.frombuffer(msg, np.uint8, lay.data_bytes, lay.data_offset).reshape(5, step)
        assert (data[:, :row].reshape(px.shape) == px).all()


def test_parse_image_any_refusals_and_the_narrow_parser():
    px = noise(7, 5)
    for enc in ("mono16", "bayer_rggb16", "bayer_rggb", "BAYER_RGGB8", "bayer_rggb8 "):
        assert enc in _raises(lambda: CI.parse_image_any(R.image_msg(px, enc)))
    for w, h in ((2, 5), (5, 2), (1, 1)):
        assert "3 x 3" in _raises(lambda: CI.parse_image_any(R.image_msg(noise(w, h), "bayer_gbrg8")))
    assert CI.parse_image_any(R.image_msg(noise(2, 1), "mono8")).width == 2          # the minimum is Bayer's alone
    assert CI.parse_image_any(R.image_msg(noise(3, 3), "bayer_gbrg8")).encoding == 18
    assert "step" in _raises(lambda: CI.parse_image_any(R.image_msg(px, "bayer_bggr8", step=6, data=bytes(6 * 5))))
    good = R.image_msg(px, "bayer_grbg8")
    for cut in (0, 3, 11, 20, 30, 40, len(good) - 1):
        _raises(lambda: CI.parse_image_any(good[:cut]))
    for enc in B.PATTERNS:                                                           # ilcc_image_parse keeps refusing them, by name
        assert enc in _raises(lambda: CI.parse_image(R.image_msg(px, enc)))


# ------------------------------------------------------------------------------------------ csrc/bayer_tap.h under sanitizers

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/bayer_host_check.cpp + csrc/bayer_tap.h only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("bayer_host_check")
    exe = str(out / "bayer_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wall", "-I" + csrc, os.path.join(ROOT, "tests", "bayer_host_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe, str(out / "cases.bin")


def test_tap_code_under_sanitizers(host_check):
    exe, dump = host_check
    assert '#include "bayer_tap.h"' in open(os.path.join(ROOT, "tests", "bayer_host_check.cpp")).read()
    n = 0
    with open(dump, "wb") as f:
        for k, encoding in enumerate(B.PATTERNS):
            assert B.BAYER_ENCODINGS[encoding] - 16 == k
            for w, h in SIZES[:-1] + [(9, 7), (8, 8)]:
                for raw in (noise(w, h, seed=11 * w + h + k), np.full((h, w), 255, np.uint8)):
                    f.write(struct.pack("<3i", k, w, h) + raw.tobytes() + B.demosaic(raw, encoding).tobytes()
                            + B.demosaic(raw, encoding, gray=True).tobytes())
                    n += 1
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.startswith("%d cases" % n) and "every tap, window and quad reproduced" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ the closed loop

TINT_BGR = (0.55, 0.85, 1.0)       # a warm cast: the board's white is (121, 187, 220), so the three raw planes differ


@functools.lru_cache(maxsize=None)
def colour_loop_case():
    """The existing loop's distorted frame tinted into a colour scene, and the true pinhole corners (computed once)."""
    gray, truth = R.render_board((320, 240), cam=LOOP_CAM, **LOOP_BOARD)
    scene = np.rint(gray[..., None].astype(np.float64) * np.array(TINT_BGR)).astype(np.uint8)
    scene.setflags(write=False)
    return scene, truth


@functools.lru_cache(maxsize=None)
def colour_loop_flat(encoding):
    """The restatement's undistorted gray frame of the scene seen through `encoding`'s filter array."""
    scene, _ = colour_loop_case()
    flat = B.to_mono8(B.mosaic(scene, encoding), encoding, LOOP_CAM)
    flat.setflags(write=False)
    return flat


LOOP_BAR = 0.25        # px: the bar of the mono8 loop (test_camera_image.test_closed_loop_on_the_cpu)


@pytest.mark.parametrize("encoding", B.PATTERNS)
def test_closed_loop_on_the_restatement(encoding):
    """Colour scene -> colour filter array -> demosaiced gray -> undistorted -> cbdetect_ref.find_corners.
    Measured, worst distance to the true pinhole corners over the 35 / RMS: rggb 0.090 / 0.043 px, bggr 0.069 / 0.036,
    gbrg 0.062 / 0.036, grbg 0.069 / 0.035 (the mono8 loop: 0.055 / 0.032).  The worst is below half of the mono8 loop's
    0.25 px, so that bar stands here unchanged."""
    _, truth = colour_loop_case()
    found = cbdetect_ref.find_corners(np.asarray(colour_loop_flat(encoding)))["p"]
    d = np.linalg.norm(found.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2).min(0)
    print("%s: max %.3f px, rms %.3f px over %d corners" % (encoding, d.max(), float(np.sqrt(np.mean(d * d))), d.size))
    assert d.size == 35 and d.max() < LOOP_BAR
