"""Camera corners from every CompressedImage of a bag, the part that needs no GPU (include/ilcc_jpeg_sequence.h): the header
against the Python export list, the pinned struct sizes, ilcc_jpeg_sequence_bytes against its formula restated here, and the
decode pool (csrc/jpeg_decode_pool.cpp) as a stand-alone program under ThreadSanitizer and under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import image_sequence_ref as SR
import jpeg_cases as J
import jpeg_ref as R
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_sequence as IS
from lidar_camera_calibration_amd import jpeg as JP
from lidar_camera_calibration_amd import jpeg_sequence as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# refusals of jpeg_cases whose headers parse: the scan is what fails, on a worker thread
CORRUPT_SCANS = ["a code in no table", "four ZRL", "a run of 15 at coefficient 49", "DC sum above 32767", "DC sum below -32768", "cut inside the scan"]


def test_exports_match_header():
    hdr = open(os.path.join(ROOT, "include", "ilcc_jpeg_sequence.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|uint64_t|void|double)\s+(ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(JS.JPEG_SEQUENCE_EXPORTS) and len(set(declared)) == len(declared)
    L = JS.lib()
    for s in JS.JPEG_SEQUENCE_EXPORTS:
        assert hasattr(L, s), s
    # ilcc_image_sequence_params (40) + two uint32; the result and record types are ilcc_image_sequence.h's, unchanged
    assert C.sizeof(JS.JpegSequenceParams) == 48 and JS.JpegSequenceParams.decode_threads.offset == 40
    assert C.sizeof(IS.ImageSequenceParams) == 40 and C.sizeof(IS.ImageRecord) == 48 + 8 + 4096 and C.sizeof(IS.ImageSequenceResult) == 32 + 32 + 4096
    assert C.sizeof(JP.Info) == 664
    # the headers whose export tests compare them with their own lists got none of the new names
    for name in ("ilcc_jpeg.h", "ilcc_image_sequence.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(ilcc_\w+)\s*\(", other)) & set(JS.JPEG_SEQUENCE_EXPORTS)


def test_default_params():
    sp = JS.default_params()
    want = IS.default_params()
    assert bytes(sp.seq) == bytes(want) and (sp.decode_threads, sp.reserved0) == (0, 0)


def _restated_bytes(w, h, sampling):
    """the header's formula: staged = up(2 coef_count) + up(384); device = staged + planes + up(bpp w h) + up(w h) + K10b's"""
    info = R.make_info(w, h, sampling)
    staged = SR._up(2 * info.coef_count) + SR._up(2 * 3 * 64)
    planes = sum(SR._up(64 * c.blocks_w * c.blocks_h) for c in info.comps) if sampling is not None else 0
    bpp = 1 if sampling is None else 3
    return staged, staged + planes + SR._up(bpp * w * h) + SR._up(w * h) + SR.scratch_bytes(w, h)


def test_sequence_bytes_equal_the_restated_formula():
    sizes = sorted({(J.expected()[n]["width"], J.expected()[n]["height"]) for n in J.small_fixtures()}) + [(1920, 1200), (702, 629), (480, 400)]
    assert (1, 1) in sizes and (257, 9) in sizes
    for w, h in sizes:
        for sampling in (None, "444", "422", "420"):
            layout = JP.make_info(w, h, sampling)
            assert JS.sequence_bytes(layout) == _restated_bytes(w, h, None if sampling is None else JP.SAMPLINGS[sampling]), (w, h, sampling)
            planes = JS.batch_scratch_bytes(layout, 1)
            assert planes == JP.scratch_bytes(layout) and JS.batch_scratch_bytes(layout, 7) == 7 * planes and planes % 256 == 0
    staged, device = JS.sequence_bytes(JP.make_info(1920, 1200, "420"))
    assert staged % 256 == 0 and device % 256 == 0 and staged == 2 * 64 * (240 * 150 + 2 * 120 * 75) + 512
    bad = JP.make_info(64, 64, "420")
    bad.comp[1].blocks_w += 1
    with pytest.raises(IS.ImageSequenceError) as e:
        JS.sequence_bytes(bad)
    assert e.value.status == N.BAD_ARGUMENT and "ilcc_jpeg_layout" in str(e.value)
    assert JS.batch_scratch_bytes(bad, 3) == 0


def test_entropy_decode_many_on_the_host():
    """the library's own build of the pool, from Python: every thread count gives the restatement's coefficients"""
    names = J.small_fixtures()[::7] + ["pointgrey1.jpg"]
    for threads in (1, 3, 16):
        coefs, statuses = JS.entropy_decode_many([J.data(n) for n in names], threads)
        assert statuses == [N.OK] * len(names)
        for n, c in zip(names, coefs):
            assert np.array_equal(c, J.restated(n)[1]), (n, threads)
    assert JS.entropy_decode_many([], 4) == ([], [])


def _build(tmp_path_factory, flags, tag):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("jpeg_sequence_host_check_" + tag)
    exe = str(out / "jpeg_sequence_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tests", "jpeg_sequence_host_check.cpp"), os.path.join(csrc, "jpeg_entropy.cpp"),
                    os.path.join(csrc, "jpeg_decode_pool.cpp"), "-o", exe], check=True, timeout=300)
    corrupt = []
    for k, name in enumerate(CORRUPT_SCANS):
        path = out / ("corrupt%d.jpg" % k)
        path.write_bytes(J.refusals()[name][0])
        corrupt.append(str(path))
    return exe, str(out / "coefficients.bin"), corrupt


def _run_and_compare(exe, dump, corrupt):
    names = J.small_fixtures() + J.reference_images()
    r = subprocess.run([exe, dump] + [os.path.join(J.HERE, n) for n in names] + ["--"] + corrupt, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "%d jobs (%d corrupt) on 1, 4 and 16 threads" % (len(names) + len(corrupt), len(corrupt)) in r.stdout
    for word in ("ThreadSanitizer", "AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in r.stderr, r.stderr[-3000:]
    raw = np.fromfile(dump, np.uint8)
    at = 0
    for name in names:
        count = int(raw[at:at + 8].view(np.uint64)[0])
        coef = raw[at + 8:at + 8 + 2 * count].view(np.int16)
        at += 8 + 2 * count
        assert count == J.restated(name)[0].coef_count and np.array_equal(coef, J.restated(name)[1]), name
    assert at == raw.size


def test_corrupt_scans_parse_but_do_not_decode():
    for name in CORRUPT_SCANS:
        jpg = J.refusals()[name][0]
        R.parse(jpg)
        assert J.restatement_refuses(jpg) is not None


def test_decode_pool_under_thread_sanitizer(tmp_path_factory):
    _run_and_compare(*_build(tmp_path_factory, ["-fsanitize=thread"], "tsan"))


def test_decode_pool_under_address_and_ub_sanitizers(tmp_path_factory):
    _run_and_compare(*_build(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "asan"))
