"""K16, the part that needs no GPU (include/ilcc_jpeg_huffman.h): the header against the Python export list and the pinned struct
sizes; the plain-Python restatement of the staged decoder (tests/jpeg_huffman_ref.py) against jpeg_ref.entropy_decode, and on the
inputs on which the decoder never synchronises; ilcc_jpeg_scan_prepare against the restatement, on constructed scans and on every
refusal; and csrc/jpeg_scan_prepare.cpp as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_huffman_ref as H
import jpeg_ref as R
import jpeg_write_ref as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import jpeg as JP
from lidar_camera_calibration_amd import jpeg_huffman as JH
from lidar_camera_calibration_amd.camera_image import CameraImageError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_header_and_structs_have_their_sizes():
    hdr = open(os.path.join(ROOT, "include", "ilcc_jpeg_huffman.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|uint64_t|void|double)\s+(ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(JH.JPEG_HUFFMAN_EXPORTS) and len(set(declared)) == len(declared)
    L = JH.lib()
    for s in JH.JPEG_HUFFMAN_EXPORTS:
        assert hasattr(L, s), s
    for name, (cls, size) in JH.STRUCT_SIZES.items():
        assert C.sizeof(cls) == size, name
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), hdr), name          # the header states the same size
    assert JH.Job.hip_stream.offset == 104 and JH.Table.maxcode.offset == 1024 and JH.Table.values.offset == 1160
    assert not re.search(r"\(.*void\*\s*hip_stream", hdr)                                 # the stream travels inside the job
    assert JH.DEFAULT_BITS == int(re.search(r"#define ILCC_JPEG_HUFFMAN_DEFAULT_BITS (\d+)u", hdr).group(1))
    for bit in ("NO_CODE", "RUN_PAST_63", "DC_CATEGORY", "DC_RANGE", "ENDS_EARLY", "BAD_ROWS"):
        value = int(re.search(r"#define ILCC_JPEG_HUFFMAN_%s\s+0x([0-9a-f]+)u" % bit, hdr).group(1), 16)
        assert getattr(JH, bit) == getattr(H, bit) == value
    # the headers whose export tests compare them with their own lists got none of the new names
    for name in ("ilcc_jpeg.h", "ilcc_jpeg_sequence.h", "ilcc_jpeg_write.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(ilcc_\w+)\s*\(", other)) & set(JH.JPEG_HUFFMAN_EXPORTS)
    assert JH.scratch_bytes(0) == 0 and JH.scratch_bytes(7) == 7 * 16


@pytest.mark.parametrize("bits", [256, 1024])
def test_restatement_equals_the_sequential_decoder_on_every_small_fixture(bits):
    for name in J.small_fixtures():
        info, want, _ = J.restated(name)
        _, coef, status, rounds = H.decode_file(J.data(name), bits)
        assert status == 0 and np.array_equal(coef, want), (name, bits)
        assert all(r <= max(n - 1, 0) for _, n, r in rounds), (name, rounds)


def test_restatement_does_not_depend_on_the_chunk_size():
    """chunks of 3 subsequences: the exact exit of a chunk carries into the next one"""
    for name in J.small_fixtures()[::9] + ["checker_40x24_420_q100.jpg", "noise_50x35_444_q95_r2.jpg"]:
        _, coef, status, rounds = H.decode_file(J.data(name), 256, chunk=3)
        assert status == 0 and np.array_equal(coef, J.restated(name)[1]), name
        assert max(n for _, n, _ in rounds) <= 3


def _flat(shape, value, sampling):
    return W.encode(np.full(shape, value, np.uint8), 90, sampling)


def test_restatement_on_the_inputs_that_never_synchronise():
    """A flat image's scan is one short pattern repeated (6 bits a gray block): a decoder that starts out of phase stays out of
    phase, so subsequence i is right only after round i and the rounds reach the bound, (subsequences of the chunk) - 1.  (The
    round that would only confirm that nothing changed is not run: after n - 1 rounds every subsequence is exact.)  The colour
    image is the flat value 200: at 128 every DC difference is 0, an MCU is 32 bits and every subsequence starts in phase by
    luck."""
    for jpg, bits in ((_flat((480, 640), 128, None), 1024), (_flat((240, 320, 3), 200, (2, 2)), 1024), (_flat((240, 320, 3), 200, (2, 2)), 256)):
        info, coef, status, rounds = H.decode_file(jpg, bits)
        assert status == 0 and np.array_equal(coef, R.entropy_decode(jpg, info))
        assert len(rounds) == 1 and rounds[0][1] >= 10 and rounds[0][2] == rounds[0][1] - 1, rounds
    # the checker fixtures at q100: long codes, and still out of phase for all but the last few subsequences
    for name, subsequences in (("checker_40x24_420_q100.jpg", 15), ("checker_40x24_gray_q100.jpg", 11)):
        _, coef, status, rounds = H.decode_file(J.data(name), 1024)
        assert status == 0 and np.array_equal(coef, J.restated(name)[1])
        assert len(rounds) == 1 and rounds[0][1] == subsequences and subsequences - 3 <= rounds[0][2] <= subsequences - 1, rounds
    # a decoder that gave up after a fixed small number of rounds would be wrong here: far more than 3 are needed
    assert H.decode_file(_flat((480, 640), 128, None), 1024)[3][0][2] == 28


def test_restatement_flags_what_the_sequential_decoder_refuses_inside_a_scan():
    for name in ("a code in no table", "four ZRL", "a run of 15 at coefficient 49", "DC sum above 32767", "DC sum below -32768", "cut inside the scan"):
        jpg = J.refusals()[name][0]
        for bits in (256, 1024):
            assert H.decode_file(jpg, bits)[2] != 0, name
    want = {"a code in no table": H.NO_CODE, "four ZRL": H.RUN_PAST_63, "DC sum above 32767": H.DC_RANGE, "cut inside the scan": H.ENDS_EARLY}
    for name, bit in want.items():
        assert H.decode_file(J.refusals()[name][0], 256)[2] & bit, name


def _library_equals_restatement(jpg):
    info = R.parse(jpg)
    scan, rows, tables = H.prepare(jpg, info)
    got_scan, got_rows, got_tables = JH.scan_prepare(jpg)
    assert got_scan.tobytes() == scan
    assert got_rows.tolist() == [list(r) for r in rows]
    assert bytes(got_tables) == H.packed_tables(tables)
    nb, ns = JH.scan_bound(JP.parse(jpg), len(jpg))
    assert len(scan) <= nb and ns == len(rows)
    return scan, rows


def test_scan_prepare_equals_the_restatement_on_every_fixture():
    intervals = set()
    for name in J.small_fixtures() + J.reference_images():
        _, rows = _library_equals_restatement(J.data(name))
        intervals.add(len(rows) > 1)
    assert intervals == {False, True}


def _with_raw_scan(jpg, raw):
    """the file with its entropy-coded bytes replaced by `raw`, as they are"""
    return jpg[:R.parse(jpg).scan_offset] + raw


def test_scan_prepare_on_constructed_scans():
    g = J.data(J.GRAY)
    # runs of 0xFF in front of a stuffed 0x00 are one data byte 0xFF; in front of a marker they are fill bytes
    scan, rows = _library_equals_restatement(_with_raw_scan(g, b"\x12\xff\xff\x00\x34\xff\xff\xff\x00\xff\x00\x56\xff\xff\xd9"))
    assert scan == b"\x12\xff\x34\xff\xff\x56" and rows == [(0, 6, 0, 2)]
    # a scan that ends in 0xFF, and in a run of them: the data has stopped, the run is not data
    for tail in (b"\xff", b"\xff\xff\xff"):
        scan, rows = _library_equals_restatement(_with_raw_scan(g, b"\x12\x34" + tail))
        assert scan == b"\x12\x34" and rows == [(0, 2, 0, 2)]
    scan, _ = _library_equals_restatement(_with_raw_scan(g, b""))
    assert scan == b""
    # r = 1: one segment per MCU; the rows tile the scan
    many = J.data(J.MANY_BLOCKS)
    info = R.parse(many)
    coef = R.entropy_decode(many, info)
    jpg = W.entropy_encode(W.make_info(info.width, info.height, None, 50, restart_interval=1), coef)
    assert b"\xff\xdd\x00\x04\x00\x01" in jpg
    scan, rows = _library_equals_restatement(jpg)
    assert len(rows) == 7 * 5 and [r[2:] for r in rows] == [(k, 1) for k in range(35)]
    assert all(rows[k][0] + rows[k][1] == rows[k + 1][0] for k in range(34)) and rows[-1][0] + rows[-1][1] == len(scan)
    assert np.array_equal(H.decode(R.parse(jpg), scan, rows, H.prepare(jpg, R.parse(jpg))[2], 256)[0], coef)
    # markers out of order, a marker missing: the decoder's words
    r2 = J.data("noise_31x16_gray_q50_r2.jpg")
    at = r2.index(b"\xff\xd1")
    for bad in (r2[:at + 1] + b"\xd2" + r2[at + 2:], r2[:at] + r2[at + 2:], r2[:at]):
        with pytest.raises(CameraImageError) as e:
            JH.scan_prepare(bad)
        assert e.value.status == N.BAD_ARGUMENT and "ends early" in str(e.value) and "restart marker" in str(e.value)
        with pytest.raises(R.JpegRefusal):
            H.prepare(bad, R.parse(bad))
    # fill bytes in front of a restart marker change nothing
    padded = r2[:at] + b"\xff\xff" + r2[at:]
    assert JH.scan_prepare(padded)[0].tobytes() == JH.scan_prepare(r2)[0].tobytes()


def test_scan_prepare_refuses_what_the_host_decoder_refuses_outside_the_bits_in_its_words():
    inside = 0
    for name, (jpg, cause, words) in J.refusals().items():
        try:
            info = JP.parse(jpg)
        except CameraImageError as e:                        # headers that do not parse: prepare says the same without an info
            with pytest.raises(CameraImageError) as p:
                JH.scan_prepare(jpg, JP.Info(), scan_cap=len(jpg), segment_cap=4)
            assert p.value.status == e.status and words in str(p.value), name
            continue
        try:
            JP.entropy_decode(jpg, info)
            raise AssertionError(name)
        except CameraImageError as e:
            host = e
        try:
            JH.scan_prepare(jpg, info)
        except CameraImageError as p:                        # several scans, DNL behind the scan
            assert p.status == host.status and words in str(p) and str(p) == str(host), name
            continue
        inside += 1                                          # what is wrong is inside the bits: K16's part
        assert H.decode_file(jpg, 256)[2] != 0, name
    assert inside == 6
    g = J.data(J.GRAY)
    other = JP.parse(J.data(J.COLOUR))
    with pytest.raises(CameraImageError) as e:
        JH.scan_prepare(g, other, scan_cap=len(g), segment_cap=4)
    assert e.value.status == N.BAD_ARGUMENT and "info is not ilcc_jpeg_parse's of these bytes" in str(e.value)
    scan, rows, _ = JH.scan_prepare(g)
    for kw in ({"scan_cap": len(scan) - 1}, {"segment_cap": 0}):
        with pytest.raises(CameraImageError) as e:
            JH.scan_prepare(g, **kw)
        assert e.value.status == N.CAPACITY, kw
    assert JH.scan_prepare(g, scan_cap=len(scan), segment_cap=1)[0].tobytes() == scan.tobytes()


def test_scan_prepare_under_address_and_ub_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    exe = str(tmp_path / "jpeg_huffman_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "jpeg_huffman_host_check.cpp"),
                    os.path.join(csrc, "jpeg_entropy.cpp"), os.path.join(csrc, "jpeg_scan_prepare.cpp"), "-o", exe], check=True, timeout=300)
    # two files with restart intervals; in the second pair the bytes between two restart markers are cut out
    names = ["noise_50x35_444_q95_r2.jpg", "noise_31x16_gray_q50_r2.jpg"]
    empties = []
    for k, name in enumerate(names):
        jpg = J.data(name)
        a, b = jpg.index(b"\xff\xd0", R.parse(jpg).scan_offset), jpg.index(b"\xff\xd1", R.parse(jpg).scan_offset)
        assert a < b
        path = tmp_path / ("empty%d.jpg" % k)
        path.write_bytes(jpg[:a + 2] + jpg[b:])
        empties.append(str(path))
    r = subprocess.run([exe] + [os.path.join(J.HERE, n) for n in names] + ["--"] + empties, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "%d prefixes" % sum(len(J.data(n)) for n in names) in r.stdout and "2 empty segments accepted" in r.stdout
    for word in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in r.stderr, r.stderr[-3000:]


def test_chain_bytes_equal_the_restated_formula():
    """the header's arithmetic: staged = up(data) + up(8496) + up(384) + up(24) + up(16 segments); device = staged + up(2 coef_count) +
    512 + what ilcc_jpeg_sequence_bytes counts behind its own staged bytes"""
    from lidar_camera_calibration_amd import jpeg_sequence as JS

    def up(x):
        return -(-x // 256) * 256

    for w, h, sampling in ((1920, 1200, None), (702, 629, "420"), (64, 48, "422"), (35, 50, "444")):
        layout = JP.make_info(w, h, sampling)
        old_staged, old_device = JS.sequence_bytes(layout)
        for data_bytes, segments in ((1, 1), (255, 1), (256, 16), (373123, 1), (100000, 36000)):
            staged = up(data_bytes) + up(8496) + up(384) + up(24) + up(16 * segments)
            assert JH.sequence_bytes(layout, data_bytes, segments) == (staged, staged + up(2 * layout.coef_count) + 512 + old_device - old_staged)
    # a full gray frame of 373 KB stages a twelfth of its coefficients
    assert JH.sequence_bytes(JP.make_info(1920, 1200), 373123, 1)[0] * 11 < JS.sequence_bytes(JP.make_info(1920, 1200))[0]
    bad = JP.make_info(64, 64, "420")
    bad.comp[1].blocks_w += 1
    with pytest.raises(CameraImageError) as e:
        JH.sequence_bytes(bad, 100, 1)
    assert e.value.status == N.BAD_ARGUMENT
