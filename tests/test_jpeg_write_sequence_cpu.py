"""The JPEG batch writer (include/ilcc_jpeg_write_sequence.h), the part that needs no GPU: the numpy restatement of K17's steps
(tests/jpeg_huffman_enc_ref.py) against the sequential encoder of tests/jpeg_write_ref.py over the writer's case grid, the host
entry that writes the bytes in front of a scan against ilcc_jpeg_entropy_encode, the header, the export list and the library, the
chain's host arithmetic, and ilcc_jpeg_write_headers as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_huffman_enc_ref as E
import jpeg_ref as R
import jpeg_write_cases as K
import jpeg_write_ref as W
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_sequence as IS
from lidar_camera_calibration_amd import jpeg_write
from lidar_camera_calibration_amd import jpeg_write_sequence as S
from lidar_camera_calibration_amd.camera_image import CameraImageError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(w, h, mode, r) for w, h in K.SIZES for mode in K.MODES for r in K.RESTARTS]


def _case(w, h, mode, r, q=95):
    """(restated Info, coefficients, file, the file's scan) of the grid's noise case"""
    info, coef, data = K.restated(K.case_name("noise", w, h, mode, q, r))
    head = W.headers(info)
    assert data.startswith(head) and data.endswith(b"\xff\xd9")
    return info, coef, data, data[len(head):-2]


def test_exports_match_header_and_structs_have_their_sizes():
    hdr = open(os.path.join(ROOT, "include", "ilcc_jpeg_write_sequence.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|uint64_t|void|double)\s+(ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(S.JPEG_WRITE_SEQUENCE_EXPORTS) and len(set(declared)) == len(declared)
    L = S.lib()
    for s in S.JPEG_WRITE_SEQUENCE_EXPORTS:
        assert hasattr(L, s), s
    for name, (cls, size) in S.STRUCT_SIZES.items():
        assert C.sizeof(cls) == size, name
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), hdr), name          # the header states the same size
    assert S.EncodeJob.hip_stream.offset == 72 and S.FdctBatchJob.hip_stream.offset == 72
    assert not re.search(r"\(.*void\*\s*hip_stream", hdr)                                 # the stream travels inside the jobs
    for bit in ("DC_RANGE", "AC_RANGE", "CAPACITY"):
        value = int(re.search(r"#define ILCC_JPEG_ENCODE_%s\s+0x([0-9a-f]+)u" % bit, hdr).group(1), 16)
        assert getattr(S, bit) == getattr(E, bit) == value
    assert re.search(r"EIGHT launches", hdr) and len(re.findall(r"^ \*   (k17_\w+) ", hdr, re.M)) == 8
    # the writer's own header got none of the new names
    other = open(os.path.join(ROOT, "include", "ilcc_jpeg_write.h")).read()
    assert not set(re.findall(r"\b(ilcc_\w+)\s*\(", other)) & set(S.JPEG_WRITE_SEQUENCE_EXPORTS)


def test_restatement_equals_the_sequential_encoder_on_the_case_grid():
    assert len(GRID) == 14 * 4 * 2
    for w, h, mode, r in GRID:
        info, coef, _, scan = _case(w, h, mode, r)
        got, status = E.encode_image(info, coef)
        assert status == 0 and got == scan, (w, h, mode, r)
    for q in (1, 50, 100):                                     # the other qualities where the blocks are fewest and most
        for w, h in ((1, 1), (263, 15)):
            info, coef, _, scan = _case(w, h, "420", 2, q)
            assert E.encode_image(info, coef) == (scan, 0), (w, h, q)


def test_write_headers_and_the_scan_and_eoi_are_the_host_encoders_file():
    for w, h, mode, r in GRID:
        ref_info, coef, data, scan = _case(w, h, mode, r)
        info = jpeg_write.write_info(w, h, W.SAMPLINGS[mode], 95, r)
        head = S.write_headers(info)
        assert head == W.headers(ref_info), (w, h, mode, r)
        assert S.file_of(info, scan) == jpeg_write.entropy_encode(info, coef) == data, (w, h, mode, r)
    info = jpeg_write.write_info(64, 48, (2, 2), 90, 7)
    need = len(S.write_headers(info))
    assert need == 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14 == 629
    out, n = np.full(need + 8, 0xA5, np.uint8), C.c_uint64(5)
    assert S.lib().ilcc_jpeg_write_headers(C.byref(info), out.ctypes.data_as(C.c_void_p), need - 1, C.byref(n)) == N.CAPACITY and n.value == 0
    assert (out[need - 1:] == 0xA5).all()
    assert S.lib().ilcc_jpeg_write_headers(C.byref(info), out.ctypes.data_as(C.c_void_p), need, C.byref(n)) == N.OK and n.value == need
    assert (out[need:] == 0xA5).all()
    info.comp[2].ac_table = 3
    with pytest.raises(CameraImageError) as e:
        S.write_headers(info)
    assert e.value.status == N.BAD_ARGUMENT


def _blocks(info, fill):
    b = np.zeros((info.coef_count // 64, 64), np.int64)
    fill(b)
    return b.reshape(-1).astype(np.int16)


def test_restatement_on_constructed_coefficients():
    """what the steps can get wrong: blocks of 4 bits that share a byte, runs of 1-bits whose 0xFF bytes outnumber a chunk's
    bytes in front of it, padding that completes an 0xFF in front of RSTn, and more than 8 segments"""
    rng = np.random.default_rng(17)
    for sampling, interval in ((None, 0), (None, 1), ((2, 2), 1), ((2, 2), 3), ((2, 1), 2), ((1, 1), 5)):
        info = W.make_info(40, 72, sampling, 90, interval)
        n = info.coef_count // 64
        fills = {"zero": lambda b: None,
                 "ones": lambda b: (b.__setitem__((slice(None), slice(1, None)), (1 << rng.integers(1, 11, (n, 63))) - 1),
                                    b.__setitem__((slice(None), 0), rng.integers(0, 2, n) * 1023)),
                 "dense": lambda b: b.__setitem__((slice(None), slice(1, None)), rng.integers(512, 1024, (n, 63)) * rng.choice([-1, 1], (n, 63)))}
        for name, fill in fills.items():
            coef = _blocks(info, fill)
            want = W.entropy_encode(info, coef)
            got, status = E.encode_image(info, coef)
            assert status == 0 and W.headers(info) + got + b"\xff\xd9" == want, (sampling, interval, name)
            if name == "ones":
                assert got.count(b"\xff\x00") > len(got) // 8
    info = W.make_info(8, 8, None, 90, 0)                       # one gray block of zeros: 6 bits and two of padding, one byte
    assert E.encode_image(info, np.zeros(64, np.int16)) == (bytes([0b00101011]), 0)
    info = W.make_info(16, 16, (2, 2), 90, 0)                   # six zero blocks: 4 x 6 + 2 x 4 = 32 bits, no padding
    assert len(E.encode_image(info, np.zeros(info.coef_count, np.int16))[0]) == 4


def test_restatement_refuses_what_the_sequential_encoder_refuses_and_places_a_batch():
    info = W.make_info(24, 24, (2, 2), 90, 2)
    good = K.restated(K.case_name("noise", 24, 24, "420", 95, 2))[1]
    for at, value, bit in ((0, 2048, E.DC_RANGE), (0, -2048, E.DC_RANGE), (64 * 3, 2047, 0), (5, 1024, E.AC_RANGE), (64 * 7 + 9, -1024, E.AC_RANGE),
                           (64 * 2 + 1, -32768, E.AC_RANGE)):
        coef = np.zeros(info.coef_count, np.int16)
        coef[at] = value
        refused = False
        try:
            W.entropy_encode(info, coef)
        except W.Unencodable:
            refused = True
        scan, status = E.encode_image(info, coef)
        assert refused == (status != 0) and status == bit and (scan == b"") == refused, (at, value)
    bad = np.zeros(info.coef_count, np.int16)
    bad[0] = 2048
    scans, rows = E.encode_batch(info, [good, bad, good], 1 << 20)
    size = len(scans[0])
    assert rows ==[(0, size, 0), (-(-size // 16) * 16, 0, E.DC_RANGE), (-(-size // 16) * 16, size, 0)]
    need = -(-size // 16) * 16 + size
    assert E.encode_batch(info, [good, bad, good], need)[1] == rows
    scans, rows = E.encode_batch(info, [good, bad, good, bad], need - 1)
    assert [r[1:] for r in rows] == [(size, 0), (0, E.DC_RANGE), (0, E.CAPACITY), (0, E.DC_RANGE | E.CAPACITY)] and scans[2] == b""
    assert [r[2] for r in E.encode_batch(info, [good, good], size - 1)[1]] == [E.CAPACITY, E.CAPACITY]


def test_chain_bytes_and_cutting():
    """ilcc_jpeg_write_sequence_bytes is the header's sum, and what the chain cuts with gives the batches ilcc_image_sequence_cut
    gives; K17's scratch for a batch is never more than its images' shares"""
    def up(x, a=256):
        return -(-x // a) * a

    for w, h, per in ((64, 48, 0), (64, 48, 100), (1920, 1200, 0), (35, 50, 4097)):
        info = jpeg_write.write_info(w, h, None, 95, 0)
        out = up(per or w * h, 16)
        one = S.huffman_encode_scratch_bytes(info, 1, out)
        assert S.sequence_bytes(w, h, per) == up(w * h) + up(2 * info.coef_count) + up(out) + 256 + one
        for n in (2, 9, 33):
            assert 0 < S.huffman_encode_scratch_bytes(info, n, n * out) <= n * one
        assert one >= up(out, 4096) + 4096
    assert S.sequence_bytes(0, 5) == 0 and S.sequence_bytes(70000, 5) == 0
    assert S.huffman_encode_scratch_bytes(jpeg_write.write_info(64, 48, None, 95, 0), 65536, 100) == 0
    device = S.sequence_bytes(64, 48)
    raw = [64 * 48 + 60] * 8
    assert [len(IS.sequence_cut(raw, device, 0, budget)) - 1 for budget in (8 * device, 3 * device, device)] == [1, 3, 8]
    # host refusals of the chain come before any device is touched
    out = S.WriteSequenceResult()
    p = S.default_params()
    assert C.sizeof(p) == 40 and bytes(p) == bytes(40)
    L = S.lib()
    assert L.ilcc_bag_save_jpeg_all(0, b"x.bag", b"/t", None, None, 95, C.byref(p), C.byref(out), None, 0) == N.BAD_ARGUMENT
    p.route = 2
    assert L.ilcc_bag_save_jpeg_all(0, b"x.bag", b"/t", None, b"/tmp/x", 95, C.byref(p), C.byref(out), None, 0) == N.BAD_ARGUMENT
    assert b"route" in N.lib().ilcc_last_error(None) and out.status == N.BAD_ARGUMENT


def test_write_headers_under_address_and_ub_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    exe = str(tmp_path / "jpeg_write_sequence_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "jpeg_write_sequence_host_check.cpp"),
                    os.path.join(csrc, "jpeg_entropy_enc.cpp"), os.path.join(csrc, "jpeg_entropy.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "144 infos checked" in r.stdout
    for word in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in r.stderr, r.stderr[-3000:]
