"""JPEG writing, the part that needs no GPU: the numpy restatement (tests/jpeg_write_ref.py) is tied to libjpeg by the
recorded hashes of tests/golden/jpeg_write/expected.json (and to Pillow directly where it is installed); the reciprocal K14
divides with is proved exact; the header, the export list and the library agree; and the host encoder
(csrc/jpeg_entropy_enc.cpp) runs as a stand-alone program under AddressSanitizer and UBSan over every case."""
import ctypes as C
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_ref as R
import jpeg_write_cases as K
import jpeg_write_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_grid_and_fixture_set_are_the_ones_the_generator_writes():
    names = set(K.cases())
    for w, h in [(1, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (33, 17), (31, 16), (24, 24), (40, 24), (255, 9), (257, 9),
                 (263, 15)]:
        for mode in ("gray", "444", "422", "420"):
            for q in (1, 50, 95, 100):
                for r in (0, 2):
                    assert K.case_name("noise", w, h, mode, q, r) in names
            assert K.case_name("ramp", w, h, mode, 95, 0) in names and K.case_name("checker", w, h, mode, 100, 0) in names
    assert sorted(K.expected()) == sorted(list(names) + ["pointgrey1_reencoded_q95"])
    assert sorted(os.listdir(K.HERE)) == sorted(K.committed_files() + ["README.md", "expected.json", "make_jpeg_write_fixtures.py"])
    assert len(K.committed_files()) == 12
    for name in K.committed_files():
        data = open(os.path.join(K.HERE, name), "rb").read()
        assert (len(data), K.sha256(data)) == (K.expected()[name[:-4]]["bytes"], K.expected()[name[:-4]]["sha256"]), name


def test_the_grid_covers_dummy_blocks_and_padded_chroma():
    """A dummy column alone, a dummy row alone and both; chroma planes whose padded columns and rows are no real samples."""
    seen = set()
    for w, h in K.SIZES:
        info = W.make_info(w, h, (2, 2))
        luma = info.comps[0]
        seen.add((luma.blocks_w > -(-w // 8), luma.blocks_h > -(-h // 8)))
    assert seen == {(False, False), (True, False), (False, True), (True, True)}
    assert any(-(-w // 2) % 8 and -(-h // 2) % 8 for w, h in K.SIZES) and any(w % 2 and h % 2 for w, h in K.SIZES)


def test_restated_files_hash_to_the_recorded_results():
    for name in K.cases():
        _, _, data = K.restated(name)
        assert (len(data), K.sha256(data)) == (K.expected()[name]["bytes"], K.expected()[name]["sha256"]), name


def test_restated_reference_frame_hashes_to_the_recorded_result():
    data = W.encode(J.restated("pointgrey1.jpg")[2], 95)
    want = K.expected()["pointgrey1_reencoded_q95"]
    assert (len(data), K.sha256(data)) == (want["bytes"], want["sha256"]) == (374872, want["sha256"])
    assert data != J.data("pointgrey1.jpg")                         # a generation, not the shipped file


def test_restatement_equals_pillow_directly():
    Image = pytest.importorskip("PIL.Image")
    for name, (_, w, h, mode, q, r) in K.cases().items():
        px = np.asarray(K.source(name))
        buf = io.BytesIO()
        if mode == "gray":
            Image.fromarray(px, "L").save(buf, "JPEG", quality=q, restart_marker_blocks=r)
        else:
            Image.fromarray(np.ascontiguousarray(px[..., ::-1]), "RGB").save(buf, "JPEG", quality=q, subsampling={"444": 0, "422": 1, "420": 2}[mode],
                                                                             restart_marker_blocks=r)
        assert K.restated(name)[2] == buf.getvalue(), name


def test_restated_files_decode_back_to_the_restated_coefficients():
    for name in K.cases():
        info, coef, data = K.restated(name)
        parsed = R.parse(data)
        assert (parsed.width, parsed.height, parsed.restart_interval, parsed.coef_count) == (info.width, info.height, info.restart_interval,
                                                                                             info.coef_count), name
        used = 1 if info.n_components == 1 else 2                   # a 1-component file carries the luminance table alone
        assert np.array_equal(parsed.quant[:used], info.quant[:used]) and not parsed.quant[used:].any(), name
        assert np.array_equal(R.entropy_decode(data, parsed), coef), name


def test_restatement_refuses_what_libjpeg_refuses():
    info = W.make_info(8, 8)
    for k, value, ok in ((0, 2047, True), (0, -2047, True), (0, 2048, False), (0, -2048, False), (1, 1023, True), (1, -1023, True),
                         (1, 1024, False), (63, -1024, False)):
        c = np.zeros(64, np.int16)
        c[k] = value
        if ok:
            assert np.array_equal(R.entropy_decode(W.entropy_encode(info, c), R.parse(W.entropy_encode(info, c))), c)
        else:
            with pytest.raises(W.Unencodable):
                W.entropy_encode(info, c)


def test_quantisation_tables_scale_as_libjpeg():
    assert W.quant_tables(50).tolist() == [W.STD_LUMA, W.STD_CHROMA]
    assert (W.quant_tables(100) == 1).all() and W.quant_tables(1).max() == 255 and (W.quant_tables(1)[1] == 255).all()
    assert np.array_equal(W.quant_tables(0), W.quant_tables(1)) and np.array_equal(W.quant_tables(101), W.quant_tables(100))
    shipped = R.parse(J.data("pointgrey1.jpg"))                      # the reference's own files: quality 95
    assert np.array_equal(shipped.quant[0], W.quant_tables(95)[0])


def test_reciprocal_division_is_exact():
    """K14 quantises with q = umulhi(n, ceil(2^32 / d)), n = |c| + d / 2.  Exact for every divisor d = 8 quant (8, 16, ..
    2040) and every numerator 0 .. 2^18 + 1020: beyond what the DCT produces (|c| <= 2^16 for 8-bit samples)."""
    n = np.arange((1 << 18) + 1021, dtype=np.uint64)
    for d in range(8, 2041, 8):
        m = ((1 << 32) + d - 1) // d
        assert m <= (1 << 29)
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(d)), d
    # and the DCT's output stays far inside that domain: the extreme blocks
    y, x = np.mgrid[0:8, 0:8]
    worst = 0
    for u in range(8):
        for v in range(8):
            block = (np.cos((2 * y + 1) * u * np.pi / 16) * np.cos((2 * x + 1) * v * np.pi / 16) > 0) * 255
            worst = max(worst, int(np.abs(W.fdct_blocks(block[None])).max()))
    assert 8000 < worst < (1 << 16)


def test_exports_match_header():
    from lidar_camera_calibration_amd import jpeg, jpeg_write
    hdr = open(os.path.join(ROOT, "include", "ilcc_jpeg_write.h")).read()
    declared = re.findall(r"^(?:int32_t|uint64_t) (ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(jpeg_write.JPEG_WRITE_EXPORTS) and len(declared) == 8
    L = jpeg_write.lib()
    for s in jpeg_write.JPEG_WRITE_EXPORTS:
        assert hasattr(L, s), s
    assert '#include "ilcc_jpeg.h"' in hdr and "struct" not in hdr.split("#ifndef")[1]      # the reader's structs, unchanged
    assert (C.sizeof(jpeg.Component), C.sizeof(jpeg.Info)) == (40, 664) and L.ilcc_abi_version() == 5
    reader = open(os.path.join(ROOT, "include", "ilcc_jpeg.h")).read()
    assert " * Not here: progressive JPEG, PNG.\n" in reader and "JPEG output" not in reader


def test_host_info_and_encoder_through_the_library():
    """ilcc_jpeg_write_info, ilcc_jpeg_file_bound and ilcc_jpeg_entropy_encode are host code: they run without a GPU."""
    from lidar_camera_calibration_amd import jpeg_write as JW
    for name in ("noise_17x33_420_q95_r2", "noise_9x9_422_q1_r0", "noise_257x9_gray_q100_r2", "ramp_40x24_444_q95_r0"):
        _, w, h, mode, q, r = K.cases()[name]
        want_info, coef, data = K.restated(name)
        info = JW.write_info(w, h, None if mode == "gray" else mode, q, r)
        assert np.array_equal(info.quant_array()[:2], want_info.quant[:2]) and info.coef_count == want_info.coef_count
        assert JW.entropy_encode(info, np.array(coef)) == data and len(data) <= JW.file_bound(info)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/jpeg_write_host_check.cpp + csrc/jpeg_entropy_enc.cpp + csrc/jpeg_entropy.cpp only, under
    ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("jpeg_write_host_check")
    exe = str(out / "jpeg_write_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "jpeg_write_host_check.cpp"),
                    os.path.join(csrc, "jpeg_entropy_enc.cpp"), os.path.join(csrc, "jpeg_entropy.cpp"), "-o", exe], check=True, timeout=300)
    return exe, str(out / "cases.bin")


def test_host_encoder_under_sanitizers(host_check):
    exe, dump = host_check
    names = list(K.cases())
    with open(dump, "wb") as f:
        for name in names:
            _, w, h, mode, q, r = K.cases()[name]
            _, coef, data = K.restated(name)                         # the files hash to the recorded ones (tested above)
            s = W.SAMPLINGS[mode]
            f.write(struct.pack("<7i", w, h, 1 if s is None else 3, *(s or (1, 1)), q, r))
            f.write(struct.pack("<Q", coef.size) + coef.tobytes() + struct.pack("<Q", len(data)) + data)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "%d cases" % len(names) in r.stdout and "every file reproduced, decoded back and bounded" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
