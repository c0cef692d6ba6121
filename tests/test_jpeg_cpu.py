"""JPEG reading, the part that needs no GPU: the numpy restatement (tests/jpeg_ref.py) is tied to libjpeg by the recorded
hashes of tests/golden/jpeg/expected.json (and to Pillow directly where it is installed), and the host decoder
(csrc/jpeg_entropy.cpp) runs as a stand-alone program under AddressSanitizer and UBSan over every fixture, every prefix
and every single-byte corruption of three small files; its coefficients are compared with the restatement's."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZED = ["noise_9x7_gray_q50_r0.jpg", "noise_17x33_420_q50_r0.jpg", "noise_31x16_422_q95_r2.jpg"]   # 1 component, 4:2:0, restart


def test_fixture_set_is_the_one_the_generator_writes():
    names = J.small_fixtures()
    for kind in ("noise", "ramp"):
        for size in ("1x1", "4x3", "7x5", "8x8", "9x7", "16x16", "17x33", "31x16", "33x17", "50x35", "255x9", "257x9"):
            for mode in ("gray", "444", "422", "420"):
                for q in (50, 95):
                    for r in (0, 2):
                        assert "%s_%s_%s_q%d_r%d.jpg" % (kind, size, mode, q, r) in names
    assert sorted(os.listdir(J.HERE)) == sorted(list(J.expected()) + ["README.md", "expected.json", "make_jpeg_fixtures.py"])
    for name in J.expected():
        assert os.path.getsize(os.path.join(J.HERE, name)) < (1 << 20)


def test_restated_parse_agrees_with_the_known_size_and_sampling():
    for name, want in J.expected().items():
        info = R.parse(J.data(name))
        assert (info.width, info.height) == (want["width"], want["height"]), name
        assert (None if info.n_components == 1 else info.sampling) == J.SAMPLING_OF[want["sampling"]], name
        assert info.restart_interval == (2 if "_r2" in name else 0), name
        for c in info.comps:
            assert c.blocks_w * 8 >= -(-info.width * c.h // info.comps[0].h) and c.blocks_h * 8 >= -(-info.height * c.v // info.comps[0].v)
    info = R.parse(J.data("pointgrey1.jpg"))
    assert (info.n_components, info.comps[0].blocks_w, info.comps[0].blocks_h, info.coef_count) == (1, 240, 150, 240 * 150 * 64)


def test_restated_pixels_hash_to_the_recorded_results_and_stay_in_the_int32_domain():
    """pixels() checks every IDCT intermediate in int64 and raises DomainError outside int32: that it returns is the guard."""
    for name in J.small_fixtures() + J.reference_images():
        _, _, px = J.restated(name)
        assert J.sha256(px) == J.expected()[name]["sha256"], name


def test_domain_guard_trips_outside_the_domain():
    info = R.make_info(8, 8, None, np.full(64, 255))
    coef = np.full(64, 32767, np.int16)
    with pytest.raises(R.DomainError):
        R.pixels(info, coef)
    coef[:] = 0
    coef[0] = 100                                                # 100 * 255 / 8 + 128: far above 255, still inside the domain
    assert (R.pixels(info, coef) == 255).all()


def test_checker_fixture_clamps_at_both_ends():
    info, coef, px = J.restated("checker_40x24_gray_q100.jpg")
    raw = R._pass(R._pass((coef.reshape(-1, 8, 8).astype(np.int64) * info.quant[0].reshape(8, 8)).transpose(0, 2, 1), 11)
                  .transpose(0, 2, 1), 18) + 128
    assert raw.min() < 0 and raw.max() > 255 and px.min() == 0 and px.max() == 255


def test_restatement_equals_pillow_directly():
    Image = pytest.importorskip("PIL.Image")
    for name in J.small_fixtures() + ["pointgrey2.jpg"]:
        im = Image.open(io.BytesIO(J.data(name)))
        want = np.asarray(im)
        if im.mode == "RGB":
            want = want[..., ::-1]
        assert np.array_equal(J.restated(name)[2], want), name


def test_restatement_flags_every_refusal():
    cases = J.refusals()
    for cause in R.REFUSALS:                                     # every cause the header lists is provoked at least once
        assert any(c == cause for _, c, _ in cases.values()), cause
    for name, (jpg, cause, _) in cases.items():
        assert J.restatement_refuses(jpg) == cause, name
    for name in (J.GRAY, J.COLOUR, J.MANY_BLOCKS):               # the files they were patched from are accepted
        assert J.restatement_refuses(J.data(name)) is None


def test_restart_markers_out_of_order_or_missing_are_refused():
    jpg = J.data("noise_31x16_gray_q50_r2.jpg")
    at = jpg.index(b"\xff\xd1")
    assert J.restatement_refuses(jpg[:at + 1] + b"\xd2" + jpg[at + 2:]) == "ends early"
    assert J.restatement_refuses(jpg[:at] + jpg[at + 2:]) in ("ends early", "Huffman code in no table", "run past coefficient 63")


def test_fill_bytes_in_front_of_markers_are_skipped():
    jpg = J.data("noise_31x16_gray_q50_r2.jpg")
    at = jpg.index(b"\xff\xd1")
    padded = jpg[:at] + b"\xff\xff" + jpg[at:]
    assert np.array_equal(R.decode(padded), J.restated("noise_31x16_gray_q50_r2.jpg")[2])


def test_compressed_image_message_layout():
    msg = R.compressed_image_msg(b"\xff\xd8data", "bgr8; jpeg compressed bgr8", seq=7, stamp=(3, 4), frame_id="cam")
    assert msg[:12] == np.array([7, 3, 4], "<u4").tobytes() and msg[16:19] == b"cam" and msg.endswith(b"\xff\xd8data")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/jpeg_host_check.cpp + csrc/jpeg_entropy.cpp only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("jpeg_host_check")
    exe = str(out / "jpeg_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "jpeg_host_check.cpp"),
                    os.path.join(csrc, "jpeg_entropy.cpp"), "-o", exe], check=True, timeout=300)
    return exe, str(out / "coefficients.bin")


def test_host_decoder_under_sanitizers(host_check):
    exe, dump = host_check
    names = J.small_fixtures() + J.reference_images()
    r = subprocess.run([exe, dump] + [os.path.join(J.HERE, n) for n in names] + ["--"] + [os.path.join(J.HERE, n) for n in FUZZED],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "every status ILCC_OK or ILCC_BAD_ARGUMENT" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    raw = np.fromfile(dump, np.uint8)
    at = 0
    for name in names:                                           # the intact files: the program's coefficients are the restatement's
        count = int(raw[at:at + 8].view(np.uint64)[0])
        coef = raw[at + 8:at + 8 + 2 * count].view(np.int16)
        at += 8 + 2 * count
        assert count == J.restated(name)[0].coef_count and np.array_equal(coef, J.restated(name)[1]), name
    assert at == raw.size
