"""Every scan of a batch drawn on a copy of its image, the part that needs no GPU (include/ilcc_overlay_sequence.h): the exports
against the header, the identity K12b's design rests on -- "the highest in-scan point index wins" equals the sequential loop over the
hits -- on the collision cases, the scratch arithmetic, ilcc_overlay_sequence_bytes against its restatement, guards on the
constructed inputs of the GPU tests, the argument errors of ilcc_pcd2image --all-pairs, and csrc/overlay_sequence_host.cpp alone as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import overlay_ref as O
import overlay_sequence_cases as OC
import overlay_sequence_ref as R
import paired_cases as K
import project_cases as P
from lidar_camera_calibration_amd import jpeg_write, jpeg_write_sequence, overlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_pcd2image")
SIZES = [(64, 48, 0), (64, 48, 700), (1, 1, 0), (37, 23, 1), (702, 629, 0), (1920, 1200, 0), (1920, 1200, 123457), (65535, 3, 0)]
REFUSED = [(0, 5, 0), (5, 0, 0), (-3, 4, 0), (65536, 4, 0), (4, 65536, 0), (64, 48, 2 ** 40 + 1)]


def test_exports_match_the_header():
    text = open(os.path.join(ROOT, "include", "ilcc_overlay_sequence.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|uint64_t|void|ilcc_overlay_plan\*) (ilcc_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(overlay.OVERLAY_SEQUENCE_EXPORTS) and len(declared) == 9
    L = overlay.lib()
    for s in overlay.OVERLAY_SEQUENCE_EXPORTS:
        assert hasattr(L, s), s
    assert C.sizeof(overlay.OverlayBatchJob) == 144                               # the header's structs, no padding surprises
    assert C.sizeof(overlay.OverlaySequenceParams) == 64 and C.sizeof(overlay.OverlayRecord) == 56
    assert len(L.ilcc_bag_pcd2image_all_pairs.argtypes) == 14
    sp = overlay.default_overlay_sequence_params()
    assert (sp.first, sp.stride, sp.max_scans, sp.route, sp.keep_pixels, sp.max_dt_ns, sp.staging_bytes, sp.image_bytes, sp.device_bytes, sp.out_bytes_per_image) == \
        (0, 1, 0, 0, 0, 50 * 1000000, 256 << 20, 512 << 20, 1 << 30, 0)
    assert "void* hip_stream;" in text and not re.search(r"\(\s*[^;{}()]*void\s*\*\s*hip_stream[^;{}()]*\)\s*;", text)   # the stream travels in the job
    # the overlay header points here where it says that it takes the first message of each topic
    assert "ilcc_overlay_sequence.h" in open(os.path.join(ROOT, "include", "ilcc_overlay.h")).read()


def test_scratch_bytes():
    f = overlay.overlay_batch_scratch_bytes
    for w, h, n in ((1, 1, 1), (3, 3, 5), (37, 23, 300), (128, 128, 34), (1920, 1200, 32), (65536, 65536, 65535)):
        assert f(w, h, n) == n * ((4 * w * h + 15) // 16 * 16), (w, h, n)
    assert f(4, 4, 0) == 0
    for w, h in ((0, 1), (1, 0), (-1, 5), (65537, 1), (1, 65537)):                 # a refused size
        assert f(w, h, 3) == 0


def _scans(b):
    for s, k in enumerate(b["image_of_scan"]):
        if k >= 0:
            yield s, b["xyzi"][int(b["offsets"][s]):int(b["offsets"][s + 1])], b["images"][k]


@pytest.mark.parametrize("stamp", [R.REFERENCE_STAMP, OC.stamp_of_64(), [(0, 0)]], ids=["reference stamp", "stamp of 64", "one pixel"])
def test_highest_in_scan_point_index_wins_equals_the_sequential_loop(stamp):
    """K8's compaction keeps point order, so the hit with the highest index is the kept point with the highest in-scan index."""
    batches = [OC.collision_batch(), K.camera_batches()[6], K.keep_batch(4)]
    for b in batches:
        canvases, n_drawn = R.overlay_batch(b["xyzi"], b["offsets"], b["images"], b["image_of_scan"], b["cam"], b["dis"], 0.0, 60.0, stamp)
        for s, pts, image in _scans(b):
            if len(pts) > 5000 and len(stamp) > 5:
                continue                                                           # the long scans with the long stamp add minutes, not cases
            got, n = R.highest_point_wins(pts, image, b["cam"], b["dis"], 0.0, 60.0, stamp)
            assert got.tobytes() == canvases[s].tobytes() and n == n_drawn[s], (b["name"], s)
            hits = P.project_intensity(pts, b["cam"], b["dis"], 0.0, 60.0)
            assert O.draw_hits_highest_wins(R.packed(image, b["cam"]), hits, stamp).tobytes() == got.tobytes()


def test_collision_cases_are_what_they_are_named():
    b = OC.collision_batch()
    cam = b["cam"]
    n = np.diff(b["offsets"].astype(np.int64)).tolist()
    assert n == [P.CHUNK + 1 + 300, 400, 150, 150] and b["image_of_scan"].tolist() == [0, 0, 1, 1]
    scans = [pts for _, pts, _ in _scans(b)]
    hits = [P.project_intensity(pts, cam, b["dis"]) for pts in scans]
    assert [len(h) for h in hits] == n                                             # every point is kept
    assert set(zip(hits[0]["x"].tolist(), hits[0]["y"].tolist())) == {OC.ONE_PIXEL}
    colours = np.stack([hits[0]["r"], hits[0]["g"], hits[0]["b"]], 1)
    assert len({tuple(c) for c in colours.tolist()}) > 50                          # distinct intensities give distinct colours
    assert colours[-1].tolist() != colours[P.CHUNK - 1].tolist() and colours[-1].tolist() != colours[P.CHUNK].tolist()
    assert set(zip(hits[1]["x"].tolist(), hits[1]["y"].tolist())) == {(x, y) for x in (9, 10, 11) for y in (3, 4, 5)}
    assert sorted(zip(hits[2]["x"].tolist(), hits[2]["y"].tolist())) == sorted(zip(hits[3]["x"].tolist(), hits[3]["y"].tolist()))
    canvases, _ = R.overlay_batch(b["xyzi"], b["offsets"], b["images"], b["image_of_scan"], cam, b["dis"])
    assert canvases[2].tobytes() != canvases[3].tobytes()
    # in the block an earlier point's centre is overdrawn by a later neighbour's arm: order matters there
    reverse = O.draw_hits(R.packed(b["images"][0], cam), hits[1][::-1])
    assert reverse.tobytes() != canvases[1].tobytes()
    big = OC.hundreds()
    assert len(big["image_of_scan"]) == 300 and set(np.diff(big["offsets"].astype(np.int64)).tolist()) == {1, 2, 3, 4, 5}
    assert len(OC.stamp_of_64()) == 64 and all(-128 <= v <= 127 for pair in OC.stamp_of_64() for v in pair)


def test_canvas_bytes_places_rows_and_nothing_else():
    cam = P.camera(width=3, height=2)
    a = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    out = R.canvas_bytes([a, None, a + 100], cam, 11, 25, 3 * 25 + 4, 0xAB)
    want = np.full(79, 0xAB, np.uint8)
    want[0:9], want[11:20] = np.arange(9), np.arange(9, 18)
    want[50:59], want[61:70] = np.arange(100, 109), np.arange(109, 118)
    assert out.tolist() == want.tolist()


# ------------------------------------------------------------------------------------------ the bytes of a paired scan

def test_sequence_bytes_equal_the_restatement():
    for w, h, out in SIZES:
        info = jpeg_write.write_info(w, h, "420")
        want = R.sequence_bytes(w, h, out, info.coef_count, jpeg_write.fdct_scratch_bytes(info),
                                lambda cap, info=info: jpeg_write_sequence.huffman_encode_scratch_bytes(info, 1, cap))
        assert overlay.overlay_sequence_bytes(w, h, out) == want > 7 * w * h, (w, h, out)
    # canvas and owner words beside what the JPEG chain counts for the picture: more than a mono8 image of that size takes there
    assert overlay.overlay_sequence_bytes(1920, 1200) > jpeg_write_sequence.sequence_bytes(1920, 1200) + 7 * 1920 * 1200
    for w, h, out in REFUSED:
        assert overlay.overlay_sequence_bytes(w, h, out) == 0, (w, h, out)


def test_the_recording_is_what_the_chain_tests_claim():
    clouds, images = K.recording()
    want = R.chain(clouds, [(s, px, enc) for s, px, enc, _ in images], K.recording_camera(), K.T_LIDAR2CAM, K.DISTANCE, K.MAX_DT_NS)
    assert [r["image_message"] for r, _, _ in want] == [0, 1, 1, 2, 3, -1, 4]
    assert want[5][1] is None and want[5][2] is None and want[5][0]["n_drawn"] == 0
    drawn = [r["n_drawn"] for r, _, _ in want]
    assert all(100 < n < len(clouds[k][1]) for k, n in enumerate(drawn) if k != 5), drawn
    assert want[1][2].tobytes() != want[2][2].tobytes()                            # clouds 1 and 2 share image 1 and differ in their dots
    sizes = [r["file_bytes"] for r, _, _ in want if r["image_message"] >= 0]
    assert all(blob[:2] == b"\xff\xd8" and blob[-2:] == b"\xff\xd9" for _, blob, _ in want if blob is not None)
    # the budget of the GPU test that asks for a capacity fallback: 16-byte steps, below the largest scan and above the smallest
    import jpeg_write_ref as JW
    scans = sorted(n - len(JW.headers(JW.make_info(64, 48, (2, 2), 95))) - 2 for n in sizes)
    assert scans[0] < scans[-1]


# ------------------------------------------------------------------------------------------ the program's arguments

def test_cli_argument_errors(tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_pcd2image"
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, timeout=120)
    common = ["--bag", str(tmp_path / "a.bag"), "--image-topic", K.IMAGE_TOPIC, "--lidar-topic", K.LIDAR_TOPIC, "--yaml", str(tmp_path / "missing.yaml"),
              "--extrinsic", str(tmp_path / "missing.bin")]
    r = run("--all-pairs", *common)                                                 # --all-pairs without a prefix
    assert r.returncode == 2 and "usage: ilcc_pcd2image" in r.stderr and "--jpg-out-all PREFIX" in r.stderr
    r = run("--all-pairs", "--ppm-out-all", str(tmp_path / "p"), *common)
    assert r.returncode == 2 and "usage" in r.stderr
    r = run("--all-pairs", "--jpg-out-all")
    assert r.returncode == 2 and "unknown or incomplete argument: --jpg-out-all" in r.stderr
    r = run("--all-pairs", "--jpg-out-all", str(tmp_path / "j"), "--huffman", "fpga", *common)
    assert r.returncode == 2 and "usage" in r.stderr
    r = run("--all-pairs", "--jpg-out-all", str(tmp_path / "j"), "--out", str(tmp_path / "o.ppm"), *common)      # one picture or all of them
    assert r.returncode == 2 and "usage" in r.stderr
    r = run("--jpg-out-all", str(tmp_path / "j"), "--out", str(tmp_path / "o.ppm"), *common)                     # a prefix without --all-pairs
    assert r.returncode == 2 and "usage" in r.stderr
    r = run("--all-pairs", "--jpg-out-all", str(tmp_path / "j"), "--max-dt-ms")
    assert r.returncode == 2 and "--max-dt-ms" in r.stderr
    # complete: the first thing it misses is the yaml, then the extrinsic; --out is not asked for
    r = run("--all-pairs", "--jpg-out-all", str(tmp_path / "j"), "--first", "1", "--stride", "2", "--max-scans", "3", "--huffman", "host", *common)
    assert r.returncode == 1 and "missing.yaml" in r.stderr
    open(tmp_path / "cam.yaml", "w").write(K.yaml_text(K.recording_camera()))
    common[7] = str(tmp_path / "cam.yaml")
    r = run("--all-pairs", "--jpg-out-all", str(tmp_path / "j"), *common)
    assert r.returncode == 1 and "can not open" in r.stderr and "missing.bin" in r.stderr
    # without --all-pairs nothing changes: --out is still required
    r = run(*common)
    assert r.returncode == 2 and "usage" in r.stderr


# ------------------------------------------------------------------------------------------ under sanitizers, stand-alone

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/overlay_sequence_host_check.cpp + csrc/overlay_sequence_host.cpp only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("overlay_sequence_host_check")
    exe = str(out / "overlay_sequence_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "overlay_sequence_host_check.cpp"),
                    os.path.join(csrc, "overlay_sequence_host.cpp"), "-o", exe], check=True, timeout=300)
    return exe, out


def _stand_in_bytes(w, h, out_bytes):
    """the restatement over the stand-ins of overlay_sequence_host_check.cpp"""
    if not (1 <= w <= 65535 and 1 <= h <= 65535) or out_bytes > 2 ** 40:
        return 0
    coef = ((w + 15) // 16) * ((h + 15) // 16) * 6 * 64
    if coef * 32 >= 2 ** 32:
        return 0
    return R.sequence_bytes(w, h, out_bytes, coef, coef + 3, lambda cap: 256 * ((cap + 4096 + coef // 8) // 256 + 1))


def test_host_layer_under_sanitizers_equals_the_restatement(host_check):
    exe, out = host_check
    cases = SIZES + REFUSED + [(65535, 65535, 0), (2 ** 31 - 1, 1, 0), (-2 ** 31, -2 ** 31, 0), (17, 33, 2 ** 40), (17, 33, 2 ** 64 - 1)]
    with open(out / "cases.txt", "w") as fh:
        fh.write("%d\n" % len(cases) + "".join("%d %d %d\n" % c for c in cases))
    r = subprocess.run([exe, str(out / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    for line, (w, h, o) in zip(lines, cases):
        assert line == "%d %d %d %d" % (w, h, o, _stand_in_bytes(w, h, o)), line
    assert sum(_stand_in_bytes(*c) > 0 for c in cases) >= len(SIZES) and _stand_in_bytes(65535, 65535, 0) == 0
    assert lines[-1] == "defaults 0 1 0 0 0 0 50000000 %d %d %d 0 size 64 56" % (256 << 20, 512 << 20, 1 << 30)
