"""Every scan coloured from its time-paired image, the part that needs no GPU (include/ilcc_paired.h): the exports against the
header, the pairing against the brute force of tests/paired_ref.py, the PCD writer against its restated bytes, guards on the
constructed inputs of the GPU tests, and csrc/paired_host.cpp alone as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import paired_cases as K
import paired_ref as R
import project_cases as P
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import paired

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_rgblidar")
CASES = K.pairing_cases()


def test_exports_match_the_header():
    text = open(os.path.join(ROOT, "include", "ilcc_paired.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|uint64_t|void|ilcc_colourise_plan\*) (ilcc_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(paired.PAIRED_EXPORTS) and len(declared) == 9
    L = paired.lib()
    for s in paired.PAIRED_EXPORTS:
        assert hasattr(L, s), s
    assert len(L.ilcc_colourise_batch_device.argtypes) == 13 and len(L.ilcc_bag_rgblidar_all_scans.argtypes) == 13
    assert C.sizeof(paired.PairedParams) == 40 and C.sizeof(paired.PairRecord) == 48          # the header's structs, no padding surprises
    pp = paired.default_paired_params()
    assert (pp.first, pp.stride, pp.max_scans, pp.sample_raw, pp.max_dt_ns, pp.staging_bytes, pp.image_bytes) == \
        (0, 1, 0, 0, 50 * 1000000, 256 << 20, 512 << 20)
    # the overlay header no longer lists what this header brings
    overlay = open(os.path.join(ROOT, "include", "ilcc_overlay.h")).read()
    assert "rgblidar from bags" not in overlay and "time-synchronised pairing" not in overlay


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pairing_equals_the_brute_force(case):
    _, clouds, images, max_dt = case
    want_of, want_dt = R.pair_by_stamp(clouds, images, max_dt)
    got_of, got_dt = paired.pair_by_stamp(clouds, images, max_dt)
    assert got_of.tolist() == want_of and got_dt.tolist() == want_dt


def test_pairing_cases_are_what_they_are_named():
    by = {c[0]: R.pair_by_stamp(*c[1:]) for c in CASES}
    assert by["exact tie: the lower image wins"] == ([0, 0], [100, 100])
    assert by["equal stamps: the lower image wins"] == ([1, 1, 1], [0, 10, -10])
    assert by["dt == max_dt accepted, one ns above rejected"] == ([0, 0, -1, -1], [50, 50, 51, 51])       # 2051 and 1949 tie at 51: the lower image, rejected
    assert by["dt == max_dt on the early side"] == ([0, -1], [-50, -51])
    assert by["max_dt 0: equal stamps only"] == ([1, -1, 0], [0, 1, 0])              # 6 ties between 7 and 5: the lower image
    assert by["one image serves three clouds"][0] == [0, 0, 0, -1]
    assert by["no images"] == ([-1, -1, -1], [0, 0, 0])
    far = (2 ** 32 - 1) * K.SEC
    assert by["near 2^32 s: the subtraction does not wrap"] == ([2, 0, 1, 4], [2, -9, 3, -17])
    assert by["near 2^32 s, tight limit"][0] == [2, -1, 1] and far + 999999999 < 2 ** 63
    of, dt = by["random 2000 x 1500"]
    assert 300 < sum(j < 0 for j in of) < 1700 and len(set(of)) > 300 and any(d == 0 for d in dt)
    clouds, images = CASES[-1][1], CASES[-1][2]
    ties = sum(1 for c in clouds[:300] if sorted(abs(m - c) for m in images)[0] == sorted(abs(m - c) for m in images)[1])
    assert ties > 10                                                                                    # equal distances do occur


def test_pairing_beyond_int64_and_refusals():
    L = paired.lib()
    of, dt = paired.pair_by_stamp([0, 2 ** 64 - 1], [2 ** 64 - 1], 2 ** 64 - 1)
    assert of.tolist() == [-1, 0] and dt.tolist() == [2 ** 63 - 1, 0]                    # a |dt| of 2^63 ns or more is beyond every limit
    of, dt = paired.pair_by_stamp([2 ** 64 - 1], [0], 2 ** 64 - 1)
    assert of.tolist() == [-1] and dt.tolist() == [-2 ** 63]
    one = (C.c_uint64 * 1)(5)
    out = (C.c_int64 * 1)(0)
    assert L.ilcc_pair_by_stamp(None, 1, one, 1, 0, out, out) == N.BAD_ARGUMENT
    assert L.ilcc_pair_by_stamp(one, 1, None, 1, 0, out, out) == N.BAD_ARGUMENT
    assert L.ilcc_pair_by_stamp(one, 1, one, 1, 0, None, out) == N.BAD_ARGUMENT
    assert L.ilcc_pair_by_stamp(one, 1, one, 1, 0, out, None) == N.BAD_ARGUMENT
    assert L.ilcc_pair_by_stamp(None, 0, None, 0, 0, None, None) == N.OK
    assert L.ilcc_pair_by_stamp(one, 1, None, 0, 0, out, out) == N.OK and out[0] == 0


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = rng.normal(0, 10, (n, 4)).astype(np.float32)
    rec.view(np.uint32)[:, 3] = rng.integers(0, 1 << 24, n)                # packed rgb: denormal float patterns
    return rec


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_pcd_bytes(tmp_path, n):
    rec = _records(n)
    path = tmp_path / "a.pcd"
    paired.save_pcd_xyzrgb(str(path), rec)
    blob = path.read_bytes()
    assert blob == R.pcd_bytes(rec)
    assert blob.startswith(b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                           b"WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n))
    assert R.read_pcd(str(path)).tobytes() == rec.tobytes()


def test_pcd_refusals(tmp_path):
    rec = _records(3)
    with pytest.raises(paired.PairedError) as e:
        paired.save_pcd_xyzrgb(str(tmp_path / "no_such_dir" / "a.pcd"), rec)
    assert e.value.status == N.IO_ERROR
    L = paired.lib()
    assert L.ilcc_save_pcd_xyzrgb(None, rec.ctypes.data_as(C.c_void_p), 3) == N.BAD_ARGUMENT
    assert L.ilcc_save_pcd_xyzrgb(str(tmp_path / "b.pcd").encode(), None, 3) == N.BAD_ARGUMENT
    assert not (tmp_path / "b.pcd").exists()


def test_write_helper_numbers_the_paired_scans(tmp_path):
    items = [(paired.PairRecord(image_message=2), _records(5, 1)), (paired.PairRecord(image_message=-1), np.zeros((0, 4), np.float32)),
             (paired.PairRecord(image_message=0), _records(0)), (paired.PairRecord(image_message=2), _records(7, 2))]
    files = paired.write_rgblidar_pcds(items, str(tmp_path), merged=str(tmp_path / "all.pcd"))
    assert [os.path.basename(f) for f in files] == ["rgb_lidar_0.pcd", "rgb_lidar_1.pcd", "rgb_lidar_2.pcd", "all.pcd"]
    assert open(files[2], "rb").read() == R.pcd_bytes(items[3][1])
    assert open(files[3], "rb").read() == R.pcd_bytes(np.concatenate([items[0][1], items[3][1]]))


# ------------------------------------------------------------------------------------------ guards on the GPU tests' inputs

def test_constructed_batches_are_what_they_are_named():
    assert K.N_KEEP_PATTERNS == 22
    for p in (0, 1, 2, 21):
        b = K.keep_batch(p)
        n = np.diff(b["offsets"].astype(np.int64)).tolist()
        assert set(P.KEEP_N) <= set(n) and n.count(0) >= 4
        first, last = (b["image_of_scan"][0], n[0]), (b["image_of_scan"][-1], n[-1])
        assert first == last == ((0, 0) if p % 2 == 0 else (-1, 100))
        for s in np.flatnonzero(b["image_of_scan"] < 0):
            assert np.isnan(b["xyzi"][int(b["offsets"][s]):int(b["offsets"][s + 1])]).all()
        assert b["images"][0].shape[1] == 384 and b["images"][1].shape[1] == 384 + P.CAMERA_PAD
        rec, off = R.colourise_batch(b["xyzi"], b["offsets"], b["images"], b["image_of_scan"], b["cam"], b["dis"])
        assert (len(rec) == 0) == (p == 0) and off[-1] == len(rec)                        # pattern 0: no point survives anywhere
        assert not np.isnan(rec[:, :3]).any()
    assert K.n_chunks(K.many_chunks_small()) == 304 > 256
    assert K.n_chunks(K.many_chunks_1030()) == 1030
    names = [b["name"] for b in K.camera_batches()]
    assert all(any(("%dx%d" % wh) in n for n in names) for wh in P.CAMERA_SIZES)


def test_the_recording_is_what_it_claims(tmp_path):
    clouds, images = K.recording()
    assert len(clouds) == 7 and [e for _, _, e, _ in images] == ["mono8", "bgr8", "rgb8", "bayer_rggb8", "bgr8"]
    of, dt = R.pair_by_stamp([R.stamp_ns(s) for s, _ in clouds], [R.stamp_ns(s) for s, _, _, _ in images], K.MAX_DT_NS)
    assert of == [0, 1, 1, 2, 3, -1, 4] and dt[5] == -300 * 1000000 and dt[4] == 40 * 1000000
    want = R.chain(clouds, [(s, px, enc) for s, px, enc, _ in images], K.recording_camera(), K.T_LIDAR2CAM, K.DISTANCE, K.MAX_DT_NS)
    counts = [len(c) for _, c in want]
    assert counts[5] == 0 and all(100 < n < len(clouds[k][1]) for k, n in enumerate(counts) if k != 5), counts
    raw = R.chain(clouds, [(s, px, enc) for s, px, enc, _ in images], K.recording_camera(), K.T_LIDAR2CAM, K.DISTANCE, K.MAX_DT_NS, sample_raw=True)
    assert any(a.tobytes() != b.tobytes() for (_, a), (_, b) in zip(want, raw))            # the lens matters
    # budgets of the chain test: two clouds per batch by staging_bytes, so that clouds 1 and 2, which share image 1, fall apart
    sizes = K.cloud_data_bytes()
    assert all(sizes[k] + sizes[k + 1] + 16 <= 200000 < sizes[k] + sizes[k + 1] + sizes[k + 2] for k in range(5))


def test_cli_argument_errors(tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_rgblidar"
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, timeout=120)
    r = run()
    assert r.returncode == 2 and "usage: ilcc_rgblidar" in r.stderr
    r = run("--frobnicate")
    assert r.returncode == 2 and "unknown or incomplete argument: --frobnicate" in r.stderr
    r = run("--image-bag")
    assert r.returncode == 2 and "--image-bag" in r.stderr
    full = ["--image-bag", str(tmp_path / "a.bag"), "--image-topic", K.IMAGE_TOPIC, "--lidar-bag", str(tmp_path / "a.bag"), "--lidar-topic", K.LIDAR_TOPIC,
            "--yaml", str(tmp_path / "missing.yaml"), "--extrinsic", str(tmp_path / "missing.bin"), "--out-dir", str(tmp_path)]
    r = run(*full[:-2])
    assert r.returncode == 2 and "usage" in r.stderr
    r = run(*full)
    assert r.returncode == 1 and "missing.yaml" in r.stderr
    open(tmp_path / "cam.yaml", "w").write(K.yaml_text(K.recording_camera()))
    full[9] = str(tmp_path / "cam.yaml")
    r = run(*full)
    assert r.returncode == 1 and "can not open" in r.stderr and "missing.bin" in r.stderr


# ------------------------------------------------------------------------------------------ under sanitizers, stand-alone

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/paired_host_check.cpp + csrc/paired_host.cpp only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("paired_host_check")
    exe = str(out / "paired_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "paired_host_check.cpp"), os.path.join(csrc, "paired_host.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe, out


def _write_cases(path, cases, spoil=None):
    with open(path, "w") as fh:
        fh.write("%d\n" % len(cases))
        for k, (_, clouds, images, max_dt) in enumerate(cases):
            of, dt = R.pair_by_stamp(clouds, images, max_dt)
            if spoil == k:
                of[-1] += 1
            fh.write("%d %d %d\n" % (len(clouds), len(images), max_dt))
            for row in (clouds, images, of, dt):
                fh.write(" ".join(str(int(v)) for v in row) + "\n")


def test_host_layers_under_sanitizers_equal_the_restatement(host_check):
    exe, out = host_check
    _write_cases(str(out / "cases.txt"), CASES)
    r = subprocess.run([exe, str(out / "cases.txt"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "cases %d ok" % len(CASES) in r.stdout
    assert "unwritable %d null_name %d null_records %d null_clouds %d null_images %d" % (N.IO_ERROR, N.BAD_ARGUMENT, N.BAD_ARGUMENT, N.BAD_ARGUMENT,
                                                                                      N.BAD_ARGUMENT) in r.stdout
    for n in (0, 1, 1000):
        k = np.arange(n)
        rec = np.stack([k, -(k + 1), k / 2, np.zeros(n)], 1).astype(np.float32).reshape(n, 4)
        rec.view(np.uint32)[:, 3] = 0x00010203 * (k % 7)
        assert open(str(out / ("pcd_%d.pcd" % n)), "rb").read() == R.pcd_bytes(rec), n
    # and it does notice a mismatch: one expected image index moved by one
    _write_cases(str(out / "wrong.txt"), CASES, spoil=5)
    r = subprocess.run([exe, str(out / "wrong.txt"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "mismatch in case 5" in r.stdout
