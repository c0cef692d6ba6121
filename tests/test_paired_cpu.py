"""Every scan coloured from its time-paired image, the part that needs no GPU (include/ilcc_paired.h): the exports against the
header, the pairing against the brute force of tests/paired_ref.py, the PCD writer against its restated bytes, guards on the
constructed inputs of the GPU tests, the batch cut of the paired chains (csrc/paired_cut.cpp) against the restatement of
tests/paired_ref.py and against batches stated by hand, and csrc/paired_host.cpp with csrc/paired_cut.cpp alone as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes as C
import functools
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
    """The stand-alone program: tests/paired_host_check.cpp + csrc/paired_host.cpp + csrc/paired_cut.cpp only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("paired_host_check")
    exe = str(out / "paired_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "paired_host_check.cpp"),
                    os.path.join(csrc, "paired_host.cpp"), os.path.join(csrc, "paired_cut.cpp"), "-o", exe], check=True, timeout=300)
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


# ------------------------------------------------------------------------------------------ the batch cut of the paired chains

MB = 1 << 20
PAIRED = dict(staging=256 * MB, image=512 * MB, stage_unpaired=True)                     # ilcc_bag_rgblidar_all_scans' defaults
OVERLAY = dict(staging=256 * MB, image=512 * MB, device=1 << 30, member_cap=65535)       # ilcc_bag_pcd2image_all_pairs'


def _recording_numbers():
    """The sizes of K.recording(): (scans [(data_bytes, points, pair)], image_raw, bgr_bytes)."""
    clouds, images = K.recording()
    sizes = K.cloud_data_bytes()
    assert sizes == [96000, 80000, 99200, 70400, 92800, 73600, 86400] and all(v % 16 == 0 for v in sizes)
    pair = [0, 1, 1, 2, 3, -1, 4]                                                      # test_the_recording_is_what_it_claims
    up256 = lambda v: (v + 255) // 256 * 256
    steps = [step or px.shape[1] * (px.shape[2] if px.ndim == 3 else 1) for _, px, _, step in images]
    assert steps == [64, 199, 192, 67, 192]
    raw = [up256(48 * step) for step in steps]
    assert raw == [3072, 9728, 9216, 3328, 9216]
    return [(sizes[k], len(clouds[k][1]), pair[k]) for k in range(7)], raw, up256(3 * 64 * 48)


def _by_hand(scans, raw, bgr, groups):
    """groups: [(scans of the batch, its members, its images)] stated by hand -> the batches and the largest in cut_paired's form;
    sums only (every data_bytes here is a multiple of 16)."""
    batches = []
    for group, members, images in groups:
        b = dict(first_scan=group[0], scans=len(group), members=list(members), blob_bytes=sum(scans[s][0] for s in members),
                 points=sum(scans[s][1] for s in members), raw_bytes=sum(raw[j] for j in images), bgr_bytes=bgr * len(images),
                 images=[(j, sum(raw[i] for i in images[:at]), bgr * at) for at, j in enumerate(images)])
        assert group == list(range(group[0], group[0] + len(group)))
        batches.append(b)
    largest = {key: max(b[key] for b in batches) for key in ("blob_bytes", "points", "raw_bytes", "bgr_bytes")}
    largest["members"] = max(len(b["members"]) for b in batches)
    return batches, largest


def _recording_cut_cases():
    """[(name, arguments of cut_paired, the batches stated by hand)] under each budget set of the two GPU chain tests."""
    from lidar_camera_calibration_amd import overlay
    scans, raw, bgr = _recording_numbers()
    sizes = [s[0] for s in scans]
    per_scan = overlay.overlay_sequence_bytes(64, 48)
    assert raw[1] + bgr <= 20000 < raw[0] + bgr + raw[3] + bgr                        # any two images are above image_bytes=20000
    alone = [([s], [s], [scans[s][2]] if scans[s][2] >= 0 else []) for s in range(7)]
    two_by_staging = [([0, 1], [0, 1], [0, 1]), ([2, 3], [2, 3], [1, 2]), ([4, 5], [4, 5], [3]), ([6], [6], [4])]
    unstaged = lambda groups: [(g, [s for s in m if scans[s][2] >= 0], i) for g, m, i in groups]
    cases = [
        ("paired: defaults, one batch", dict(PAIRED), [(list(range(7)), list(range(7)), [0, 1, 2, 3, 4])]),
        ("paired: staging 200000, two clouds a batch, image 1 in batches 0 and 1", dict(PAIRED, staging=200000), two_by_staging),
        ("paired: image 20000, one image a batch", dict(PAIRED, image=20000),
         [([0], [0], [0]), ([1, 2], [1, 2], [1]), ([3], [3], [2]), ([4, 5], [4, 5], [3]), ([6], [6], [4])]),
        ("paired: staging max(sizes), seven batches", dict(PAIRED, staging=max(sizes)), alone),
        ("overlay: staging 350000, scans 0 .. 3 and 4 .. 6", dict(OVERLAY, staging=350000, per_member=per_scan),
         [([0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2]), ([4, 5, 6], [4, 6], [3, 4])]),
        ("overlay: staging max(sizes), seven batches, the unpaired scan's without a member", dict(OVERLAY, staging=max(sizes), per_member=per_scan),
         unstaged(alone)),
        ("overlay: device per_scan, the unpaired scan rides with scan 4", dict(OVERLAY, device=per_scan, per_member=per_scan),
         [([0], [0], [0]), ([1], [1], [1]), ([2], [2], [1]), ([3], [3], [2]), ([4, 5], [4], [3]), ([6], [6], [4])]),
        ("overlay: staging 200000 and device 2 per_scan", dict(OVERLAY, staging=200000, device=2 * per_scan, per_member=per_scan), unstaged(two_by_staging)),
    ]
    assert sum(sizes[:4]) <= 350000 < sum(sizes[:5]) and sum(sizes[4:]) <= 350000 and min(sizes) * 2 > max(sizes)
    return [(name, dict(kw, scans=scans, image_raw=raw, bgr_bytes=bgr), _by_hand(scans, raw, bgr, groups)) for name, kw, groups in cases]


def _constructed_cut_cases():
    """[(name, arguments of cut_paired, (batches, largest) stated by hand or the refusal's kind)], each in both modes.  One image
    costs 256 + 256 bytes; a batch below is (first_scan, scans, members, blob_bytes, points, images)."""
    P32 = 2 ** 32
    big = dict(staging=1 << 40, image=1 << 40)
    modes = (("staged", dict(stage_unpaired=True)), ("unstaged", dict(stage_unpaired=False)))
    cases = []

    def add(name, scans, kw, want, n_images=2):
        for mode, flag in modes:
            w = want[mode] if isinstance(want, dict) else want
            if not isinstance(w, str):
                batches = [dict(first_scan=f, scans=n, members=list(m), blob_bytes=blob, points=pts, raw_bytes=256 * len(im), bgr_bytes=256 * len(im),
                                images=[(j, 256 * at, 256 * at) for at, j in enumerate(im)]) for f, n, m, blob, pts, im in w]
                largest = {key: max(b[key] for b in batches) for key in ("blob_bytes", "points", "raw_bytes", "bgr_bytes")}
                largest["members"] = max(len(b["members"]) for b in batches)
                w = (batches, largest)
            cases.append(("%s, %s" % (name, mode), dict(big, **dict(kw, **flag), scans=scans, image_raw=[256] * n_images, bgr_bytes=256), w))

    # 33 + 52 = 85 bytes, but the second scan starts at 48: the batch ends at 100
    add("staging: exactly at the limit", [(33, 1, 0), (52, 1, 0)], dict(staging=100), [(0, 2, [0, 1], 100, 2, [0])])
    add("staging: one byte below, the alignment decides", [(33, 1, 0), (52, 1, 0)], dict(staging=99), [(0, 1, [0], 33, 1, [0]), (1, 1, [1], 52, 1, [0])])
    add("staging: an unpaired scan counts though it is not staged", [(33, 1, -1), (52, 1, 0)], dict(staging=99),
        dict(staged=[(0, 1, [0], 33, 1, []), (1, 1, [1], 52, 1, [0])], unstaged=[(0, 1, [], 0, 0, []), (1, 1, [1], 52, 1, [0])]))
    add("staging: the blob of the staged scans alone", [(33, 1, -1), (52, 1, 0), (8, 1, 1)], dict(staging=200),
        dict(staged=[(0, 3, [0, 1, 2], 120, 3, [0, 1])], unstaged=[(0, 3, [1, 2], 72, 2, [0, 1])]))
    add("an image shared across a boundary is charged twice", [(64, 5, 0), (64, 6, 0)], dict(staging=64, image=512),
        [(0, 1, [0], 64, 5, [0]), (1, 1, [1], 64, 6, [0])])
    add("image: a second image at the limit", [(16, 1, 0), (16, 1, 1)], dict(image=1024), [(0, 2, [0, 1], 32, 2, [0, 1])])
    add("image: a second image one above", [(16, 1, 0), (16, 1, 1)], dict(image=1023), [(0, 1, [0], 16, 1, [0]), (1, 1, [1], 16, 1, [1])])
    runs = [(16, 3, j) for j in (-1, -1, 0, -1, -1, 1, -1, -1)]
    add("runs of unpaired scans at the start, in the middle and at the end", runs, dict(staging=32),
        dict(staged=[(0, 2, [0, 1], 32, 6, []), (2, 2, [2, 3], 32, 6, [0]), (4, 2, [4, 5], 32, 6, [1]), (6, 2, [6, 7], 32, 6, [])],
             unstaged=[(0, 2, [], 0, 0, []), (2, 2, [2], 16, 3, [0]), (4, 2, [5], 16, 3, [1]), (6, 2, [], 0, 0, [])]))
    add("points: 2^32 - 2 fit", [(0, P32 - 3, 0), (0, 1, 0)], {}, [(0, 2, [0, 1], 0, P32 - 2, [0])])
    add("points: 2^32 - 1 close the batch", [(0, P32 - 3, 0), (0, 2, 0)], {}, [(0, 1, [0], 0, P32 - 3, [0]), (1, 1, [1], 0, 2, [0])])
    add("points: an unpaired scan's count only where it is staged", [(0, P32 - 3, 0), (0, 5, -1), (0, 1, 0)], {},
        dict(staged=[(0, 1, [0], 0, P32 - 3, [0]), (1, 2, [1, 2], 0, 6, [0])], unstaged=[(0, 3, [0, 2], 0, P32 - 2, [0])]))
    add("points: a paired scan of 2^32 - 1", [(0, P32 - 1, 0)], {}, "BAD_ARGUMENT")
    # staged: the unpaired scan is a member, so the large one closes the batch and is then refused as the first of its own
    add("points: a paired scan of 2^32 - 1 behind an unpaired one", [(0, 1, -1), (0, P32 - 1, 0)], {}, "BAD_ARGUMENT")
    add("points: an unpaired scan of 2^32 - 1", [(0, P32 - 1, -1)], {}, dict(staged="BAD_ARGUMENT", unstaged=[(0, 1, [], 0, 0, [])]))
    add("members: 65535 under the cap", [(0, 0, 0)] * 65535, dict(member_cap=65535), [(0, 65535, range(65535), 0, 0, [0])])
    add("members: 65536, one above the cap", [(0, 0, 0)] * 65536, dict(member_cap=65535),
        [(0, 65535, range(65535), 0, 0, [0]), (65535, 1, [65535], 0, 0, [0])])
    add("device: two members at the limit", [(16, 1, 0)] * 3, dict(device=2000, per_member=1000), [(0, 2, [0, 1], 32, 2, [0]), (2, 1, [2], 16, 1, [0])])
    add("device: one member at the limit", [(16, 1, 0)] * 2, dict(device=1000, per_member=1000), [(0, 1, [0], 16, 1, [0]), (1, 1, [1], 16, 1, [0])])
    add("device: one member above it", [(16, 1, 0)] * 2, dict(device=999, per_member=1000), "CAPACITY")
    add("staging: a scan at the limit", [(100, 1, 0)], dict(staging=100), [(0, 1, [0], 100, 1, [0])])
    add("staging: a scan above it", [(16, 1, 0), (101, 1, -1)], dict(staging=100), "CAPACITY")
    add("image: an image at the limit", [(16, 1, 1)], dict(image=512), [(0, 1, [0], 16, 1, [1])])
    add("image: an image above it", [(16, 1, -1), (16, 1, 1)], dict(image=511), "CAPACITY")
    return cases


@functools.lru_cache(maxsize=None)
def _cut_cases():
    return _recording_cut_cases() + _constructed_cut_cases()


def _restated(kw):
    try:
        return R.cut_paired(**kw)
    except R.CutRefused as e:
        return e.kind


def test_cut_restatement_gives_the_batches_stated_by_hand():
    cases = _cut_cases()
    assert len(cases) == 8 + 2 * 23
    for name, kw, want in cases:
        got = _restated(kw)
        assert got == want, name
    by = {name: want for name, _, want in cases}
    shared = by["paired: staging 200000, two clouds a batch, image 1 in batches 0 and 1"][0]
    assert [b["images"] for b in shared[:2]] == [[(0, 0, 0), (1, 3072, 9216)], [(1, 0, 0), (2, 9728, 9216)]]
    assert [len(b["members"]) for b in by["overlay: staging max(sizes), seven batches, the unpaired scan's without a member"][0]] == [1, 1, 1, 1, 1, 0, 1]


def _write_cut_cases(path, cases, spoil=None):
    status = {"CAPACITY": N.CAPACITY, "BAD_ARGUMENT": N.BAD_ARGUMENT}
    with open(path, "w") as fh:
        line = lambda row: fh.write(" ".join(str(int(v)) for v in row) + "\n")
        line([len(cases)])
        for k, (_, kw, _) in enumerate(cases):
            scans = kw["scans"]
            line([len(scans), len(kw["image_raw"]), kw["bgr_bytes"], kw["staging"], kw["image"], kw.get("device", 0), kw.get("per_member", 0),
                  kw.get("member_cap", 0), kw.get("stage_unpaired", False)])
            for column in range(3):
                line([s[column] for s in scans])
            line(kw["image_raw"])
            got = _restated(kw)                                                     # the expectation is the restatement's
            if isinstance(got, str):
                line([status[got], 0])
                continue
            batches, largest = got
            line([N.OK, len(batches)])
            for at, b in enumerate(batches):
                line([b["first_scan"] + (1 if spoil == k and at == len(batches) - 1 else 0), b["scans"], b["blob_bytes"], b["points"], b["raw_bytes"],
                      b["bgr_bytes"]])
                line(b["members"])
                line([v for slot in b["images"] for v in slot])
            line([largest[key] for key in ("members", "blob_bytes", "points", "raw_bytes", "bgr_bytes")])


def test_cut_under_sanitizers_equals_the_restatement(host_check):
    exe, out = host_check
    cases = _cut_cases()
    _write_cases(str(out / "few.txt"), CASES[:2])
    _write_cut_cases(str(out / "cuts.txt"), cases)
    r = subprocess.run([exe, str(out / "few.txt"), str(out), str(out / "cuts.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "cut cases %d ok" % len(cases) in r.stdout and "cases 2 ok" in r.stdout
    assert "cut case 1 batch 1: first_scan 2 scans 2 members 2 blob 169600 points 5300 raw 18944 bgr 18432 images 2" in r.stdout
    # and it does notice a mismatch: the last batch's first_scan of one case moved by one
    _write_cut_cases(str(out / "wrong_cuts.txt"), cases, spoil=4)
    r = subprocess.run([exe, str(out / "few.txt"), str(out), str(out / "wrong_cuts.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "mismatch in cut case 4" in r.stdout and "mismatch in cut case 3" not in r.stdout
