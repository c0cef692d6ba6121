"""The parts of include/ilcc_image_structure.h that need no GPU: the host code's per-seed stage output
(ilcc_chessboard_seed_board) with the overlap rule replayed in Python, the refusals of the batch entry and of the route field
of both chains and the CLI, the ctypes layouts, and the host code under ASan and UBSan in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import structure_cases as S
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import image_sequence as IS
from lidar_camera_calibration_amd import jpeg_sequence as JS
from lidar_camera_calibration_amd.image_corners import CORNER_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_image_corners")


def host(c):
    try:
        return N.OK, IC.chessboard_from_corners(c.corners, c.board)
    except IC.BoardNotFound as e:
        return e.status, None


def test_exports_match_the_header_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "ilcc_image_structure.h")).read()
    declared = re.findall(r"^(?:int32_t|uint32_t|void|ilcc_structure_plan\*) (ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(IS.IMAGE_STRUCTURE_EXPORTS) and len(set(declared)) == len(declared)
    L = IS.lib()
    for s in IS.IMAGE_STRUCTURE_EXPORTS:
        assert hasattr(L, s), s
    assert int(re.search(r"#define ILCC_STRUCTURE_MAX_CORNERS (\d+)", hdr).group(1)) == IS.STRUCTURE_MAX_CORNERS == 4096
    assert re.search(r"#define ILCC_STRUCTURE_MAX_CELLS ILCC_MAX_CORNERS", hdr) and N.MAX_CORNERS == 256
    assert int(re.search(r"#define ILCC_STRUCTURE_MAX_SIDE (\d+)", hdr).group(1)) == 64
    # the headers whose export tests compare them with their own lists got none of the new names
    for name in ("ilcc_image_sequence.h", "ilcc_image_corners.h", "ilcc_jpeg_sequence.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert not set(re.findall(r"\b(ilcc_\w+)\s*\(", other)) & set(IS.IMAGE_STRUCTURE_EXPORTS)


def test_ctypes_layouts():
    assert C.sizeof(IS.ImageSequenceParams) == 40 and IS.ImageSequenceParams.reserved0.offset == 12
    assert JS.JpegSequenceParams.seq.offset == 0 and JS.JpegSequenceParams.reserved0.offset == 44 and C.sizeof(JS.JpegSequenceParams) == 48
    assert C.sizeof(IC.ImageCorner) == 56 == CORNER_DTYPE.itemsize
    assert IS.structure_route("host") == 0 and IS.structure_route("gpu") == 1 and IS.structure_route(2) == 2
    assert IS.default_params().reserved0 == 0 and JS.default_params().seq.reserved0 == 0        # the host route is the default


@pytest.mark.parametrize("name", ["A", "C", "K", "I"])
def test_seed_boards_and_the_replayed_overlap_rule_give_the_host_answer(name):
    c = S.case(name)
    st, idx = host(c)
    assert st == c.status
    seeds = [IS.seed_board(c.corners, s) for s in range(len(c.corners))]
    got_st, got = S.replay_overlap_rule(seeds, c.board)
    assert got_st == st
    if st == N.OK:
        assert got.shape == idx.shape and np.array_equal(got, idx)
    grown = [(b, e) for b, e in seeds if b is not None]
    assert len(grown) >= 3        # the comparison must not pass on seeds without boards (the hole of case I leaves six)
    for b, e in grown:
        assert b.shape[0] >= 3 and b.shape[1] >= 3 and len(set(b.reshape(-1).tolist())) == b.size and b.min() >= 0 and b.max() < len(c.corners)
        if b.shape in ((7, 5), (5, 7)):
            assert e < -10, e        # a full board passes the keep test: -35 + 35 x (a collinearity error of a few hundredths)
    if name != "I":
        assert any(b.shape in ((7, 5), (5, 7)) for b, _ in grown)
    for b, e in seeds:
        if b is None:
            assert e == 0.0


def test_seed_board_refusals_and_capacity():
    a = S.case("A").corners
    i32p = C.POINTER(C.c_int32)
    rows, cols, e = C.c_int32(7), C.c_int32(7), C.c_double(7)
    idx = np.full(35, -7, np.int32)
    L = IS.lib()

    def call(corners, n, seed, cap, index=idx):
        return L.ilcc_chessboard_seed_board(corners.ctypes.data_as(C.c_void_p) if corners is not None else None, n, seed, C.byref(rows), C.byref(cols),
                                            index.ctypes.data_as(i32p) if index is not None else None, cap, C.byref(e))
    for args in ((None, 35, 0, 35), (a, 0, 0, 35), (a, 35, 35, 35), (a, 35, -1, 35), (a, 35, 0, -1), (a, 35, 17, 35, None)):
        assert call(*args) == N.BAD_ARGUMENT, args[1:]
    assert (rows.value, cols.value, e.value) == (7, 7, 7.0) and (idx == -7).all()
    full = next(s for s in range(35) if (IS.seed_board(a, s)[0] is not None and IS.seed_board(a, s)[0].size == 35))
    assert call(a, 35, full, 34) == N.CAPACITY and rows.value * cols.value == 35 and (idx == -7).all()
    assert call(a, 35, full, 35) == N.OK and sorted(idx.tolist()) == list(range(35))
    with pytest.raises(IS.ImageSequenceError):
        IS.seed_board(a, 35)


def test_batch_refusals_that_need_no_device():
    a = S.case("A").corners
    i32p = C.POINTER(C.c_int32)
    cnt = np.array([35], np.int32)
    out = [np.full(1, 77, np.int32) for _ in range(3)] + [np.full(256, 77, np.int32)]
    L = IS.lib()

    def call(board, plan=None):
        return L.ilcc_chessboards_from_corners_batch(a.ctypes.data_as(C.c_void_p), 35, cnt.ctypes.data_as(i32p), 1, board[0], board[1],
                                                     *[o.ctypes.data_as(i32p) for o in out], plan, None)
    for board in ((7, 5), (2, 5), (7, 2), (16, 17), (0, 0), (-3, -3)):
        assert call(board) == N.BAD_ARGUMENT, board          # a null plan, and a bad board on top
        assert L.ilcc_last_error(None).decode().startswith("ilcc_chessboards_from_corners_batch: ")
    assert all((o == 77).all() for o in out)
    assert L.ilcc_structure_plan_launches(None) == 0 and L.ilcc_structure_plan_fallbacks(None) == 0 and L.ilcc_structure_plan_allocations(None) == 0
    L.ilcc_structure_plan_destroy(None)
    assert L.ilcc_structure_plan_create(0, 100) is None and L.ilcc_structure_plan_create(70000, 100) is None and L.ilcc_structure_plan_create(4, 0) is None
    r, k, e = C.c_int32(0), C.c_int32(0), C.c_double(0)
    assert L.ilcc_structure_plan_seed_board(None, 0, 0, C.byref(r), C.byref(k), None, 0, C.byref(e)) == N.BAD_ARGUMENT


def test_a_route_above_one_is_refused_by_both_chains_and_the_cli(tmp_path):
    missing = str(tmp_path / "none.bag")       # refused before the bag is opened
    for fn in (IS.bag_corners_all_images, JS.bag_corners_all_compressed_images):
        with pytest.raises(ValueError):
            fn(missing, "/t", None, (7, 5), structure="x")
        with pytest.raises(IS.ImageSequenceError) as e:
            fn(missing, "/t", None, (7, 5), structure=2)
        assert e.value.status == N.BAD_ARGUMENT and "route of structure recovery" in str(e.value)
        out, records = fn(missing, "/t", None, (7, 5), structure=2, raise_on_failure=False)
        assert out.status == N.BAD_ARGUMENT and records == []
        with pytest.raises(IS.ImageSequenceError) as e:      # the routes themselves get as far as the missing bag
            fn(missing, "/t", None, (7, 5), structure="gpu")
        assert e.value.status == N.IO_ERROR
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_image_corners"
    base = [CLI, "--bag", missing, "--topic", "/t", "--yaml", str(tmp_path / "none.yaml"), "--out", str(tmp_path / "o.txt")]
    r = subprocess.run(base + ["--all-images", "--structure", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--structure" in r.stderr
    r = subprocess.run(base + ["--all-images", "--structure"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    r = subprocess.run(base + ["--structure", "gpu"], capture_output=True, text=True, timeout=60)      # needs --all-images, like --huffman
    assert r.returncode == 2 and "--structure, --decode-threads and --huffman need it" in r.stderr
    r = subprocess.run(base + ["--all-images", "--structure", "gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "none.yaml" in r.stderr       # accepted: it gets as far as the missing yaml


def _hip_include():
    for root in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    return None


def test_host_code_under_sanitizers_equals_the_library(tmp_path):
    """tests/image_structure_host_check.cpp + csrc/image_corners_host.cpp only, under ASan and UBSan, on cases A, C and I"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    hip = _hip_include()
    if not cxx or not hip:
        pytest.skip("needs a C++ compiler and the HIP headers that csrc/host_util.h includes")
    exe = str(tmp_path / "image_structure_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-isystem", hip,
                    os.path.join(ROOT, "tests", "image_structure_host_check.cpp"), os.path.join(csrc, "image_corners_host.cpp"), "-o", exe],
                   check=True, timeout=300)
    names = ["A", "C", "I"]
    src, dst = str(tmp_path / "corners.txt"), str(tmp_path / "boards.txt")
    with open(src, "w") as fh:
        for n in names:
            c = S.case(n)
            fh.write("%d %d %d\n" % (len(c.corners), c.board[0], c.board[1]))
            for k in c.corners:
                fh.write("%r %r %r %r %r %r\n" % (float(k["u"]), float(k["v"]), float(k["v1"][0]), float(k["v1"][1]), float(k["v2"][0]), float(k["v2"][1])))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "cases 3" in r.stdout
    lines = open(dst).read().split("\n")
    at = 0
    for n in names:
        c = S.case(n)
        st, idx = host(c)
        head = [int(v) for v in lines[at].split()]
        at += 1
        assert head[0] == st == c.status
        if st == N.OK:
            assert tuple(head[1:3]) == idx.shape and head[3:] == idx.reshape(-1).tolist()
        else:
            assert head[1:] == [0, 0]
        for seed in range(len(c.corners)):
            want, want_e = IS.seed_board(c.corners, seed)
            f = lines[at].split()
            at += 1
            assert float(f[2]) == want_e, (n, seed)
            if want is None:
                assert f[:2] == ["0", "0"] and len(f) == 3
            else:
                assert (int(f[0]), int(f[1])) == want.shape and [int(v) for v in f[3:]] == want.reshape(-1).tolist()
    assert lines[at:] == [""]
