"""Corners from every scan of a bag, the part that needs no GPU (include/ilcc_sequence.h): the topic iterator against the
restated message order (tests/sequence_ref.py), the fusion against its restatement on constructed corner sets and on the
CPU oracle's corners of synthetic sequences, and the fusion alone as a stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rosbag_writer as W
import sequence_cases as K
import sequence_ref as R
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import ingest, sequence, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC2 = ("sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5)
TOPIC, OTHER = "/velodyne_points", "/other"


def _payload(tag, n=3):
    pts = np.full((n, 4), float(tag), np.float32)
    a, fields, step = W.velodyne_points(pts)
    return W.pointcloud2(a, fields, step, seq=tag)


def _mixed_bag(path, compression):
    """Three chunks: times out of order across chunks, equal times across chunks and inside one, a second connection on the topic with
    a foreign md5, another topic in between."""
    w = W.BagWriter(str(path), compression)
    good = (TOPIC,) + PC2
    foreign = (TOPIC, "sensor_msgs/Image", "060021388200f6f0f447d0fcd9c64743")
    other = (OTHER,) + PC2
    w.add_chunk([good + ((20, 0), _payload(1)), other + ((20, 1), _payload(2)), good + ((30, 5), _payload(3)), good + ((30, 5), _payload(4, 0))])
    w.add_chunk([foreign + ((5, 0), b"not a cloud"), good + ((10, 7), _payload(5)), good + ((30, 5), _payload(6)), other + ((1, 0), _payload(7))])
    w.add_chunk([good + ((20, 0), _payload(8)), good + ((10, 6), _payload(9, 1)), good + ((40, 0), _payload(10))])
    w.write()
    return w


@pytest.mark.parametrize("compression", ["none", "bz2", "lz4"])
def test_iterator_order_count_and_stamps(tmp_path, compression):
    w = _mixed_bag(tmp_path / "mixed.bag", compression)
    want = R.message_order(w.chunks, {w.conns[(TOPIC,) + PC2]})
    assert [R.parse_pointcloud2(p)["seq"] for _, p in want] == [9, 5, 1, 8, 3, 4, 6, 10]     # the order, written out once
    with sequence.BagTopic(str(tmp_path / "mixed.bag"), TOPIC) as it:
        assert len(it) == len(want)
        for i, (tm, payload) in enumerate(want):
            assert it.time(i) == tm
            assert it.size(i) == len(payload)
            assert it.read(i) == payload
        assert it.read(0) == ingest.bag_first_message(str(tmp_path / "mixed.bag"), TOPIC)
        for i in (5, 0, 7, 2):                                   # any order: the chunk cache follows
            assert it.read(i) == want[i][1]
    got = list(sequence.bag_messages(str(tmp_path / "mixed.bag"), TOPIC))
    assert got == want
    # the other topic, "*" on the wanted side, and the foreign type by its own md5
    other = R.message_order(w.chunks, {w.conns[(OTHER,) + PC2]})
    assert list(sequence.bag_messages(str(tmp_path / "mixed.bag"), OTHER)) == other
    both = R.message_order(w.chunks, {c for k, c in w.conns.items() if k[0] == TOPIC})
    assert list(sequence.bag_messages(str(tmp_path / "mixed.bag"), TOPIC, "*")) == both
    assert both[0][1] == ingest.bag_first_message(str(tmp_path / "mixed.bag"), TOPIC, "*")
    assert [p for _, p in sequence.bag_messages(str(tmp_path / "mixed.bag"), TOPIC, "060021388200f6f0f447d0fcd9c64743")] == [b"not a cloud"]


def test_iterator_topic_with_one_message_and_capacity_contract(tmp_path):
    w = W.BagWriter(str(tmp_path / "one.bag"))
    w.add_chunk([(TOPIC,) + PC2 + ((3, 4), _payload(1, 5)), (OTHER,) + PC2 + ((1, 0), _payload(2))])
    w.write()
    L = sequence.lib()
    with sequence.BagTopic(str(tmp_path / "one.bag"), TOPIC) as it:
        assert len(it) == 1 and it.time(0) == (3, 4)
        msg = it.read(0)
        assert msg == _payload(1, 5) == ingest.bag_first_message(str(tmp_path / "one.bag"), TOPIC)
        import ctypes as C
        n = C.c_uint64(0)
        buf = (C.c_uint8 * len(msg))(*([0xEE] * len(msg)))
        assert L.ilcc_bag_topic_read(it._it, 0, buf, len(msg) - 1, C.byref(n)) == N.CAPACITY       # one byte short: the size, nothing copied
        assert n.value == len(msg) and bytes(buf) == b"\xEE" * len(msg)
        assert "message larger than the buffer" in L.ilcc_last_error(None).decode()
        assert L.ilcc_bag_topic_read(it._it, 0, None, 0, C.byref(n)) == N.CAPACITY and n.value == len(msg)
        assert L.ilcc_bag_topic_read(it._it, 0, buf, len(msg), C.byref(n)) == N.OK and bytes(buf) == msg
        assert L.ilcc_bag_topic_read(it._it, 1, buf, len(msg), C.byref(n)) == N.BAD_ARGUMENT
        sec = C.c_uint32(0)
        assert L.ilcc_bag_topic_time(it._it, 1, C.byref(sec), C.byref(sec)) == N.BAD_ARGUMENT
        assert L.ilcc_bag_topic_read(it._it, 0, None, 4, C.byref(n)) == N.BAD_ARGUMENT


def _refusal(path, topic=TOPIC, md5=None):
    with pytest.raises(ingest.IngestError) as first:
        ingest.bag_first_message(str(path), topic, md5)
    with pytest.raises(ingest.IngestError) as every:
        sequence.BagTopic(str(path), topic, md5)
    assert (every.value.status, str(every.value)) == (first.value.status, str(first.value))      # the same refusal, the same text
    return every.value


def test_iterator_refusals_are_those_of_the_first_message_entry(tmp_path):
    w = W.BagWriter(str(tmp_path / "unindexed.bag"))
    w.add_chunk([(TOPIC,) + PC2 + ((1, 0), _payload(1))])
    w.write(indexed=False)
    e = _refusal(tmp_path / "unindexed.bag")
    assert e.status == N.IO_ERROR and "unindexed" in str(e)

    w = W.BagWriter(str(tmp_path / "zstd.bag"))
    w.compression = "none"
    w.add_chunk([(TOPIC,) + PC2 + ((1, 0), _payload(1))])
    w.write()
    raw = open(tmp_path / "zstd.bag", "rb").read()
    assert raw.count(b"compression=none") == 1
    open(tmp_path / "zstd.bag", "wb").write(raw.replace(b"compression=none", b"compression=zstd"))
    e = _refusal(tmp_path / "zstd.bag")
    assert e.status == N.IO_ERROR and "unknown chunk compression 'zstd'" in str(e)

    w = W.BagWriter(str(tmp_path / "ok.bag"))
    w.add_chunk([(TOPIC,) + PC2 + ((1, 0), _payload(1))])
    w.write()
    e = _refusal(tmp_path / "ok.bag", "/nothing_here")
    assert e.status == N.BAD_ARGUMENT and "no message of that type on topic /nothing_here" in str(e)
    e = _refusal(tmp_path / "ok.bag", TOPIC, "0123456789abcdef0123456789abcdef")
    assert e.status == N.BAD_ARGUMENT and "no message of that type on topic" in str(e)
    e = _refusal(tmp_path / "missing.bag")
    assert e.status == N.IO_ERROR and "cannot open" in str(e)
    open(tmp_path / "text.bag", "wb").write(b"hello, this is no bag at all")
    e = _refusal(tmp_path / "text.bag")
    assert e.status == N.IO_ERROR and "not a ROS bag V2.0" in str(e)
    raw = open(tmp_path / "ok.bag", "rb").read()
    open(tmp_path / "cut.bag", "wb").write(raw[:len(raw) - 40])
    assert _refusal(tmp_path / "cut.bag").status == N.IO_ERROR


def _same(got, used, dist, want):
    assert (got.status, got.n_scans, got.n_ok, got.n_used, got.ref_scan, got.n_corners) == \
        (want.status, want.n_scans, want.n_ok, want.n_used, want.ref_scan, want.n_corners)
    assert list(used) == list(want.used)
    assert got.corners_array().tobytes() == want.corners.tobytes()                     # exactly
    assert got.spread_max == want.spread_max                                             # exactly
    assert abs(got.spread_rms - want.spread_rms) <= 1e-12 * abs(want.spread_rms)      # the summation order is the only freedom
    assert np.allclose(dist, want.dist, rtol=1e-15, atol=0)


CASES = K.fusion_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fusion_equals_the_restatement_on_constructed_corners(case):
    name, corners, accepted, a, b, gate = case
    want = R.fuse(corners, accepted, a, b, gate)
    got, used, dist = sequence.fuse_corners(corners, accepted, a, b, gate)
    _same(got, used, dist, want)


def test_constructed_cases_are_what_they_are_named():
    by = {c[0]: R.fuse(*c[1:]) for c in CASES}
    for n in (7, 6):
        f = by["variants_n%d" % n]
        assert (f.status, f.n_used) == (R.OK, n) and list(f.variants) == [k % 4 for k in range(n)]
        assert f.spread_max <= 8 * K.Q * 3 ** 0.5
    t = by["tie"]
    assert t.status == R.OK and set(t.variants) == {0}                  # outer flip ties with "as is" everywhere: the lower index wins
    o = by["one_square_off"]
    assert o.status == R.OK and o.ref_scan == 0 and [i for i in range(9) if not o.used[i]] == [0, 4]
    assert by["at_gate"].n_used == 5 and by["at_gate"].dist[3] == 0.0625
    assert by["gate_one_ulp_below"].n_used == 4 and not by["gate_one_ulp_below"].used[3]
    assert by["coordinate_one_ulp_above"].n_used == 4 and not by["coordinate_one_ulp_above"].used[3]
    assert (by["no_majority"].status, by["no_majority"].n_ok, by["no_majority"].n_used, by["no_majority"].n_corners) == (R.AMBIGUOUS, 4, 2, 0)
    assert (by["none_used"].status, by["none_used"].n_used) == (R.AMBIGUOUS, 0)
    assert (by["none_accepted"].status, by["none_accepted"].n_corners) == (R.BOARD_NOT_FOUND, 0)
    assert (by["no_scans"].status, by["no_scans"].n_scans) == (R.BOARD_NOT_FOUND, 0)
    assert (by["nan_not_accepted"].status, by["nan_not_accepted"].n_ok, by["nan_not_accepted"].ref_scan) == (R.OK, 3, 1)
    assert (by["single"].status, by["single"].n_used, by["single"].spread_max) == (R.OK, 1, 0.0)
    # scan k is numbered by variant (k + 1) % 4; relative to the reference scan's own numbering (variant 1) that is ((k + 1) % 4) ^ 1
    assert by["square"].status == R.OK and list(by["square"].variants) == [0, 3, 2, 1, 0, 3]


def test_fusion_refuses_bad_arguments():
    base = K.lattice(4, 6)[None]
    for a, b, gate in ((0, 6, 1.0), (4, 0, 1.0), (32, 32, 1.0), (4, 6, 0.0), (4, 6, -1.0), (4, 6, float("nan")), (4, 6, float("inf"))):
        c = np.zeros((1, a * b, 3), np.float32) if (a, b) != (4, 6) else base
        got, _, _ = sequence.fuse_corners(c, [1], a, b, gate)
        assert (got.status, got.n_corners) == (N.BAD_ARGUMENT, 0), (a, b, gate)
    bad = base.copy()
    bad[0, 3, 1] = np.inf
    got, _, _ = sequence.fuse_corners(bad, [1], 4, 6, 1.0)
    assert got.status == N.BAD_ARGUMENT == R.fuse(bad, [1], 4, 6, 1.0).status


@pytest.mark.parametrize("pose_index", [0, 1, 2])
def test_fusion_on_the_oracle_s_corners_rejects_the_shifted_scans_and_beats_a_single_scan(pose_index):
    corners, accepted, status, flags = K.oracle_sequence(pose_index)
    _, _, pose, board = K.sequence(pose_index)
    a, b = board.w - 1, board.h - 1
    want = R.fuse(corners, accepted, a, b, board.g / 2)
    got, used, dist = sequence.fuse_corners(corners, accepted, a, b, board.g / 2)
    _same(got, used, dist, want)
    assert got.status == N.OK
    assert [int(i) for i in np.flatnonzero(used)] == K.ORACLE_USED[pose_index]
    gt = synth.true_corners(pose, board)
    per_scan = [synth.corner_error(corners[s], gt, board) for s in range(K.N_SCANS) if s not in K.SHIFTED and status[s] in (N.OK, N.AMBIGUOUS)]
    fused = synth.corner_error(got.corners_array(), gt, board)
    print("pose %d: fused %.2f mm, per scan median %.2f mm, spread rms %.2f max %.2f mm, distances %s"
          % (pose_index, fused * 1e3, np.median(per_scan) * 1e3, got.spread_rms * 1e3, got.spread_max * 1e3, np.round(dist * 1e3, 1)))
    assert fused < np.median(per_scan)


@pytest.mark.parametrize("solver", [N.SOLVER_REFERENCE_LOCAL, N.SOLVER_GRID])
def test_committed_oracle_corners_are_the_oracle_s(golden_dir, solver):
    """tests/golden/sequence_pose0_oracle.npz spares the GPU tests the oracle's twelve CPU solves per solver mode."""
    corners, accepted = K.golden_oracle_sequence(golden_dir, solver)
    want_corners, want_accepted, _, _ = K.oracle_sequence(0, solver)
    assert list(accepted) == list(want_accepted)
    assert corners.dtype == np.float32 and np.abs(corners - want_corners).max() <= 1e-6


# ---- the K0b batches of hundreds of messages: each is what tests/test_sequence.py takes it for ------------------------------------

def test_unpack_batches_have_the_entry_counts_and_tile_patterns_they_are_named_for():
    seen = {c: set() for c in range(K.UNPACK_CLASSES)}
    patterns = set()
    plan_bytes = set()
    for name, spec in K.UNPACK_BATCHES.items():
        batch = K.unpack_batch(name)
        table, offsets = K.unpack_table(batch)
        points = np.diff(offsets)
        assert 300 <= len(batch) <= 1100 and 150_000 <= offsets[-1] <= 340_000, (name, len(batch), offsets[-1])
        assert set(points) <= set(K.UNPACK_COUNTS) | {K.UNPACK_BIG}
        assert len({id(m) for m, _ in batch}) <= 8 * len(K.UNPACK_COUNTS)                # a pool of few distinct members
        plan_bytes.add(len(batch) * K.UNPACK_ARGS_BYTES % 256 == 0)
        assert points[0] == 0 and points[-1] == 0 and (points == 0).sum() >= len(batch) // 8
        for c, (rows, n, first, tiles) in enumerate(table):
            pattern, entries = spec.get(c, (None, 0))
            assert len(rows) == entries, (name, c)
            if not entries:
                continue
            seen[c].add(entries)
            patterns.add(pattern)
            tiles_of = -(-n // K.tile_points(c))
            assert first[0] == 0 and np.array_equal(first[1:], np.cumsum(tiles_of)[:-1]) and tiles == tiles_of.sum()
            assert (rows != np.arange(entries)).all()                                     # no message's row is its entry index
            if entries > 3:
                assert (np.diff(rows) > 1).any() and (points[rows[0]:rows[-1]] == 0).any()   # other classes' and empty messages in between
            if pattern == "one_tile":
                assert (tiles_of == 1).all() and np.array_equal(first, np.arange(entries))
            elif pattern == "several":
                assert (tiles_of > 1).all()
            elif pattern == "last_several":
                assert (tiles_of[:-1] == 1).all() and tiles_of[-1] > 1 and tiles > first[-1] + 1
            elif pattern == "big_first":
                assert tiles_of[0] == 201 and (tiles_of[1:] == 1).all() and first[1] == 201
            else:
                assert pattern == "mixed"
        if name == "f":
            assert [len(t[0]) > 0 for t in table] == [True, True, False, True, True]     # an absent class between two populated ones
    for c in range(K.UNPACK_CLASSES):
        assert seen[c] >= set(K.ENTRY_COUNTS), (c, seen[c])                               # every kernel: 1, 2, 3, 2^8 and 2^8 + 1 entries
    assert patterns == {"one_tile", "several", "mixed", "last_several", "big_first"}
    assert plan_bytes == {True, False}               # tables whose UnpackArgs part is and is not a multiple of 256 bytes
    assert len(K.unpack_batch(K.UNPACK_PADDED_TO_32)) % 32 == 0


def test_restated_layout_class_is_the_pool_s():
    for layout, (c, step, _, height, _, align) in K.UNPACK_LAYOUTS.items():
        n = 1024
        assert K.unpack_class(K.unpack_member(layout, n), align) == (c, n), layout
        assert ingest.parse_pointcloud2(K.unpack_member(layout, n)).point_step == step
    assert K.unpack_class(K.unpack_member("velo", 1024), 4) == (0, 1024)                 # the source's alignment decides too
    assert sorted({lay[0] for lay in K.UNPACK_LAYOUTS.values()}) == list(range(K.UNPACK_CLASSES))


@pytest.mark.parametrize("name", list(K.UNPACK_BATCHES))
def test_unpack_batches_tell_the_wrong_entry_searches_from_the_right_one(name):
    """The map workgroup -> (entry, tile) as a numpy model, with find_entry's rule and with three wrong ones: on every batch each
    wrong rule leaves other bytes in the output than the right one, which leaves the numpy unpack."""
    batch = K.unpack_batch(name)
    unpacked = {m: R.unpack(m) for m in dict.fromkeys(m for m, _ in batch)}              # the distinct members, once each
    whole = np.concatenate([unpacked[m] for m, _ in batch])
    right, src = K.unpack_model(batch, whole, "right")
    assert right.tobytes() == whole.tobytes() and np.array_equal(src, np.arange(len(whole)))
    for rule in K.FIND_ENTRY_RULES[1:]:
        wrong, _ = K.unpack_model(batch, whole, rule)
        assert wrong.tobytes() != right.tobytes(), rule
    # ... and every class with two entries or more does so by itself
    table, _ = K.unpack_table(batch)
    for c, (rows, n, first, tiles) in enumerate(table):
        w = np.arange(tiles)
        for rule in K.FIND_ENTRY_RULES[1:]:
            assert len(rows) < 2 or not np.array_equal(K.find_entry(first, w, rule), K.find_entry(first, w)), (c, rule)
        if len(rows):
            assert np.array_equal(K.find_entry(first, w), np.searchsorted(first, w, side="right") - 1)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program: tests/sequence_host_check.cpp + csrc/sequence_host.cpp only, under ASan and UBSan."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("sequence_host_check")
    exe = str(out / "sequence_host_check")
    csrc = os.path.join(ROOT, "lidar_camera_calibration_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sequence_host_check.cpp"),
                    os.path.join(csrc, "sequence_host.cpp"), "-o", exe], check=True, timeout=300)
    return exe, out


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).reshape(-1))


def test_fusion_under_sanitizers_equals_the_restatement(host_check):
    """Every constructed case with the restatement's answer beside it; the program compares and exits non-zero on a mismatch."""
    exe, out = host_check
    src = str(out / "cases.txt")
    with open(src, "w") as fh:
        fh.write("%d\n" % len(CASES))
        for name, corners, accepted, a, b, gate in CASES:
            w = R.fuse(corners, accepted, a, b, gate)
            fh.write("%s %d %d %d %s\n" % (name, len(accepted), a, b, float(gate).hex()))
            fh.write(" ".join(str(int(v)) for v in accepted) + "\n")
            fh.write(" ".join("nan" if np.isnan(v) else float(v).hex() for v in corners.reshape(-1).astype(np.float64)) + "\n")
            fh.write("%d %d %d %d %d %s %s\n" % (w.status, w.n_ok, w.n_used, w.ref_scan, w.n_corners, float(w.spread_max).hex(), float(w.spread_rms).hex()))
            fh.write(" ".join(str(int(v)) for v in w.used) + "\n")
            fh.write(_hex(w.corners) + "\n")
    r = subprocess.run([exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "cases %d ok" % len(CASES) in r.stdout
    # and it does notice a mismatch: one expected coordinate moved by one fp32 ulp
    text = open(src).read().split("\n")
    k = 1 + 6 * 0 + 5
    vals = text[k].split()
    vals[0] = float(np.nextafter(np.float32(float.fromhex(vals[0])), np.float32(np.inf))).hex()
    text[k] = " ".join(vals)
    open(str(out / "wrong.txt"), "w").write("\n".join(text))
    r = subprocess.run([exe, str(out / "wrong.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "mismatch" in r.stdout
