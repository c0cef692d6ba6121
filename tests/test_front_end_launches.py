"""The front end's two large-batch paths against what small batches run: K3 -> K4/K5 -> K5w as ONE launch (k345_front_end,
batches above 64 frames) and the ROI crop in ONE pass (k1_roi_crop_frame, batches of 512 frames and more).  Almost every other
test runs batches of <= 64 frames, i.e. the separate launches; these run the new kernels, against the oracle and against a handle
that `debug_separate_launches(True)` keeps on the separate launches at any batch size."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

from lidar_camera_calibration_amd import LidarCornersBatch, synth
from lidar_camera_calibration_amd import _native as N

pytestmark = pytest.mark.gpu

SOLVED = (N.OK, N.AMBIGUOUS)
# how many candidates the full pass LISTED as near ties depends on how far the frame's bound had come down when each completed
# (test_fused_locate_equals_the_three_launches): a superset of the true near ties either way, re-ranked exactly by K7r
TIMING_DEPENDENT_FIELDS = ("grid_ties",)


class _CachedOracle:
    """The oracle module with extract / roi_crop / cluster remembered per (cloud, click): a tiled batch repeats its frames."""

    def __init__(self, ob):
        self._ob = ob
        self._memo = {}

    def __getattr__(self, name):
        return getattr(self._ob, name)

    def _cached(self, name, cloud, click, *args, **kw):
        key = (name, hashlib.sha1(np.ascontiguousarray(cloud).tobytes()).hexdigest(), np.asarray(click).tobytes(),
               tuple(sorted(kw.items())))
        if key not in self._memo:
            self._memo[key] = getattr(self._ob, name)(cloud, click, *args, **kw)
        return self._memo[key]

    def extract(self, cloud, click, op, **kw):
        return self._cached("extract", cloud, click, op, **kw)

    def roi_crop(self, cloud, click, op):
        return self._cached("roi_crop", cloud, click, op)

    def cluster(self, cloud, click, op):
        return self._cached("cluster", cloud, click, op)


@pytest.mark.parametrize("solver", [N.SOLVER_GRID, N.SOLVER_REFERENCE_LOCAL])
def test_one_launch_front_end_matches_the_oracle(ob, solver):
    """The 16 frames of test_every_stage_matches_the_oracle, tiled 5 x into one 80-frame batch (above kSmallBatchFrames: K3, K4/K5 and
    K5w run as one launch), stage by stage against the oracle with that test's own comparisons."""
    from test_gpu_parity import _assert_every_stage, _oparams
    c1, k1, _, _ = synth.make_batch(6, fixture_poses=True)
    c2, k2, _, _ = synth.make_batch(10, seed=4242, range_m=(2.0, 3.0))
    clouds, clicks = np.tile(np.concatenate([c1, c2]), (5, 1, 1)), np.tile(np.concatenate([k1, k2]), (5, 1))
    p = N.default_params()
    p.solver = solver
    est = LidarCornersBatch(len(clicks), clouds.shape[1], p)
    try:
        n_solved = _assert_every_stage(_CachedOracle(ob), est, clouds, clicks, p, _oparams(ob, solver), solver)
    finally:
        est.close()
    assert n_solved >= 5 * 6   # the fixture poses at the least


def _fields(r):
    """Every field of the record as its bytes (the corners: those the frame has), but the timing-dependent ones."""
    raw = bytes(r)
    out = {}
    for name, _ in N.Result._fields_:
        d = getattr(N.Result, name)
        if name == "corners":
            out[name] = raw[d.offset:d.offset + 12 * r.n_corners]
        elif name not in TIMING_DEPENDENT_FIELDS:
            out[name] = raw[d.offset:d.offset + d.size]
    return out


def _status(x):
    return int(np.frombuffer(x["result"]["status"], np.int32)[0])


def _everything(est, res, f, walk):
    """Every output of frame f of the handle's last batch, as comparable values."""
    r = res[f]
    out = {"result": _fields(r)}
    for which in (N.CLOUD_ROI, N.CLOUD_CLUSTER, N.CLOUD_CHESSBOARD, N.CLOUD_PCA):
        out["cloud%d" % which] = est.fetch_cloud(f, which).tobytes()
    yz, lab = est.fetch_labelled(f)
    out["labelled"] = (yz.tobytes(), lab.tobytes())
    out["classes"] = est.fetch_classes(f).tobytes()
    if walk and r.status in SOLVED:   # (a frame that left the chain has no walk layout; its counters are whatever the slot held)
        wyz, wlab, n_in, n_rim = est.fetch_walk(f)
        out["walk"] = (wyz.tobytes(), wlab.tobytes(), int(n_in), int(n_rim))
    return out


def _run_both(clouds, clicks, offsets=None, solver=N.SOLVER_GRID, max_points=None):
    """The same batch on a default handle and on one kept on the separate launches: per frame, everything each produced.
    (max_points: of the longest frame, for batches given with offsets.)"""
    out = []
    for separate in (False, True):
        p = N.default_params()
        p.solver = solver
        est = LidarCornersBatch(len(clicks), max_points or clouds.shape[1], p)
        try:
            est.reserve(2048, 4096)
            est.debug_separate_launches(separate)
            res = est.extract(clouds, clicks, offsets)
            out.append([_everything(est, res, f, solver == N.SOLVER_GRID) for f in range(len(clicks))])
        finally:
            est.close()
    return out


def _assert_same(new, old):
    assert len(new) == len(old)
    for f, (a, b) in enumerate(zip(new, old)):
        assert a.keys() == b.keys(), f
        for k in a:
            assert a[k] == b[k], (f, k)


@pytest.fixture(scope="module")
def tiled_512():
    clouds, clicks, _, _ = synth.make_batch(64, seed=0xF05ED)
    return _run_both(np.tile(clouds, (8, 1, 1)), np.tile(clicks, (8, 1)))


def test_one_pass_crop_and_one_launch_equal_the_separate_launches(tiled_512):
    """make_batch(64, seed=0xF05ED) tiled to 512 frames (one-pass crop and one-launch front end both active) against the same batch on
    the separate launches: every fetched cloud, the labelled points, the classes and every result field identical (but the listed
    near-tie count, timing-dependent by design), and at least 55 of each 64 distinct frames solved."""
    new, old = tiled_512
    _assert_same(new, old)
    for t in range(8):
        assert sum(_status(new[64 * t + k]) in SOLVED for k in range(64)) >= 55, t
    for f in range(64, 512):   # a tile is a tile
        assert new[f] == new[f % 64], f


def test_one_launch_walk_layout_equals_k5w(tiled_512):
    """The walk layout the one launch writes (the laid-out points and labels, n_in, n_rim) is K5w's, frame by frame."""
    new, old = tiled_512
    n = 0
    for f, (a, b) in enumerate(zip(new, old)):
        assert ("walk" in a) == ("walk" in b), f
        if "walk" in a:
            assert a["walk"] == b["walk"], f
            assert a["walk"][2] + a["walk"][3] <= len(a["walk"][1]) == len(a["labelled"][1]), f
            n += 1
    assert n >= 8 * 55


def _near(cloud, click, n):
    """The n points of the cloud nearest the click, in input order."""
    d = np.linalg.norm(cloud[:, :3] - click[None, :], axis=1)
    return np.ascontiguousarray(cloud[np.sort(np.argsort(d, kind="stable")[:n])])


def _special_frames():
    """(name, cloud, click, the status the oracle gives it) of frames that leave the chain early or take a fallback."""
    good, clicks, _, _ = synth.make_batch(8, seed=0x5EC1A1, range_m=(2.0, 3.0))
    c0, k0 = good[0], clicks[0]
    p = N.default_params()
    out = [("click far from every point", c0, k0 + np.float32(100.0), N.NO_ROI_POINTS),
           ("all-NaN cloud", np.full_like(c0, np.nan), k0, N.NO_ROI_POINTS)]
    out.append(("cluster below cluster_min", _near(c0, k0, max(3, p.cluster_min // 2)), k0, N.NO_CLUSTER))
    # every sample of three is collinear (exactly: y, z constant): no hypothesis, no inliers
    line = np.zeros((max(150, p.cluster_min + 50), 4), np.float32)
    line[:, 0] = k0[0] + (np.arange(len(line), dtype=np.float32) - len(line) // 2) * np.float32(0.004)
    line[:, 1], line[:, 2], line[:, 3] = k0[1], k0[2], 50.0
    out.append(("fewer than three inliers", line, k0, N.NO_PLANE))
    flat = c0.copy()
    flat[:, 3] = 37.0
    out.append(("flat-intensity board", flat, k0, N.DEGENERATE_HIST))
    # twice the points, the copy 0.5 mm beside the original: a cluster above K3's LDS staging (2048 points) -- every stage of the
    # one launch on its global-memory path
    half = _near(c0, k0, len(c0) // 2)
    twin = half.copy()
    twin[:, 0] += np.float32(0.0005)
    out.append(("cluster above the LDS staging", np.concatenate([half, twin]), k0, N.OK))
    for n in (0, 1, 4095, 4096, 4097, 5000):   # ragged lengths: none, one, around a 4096-point chunk, not a multiple of 256
        out.append(("%d points" % n, _near(good[1], clicks[1], n), clicks[1], N.NO_ROI_POINTS if n == 0 else N.NO_CLUSTER if n == 1 else N.OK))
    return good, clicks, out


def test_early_exits_and_fallbacks_in_a_large_batch():
    """Frames that leave the chain early, between good ones, in one ragged 512-frame batch: statuses, counts and every cloud as the
    separate launches give them -- the neighbours' included."""
    good, clicks, special = _special_frames()
    frames, cl, names = [], [], []
    k = 0
    while len(frames) < 512:   # good, special, good, special, ...
        frames.append(good[len(frames) % len(good)])
        cl.append(clicks[(len(frames) - 1) % len(good)])
        names.append(None)
        name, c, kk, _ = special[k % len(special)]
        frames.append(c)
        cl.append(kk)
        names.append(name)
        k += 1
    frames, cl, names = frames[:512], cl[:512], names[:512]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in frames])]).astype(np.uint64)
    flat = np.ascontiguousarray(np.concatenate([c.reshape(-1, 4) for c in frames]), dtype=np.float32)
    new, old = _run_both(flat, np.asarray(cl, np.float32), offsets, max_points=max(len(c) for c in frames))
    _assert_same(new, old)
    expected = {name: st for name, _, _, st in special}
    for f, name in enumerate(names):
        if name is None:
            assert _status(new[f]) == N.OK, f             # (all eight are, by the oracle)
            assert new[f] == new[f % (2 * len(good))], f   # a good frame is what it is wherever it stands
        else:
            assert _status(new[f]) == expected[name], (f, name, _status(new[f]))
        assert int(np.frombuffer(new[f]["result"]["n_points"], np.int32)[0]) == len(frames[f]), f
    big = names.index("cluster above the LDS staging")
    assert int(np.frombuffer(new[big]["result"]["n_cluster"], np.int32)[0]) > 2048
