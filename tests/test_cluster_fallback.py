"""K2's fallback launch: k2_seeded_cluster keeps the LDS-grid path and LISTS the frames that path cannot hold;
k2_fallback_cluster, launched behind it, clusters the listed frames on hashed cells or on points.

What the paths compute is held to the oracle by tests/test_cluster_constructed.py, whose constructed sets, oracle bookkeeping
and frame check this file reuses.  This file is about the hand-over: which frames are listed, how many (the count comes back
with the batch's counters: debug_cluster_launch()["fallback_frames"]), the fixed grid of the fallback launch walking a list
shorter than, as long as and longer than itself (G = debug_cluster_launch()["fallback_grid"]), the list of a slot's earlier
batch, and frames that left the chain before K2.

Every batch but those of the last test has more than 64 frames (K2 and its fallback at 256 threads); the frames hold 268
input points (18 where a frame is meant for the point-level search: fewer than 256 input points).  Every comparison is
`==`, against the oracle and against the construction.
"""
import functools

import numpy as np
import pytest

import constructed_clusters as cc
import test_cluster_constructed as tcc

HALF = 8.0              # roi_half of the wide sets: one box for every frame of a batch
FAR = 100.0             # a click this far (per axis) from the cloud crops nothing


# ------------------------------------------------------------------------------------------------------------------ the sets
@functools.lru_cache(maxsize=None)
def _grid_frames():
    """124 compact link probes plus a sheet of points over 12 x 12 cells, as many input points as a wide frame: the padded
    bounding grid fits the bitmap and ~150 cells are occupied -- fine_cluster_frame<true>"""
    core = cc.subset(tcc._core("compact"), np.arange(124))
    n_extra = tcc._frames("wide")["clouds"].shape[1] - core["xyz"].shape[1]
    clouds, lab = cc.assemble(core, seed=12, extra=cc.sheet(core, n_extra, 12, seed=121))
    return dict(clouds=clouds, lab=lab, linked=core["linked"], click=core["click"], point=core["point"], tol=core["tol"],
                roi_half=HALF, core=core)


def _set(name):
    return _grid_frames() if name == "grid" else tcc._frames(name)


_GRID_ORACLE = []


def _want(ob, name):
    """per frame (status, n_roi, n_cluster, ROI cloud, cluster cloud) of the oracle, computed once per set"""
    if name != "grid":
        return tcc._oracle(ob, name)
    if not _GRID_ORACLE:
        fr = _grid_frames()
        op = tcc._oparams(ob, fr)
        for f, cloud in enumerate(fr["clouds"]):
            o = ob.extract(cloud, fr["click"][f], op)
            roi = cloud[ob.roi_crop(cloud, fr["click"][f], op)]
            idx, _ = ob.cluster(roi, fr["click"][f], op)
            _GRID_ORACLE.append((o.status, o.n_roi, o.n_cluster, roi, roi[idx]))
    return _GRID_ORACLE


def test_every_set_takes_the_path_it_is_meant_for(ob):
    """grid: the LDS grid; wide: hashed cells; wide_tiny: the point-level search -- under one box and one tolerance, at one
    input size (wide_tiny: below the hashed path's 256 input points).  The oracle returns the construction's cluster on the
    grid set (on the others: tests/test_cluster_constructed.py)."""
    grid, wide, tiny = _set("grid"), _set("wide"), _set("wide_tiny")
    assert tcc._paths(grid) == {"fine_lds"} and tcc._paths(wide, range(0, 1984, 61)) == {"hashed"} and tcc._paths(tiny) == {"point"}
    assert grid["clouds"].shape[1] == wide["clouds"].shape[1] == 268 and tiny["clouds"].shape[1] < cc.HASH_MIN_FRAME_POINTS
    assert grid["roi_half"] == wide["roi_half"] == tiny["roi_half"] == HALF and grid["tol"] == wide["tol"] == tiny["tol"]
    for f, (status, n_roi, n_cluster, roi, clu) in enumerate(_want(ob, "grid")):
        roi_e, clu_e = cc.expected(grid["clouds"], grid["lab"], grid["linked"], f)
        assert np.array_equal(roi, roi_e) and np.array_equal(clu, clu_e), f
        assert n_roi == 268 and n_cluster == len(clu_e)
    # a click FAR away crops nothing, whatever the cloud
    for fr in (grid, wide):
        cloud = fr["clouds"][3]
        assert not cc.crop_mask(cloud, fr["click"][3] + np.float32(FAR), (HALF,) * 3).any()


# ------------------------------------------------------------------------------------------------------------------ batches
def _batch(items):
    """items: (set name, frame, far) per frame -> flat clouds, offsets, clicks"""
    clouds = [_set(name)["clouds"][f] for name, f, _ in items]
    clicks = np.stack([_set(name)["click"][f] + np.float32(FAR if far else 0.0) for name, f, far in items])
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    return np.ascontiguousarray(np.concatenate(clouds)), offsets, clicks


def _expected_fallback(items):
    return sum(1 for name, _, far in items if name != "grid" and not far)


def _check(ob, e, res, items, threads=256):
    """every frame of a finished batch: a far click leaves ILCC_NO_ROI_POINTS and nothing else; every other frame is the
    oracle's and the construction's (tcc._check_batch); the batch's fallback count is the number of wide and tiny frames"""
    from lidar_camera_calibration_amd import _native as N
    for k, (name, f, far) in enumerate(items):
        if far:
            r = res[k]
            assert (r.status, r.n_roi, r.n_cluster, r.n_points) == (N.NO_ROI_POINTS, 0, 0, len(_set(name)["clouds"][f])), (k, name, f, r.status)
            assert len(e.fetch_cloud(k, N.CLOUD_ROI)) == 0
    for name in ("grid", "wide", "wide_tiny"):
        ks = [k for k, (n, _, far) in enumerate(items) if n == name and not far]
        if ks:
            tcc._check_batch(_Picked(e, ks), [res[k] for k in ks], _set(name), _want(ob, name), [items[k][1] for k in ks], name)
    used = e.debug_cluster_launch()
    assert used["threads"] == threads and used["fallback_frames"] == _expected_fallback(items), (used, _expected_fallback(items))


class _Picked:
    """fetch_cloud of a handle, indexed by position in a selection of the batch's frames"""

    def __init__(self, e, ks):
        self._e, self._ks = e, ks

    def fetch_cloud(self, k, which):
        return self._e.fetch_cloud(int(self._ks[k]), which)


def _params():
    return tcc._nparams(_set("wide"))


@pytest.fixture(scope="module")
def fallback_grid():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, 16, _params())
    try:
        g = e.debug_cluster_launch()["fallback_grid"]
    finally:
        e.close()
    assert 1 <= g <= 1984 - 64          # (the wide set has the frames for every boundary case)
    return g


@pytest.fixture(scope="module")
def big_handle(fallback_grid):
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(fallback_grid + 1 + 70, 268, _params())
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
def test_mixed_batch_lists_the_wide_and_the_tiny_frames(ob):
    """LDS-grid frames, wide frames (hashed cells) and frames of fewer than 256 input points (point level), interleaved in one
    ragged batch of 144: every frame's cluster is the oracle's, and 96 frames went through the fallback launch"""
    from lidar_camera_calibration_amd import LidarCornersBatch
    items = []
    for j in range(48):
        items += [("grid", 2 * j, False), ("wide", 41 * j + 7, False), ("wide_tiny", 2 * j + 1, False)]
    assert _expected_fallback(items) == 96 and cc.k2_threads(len(items)) == 256
    flat, offsets, clicks = _batch(items)
    e = LidarCornersBatch(len(items), 268, _params())
    try:
        assert e.debug_cluster_launch()["fallback_frames"] == 0
        _check(ob, e, e.extract(flat, clicks, offsets=offsets), items)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["0", "1", "G", "G+1", "all"])
def test_fallback_count_around_the_grid_size(ob, big_handle, fallback_grid, case):
    """The fallback launch is a fixed grid of at most G workgroups; workgroup b takes items b, b + G, ... of the list.  Lists
    of 0, 1, G and G + 1 frames among 70 LDS-grid frames, and a batch of G + 37 frames that are all listed."""
    G = fallback_grid
    n_wide = {"0": 0, "1": 1, "G": G, "G+1": G + 1, "all": G + 37}[case]
    n_grid = 0 if case == "all" else 70
    # the grid frames spread evenly among the wide ones
    at = set(np.linspace(0, n_wide + n_grid - 1, n_grid).astype(int).tolist()) if n_grid else set()
    assert len(at) == n_grid
    items, w, g = [], 0, 0
    for k in range(n_wide + n_grid):
        if k in at:
            items.append(("grid", (5 * g) % 124, False))
            g += 1
        else:
            items.append(("wide", (1984 - 1 - w) if case == "G+1" else w, False))
            w += 1
    assert _expected_fallback(items) == n_wide and cc.k2_threads(len(items)) == 256
    flat, offsets, clicks = _batch(items)
    _check(ob, big_handle, big_handle.extract(flat, clicks, offsets=offsets), items)


@pytest.mark.gpu
def test_a_slots_next_batch_does_not_see_the_list_of_its_last(ob):
    """Twelve batches of 96 frames through the four slots of one handle, four in flight at a time, so that every slot runs three
    batches: with, without and again with fallback frames (or the other way round).  A batch with them lists its 48 wide frames
    (odd positions); a batch without reports 0 -- and at the odd positions, where its slot's list still names frames of the
    batch before, it has frames that left the chain in K1 (a far click): clustered from a stale list they would not keep
    ILCC_NO_ROI_POINTS."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    n, slots = 96, 4
    plans = []
    for b in range(12):
        with_fallback = (b + b // slots) % 2 == 0
        items = []
        for j in range(n):
            if j % 2 == 0:
                items.append(("grid", (j // 2 + 7 * b) % 124, False))
            elif with_fallback:
                items.append(("wide", 48 * b + j // 2, False))
            else:
                items.append(("grid", (j // 2 + 7 * b + 62) % 124, True))
        plans.append(items)
    per_slot = [[_expected_fallback(plans[b]) for b in range(s, 12, slots)] for s in range(slots)]
    assert per_slot == [[48, 0, 48], [0, 48, 0], [48, 0, 48], [0, 48, 0]]
    e = LidarCornersBatch(n, 268, _params())
    try:
        for first in range(0, 12, slots):
            held = []
            for b in range(first, first + slots):
                flat, _, clicks = _batch(plans[b])
                clicks = np.ascontiguousarray(clicks, np.float32)
                held.append((e.submit_host(flat.ctypes.data, n, 268, clicks.ctypes.data), flat, clicks, plans[b]))
            for ticket, _, _, items in held:
                _check(ob, e, e.wait(ticket), items)
    finally:
        e.close()


@pytest.mark.gpu
def test_frames_that_left_the_chain_in_k1_are_not_listed(ob):
    """A click far from every point: ILCC_NO_ROI_POINTS.  32 such frames among 64 wide and tiny ones: they keep their status,
    and the fallback count is 64."""
    items = []
    for j in range(32):
        items += [("wide", 59 * j + 3, False), ("wide" if j % 2 else "wide_tiny", 3 * j + 1, True), ("wide_tiny", 3 * j, False)]
    assert _expected_fallback(items) == 64 and cc.k2_threads(len(items)) == 256
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    flat, offsets, clicks = _batch(items)
    op = tcc._oparams(ob, _set("wide"))
    for k in (1, 4):                     # (one tiny and one wide cloud: the oracle's status for a far click)
        name, f, far = items[k]
        assert far and ob.extract(_set(name)["clouds"][f], clicks[k], op).status == N.NO_ROI_POINTS
    e = LidarCornersBatch(len(items), 268, _params())
    try:
        _check(ob, e, e.extract(flat, clicks, offsets=offsets), items)
    finally:
        e.close()


@pytest.mark.gpu
def test_small_batches_at_1024_threads(ob):
    """Batches of at most 64 frames run K2 at 1024 threads, and behind it the fallback's one-item kernel
    (k2_fallback_cluster_wide: a workgroup per frame of the batch, no loop, so no grid boundary to cross): a mixed batch of 63,
    64 frames that are all listed, none listed, one listed."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    mixed = []
    for j in range(21):
        mixed += [("grid", 3 * j, False), ("wide", 83 * j + 11, False), ("wide_tiny", 5 * j + 2, False)]
    batches = [mixed, [("wide", 29 * j + 1, False) for j in range(64)], [("grid", j, False) for j in range(64)],
               [("wide", 1500, False) if j == 40 else ("grid", j + 60, False) for j in range(64)]]
    assert [_expected_fallback(b) for b in batches] == [42, 64, 0, 1]
    e = LidarCornersBatch(64, 268, _params())
    try:
        for items in batches:
            assert cc.k2_threads(len(items)) == 1024
            flat, offsets, clicks = _batch(items)
            _check(ob, e, e.extract(flat, clicks, offsets=offsets), items, threads=1024)
    finally:
        e.close()
