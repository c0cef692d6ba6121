"""K2 (seeded clustering) and K1 (ROI crop) on CONSTRUCTED inputs (tests/constructed_clusters.py).

K2 is five algorithms that must return the same cluster -- fine_cluster_frame<true> / <false>, hashed_cluster_frame, the k2h_*
chain, point_level_cluster_frame, at 1024 or 256 threads -- and the rest of the suite holds all but one of them to the oracle on
synthetic lidar clouds, whose components hang together through many redundant pairs: a missed or invented link does not show.
Here every frame is a LINK PROBE: two arms joined by at most one point pair, in cells at a chosen offset (all 62 unordered
offsets of the 5 x 5 x 5 neighbourhood) and at a chosen position inside the 4 x 4 x 4 block of the hashed paths, at
tol (1 -+ 1e-4) -- or exactly AT a tolerance that float32 represents, on a lattice where the arithmetic is exact.  The expected
cluster is known from the construction.  Each set goes through every path; each test asserts, from a numpy restatement of the
dispatch (k2_seeded_cluster, fine_cluster_frame, hash_setup, launch_cluster), that its frames take the path it is about.

Every GPU comparison is `==`: counts and status against the oracle, the ROI and cluster clouds against the generator's
expectation AND against the oracle's BFS.  The CPU tests (no marker) check that the inputs are what the GPU tests take them for.

K1: points on the inclusive limits and their float neighbours, non-finite points, -0.0 against a limit of 0, frame lengths around
the chunk sizes of both crop kernels, survivor patterns per wavefront load, and non-finite boxes (crop_frame<false>), through the
one-pass crop and through count + scatter, against a numpy mask of float32 comparisons and against the oracle.
"""
import functools

import numpy as np
import pytest

import constructed_clusters as cc

TOL_ROI = 0.12          # cluster_tol of EuclideanCluster()
TOL_ONLINE = 0.10       # online_cluster_tol of get_chessboard_by_point
CLUSTER_MIN = 4
N_PLAN = 62 * 16 * 2    # every offset x every block position x {linked, unlinked}


# ------------------------------------------------------------------------------------------------------------------ the sets
@functools.lru_cache(maxsize=None)
def _core(kind):
    if kind == "compact":                  # 62 x 2 x 2 seeds, any block position
        core = cc.link_probes(*cc.probe_plan(0, seeds=2), TOL_ROI, seed=101)
        cc.assert_complete(core, 0)
    elif kind == "wide":                   # 62 x 16 x 2, anchors 128 cells apart
        core = cc.link_probes(*cc.probe_plan(16), TOL_ROI, seed=202, base_cell=64, far_cells=128)
        cc.assert_complete(core, 16)
    elif kind == "wide_online":
        core = cc.link_probes(*cc.probe_plan(16), TOL_ONLINE, seed=303, base_cell=64, far_cells=128)
        cc.assert_complete(core, 16)
    elif kind == "ties":
        core = cc.tie_probes(seed=404)
    elif kind == "ties_wide":
        core = cc.tie_probes(seed=505, wide=True)
    assert core.get("draws", 0) <= 400 * 64
    return core


_FIRST_POSITION = np.arange(N_PLAN).reshape(62, 16, 2)[:, 0, :].reshape(-1)      # 62 x 2: block position (0, 0, 0)


def _small_search(p):
    """a 9 x 8 x 8 search grid: the frames that reach the back end (a cluster of 7 or 16 points passes for a plane) leave it soon"""
    p.n_th, p.n_ty, p.n_tz = 9, 8, 8
    p.th_min, p.th_step = -0.04, 0.01
    p.ty_min = p.tz_min = -0.04
    p.ty_step = p.tz_step = 0.01
    return p


@functools.lru_cache(maxsize=None)
def _frames(name):
    """-> dict(clouds [F, N, 4], lab, linked, click, point, tol, roi_half)"""
    if name == "compact":
        core = _core("compact")
        clouds, lab = cc.assemble(core, seed=1)
        half = 2.5
    elif name == "hbm":                    # + 4 200 points over 400 cells: > 4 096 ROI points, < 512 occupied cells
        core = cc.subset(_core("compact"), np.arange(124))
        clouds, lab = cc.assemble(core, seed=2, extra=cc.sheet(core, 4200, 20, seed=21))
        half = 2.5
    elif name == "sheet_small":            # + 2 500 points over ~750 cells: hashed on a fresh handle, fine<true> on the next call
        core = cc.subset(_core("compact"), np.arange(124))
        clouds, lab = cc.assemble(core, seed=3, extra=cc.sheet(core, 2500, 28, seed=31))
        half = 2.5
    elif name == "sheet_large":            # + 4 200: hashed on a fresh handle, fine<false> on the next call
        core = cc.subset(_core("compact"), np.arange(124))
        clouds, lab = cc.assemble(core, seed=4, extra=cc.sheet(core, 4200, 28, seed=41))
        half = 2.5
    elif name == "wide":                   # >= 256 input points: non-finite ones and ones outside the ROI count
        core = _core("wide")
        clouds, lab = cc.assemble(core, seed=5, n_nan=150, n_outside=100)
        half = 8.0
    elif name == "wide_tiny":              # the same probes, < 256 input points
        core = cc.subset(_core("wide"), _FIRST_POSITION)
        clouds, lab = cc.assemble(core, seed=6)
        half = 8.0
    elif name == "online":
        core = _core("wide_online")
        clouds, lab = cc.assemble(core, seed=7, n_nan=250)
        half = None
    elif name == "online_tiny":
        core = cc.subset(_core("wide_online"), _FIRST_POSITION)
        clouds, lab = cc.assemble(core, seed=8, n_nan=37)
        half = None
    elif name == "ties":
        core = _core("ties")
        clouds, lab = cc.assemble(core, seed=9)
        half = 2.5
    elif name == "ties_wide":
        core = _core("ties_wide")
        clouds, lab = cc.assemble(core, seed=10, n_nan=200, n_outside=50)
        half = 8.0
    elif name == "ties_online":
        core = _core("ties_wide")
        clouds, lab = cc.assemble(core, seed=11, n_nan=250)
        half = None
    return dict(clouds=clouds, lab=lab, linked=core["linked"], click=core["click"], point=core["point"], tol=core["tol"],
                roi_half=half, core=core)


def _oparams(ob, fr):
    op = _small_search(ob.default_params())
    op.solver = ob.SOLVER_GRID
    op.cluster_tol = fr["tol"]
    op.cluster_min = CLUSTER_MIN
    if fr["roi_half"] is not None:
        for a in range(3):
            op.roi_half[a] = fr["roi_half"]
    return op


def _nparams(fr):
    from lidar_camera_calibration_amd import _native as N
    p = _small_search(N.default_params())
    p.cluster_tol = p.online_cluster_tol = fr["tol"]
    p.cluster_min = CLUSTER_MIN
    if fr["roi_half"] is not None:
        for a in range(3):
            p.roi_half[a] = fr["roi_half"]
    return p


_ORACLE = {}


def _oracle(ob, name):
    """per frame (status, n_roi, n_cluster, ROI cloud, cluster cloud) of the oracle: computed once per set, never changed"""
    if name not in _ORACLE:
        fr = _frames(name)
        op = _oparams(ob, fr)
        out = []
        for f, cloud in enumerate(fr["clouds"]):
            if fr["roi_half"] is None:
                o = ob.chessboard_by_point(cloud, fr["point"][f], op)[0]
                roi = cloud[np.isfinite(cloud[:, :3]).all(1)]
                seed = fr["point"][f]
            else:
                o = ob.extract(cloud, fr["click"][f], op)
                roi = cloud[ob.roi_crop(cloud, fr["click"][f], op)]
                seed = fr["click"][f]
            idx, _ = ob.cluster(roi, seed, op)
            out.append((o.status, o.n_roi, o.n_cluster, roi, roi[idx]))
        _ORACLE[name] = out
    return _ORACLE[name]


def _roi_xyz(fr, f):
    return fr["clouds"][f][fr["lab"][f] >= 0][:, :3]


def _paths(fr, frames=None):
    n_in = fr["clouds"].shape[1]
    return {cc.k2_path(n_in, _roi_xyz(fr, f), fr["tol"]) for f in (range(len(fr["clouds"])) if frames is None else frames)}


# ------------------------------------------------------------------------------------------------------------------ CPU tests
_PROBE_SETS = ("compact", "hbm", "sheet_small", "sheet_large", "wide", "wide_tiny", "online", "online_tiny")
_TIE_SETS = ("ties", "ties_wide", "ties_online")


@pytest.mark.parametrize("kind", ["compact", "wide", "wide_online"])
def test_probes_hang_on_one_pair_in_the_intended_cells(kind):
    """Among all A x B pairs the float32 unfused d2 < tol2 holds for (p, q) alone when the probe is linked and for no pair when it
    is not; p's and q's cells have the intended offset and block position (measured from the cloud's own minimum corner, as the
    kernels do); the decoys share p's and q's cells; coverage is complete (asserted when the set is built)."""
    core = _core(kind)
    xyz, lab, tol = core["xyz"], core["lab"], core["tol"]
    a, b = xyz[:, lab == cc.LAB_A], xyz[:, lab == cc.LAB_B]
    near = cc.d2_f32(a[:, :, None, :], b[:, None, :, :]) < cc.tol2_f32(tol)
    assert np.array_equal(near[:, 0, 0], core["linked"])                  # (p, q) = the first point of each arm
    near[:, 0, 0] = False
    assert not near.any()
    lo = xyz.min(1)                                                       # the anchor IS the minimum corner
    assert np.array_equal(lo, core["lo"])
    cp, cq = cc.padded_cells(xyz[:, core["i_p"]], lo, tol), cc.padded_cells(xyz[:, core["i_q"]], lo, tol)
    assert np.array_equal(cq - cp, core["offsets"])
    assert np.array_equal(cp % 4, core["positions"])
    assert len({tuple(d) for d in np.concatenate([core["offsets"], -core["offsets"]])}) == 124
    ia, iq = core["i_p"], core["i_q"]
    assert (cc.padded_cells(xyz[:, ia:ia + 3], lo[:, None], tol) == cp[:, None]).all()      # p and its 2 decoys: 3 points
    assert (cc.padded_cells(xyz[:, iq:iq + 5], lo[:, None], tol) == cq[:, None]).all()      # q and its 4 decoys: 5 points
    # each arm is one component, the anchors are nobody's neighbours
    comp = cc.components_f32(xyz, tol)
    first_a, first_b = int(np.flatnonzero(lab == cc.LAB_A)[0]), int(np.flatnonzero(lab == cc.LAB_B)[0])
    assert (comp[:, lab == cc.LAB_A] == first_a).all()
    assert np.array_equal((comp[:, lab == cc.LAB_B] == first_a).all(1), core["linked"])
    assert ((comp[:, lab == cc.LAB_B] == first_b).all(1) | core["linked"]).all()
    assert (comp[:, lab == cc.LAB_OTHER] == np.flatnonzero(lab == cc.LAB_OTHER)).all()


@pytest.mark.parametrize("wide", [False, True])
def test_ties_are_exact(wide):
    """On the 1/128 lattice d2(p, q) == (float)(tol^2) == 225/16384 exactly in the 150 tie frames (no pair of A x B is within
    tol); with q pulled in by 2^-21 m (p, q) is the one pair that is."""
    core = _core("ties_wide" if wide else "ties")
    xyz, lab, tol = core["xyz"], core["lab"], core["tol"]
    assert cc.tol2_f32(tol) == np.float32(225.0 / 16384.0) and float(cc.tol2_f32(tol)) == 225.0 / 16384.0
    assert len(xyz) == 300 and int(core["linked"].sum()) == 150
    a, b = xyz[:, lab == cc.LAB_A], xyz[:, lab == cc.LAB_B]
    d2 = cc.d2_f32(a[:, :, None, :], b[:, None, :, :])
    tie = ~core["linked"]
    assert (d2[tie, 0, 0] == cc.tol2_f32(tol)).all()
    exact = ((b[tie, 0].astype(np.float64) - a[tie, 0].astype(np.float64)) ** 2).sum(1)
    assert (exact == 225.0 / 16384.0).all()                                # not a rounding accident: exact in double as well
    near = d2 < cc.tol2_f32(tol)
    assert np.array_equal(near[:, 0, 0], core["linked"])
    near[:, 0, 0] = False
    assert not near.any()
    comp = cc.components_f32(xyz, tol)
    first_a = int(np.flatnonzero(lab == cc.LAB_A)[0])
    assert (comp[:, lab == cc.LAB_A] == first_a).all()
    assert np.array_equal((comp[:, lab == cc.LAB_B] == first_a).all(1), core["linked"])


@pytest.mark.parametrize("name", _PROBE_SETS + _TIE_SETS)
def test_oracle_returns_the_constructed_cluster(ob, name):
    """The oracle's crop and BFS clustering give exactly the generator's expectation, frame by frame; the oracle's labels are
    the brute-force float32 components of the radius graph (on the probe's own points: arms and anchors)."""
    fr = _frames(name)
    op = _oparams(ob, fr)
    want = _oracle(ob, name)
    for f in range(len(fr["clouds"])):
        roi_e, clu_e = cc.expected(fr["clouds"], fr["lab"], fr["linked"], f)
        status, n_roi, n_cluster, roi, clu = want[f]
        assert n_roi == len(roi_e) and n_cluster == len(clu_e), (name, f, n_roi, n_cluster)
        assert np.array_equal(roi, roi_e), (name, f)
        assert np.array_equal(clu, clu_e), (name, f)
    core = fr["core"]
    comp = cc.components_f32(core["xyz"], core["tol"])
    for f in range(0, len(core["xyz"]), 7):
        pts = np.concatenate([core["xyz"][f], np.zeros((core["xyz"].shape[1], 1), np.float32)], axis=1)
        _, lab = ob.cluster(pts, core["click"][f], op)
        assert np.array_equal(lab, comp[f]), (name, f)


def test_every_set_takes_the_path_it_is_meant_for():
    """The numpy restatement of K2's dispatch on every set (the GPU tests assert the same before they run)."""
    assert _paths(_frames("compact")) == {"fine_lds"} and _paths(_frames("ties")) == {"fine_lds"}
    assert _paths(_frames("hbm")) == {"fine_hbm"}
    for name in ("wide", "ties_wide"):
        assert _paths(_frames(name)) == {"hashed"}
    assert _paths(_frames("wide_tiny")) == {"point"}
    # the sheets: more occupied cells than a fresh handle holds (hashed), a grid the bitmap holds (fine once the capacity has grown)
    for name, fine in (("sheet_small", "fine_either"), ("sheet_large", "fine_hbm")):
        fr = _frames(name)
        assert _paths(fr) == {"hashed"}
        n_in = fr["clouds"].shape[1]
        assert {cc.k2_path(n_in, _roi_xyz(fr, f), fr["tol"], cells_cap=1024) for f in range(len(fr["clouds"]))} == {fine}
    assert cc.LDS_POINTS_FRESH < _frames("sheet_small")["clouds"].shape[1] <= cc.LDS_POINTS_MAX    # (the LDS capacity grows to what a call saw)
    # the online caller: the window of the first tier cannot vouch for any frame (its nearest point is > 1.25 m from the
    # predicted one, which is nearer to the end of arm A than to anything else); the second tier asks hash_setup alone
    for name, verdict in (("online", "hashed"), ("ties_online", "hashed"), ("online_tiny", "point")):
        fr = _frames(name)
        n_in = fr["clouds"].shape[1]
        assert (n_in >= cc.HASH_MIN_FRAME_POINTS) == (verdict == "hashed")
        for f in range(len(fr["clouds"])):
            roi = fr["clouds"][f][fr["lab"][f] >= 0]
            d2 = cc.d2_f32(roi[:, :3], fr["point"][f])
            nn = int(np.argmin(d2))
            assert d2[nn] > np.float32(1.3 * 1.3) and np.array_equal(roi[nn, :3], fr["click"][f]), (name, f)
            assert (np.sort(d2)[1] > d2[nn])
            if f % 16 == 0:
                assert cc.k2_hashed_or_point(n_in, roi[:, :3], fr["tol"]) == verdict
    assert len(_frames("online")["clouds"]) == N_PLAN > cc.LIST_BLOCK
    assert cc.k2_threads(62) == 1024 and cc.k2_threads(248) == 256 and cc.k2_threads(N_PLAN, online=True) == 1024
    # the sheets stay > 3 tol from every arm
    for name in ("hbm", "sheet_small", "sheet_large"):
        fr = _frames(name)
        n_core = fr["core"]["xyz"].shape[1]
        for f in range(0, len(fr["clouds"]), 9):
            cloud, lab = fr["clouds"][f], fr["lab"][f]
            arms = cloud[lab > 0][:, :3].astype(np.float64)
            other = cloud[lab == 0][:, :3].astype(np.float64)
            assert len(other) == fr["clouds"].shape[1] - n_core + 1
            d = np.sqrt(((arms[:, None] - other[None]) ** 2).sum(2)).min()
            assert d > 3 * fr["tol"], (name, f, d)


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def _check_batch(e, res, fr, want, frames, name):
    """every frame of a finished call: counts and status == the oracle's; ROI and cluster clouds == the construction == the BFS"""
    from lidar_camera_calibration_amd import _native as N
    for k, f in enumerate(frames):
        r = res[k]
        status, n_roi, n_cluster, roi_o, clu_o = want[f]
        ctx = (name, int(f), "linked" if fr["linked"][f] else "unlinked")
        assert (r.status, r.n_roi, r.n_cluster) == (status, n_roi, n_cluster), ctx + ((r.status, r.n_roi, r.n_cluster), (status, n_roi, n_cluster))
        roi_e, clu_e = cc.expected(fr["clouds"], fr["lab"], fr["linked"], f)
        roi = e.fetch_cloud(k, N.CLOUD_ROI)
        assert np.array_equal(roi, roi_e) and np.array_equal(roi, roi_o), ctx
        clu = e.fetch_cloud(k, N.CLOUD_CLUSTER)
        assert np.array_equal(clu, clu_e), ctx + (len(clu), len(clu_e))
        assert np.array_equal(clu, clu_o), ctx


def _extract_batches(ob, name, batches, path, threads):
    """the set `name` through one fresh handle, one call per batch (lists of frame indices)"""
    from lidar_camera_calibration_amd import LidarCornersBatch
    fr = _frames(name)
    want = _oracle(ob, name)
    n_pts = fr["clouds"].shape[1]
    e = LidarCornersBatch(max(len(b) for b in batches), n_pts, _nparams(fr))
    try:
        for frames in batches:
            assert _paths(fr, frames) == {path} and cc.k2_threads(len(frames)) == threads
            res = e.extract(fr["clouds"][frames], fr["click"][frames])
            _check_batch(e, res, fr, want, frames, name)
    finally:
        e.close()


def _chunks(n, size):
    return [np.arange(k, min(n, k + size)) for k in range(0, n, size)]


@pytest.mark.gpu
def test_fine_lds_1024_threads_on_link_probes_and_ties(ob):
    """fine_cluster_frame<true> at 1024 threads: the 62 x 2 compact probes in batches of 62, and a sample of the ties"""
    _extract_batches(ob, "compact", _chunks(124, 62), "fine_lds", 1024)
    _extract_batches(ob, "ties", [np.arange(0, 300, 5)], "fine_lds", 1024)


@pytest.mark.gpu
def test_fine_lds_256_threads_on_link_probes_and_ties(ob):
    """fine_cluster_frame<true> at 256 threads: 62 x 2 x 2 seeds in one batch, all 300 ties in one batch"""
    _extract_batches(ob, "compact", [np.arange(248)], "fine_lds", 256)
    _extract_batches(ob, "ties", [np.arange(300)], "fine_lds", 256)


@pytest.mark.gpu
def test_fine_hbm_on_link_probes(ob):
    """fine_cluster_frame<false> (the cell-sorted points in HBM: > 4 096 ROI points): 62 x 2 in one batch (256 threads), 62 in a
    batch of <= 64 (1024 threads)"""
    _extract_batches(ob, "hbm", [np.arange(124)], "fine_hbm", 256)
    _extract_batches(ob, "hbm", [np.arange(0, 124, 2)], "fine_hbm", 1024)


@pytest.mark.gpu
def test_hashed_one_workgroup_on_link_probes_at_every_block_position(ob):
    """hashed_cluster_frame: 62 offsets x 16 block positions x {linked, unlinked} in one batch (256 threads), 64 of them in a
    small batch (1024 threads)"""
    _extract_batches(ob, "wide", [np.arange(N_PLAN)], "hashed", 256)
    _extract_batches(ob, "wide", [np.arange(5, N_PLAN, 31)], "hashed", 1024)
    assert len(np.arange(5, N_PLAN, 31)) == 64


@pytest.mark.gpu
def test_hashed_one_workgroup_on_ties(ob):
    _extract_batches(ob, "ties_wide", [np.arange(300)], "hashed", 256)
    _extract_batches(ob, "ties_wide", [np.arange(0, 300, 5)], "hashed", 1024)


@pytest.mark.gpu
def test_point_level_on_link_probes(ob):
    """point_level_cluster_frame: the wide frames with fewer than 256 input points"""
    _extract_batches(ob, "wide_tiny", [np.arange(124)], "point", 256)
    _extract_batches(ob, "wide_tiny", [np.arange(1, 124, 2)], "point", 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("name,second", [("sheet_small", "fine_lds"), ("sheet_large", "fine_hbm")])
def test_cell_level_paths_agree_on_identical_frames(ob, name, second):
    """The same 124 frames (a probe plus a sheet of ~750 occupied cells) twice through one handle: fresh, its LDS arrays hold 512
    cells and the frames take hashed_cluster_frame; the capacities grown by what that call needed, they take
    fine_cluster_frame -- <true> with 2 517 ROI points, <false> with 4 217.  Both calls must give the construction's cluster,
    and each other's bytes."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    fr = _frames(name)
    want = _oracle(ob, name)
    frames = np.arange(len(fr["clouds"]))
    n_pts = fr["clouds"].shape[1]
    assert _paths(fr) == {"hashed"}
    occupied = max(len(np.unique(cc.padded_cells(_roi_xyz(fr, f), _roi_xyz(fr, f).min(0), fr["tol"]), axis=0)) for f in frames)
    assert cc.CELLS_CAP_FRESH < occupied <= 1024
    assert (n_pts <= cc.LDS_POINTS_MAX) == (second == "fine_lds")      # (the LDS point capacity grows to what the first call saw)
    e = LidarCornersBatch(len(frames), n_pts, _nparams(fr))
    try:
        first = e.extract(fr["clouds"], fr["click"])
        _check_batch(e, first, fr, want, frames, name + " (hashed)")
        clouds1 = [e.fetch_cloud(int(f), N.CLOUD_CLUSTER) for f in frames]
        again = e.extract(fr["clouds"], fr["click"])
        _check_batch(e, again, fr, want, frames, name + " (" + second + ")")
        for f in frames:
            assert _record_bytes(first[f]) == _record_bytes(again[f]), f
            assert np.array_equal(clouds1[f], e.fetch_cloud(int(f), N.CLOUD_CLUSTER)), f
    finally:
        e.close()


def _record_bytes(r):
    """a full record's bytes, grid_ties left out: how many candidates the K6 full pass LISTED as near ties depends on how far the
    frame's bound had come down when each tile completed (test_stage_streams.py, test_gpu_parity.py); K7r re-ranks them exactly,
    so every other field is deterministic"""
    from lidar_camera_calibration_amd import _native as N
    c = N.Result.from_buffer_copy(r)
    c.grid_ties = 0
    return bytes(c)


def _online_call(ob, name, clouds, offsets, frames, n_pts):
    from lidar_camera_calibration_amd import LidarCornersBatch
    fr = _frames(name)
    want = _oracle(ob, name)
    e = LidarCornersBatch(len(frames), n_pts, _nparams(fr))
    try:
        e.reset_timing()
        res = e.chessboard_by_point(clouds, fr["point"][frames], offsets=offsets)
        assert e.timing().online_second_tier_frames == len(frames)      # every frame went through the k2h_* chain
        _check_batch(e, res, fr, want, frames, name)
    finally:
        e.close()


@pytest.mark.gpu
def test_k2h_chain_on_link_probes_in_one_call_of_more_than_1024_frames(ob):
    """The online caller's second tier: 62 x 16 x 2 frames in ONE call, so for_each_listed_chunk loops over kListBlock = 1024
    listed frames; every frame is listed (the first tier's window holds nothing within 1.25 m of the predicted point)."""
    fr = _frames("online")
    assert len(fr["clouds"]) > cc.LIST_BLOCK
    _online_call(ob, "online", fr["clouds"], None, np.arange(len(fr["clouds"])), fr["clouds"].shape[1])


@pytest.mark.gpu
def test_k2h_chain_on_ties(ob):
    fr = _frames("ties_online")
    _online_call(ob, "ties_online", fr["clouds"], None, np.arange(300), fr["clouds"].shape[1])


@pytest.mark.gpu
def test_k2h_finish_point_level_fallback_in_a_ragged_call(ob):
    """Frames of fewer than 256 input points are outside the hashed path's limits: k2h_finish clusters them with the point-level
    search.  A ragged call: every second frame loses its last 20 input points -- non-finite ones only, so that the oracle's
    answer for the frame stands."""
    fr = _frames("online_tiny")
    F, n = fr["clouds"].shape[:2]
    assert n < cc.HASH_MIN_FRAME_POINTS
    parts, lens = [], []
    for f in range(F):
        cloud = fr["clouds"][f]
        if f % 2:
            bad = np.flatnonzero(fr["lab"][f] < 0)[-20:]
            cloud = np.delete(cloud, bad, axis=0)
        parts.append(cloud)
        lens.append(len(cloud))
    assert len(set(lens)) == 2
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    _online_call(ob, "online_tiny", np.ascontiguousarray(np.concatenate(parts)), offsets, np.arange(F), n)


@pytest.mark.gpu
def test_a_click_at_no_comparable_distance_takes_point_zero_like_the_oracle(ob):
    """A click (or predicted point) with a NaN or infinite component: every squared distance is NaN or inf, none is below the
    1-NN search's initial FLT_MAX, and the reference's search keeps its initial index 0 -- the cluster of input point 0 when
    that is admissible, else the largest.  (choose_cluster used to index the frame's points with its initial 0xFFFFFFFF.)
    Link probes through the ROI path (fine grid; a NaN click component unbounds the box on that axis) and through the online
    caller (both tiers), against the oracle."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    fr = _frames("compact")
    frames = np.arange(62)                       # linked and unlinked probes alternate
    clicks = fr["click"][frames].copy()
    clicks[:, 0] = np.nan
    op = _oparams(ob, fr)
    e = LidarCornersBatch(len(frames), fr["clouds"].shape[1], _nparams(fr))
    sizes = set()
    try:
        for online in (False, True):
            if online:
                clicks[1::2, 0] = np.inf
                res = e.chessboard_by_point(fr["clouds"][frames], clicks)
            else:
                res = e.extract(fr["clouds"][frames], clicks)
            for k, f in enumerate(frames):
                cloud = fr["clouds"][f]
                roi = cloud if online else cloud[ob.roi_crop(cloud, clicks[k], op)]
                o = ob.chessboard_by_point(cloud, clicks[k], op)[0] if online else ob.extract(cloud, clicks[k], op)
                idx, lab = ob.cluster(roi, clicks[k], op)
                assert len(roi) == fr["clouds"].shape[1]
                assert (res[k].status, res[k].n_roi, res[k].n_cluster) == (o.status, o.n_roi, o.n_cluster), (online, k)
                assert np.array_equal(e.fetch_cloud(k, N.CLOUD_CLUSTER), roi[idx]), (online, k)
                sizes.add(len(idx))
                if np.count_nonzero(lab == lab[0]) >= CLUSTER_MIN:
                    assert idx[0] == np.flatnonzero(lab == lab[0])[0]       # point 0's component
    finally:
        e.close()
    assert len(sizes) >= 2


# ------------------------------------------------------------------------------------------------------------------ K1
_CROP_CLICKS = np.array([(2.5, 0.3, -0.7),                   # a box of ordinary limits
                         (1.0, 0.2, 0.1),                    # lo.x == 0
                         (3.0, -1.5, 0.4),                   # hi.y == 0
                         (7.1234567, -3.3333333, 0.1)],      # limits that round when narrowed to float
                        dtype=np.float32)
_CROP_HALF = (1.0, 1.5, 2.0)
_INF = float("inf")
_CROP_BOXES = {"finite": _CROP_HALF, "x_unbounded": (_INF, 1.5, 2.0), "y_unbounded": (1.0, _INF, 2.0),
               "z_unbounded": (1.0, 1.5, _INF), "unbounded": (_INF, _INF, _INF)}


@functools.lru_cache(maxsize=None)
def _crop_batch():
    """512 ragged frames: 4 clicks x 14 lengths x 9 survivor patterns, the 4 limit frames, and 4 frames whose click has a
    component of +inf (x, y, z) or NaN"""
    rng = np.random.default_rng(77)
    clouds, clicks, keeps = [], [], []
    for click in _CROP_CLICKS:
        for n in cc.CROP_LENGTHS:
            for pat in cc.CROP_PATTERNS:
                cloud, keep = cc.crop_frame(n, pat, click, _CROP_HALF, rng)
                clouds.append(cloud), clicks.append(click), keeps.append(keep)
    for click in _CROP_CLICKS:
        cloud, keep = cc.crop_limit_frame(click, _CROP_HALF)
        clouds.append(cloud), clicks.append(click), keeps.append(keep)
    for a, val in ((0, np.inf), (1, np.inf), (2, np.inf), (0, np.nan)):
        cloud, _ = cc.crop_frame(2049, "third", _CROP_CLICKS[0], _CROP_HALF, rng)
        click = _CROP_CLICKS[0].copy()
        click[a] = val
        clouds.append(cloud), clicks.append(click), keeps.append(None)
    assert len(clouds) == 512
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    return clouds, np.stack(clicks), keeps, offsets


def _crop_params(p, half):
    for a in range(3):
        p.roi_half[a] = half[a]
    p.cluster_min = p.cluster_max = 10_000_000          # nothing is admissible: every frame ends at K2 with ILCC_NO_CLUSTER
    return p


@pytest.mark.parametrize("box", list(_CROP_BOXES))
def test_crop_mask_is_the_oracle_crop(ob, box):
    """The numpy mask (finite and not below lo or above hi, float32) == orc_roi_crop on all 512 frames under every box; under the
    finite box it is the pattern each frame was built for; the limit frames keep what is written out by hand: both limits and
    their inward neighbours, both zeros against a limit of 0, nothing non-finite."""
    clouds, clicks, keeps, _ = _crop_batch()
    half = _CROP_BOXES[box]
    op = _crop_params(ob.default_params(), half)
    n_kept = 0
    for f, cloud in enumerate(clouds):
        mask = cc.crop_mask(cloud, clicks[f], half)
        assert np.array_equal(np.flatnonzero(mask), ob.roi_crop(cloud, clicks[f], op)), (box, f)
        if box == "finite" and keeps[f] is not None:
            assert np.array_equal(mask, keeps[f]), f
        n_kept += int(mask.sum())
    assert n_kept > 0
    if box == "finite":
        for f in range(504, 508):                         # the limit frames
            lo, hi = cc.crop_box(clicks[f], half)
            assert keeps[f].sum() >= 12 and (~keeps[f]).sum() >= 15
        assert (clouds[505][:, 0] == 0).sum() >= 3 and cc.crop_box(clicks[505], half)[0][0] == 0.0     # -0.0, +0.0 and lo.x itself
        assert cc.crop_box(clicks[506], half)[1][1] == 0.0
        # a click component of +inf keeps nothing; of NaN, every point that is finite and inside on the other two axes
        for f in (508, 509, 510):
            assert not cc.crop_mask(clouds[f], clicks[f], half).any()
        m = cc.crop_mask(clouds[511], clicks[511], half)
        assert m.sum() > (2049 + 2) // 3 and np.isfinite(clouds[511][m, :3]).all()


@pytest.fixture(scope="module")
def crop_handle():
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    e = LidarCornersBatch(512, max(cc.CROP_LENGTHS), _crop_params(N.default_params(), _CROP_HALF))
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(_CROP_BOXES))
def test_roi_crop_on_its_limits_one_pass_and_two_kernels(crop_handle, box):
    """All 512 frames in one ragged batch through k1_roi_crop_frame (a batch of >= 512 frames) and, with
    debug_separate_launches, through k1_roi_count + k1_roi_scatter: n_roi and the ROI cloud byte-identical to the numpy mask.
    The unbounded boxes and the frames with a non-finite click take keep_point<false> -- in the one-pass crop, crop_frame<false>."""
    from lidar_camera_calibration_amd import _native as N
    clouds, clicks, keeps, offsets = _crop_batch()
    half = _CROP_BOXES[box]
    e = crop_handle
    e.set_params(_crop_params(N.default_params(), half))
    flat = np.ascontiguousarray(np.concatenate(clouds))
    want = [cloud[cc.crop_mask(cloud, clicks[f], half)] for f, cloud in enumerate(clouds)]
    try:
        for separate in (False, True):
            e.debug_separate_launches(separate)
            res = e.extract(flat, clicks, offsets=offsets)
            for f in range(512):
                ctx = (box, "count + scatter" if separate else "one pass", f, len(clouds[f]))
                assert res[f].n_points == len(clouds[f]) and res[f].n_roi == len(want[f]), ctx + (res[f].n_roi, len(want[f]))
                assert res[f].status == (N.NO_CLUSTER if len(want[f]) else N.NO_ROI_POINTS), ctx
                got = e.fetch_cloud(f, N.CLOUD_ROI)
                assert got.tobytes() == want[f].tobytes(), ctx
    finally:
        e.debug_separate_launches(False)
