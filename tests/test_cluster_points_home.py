"""K2's two homes for the cell-sorted points (LDS, or the frame's slice of the cluster buffer in global memory), the rule that
picks one per launch, and the grouped pair test both homes share.

The edge phase tests a pair of cells by walking the neighbour cell's points in GROUPS OF FOUR: the loads of a group are
unconditional, from an index clamped to the cell's last point.  GROUP TAILS are frames whose answer hangs on one slot of one
group: two occupied cells one or two cells apart, one with a single point p, the other with k = 1 .. 9 points (one group, a full
group, a group plus a tail of one to three, two groups plus one) of which at most one is within tol of p, the others a few 1e-4 m
beyond.  Where a point lands inside its sorted cell is a race of atomics, so each of the k points is the near one in turn.  Both
orientations occur: the k-point cell as the neighbour walked in groups (forward offsets) and as the cell walked point by point
(backward offsets).  The expected cluster is known from the construction, as in tests/test_cluster_constructed.py, whose
constructed sets, oracle bookkeeping and batch check this file reuses.

Every GPU comparison is `==`.  A full record is compared by test_cluster_constructed._record_bytes: every byte but grid_ties,
which depends on the timing of the K6 full pass (see there), not on K2.
"""
import functools

import numpy as np
import pytest

import constructed_clusters as cc
import test_cluster_constructed as tcc

TOL = tcc.TOL_ROI
K_MAX = 9
# q's cell - p's cell: one and two cells apart along the row a cell's own window covers, and two more rows of the 5 x 5 x 5
# neighbourhood; the negated ones make the k-point cell the one that comes first
OFFSETS = ((1, 0, 0), (2, 0, 0), (-1, 0, 0), (-2, 0, 0), (0, 2, 1), (1, -1, -2))
BASE_CELL = 16
N_PAD_SLOTS = K_MAX          # B's k points + (K_MAX - k) lone padding points: every frame has the same number of points


# ------------------------------------------------------------------------------------------------------------------ the set
def _tail_plan():
    """(offset, k, near) rows: near = index of B's point within tol, -1 for the unlinked variant"""
    return [(d, k, near) for d in OFFSETS for k in range(1, K_MAX + 1) for near in list(range(k)) + [-1]]


@functools.lru_cache(maxsize=None)
def _tails():
    plan = _tail_plan()
    F = len(plan)
    rng = np.random.default_rng(707)
    s = 1.0 / float(cc.cell_inv(TOL))                      # cell side
    lo = (np.array([1.0, -2.0, -1.5]) + rng.uniform(-0.3, 0.3, (F, 3))).astype(np.float32)
    n_core = 1 + 1 + cc.N_ARM + N_PAD_SLOTS                # anchor, p, arm A, B / padding
    xyz = np.zeros((F, n_core, 3), np.float64)
    lab = np.full((F, n_core), cc.LAB_OTHER)
    linked = np.zeros(F, bool)
    ks = np.zeros(F, np.int64)
    for f, (d, k, near) in enumerate(plan):
        d = np.asarray(d, np.float64)
        v = d / np.linalg.norm(d)
        g = (TOL / s) * v                                  # q - p in cell sides (1.754 along v)
        u_lo, u_hi = np.maximum(0.0, d - g), np.minimum(1.0, d + 1.0 - g)
        assert ((u_hi - u_lo) > 0.2).all()
        p = lo[f].astype(np.float64) + (BASE_CELL + 0.5 * (u_lo + u_hi)) * s      # the middle of the room p has in its cell
        w1 = cc._perp(v[None])[0]
        w2 = np.cross(v, w1)
        # B's points: directions fanned out by up to 0.03 rad around v, the near one at tol (1 - 1e-4), the others 2 .. 5 e-4 m beyond tol
        ang = 0.03 * np.stack([np.cos(2.4 * np.arange(k)), np.sin(2.4 * np.arange(k))], axis=1) * np.sqrt((np.arange(k) + 1.0) / k)[:, None]
        dirs = v[None] + ang[:, :1] * w1[None] + ang[:, 1:] * w2[None]
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = TOL + (2.0 + (np.arange(k) * 7 % 4)) * 1e-4
        if near >= 0:
            r[near] = TOL * (1.0 - 1e-4)
        q = p[None] + r[:, None] * dirs
        arm_a, _ = cc._arms(p[None], q[:1], v[None], TOL)
        pads = lo[f].astype(np.float64)[None] + np.stack([(4.0 + 3.0 * np.arange(K_MAX - k)) * s, np.zeros(K_MAX - k), np.zeros(K_MAX - k)], axis=1)
        xyz[f] = np.concatenate([lo[f][None].astype(np.float64), p[None], arm_a[0], q, pads])
        lab[f, 1:2 + cc.N_ARM] = cc.LAB_A
        lab[f, 2 + cc.N_ARM:2 + cc.N_ARM + k] = cc.LAB_B
        linked[f] = near >= 0
        ks[f] = k
    xyz = xyz.astype(np.float32)
    click = xyz[:, 1 + cc.N_ARM].copy()                    # the far end of arm A
    core = dict(xyz=xyz, lab=lab, click=click, lo=lo, tol=TOL, linked=linked)
    clouds, clab = cc.assemble(core, seed=77)
    return dict(clouds=clouds, lab=clab, linked=linked, click=click, tol=TOL, roi_half=2.5, core=core, k=ks, plan=plan)


def test_group_tails_are_what_they_claim():
    """On the kernels' own float32 arithmetic: p alone in its cell, B's k points together in the cell at the planned offset, the
    planned point and no other within tol of p, no other pair of A x B within tol, arm A one component with p, the padding
    points and the anchor nobody's neighbours; every k = 1 .. 9 with every slot near in turn and once with none, at every offset."""
    fr = _tails()
    core = fr["core"]
    xyz, lab, lo = core["xyz"], core["lab"], core["lo"]
    assert np.array_equal(xyz.min(1), lo)                  # the anchor is the minimum corner
    t2 = cc.tol2_f32(TOL)
    seen = set()
    for f, (d, k, near) in enumerate(fr["plan"]):
        cells = cc.padded_cells(xyz[f], lo[f], TOL)
        cp = cells[1]
        b = np.flatnonzero(lab[f] == cc.LAB_B)
        assert len(b) == k and (cells[b] - cp == np.asarray(d)).all(), (f, d, k)
        assert (np.flatnonzero((cells == cp).all(1)) == [1]).all()                    # p's cell holds p alone
        assert sorted(np.flatnonzero((cells == cells[b[0]]).all(1))) == sorted(b)     # B's cell holds B's points alone
        d2 = cc.d2_f32(xyz[f, 1], xyz[f, b])
        assert np.array_equal(np.flatnonzero(d2 < t2), [near] if near >= 0 else []), (f, d2, t2)
        beyond = np.sqrt(d2.astype(np.float64)) - TOL
        assert (np.delete(beyond, near) if near >= 0 else beyond).max(initial=0.0) < 6e-4
        a = np.flatnonzero(lab[f] == cc.LAB_A)
        cross = cc.d2_f32(xyz[f, a][:, None, :], xyz[f, b][None, :, :]) < t2
        assert int(cross.sum()) == (1 if near >= 0 else 0)
        comp = cc.components_f32(xyz[f][None], TOL)[0]
        assert (comp[a] == 1).all() and ((comp[b] == 1).all() if near >= 0 else (comp[b] == b[0]).all())
        other = np.flatnonzero(lab[f] == cc.LAB_OTHER)
        assert np.array_equal(comp[other], other)
        seen.add((d, k, near))
    assert seen == {(d, k, n) for d in OFFSETS for k in range(1, 10) for n in range(-1, k)} and len(seen) == 6 * 54
    n_in = fr["clouds"].shape[1]
    assert {cc.k2_path(n_in, fr["clouds"][f][:, :3], TOL) for f in range(len(fr["clouds"]))} == {"fine_lds"}
    assert cc.k2_threads(len(fr["clouds"])) == 256


_TAIL_ORACLE = []


def _tail_oracle(ob):
    """per frame (status, n_roi, n_cluster, ROI cloud, cluster cloud) of the oracle, computed once"""
    if not _TAIL_ORACLE:
        fr = _tails()
        op = tcc._oparams(ob, fr)
        for f, cloud in enumerate(fr["clouds"]):
            o = ob.extract(cloud, fr["click"][f], op)
            roi = cloud[ob.roi_crop(cloud, fr["click"][f], op)]
            idx, _ = ob.cluster(roi, fr["click"][f], op)
            _TAIL_ORACLE.append((o.status, o.n_roi, o.n_cluster, roi, roi[idx]))
    return _TAIL_ORACLE


def test_oracle_returns_the_constructed_tail_cluster(ob):
    fr = _tails()
    for f, (status, n_roi, n_cluster, roi, clu) in enumerate(_tail_oracle(ob)):
        roi_e, clu_e = cc.expected(fr["clouds"], fr["lab"], fr["linked"], f)
        assert np.array_equal(roi, roi_e) and np.array_equal(clu, clu_e), f
        assert (n_roi, n_cluster) == (len(roi_e), len(clu_e)) and len(clu_e) == 1 + cc.N_ARM + (fr["k"][f] if fr["linked"][f] else 0)


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def _run_forced(fr, want, batches, home, threads, name):
    """the frames through one fresh handle with the home forced, one call per batch: every frame checked as _check_batch checks it,
    every launch asked what it used.  -> per frame (record bytes, cluster cloud)"""
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    out = {}
    e = LidarCornersBatch(max(len(b) for b in batches), fr["clouds"].shape[1], tcc._nparams(fr))
    try:
        e.debug_cluster_home(home)
        for frames in batches:
            res = e.extract(fr["clouds"][frames], fr["click"][frames])
            used = e.debug_cluster_launch()
            assert (used["home"], used["threads"]) == (home, threads), used
            tcc._check_batch(e, res, fr, want, frames, name)
            for k, f in enumerate(frames):
                out[int(f)] = (tcc._record_bytes(res[k]), e.fetch_cloud(k, N.CLOUD_CLUSTER))
    finally:
        e.close()
    return out


def _both_homes(fr, want, batches, threads, name):
    from lidar_camera_calibration_amd import _native as N
    lds = _run_forced(fr, want, batches, N.CLUSTER_HOME_LDS, threads, name + " (LDS home)")
    l2 = _run_forced(fr, want, batches, N.CLUSTER_HOME_L2, threads, name + " (L2 home)")
    assert lds.keys() == l2.keys()
    for f in lds:
        assert lds[f][0] == l2[f][0], (name, f)
        assert lds[f][1].tobytes() == l2[f][1].tobytes(), (name, f)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
def test_group_tails_in_both_homes(ob, threads):
    """Every tail frame in both homes: one batch of all 324 (256 threads), batches of 64 (1024 threads)"""
    fr = _tails()
    n = len(fr["clouds"])
    batches = [np.arange(n)] if threads == 256 else tcc._chunks(n, cc.SMALL_BATCH)
    assert all(cc.k2_threads(len(b)) == threads for b in batches)
    _both_homes(fr, _tail_oracle(ob), batches, threads, "tails")


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["compact", "ties"])
def test_constructed_sets_in_the_forced_l2_home(ob, name, threads):
    """The link probes (every offset of the neighbourhood) and the exact ties with the sorted points in global memory"""
    from lidar_camera_calibration_amd import _native as N
    fr = tcc._frames(name)
    n = len(fr["clouds"])
    batches = [np.arange(n)] if threads == 256 else ([np.arange(0, 124, 2), np.arange(1, 124, 2)] if name == "compact" else [np.arange(0, n, 5)])
    assert all(cc.k2_threads(len(b)) == threads for b in batches) and tcc._paths(fr) == {"fine_lds"}
    _run_forced(fr, tcc._oracle(ob, name), batches, N.CLUSTER_HOME_L2, threads, name)


@pytest.mark.gpu
def test_real_shapes_are_byte_identical_in_both_homes():
    """128 synthetic VLP-16 frames through the whole path with each home forced: records, ROI clouds and cluster clouds"""
    from lidar_camera_calibration_amd import LidarCornersBatch, synth
    from lidar_camera_calibration_amd import _native as N
    clouds, clicks, _, _ = synth.make_batch(128, seed=0x2B0B)
    got = {}
    for home in (N.CLUSTER_HOME_LDS, N.CLUSTER_HOME_L2):
        e = LidarCornersBatch(128, clouds.shape[1], N.default_params())
        try:
            e.debug_cluster_home(home)
            res = e.extract(clouds, clicks)
            assert e.debug_cluster_launch()["home"] == home
            got[home] = [(tcc._record_bytes(res[f]), e.fetch_cloud(f, N.CLOUD_ROI).tobytes(), e.fetch_cloud(f, N.CLOUD_CLUSTER).tobytes())
                         for f in range(128)]
        finally:
            e.close()
    assert sum(N.Result.from_buffer_copy(r[0]).status == N.OK for r in got[N.CLUSTER_HOME_LDS]) >= 120
    for f in range(128):
        assert got[N.CLUSTER_HOME_LDS][f] == got[N.CLUSTER_HOME_L2][f], f


@pytest.mark.gpu
def test_the_rule_picks_the_home_per_launch(ob):
    """On a handle reserved (1792, 2560): 1024 frames do not fit the device with the LDS copy and run without it, in at most a
    quarter of a compute unit's LDS each; 248 and 64 frames fit and keep it (at 256 and 1024 threads); a forced home overrides
    both.  Frames: the compact link probes, tiled -- and still clustered right."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    fr = tcc._frames("compact")
    want = tcc._oracle(ob, "compact")
    n = len(fr["clouds"])
    assert n == 248
    pick = {1024: np.arange(1024) % n, 248: np.arange(248), 64: np.arange(0, 248, 4)[:64]}
    e = LidarCornersBatch(1024, fr["clouds"].shape[1], tcc._nparams(fr))
    try:
        e.reserve(1792, 2560)

        def call(n_frames):
            frames = pick[n_frames]
            res = e.extract(fr["clouds"][frames], fr["click"][frames])
            tcc._check_batch(e, res, fr, want, frames, "rule, %d frames" % n_frames)
            return e.debug_cluster_launch()

        used = call(1024)
        print("K2 launch of 1024 frames:", used)
        assert used["cus"] > 0 and used["lds_per_cu"] > 0
        assert (used["home"], used["threads"]) == (N.CLUSTER_HOME_L2, 256), used
        assert used["lds_bytes"] <= used["lds_per_cu"] // 4 - used["static_lds_bytes"], used
        used = call(248)
        assert (used["home"], used["threads"]) == (N.CLUSTER_HOME_LDS, 256), used
        with_copy = used["lds_bytes"]
        used = call(64)
        assert (used["home"], used["threads"], used["lds_bytes"]) == (N.CLUSTER_HOME_LDS, 1024, with_copy), used
        e.debug_cluster_home(N.CLUSTER_HOME_LDS)
        used = call(1024)
        assert (used["home"], used["threads"], used["lds_bytes"]) == (N.CLUSTER_HOME_LDS, 256, with_copy), used
        e.debug_cluster_home(N.CLUSTER_HOME_L2)
        used = call(64)
        assert (used["home"], used["threads"]) == (N.CLUSTER_HOME_L2, 1024) and used["lds_bytes"] < with_copy, used
        e.debug_cluster_home(N.CLUSTER_HOME_RULE)
        used = call(64)
        assert (used["home"], used["threads"]) == (N.CLUSTER_HOME_LDS, 1024), used
        with pytest.raises(Exception):
            e.debug_cluster_home(3)
    finally:
        e.close()
