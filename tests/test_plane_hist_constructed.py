"""K3 (RANSAC plane), K4 (plane frame) and K5 (gray-zone histogram) on CONSTRUCTED clusters (tests/constructed_planes.py).

The rest of the suite feeds these stages the board clusters of synthetic frames: 90 % inliers, a loop that stops after 3 to 5
hypotheses, ~950 continuous intensities.  Here every frame is built for one decision of the kernels:

  A  an exact plane and points exactly AT the threshold, 2^-21 inside and 2^-21 outside it; winners of either orientation
  B  noisy planes on which PCL's loop stops at every position of a round of 4 and of 16 wavefronts, with a better hypothesis
     scored behind the stop; the iteration cap in mid-round
  C  clusters whose samples are nearly all degenerate: the first valid hypothesis just before and just behind the skip cap
  D  3 inliers (no refit, K4 on three points) and 4 (the first refit)
  E  cluster sizes around the wavefront, the workgroup and the LDS staging, with keep masks for both in-place compactions
  F  the histogram rule on patterns of per-bin counts: ties across the mean, empty bins, the mean on a bin edge, half bins, points
     on the zone's ends

Every frame goes through the three paths that share the stage functions -- K3 at 1024 threads (batches of <= 64 frames), the one
launch k345_front_end, and the separate launches at 256 threads -- which must agree byte for byte in everything they produce.
The reference of each stage is the CPU oracle FED WHAT THE GPU FETCHED for the stage before (K1 and K2 only have to hand the
whole cloud over, which is asserted).  The CPU tests (no marker) check that every constructed input is what the GPU tests take it
for, with the numpy restatements of constructed_planes, and bind those restatements to the oracle.  Nothing here is tuned against
the kernels: seeds, orders and patterns were picked on those CPU conditions alone.
"""
import functools
import itertools

import numpy as np
import pytest

import constructed_planes as cp
from test_oracle_golden import _gray_zone_python

SEED = 12345              # ransac_seed of every group but E's minority masks
ROI_HALF = 8.0
NO_PLANE, DEGENERATE_HIST = 3, 4
F_KEYS = tuple(("F", k) for k in range(len(cp.F_BY_HAND) + cp.F_RANDOM))


# ------------------------------------------------------------------------------------------------------------------ the frames
@functools.lru_cache(maxsize=None)
def _patterns():
    return [i for _, i in cp.F_BY_HAND] + cp.random_patterns()


def _e_data_seed(m, k3, k5):
    return 131 * m + 17 * cp.E_MASKS.index(k3) + cp.E_MASKS.index(k5)


@functools.lru_cache(maxsize=None)
def _frame(key):
    """-> dict(cloud, ...): built once, shared, never modified.  exact_plane: the plane must be +-(1, 0, 0, -+2) to the bit;
    exact_pca: a symmetric lattice, K4's sums and eigenvectors are exact too"""
    kind = key[0]
    if kind == "A":
        cloud, inl = cp.exact_plane_frame(key[1])
        fr = dict(cloud=cloud, inliers=inl, exact_plane=True, exact_pca=True)
    elif kind == "B":
        fr = dict(cloud=cp.noisy_plane(key[1]))
    elif kind == "C":
        cloud, off = cp.line_frame_first_valid_at(key[2], SEED)
        fr = dict(cloud=cloud, off=off, exact_plane=True)
    elif kind == "D":
        cloud, h, members = cp.few_inliers_frame(SEED, key[1])
        fr = dict(cloud=cloud, h=h, members=members)
    elif kind == "D3":
        fr = dict(cloud=cp.three_point_frame(), exact_plane=True)
    elif kind == "E":
        cloud, inl, lab = cp.mask_frame(key[1], key[2], key[3], _e_data_seed(*key[1:]))
        fr = dict(cloud=cloud, inliers=inl, labelled=lab, exact_plane=True)
    elif kind == "F":
        fr = dict(cloud=cp.pattern_frame(_patterns()[key[1]], key[1]), exact_plane=True, exact_pca=True)
    elif kind == "Z":
        fr = dict(cloud=cp.pattern_frame(cp.ZONE_ENDS_100, 1), exact_plane=True, exact_pca=True)
    fr["cloud"].setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _groups():
    """name -> (parameter fields, frame keys): parameters are per handle, so the frames are grouped by parameter set"""
    g = {}
    exact = dict(ransac_thresh=cp.THR_EXACT, hist_bins=cp.F_BINS)
    g["exact"] = (exact, tuple(("A", o) for o in cp.A_CASES["adaptive"]) + F_KEYS)
    g["exact_rate1.2"] = (dict(exact, gray_rate=1.2), F_KEYS)
    for hyp in (1, 4, 7, 16, 17):
        g["fixed_%d" % hyp] = (dict(exact, ransac_probability=0.0, ransac_hyp=hyp), tuple(("A", o) for o in cp.A_CASES[hyp]))
    g["noisy"] = ({}, tuple(("B", s) for s in cp.B_SEEDS))
    g["noisy_p20"] = (dict(ransac_probability=cp.B_P20), tuple(("B", s) for s in cp.B_SEEDS_P20))
    for hyp in cp.B_HYP_CAPS:
        g["noisy_hyp%d" % hyp] = (dict(ransac_hyp=hyp), tuple(("B", s) for s in cp.B_SEEDS))
    for hyp in (1, 2):
        g["skips_%d" % hyp] = (dict(exact, ransac_hyp=hyp), (("C", hyp, 10 * hyp - 1), ("C", hyp, 10 * hyp)))
    g["few"] = (dict(ransac_thresh=cp.D_THR, hist_bins=2), (("D", False), ("D", True), ("D3",)))
    masks = dict(ransac_thresh=cp.E_THR, hist_bins=cp.E_BINS)
    g["masks"] = (masks, tuple(("E",) + c for c in cp.e_cases() if c[1] not in cp.E_MINORITY))
    for c in cp.e_cases():
        if c[1] in cp.E_MINORITY:
            fr = _frame(("E",) + c)
            seed = cp.seed_whose_first_sample_is_kept(fr["inliers"], fr["cloud"][:, :3])
            g["masks_%d_%s" % c[:2]] = (dict(masks, ransac_seed=seed), (("E",) + c,))
    g["zone_ends"] = (dict(exact, hist_bins=100), (("Z",),))
    return g


GROUP_NAMES = ("exact", "exact_rate1.2", "fixed_1", "fixed_4", "fixed_7", "fixed_16", "fixed_17", "noisy", "noisy_p20", "noisy_hyp1",
               "noisy_hyp2", "noisy_hyp3", "noisy_hyp5", "skips_1", "skips_2", "few", "masks") + \
    tuple("masks_%d_%s" % c[:2] for c in cp.e_cases() if c[1] in cp.E_MINORITY) + ("zone_ends",)


def _cut_grid(p):
    """test_grid_backend_constructed._cut_grid: the default grid's steps on 9 x 12 x 12 candidates"""
    return dict(n_th=9, th_min=-4 * p.th_step, n_ty=12, ty_min=-6 * p.ty_step, n_tz=12, tz_min=-6 * p.tz_step)


def _apply(p, solver_grid, fields):
    p.solver = solver_grid
    p.cluster_tol, p.cluster_min = 1.0, 3
    for a in range(3):
        p.roi_half[a] = ROI_HALF
    for k, v in dict(_cut_grid(p), **fields).items():
        setattr(p, k, v)
    return p


def _oparams(ob, group):
    return _apply(ob.default_params(), ob.SOLVER_GRID, _groups()[group][0])


def _nparams(group):
    from lidar_camera_calibration_amd import _native as N
    return _apply(N.default_params(), N.SOLVER_GRID, _groups()[group][0])


def _all_frames():
    return [(g, key) for g in GROUP_NAMES for key in _groups()[g][1]]


# ------------------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def _reference(ob, group, key):
    """The oracle's K3 -> K4 -> K5 on the frame's cloud under the group's parameters, each stage fed the one before: computed
    once per (group, frame), shared, never modified.  (The GPU tests first assert that what the GPU fetched for a stage's input
    is byte for byte what the oracle was fed here.)"""
    op = _oparams(ob, group)
    cloud = _frame(key)["cloud"]
    idx, plane = ob.ransac_plane(cloud, op)
    ref = dict(idx=idx, plane=plane, board=np.ascontiguousarray(cloud[idx]), no_plane=len(idx) < 3)
    if ref["no_plane"]:
        return ref
    board = ref["board"]
    st, pca, pts = ob.plane_frame(board, op)
    assert st == 0
    hist_status, rl, gz = ob.gray_zone(board[:, 3], op)
    ref.update(pca=pca, pca_cloud=pts, degenerate=hist_status != 0, rl=tuple(rl), gz=tuple(gz),
               python=_gray_zone_python(board[:, 3], op.hist_bins, op.gray_rate))
    if not ref["degenerate"]:
        ref["classes"] = cp.classes(board[:, 3], gz)
    return ref


@functools.lru_cache(maxsize=None)
def _loop(ob, group, key):
    """the restatement's account of K3's loop on the frame: (best_count, best_h, h_stop, iterations, skipped, counts); in the
    fixed mode (best_count, best_h)"""
    op = _oparams(ob, group)
    cloud = _frame(key)["cloud"]
    if op.ransac_probability > 0.0:
        return cp.pcl_loop(cloud, op.ransac_thresh, op.ransac_seed, op.ransac_probability, op.ransac_hyp)
    return cp.fixed_best(cloud, op.ransac_thresh, op.ransac_seed, op.ransac_hyp)


def _fixed(ob, group, cloud, n_hyp):
    """the oracle with ransac_probability = 0 and n_hyp hypotheses, the group's other parameters kept"""
    op = _oparams(ob, group)
    op.ransac_probability, op.ransac_hyp = 0.0, n_hyp
    return ob.ransac_plane(cloud, op)


# ================================================================================================================== CPU tests
def test_group_names_are_the_groups():
    assert tuple(_groups()) == GROUP_NAMES
    assert len({key for _, key in _all_frames()}) >= 450


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_restatement_of_the_loop_is_bound_to_the_oracle(ob, group):
    """The oracle reports neither its winner nor where it stopped; the restatement (sample_index, plane_from_3, plane_dist in
    float32, PCL's loop) does.  For every frame used: the oracle's result == the oracle's result with ransac_probability = 0 and
    ransac_hyp = the restatement's best_h + 1, as plane bytes and indices -- the restatement's winner IS the oracle's, with the
    most inliers and the lowest index of all hypotheses up to it."""
    for key in _groups()[group][1]:
        cloud = _frame(key)["cloud"]
        ref = _reference(ob, group, key)
        best, best_h = _loop(ob, group, key)[:2]
        if best == 0:
            assert best_h == -1 and len(ref["idx"]) == 0, key
            continue
        idx, plane = _fixed(ob, group, cloud, best_h + 1)
        assert np.array_equal(idx, ref["idx"]) and plane.tobytes() == ref["plane"].tobytes(), (group, key, best, best_h)
        loop = _loop(ob, group, key)
        if len(loop) > 2:   # (the adaptive loop: a strict maximum of what was drawn before it, and no later one beats it)
            counts = loop[5]
            assert all(c is None or c < best for c in counts[:best_h]) and all(c is None or c <= best for c in counts), (group, key)
        pl = cp.hypothesis(cloud, _oparams(ob, group).ransac_seed, best_h, _oparams(ob, group).ransac_thresh)[1]
        if best <= 3:       # no refit: the sample plane itself, to the bit
            assert pl.tobytes() == ref["plane"].tobytes(), (group, key)
        if best <= 3 or _is_exact(pl):      # the refit returns the winner's own plane: its count is the oracle's
            assert best == len(ref["idx"]), (group, key, best, len(ref["idx"]))


def test_every_frame_is_one_cluster_with_both_colours(ob):
    """What lets K1 and K2 drop out of the comparison, and K6 never see an empty frame: a frame's bounding box has a diagonal
    below cluster_tol = 1 m (every pair of points links) inside the ROI around its first point; frames of up to 400 points go
    through the oracle's whole chain (n_cluster == all; the larger ones would take its O(n^2) clustering a minute each).
    Every frame that passes K5 has a black and a white point, gz0 > low >= min and gz1 < high < max; where K4 is compared
    within 1e-6 (no symmetric lattice) the plane frame's eigenvalues are well apart."""
    for group, key in _all_frames():
        fr, ref = _frame(key), _reference(ob, group, key)
        cloud = fr["cloud"]
        xyz = cloud[:, :3].astype(np.float64)
        assert np.linalg.norm(xyz.max(0) - xyz.min(0)) < 0.999 and np.abs(xyz - xyz[0]).max() < 1.0 < ROI_HALF, key
        assert len(np.unique(xyz, axis=0)) == len(xyz) <= 4097
        if len(cloud) <= 400:
            o = ob.extract(cloud, cloud[0, :3], _oparams(ob, group))
            assert (o.n_roi, o.n_cluster, o.n_plane) == (len(cloud), len(cloud), len(ref["idx"])), (group, key)
            assert (o.status == NO_PLANE) == ref["no_plane"] and (o.status == DEGENERATE_HIST) == bool(ref.get("degenerate")), (group, key, o.status)
        if ref["no_plane"] or ref["degenerate"]:
            continue
        cls, inten = ref["classes"], ref["board"][:, 3].astype(np.float64)
        assert (cls == 0).any() and (cls == 2).any(), (group, key)
        low, high = ref["rl"]
        if _oparams(ob, group).gray_rate > 2:
            assert ref["gz"][0] > low >= inten.min() and ref["gz"][1] < high < inten.max(), (group, key)
        if not fr.get("exact_pca"):
            b = ref["board"][:, :3].astype(np.float64)
            w = np.linalg.eigvalsh(np.cov(b.T, bias=True))
            assert w[1] - w[0] > 1e-3 * w[2] and w[2] - w[1] > 1e-3 * w[2], (group, key, w)


def _is_exact(plane):
    """+-(1, 0, 0, -+2) exactly (a zero of either sign)"""
    return plane.dtype == np.float32 and abs(plane[0]) == 1 and plane[1] == 0 and plane[2] == 0 and plane[3] == -2 * plane[0]


# ---- A
def test_exact_planes_are_exact_and_of_both_signs(ob):
    """A: the distances of the 165 points from x = 2 are 0, thr, thr - 2^-21 and thr + 2^-21 exactly; under every listed mode and
    order the oracle's plane is +-(1, 0, 0, -+2) to the bit and its inliers are the lattice and the thr - 2^-21 quadruple -- the
    points AT thr are out.  Both signs occur in every mode with more than one hypothesis (the sign is that of the first hypothesis
    to reach the winning count), and under some orders the winner is not hypothesis 0.  K4 of those inliers is exact as well:
    the plane frame is a permutation matrix.  All coordinates are multiples of 2^-21 below 4 and the squares summed are those
    of multiples of 2^-10 (and of four equal offsets): exact in a double in any order."""
    thr = np.float32(cp.THR_EXACT)
    assert float(thr) == cp.THR_EXACT
    pca_exact = np.array([[-1, 0, 0, 2], [0, 0, 1, -0.25], [0, 1, 0, -0.5], [0, 0, 0, 1]], np.float32)
    for mode, orders in cp.A_CASES.items():
        group = "exact" if mode == "adaptive" else "fixed_%d" % mode
        signs, winners = set(), set()
        for o in orders:
            fr, ref = _frame(("A", o)), _reference(ob, group, ("A", o))
            cloud, inl = fr["cloud"], fr["inliers"]
            d = np.abs(cloud[:, 0].astype(np.float64) - 2.0)
            assert sorted(set(d)) == sorted({0.0} | set(cp.A_OFFSETS)) and len(cloud) == 165
            assert np.array_equal(cp.plane_dist(np.array([1, 0, 0, -2], np.float32), cloud).astype(np.float64), d)
            assert np.array_equal(inl, d < cp.THR_EXACT) and not inl[d == cp.THR_EXACT].any() and int(inl.sum()) == 157
            assert (cloud[:, :3].astype(np.float64) * 2.0 ** 21 % 1 == 0).all() and np.abs(cloud[:, :3]).max() < 4
            assert _is_exact(ref["plane"]) and np.array_equal(ref["idx"], np.flatnonzero(inl)), (mode, o)
            assert np.array_equal(ref["pca"], pca_exact), (mode, o)
            signs.add(float(ref["plane"][0]))
            winners.add(_loop(ob, group, ("A", o))[1])
        assert signs == {1.0, -1.0}, mode
        assert mode == 1 or max(winners) >= 1, mode


# ---- B
def _margin(ref, cloud, thr):
    pl = ref["plane"].astype(np.float64)
    return np.abs(np.abs(cloud[:, :3].astype(np.float64) @ pl[:3] + pl[3]) - thr).min()


def test_noisy_planes_stop_where_intended(ob):
    """B: with the restatement's account of the loop.  ransac_probability 0.99: h_stop (the first hypothesis not drawn) falls on
    every position of a round of 4; on one frame at least a hypothesis with MORE inliers than the winner lies behind the stop
    inside the same round of 4, on one inside the same round of 16 -- visibly: the oracle run to the round's end returns other
    inliers and a plane more than 1e-4 away.  ransac_probability 1 - 2^-20: h_stop on the last position of a round of 16 (15), on
    the first of the next (16: the round ends exactly at the stop) and behind it (17).  ransac_hyp 1, 2, 3, 5: the iteration cap
    ends the loop (iterations == ransac_hyp + 1) in mid-round.  On every frame under every parameter set no point lies within
    1e-5 of the threshold of the oracle's plane: the GPU's refit may differ in the last bits, the inliers may not."""
    stops = {s: _loop(ob, "noisy", ("B", s))[2] for s in cp.B_SEEDS}
    assert {h % 4 for h in stops.values()} == {0, 1, 2, 3}, stops
    visible = {4: 0, 16: 0}
    for s in cp.B_SEEDS:
        cloud, ref = _frame(("B", s))["cloud"], _reference(ob, "noisy", ("B", s))
        best, best_h, h_stop = _loop(ob, "noisy", ("B", s))[:3]
        for width in (4, 16):
            behind = cp.behind_the_stop(cloud, cp.B_THR, SEED, best, h_stop, width)
            if behind:
                end = -(-h_stop // width) * width
                idx, plane = _fixed(ob, "noisy", cloud, end)
                assert not np.array_equal(idx, ref["idx"]) and np.abs(plane - ref["plane"]).max() > 1e-4, (s, width)
                visible[width] += 1
    assert visible[4] >= 2 and visible[16] >= 4, visible
    stops20 = {s: _loop(ob, "noisy_p20", ("B", s))[2] for s in cp.B_SEEDS_P20}
    assert {15, 16, 17} <= set(stops20.values()), stops20
    assert {h % 16 for h in list(stops.values()) + list(stops20.values())} >= {0, 1, 3, 5, 7, 9, 12, 13, 15}
    for hyp in cp.B_HYP_CAPS:
        capped = [_loop(ob, "noisy_hyp%d" % hyp, ("B", s)) for s in cp.B_SEEDS]
        capped = [b for b in capped if b[3] == hyp + 1]
        assert capped and all(b[2] == hyp + 1 + b[4] for b in capped), hyp
        assert any(b[2] % 4 != 0 for b in capped) or hyp == 3, hyp           # (hyp 3: the last position of a round of 4)
    for group in ("noisy", "noisy_p20") + tuple("noisy_hyp%d" % h for h in cp.B_HYP_CAPS):
        for key in _groups()[group][1]:
            cloud, ref = _frame(key)["cloud"], _reference(ob, group, key)
            assert len(cloud) == 300 and 200 < len(ref["idx"]) < 300
            assert _margin(ref, cloud, cp.B_THR) > 1e-5, (group, key)


# ---- C
def test_skips_end_just_before_and_just_behind_the_cap(ob):
    """C: ransac_hyp 1 / 2 (max_skip 10 / 20).  Every sample before hypothesis 10 hyp - 1 (resp. 10 hyp) is degenerate -- three
    points of the exact line, or an index drawn twice, which occurs -- and that hypothesis is valid: the loop has skipped
    10 hyp - 1 samples and finds the plane x = 2 with every point (status OK), or has skipped 10 hyp and gives up (NO_PLANE)."""
    for hyp in (1, 2):
        group = "skips_%d" % hyp
        for h_first, found in ((10 * hyp - 1, True), (10 * hyp, False)):
            key = ("C", hyp, h_first)
            cloud, ref = _frame(key)["cloud"], _reference(ob, group, key)
            best, best_h, h_stop, it, skipped, counts = _loop(ob, group, key)
            assert counts[:h_first] == [None] * h_first and cp.hypothesis(cloud, SEED, h_first, cp.THR_EXACT)[0] == len(cloud)
            assert any(len(set(cp.sample_triple(SEED, h, len(cloud)))) < 3 for h in range(h_first))
            assert any(len(set(cp.sample_triple(SEED, h, len(cloud)))) == 3 for h in range(h_first))
            if found:
                assert (best, best_h, skipped, it) == (len(cloud), h_first, 10 * hyp - 1, 1)
                assert _is_exact(ref["plane"]) and len(ref["idx"]) == len(cloud) and not ref["degenerate"]
            else:
                assert (best, skipped, h_stop, it) == (0, 10 * hyp, 10 * hyp, 0) and ref["no_plane"] and len(ref["idx"]) == 0


# ---- D
def test_few_inliers(ob):
    """D: no plane through three points of the twisted curve comes within 8 thr of a fourth, and neighbours are more than 2 thr
    apart.  Case 1: every hypothesis of the loop's 51 holds exactly its sample -- 3 inliers, no refit, the plane is hypothesis
    0's sample plane to the bit.  Case 2: the first sample without the extra point has it as a fourth inlier; the refit runs on
    exactly those four.  And the three-point cluster."""
    x = cp.twisted_curve()
    worst = np.inf
    for t in itertools.combinations(range(len(x)), 3):
        ok, pl = cp.plane_from_3(*x[list(t)])
        d = cp.plane_dist(pl, x)
        d[list(t)] = np.inf
        worst = min(worst, float(d.min()))
        assert ok
    assert worst > 8 * cp.D_THR
    assert min(np.linalg.norm(x[i] - x[j]) for i in range(len(x)) for j in range(i)) > 2 * cp.D_THR
    fr, ref = _frame(("D", False)), _reference(ob, "few", ("D", False))
    best, best_h, h_stop, it, skipped, counts = _loop(ob, "few", ("D", False))
    assert set(counts) == {3, None} and (best, best_h, it) == (3, 0, 51) and skipped > 0
    assert list(ref["idx"]) == fr["members"] and len(ref["idx"]) == 3
    assert ref["plane"].tobytes() == cp.hypothesis(fr["cloud"], SEED, 0, cp.D_THR)[1].tobytes()
    fr, ref = _frame(("D", True)), _reference(ob, "few", ("D", True))
    best, best_h, h_stop, it, skipped, counts = _loop(ob, "few", ("D", True))
    assert (best, best_h) == (4, fr["h"]) and set(counts) == {3, 4, None} and all(c in (3, None) for c in counts[:best_h])
    assert list(ref["idx"]) == fr["members"] and len(ref["idx"]) == 4
    ref = _reference(ob, "few", ("D3",))
    assert len(_frame(("D3",))["cloud"]) == 3 == len(ref["idx"]) and _is_exact(ref["plane"])
    for key in _groups()["few"][1]:
        assert not _reference(ob, "few", key)["degenerate"]


# ---- E
def test_masks_are_what_they_are_named(ob):
    """E: on every frame the oracle's plane is exact, its inliers are exactly the points of the named K3 mask, the zone is
    (1700, 2300) and the labelled points (black or white) are exactly those of the named K5 mask over the inliers; gray points
    sit ON both ends of the zone wherever there are 601 of them.  Cluster sizes up to 2048 are staged in LDS (the in-place
    compactions of the one launch), 2049 and 4097 read global memory.  The masks have the properties they are named for."""
    m = 4097
    i = np.arange(m)
    for name, prop in (("all", i >= 0), ("drop_first", i > 0), ("drop_last", i < m - 1), ("drop_lane0", i % 64 > 0),
                       ("drop_lane63", i % 64 < 63), ("only_lane0", i % 64 == 0), ("only_lane63", i % 64 == 63), ("after256", i >= 256),
                       ("after1024", i >= 1024), ("after2048", i >= 2048)):
        assert np.array_equal(cp.keep_mask(name, m), prop), name
    edges = cp.keep_mask("chunk_edges", m)
    assert edges[0] and edges[255] and edges[256] and edges[1023] and edges[1024] and not edges[1:255].any()
    sizes = {"staged": set(), "global": set()}
    seen_k3, seen_k5, on_the_ends = set(), set(), 0
    for group in GROUP_NAMES:
        if not group.startswith("masks"):
            continue
        for key in _groups()[group][1]:
            fr, ref = _frame(key), _reference(ob, group, key)
            _, m, k3, k5 = key
            inl, lab = fr["inliers"], fr["labelled"]
            assert len(fr["cloud"]) == m and np.array_equal(inl, cp.keep_mask(k3, m)) and np.array_equal(lab, cp.keep_mask(k5, int(inl.sum())))
            assert _is_exact(ref["plane"]) and np.array_equal(ref["idx"], np.flatnonzero(inl)), key
            assert not ref["degenerate"] and ref["gz"] == cp.E_ZONE and ref["rl"] == (500.0, 3500.0), key
            assert np.array_equal(ref["classes"] != 1, lab), key
            if k3 in cp.E_MINORITY:
                tri = cp.sample_triple(_oparams(ob, group).ransac_seed, 0, m)
                assert inl[list(tri)].all() and _loop(ob, group, key)[1] == 0 and int(inl.sum()) * 8 < m
            inten = ref["board"][:, 3]
            if int((~lab).sum()) >= 601:
                assert (ref["classes"][inten == 1700.0] == 1).all() and (ref["classes"][inten == 2300.0] == 1).all()
                assert (inten == 1700.0).any() and (inten == 2300.0).any()
                on_the_ends += 1
            sizes["staged" if m <= cp.LDS_POINTS else "global"].add(m)
            seen_k3.add(k3)
            seen_k5.add(k5)
    assert sizes["staged"] >= {63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048} and sizes["global"] == {2049, 4097}
    assert seen_k3 == set(cp.E_MASKS) == seen_k5 and on_the_ends >= 20
    # the combinations left out keep fewer than E_MIN_KEPT points: no plane, or no two colours
    assert int(cp.keep_mask("after256", 257).sum()) == int(cp.keep_mask("after1024", 1025).sum()) == int(cp.keep_mask("after2048", 2049).sum()) == 1


# ---- F
def _features(inten, rate=2.5):
    """what a count pattern holds for the rule, from the restated histogram"""
    hist, mean, width, mn = cp.histogram(inten, cp.F_BINS)
    first = {}
    for b in range(cp.F_BINS):
        first.setdefault(int(hist[b]), b)
    edges = {c: width * b + mn for c, b in first.items()}
    out = set()
    if any(width * b + mn == mean for b in range(cp.F_BINS)):
        out.add("mean_on_edge")
    # a bin above the mean that repeats the count of a representative below it, larger than every representative above the mean
    above = [c for c, e in edges.items() if e > mean]
    for b in range(cp.F_BINS):
        c = int(hist[b])
        if width * b + mn > mean and first[c] != b and edges[c] < mean and c > max(above, default=-1):
            out.add("tie_across_mean")
    z = _gray_zone_python(inten, cp.F_BINS, rate)
    if z is not None:
        sides = sorted(edges.items(), reverse=True)
        high = next(c for c, e in sides if e > mean)
        low = next(c for c, e in sides if e < mean)
        if high == 0 or low == 0:
            out.add("empty_bin_side")
        if (np.asarray(inten) == z[0]).any() or (np.asarray(inten) == z[1]).any():
            out.add("point_on_zone_end")
    else:
        out.add("degenerate")
    return out


def test_count_patterns(ob):
    """F: on every pattern and both rates the oracle equals the Python restatement of the std::map walk bit for bit; K3 and K4 of
    the frame are exact (all points inliers of +-(1, 0, 0, -+2), an axis-aligned plane frame).  At most half of the random
    patterns are degenerate.  The patterns written by hand hold what they are named for, and the random ones hold each feature
    many times: the mean exactly on a bin edge, a larger count above the mean that a lower bin already stands for, an empty bin
    as a side's representative, a point exactly on an end of the zone."""
    n_hand = len(cp.F_BY_HAND)
    tally = {}
    for k, inten in enumerate(_patterns()):
        key = ("F", k)
        cloud = _frame(key)["cloud"]
        assert sorted(cloud[:, 3].tolist()) == sorted(np.asarray(inten, np.float64).tolist())
        assert cloud[:, 3].min() == 0.0 and cloud[:, 3].max() == 8.0
        for group in ("exact", "exact_rate1.2"):
            ref = _reference(ob, group, key)
            assert _is_exact(ref["plane"]) and len(ref["idx"]) == len(cloud), key
            assert ref["degenerate"] == (ref["python"] is None), key
            if not ref["degenerate"]:
                assert ref["gz"] == tuple(float(v) for v in ref["python"]), (group, key)
            assert np.array_equal(np.abs(ref["pca"][:3, :3]), [[1, 0, 0], [0, 0, 1], [0, 1, 0]]), key
        for f in _features(inten):
            tally[f] = tally.get(f, 0) + (k >= n_hand)
    print("features among the %d random patterns: %s" % (cp.F_RANDOM, tally))
    assert tally["degenerate"] * 2 <= cp.F_RANDOM
    assert tally["mean_on_edge"] >= 10 and tally["tie_across_mean"] >= 10 and tally["empty_bin_side"] >= 10 and tally["point_on_zone_end"] >= 10
    hand = {name: _features(inten) for name, inten in cp.F_BY_HAND}
    assert {"tie_across_mean"} <= hand["tie_across_mean_other_count"] and "degenerate" not in hand["tie_across_mean_other_count"]
    assert {"tie_across_mean", "degenerate"} <= hand["tie_across_mean_degenerate"]
    assert "empty_bin_side" in hand["empty_bin_is_the_upper_side"]
    assert {"mean_on_edge", "degenerate"} <= hand["mean_on_the_top_bin_edge"]
    assert "mean_on_edge" in hand["mean_on_the_top_bin_edge_ok"] and "degenerate" not in hand["mean_on_the_top_bin_edge_ok"]
    for name in ("half_bins", "half_bins_both_sides"):
        inten = dict(cp.F_BY_HAND)[name]
        hist = cp.histogram(inten, cp.F_BINS)[0]
        assert int((inten == 2.5).sum()) >= 3 and hist[3] == int(((inten == 2.5) | (inten == 3)).sum()) and hist[2] == 0   # 2.5 -> bin 3
        assert hist[5] == int(((inten == 4.5) | (inten == 5)).sum()) and hist[4] == 0                                      # 4.5 -> bin 5
    assert "degenerate" not in hand["half_bins_both_sides"]
    ref = _reference(ob, "exact", ("F", [n for n, _ in cp.F_BY_HAND].index("points_on_both_zone_ends")))
    assert ref["gz"] == (3.0, 4.0) and sorted(ref["board"][:, 3][ref["classes"] == 1].tolist()) == [3.0, 4.0]
    # ... and at the default 100 bins: low = 10, high = 90, the points at 42 and 58 are gray, 41 is black and 59 white
    ref = _reference(ob, "zone_ends", ("Z",))
    inten = ref["board"][:, 3]
    assert ref["gz"] == (42.0, 58.0) and ref["rl"] == (10.0, 90.0)
    assert set(inten[ref["classes"] == 1].tolist()) == {42.0, 50.0, 58.0} and ref["classes"][inten == 41.0] == 0 and ref["classes"][inten == 59.0] == 2


# ================================================================================================================== GPU tests
PATHS = ("wide_1024", "one_launch", "separate_256")
_RUNS = {}


@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(512, 4352, _nparams("exact"))
    e.reserve(4352, 4352)
    yield e
    e.close()


def _extract(est, keys):
    """the frames of `keys` as one ragged batch (click = each frame's first point) -> per frame (its record, everything fetched)"""
    from lidar_camera_calibration_amd import _native as N
    from test_front_end_launches import _everything
    clouds = [_frame(k)["cloud"] for k in keys]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint64)
    clicks = np.stack([c[0, :3] for c in clouds])
    res = est.extract(np.ascontiguousarray(np.concatenate(clouds)), clicks, offsets)
    return [(N.Result.from_buffer_copy(res[f]), _everything(est, res, f, True)) for f in range(len(keys))]


def _run(est, group):
    """The group's frames through the three paths, once per session: {path: per frame (record, everything)}.  The two large-batch
    paths get the group padded to more than 64 frames by repeating its frames; the wide path gets slices of at most 64."""
    if group not in _RUNS:
        keys = list(_groups()[group][1])
        padded = [keys[k % len(keys)] for k in range(max(len(keys), cp.SMALL_BATCH + 1))]
        est.set_params(_nparams(group))
        out = {}
        try:
            for path, separate in (("one_launch", False), ("separate_256", True)):
                est.debug_separate_launches(separate)
                out[path] = _extract(est, padded)
        finally:
            est.debug_separate_launches(False)
        out["wide_1024"] = [r for s in range(0, len(keys), cp.SMALL_BATCH) for r in _extract(est, keys[s:s + cp.SMALL_BATCH])]
        _RUNS[group] = out
    return _RUNS[group]


def _cloud_of(everything, which):
    return np.frombuffer(everything["cloud%d" % which], np.float32).reshape(-1, 4)


def _check_frame(ob, group, key, r, got, path):
    """one frame of one path against the oracle, stage by stage, each stage's reference fed what the GPU fetched before it"""
    from lidar_camera_calibration_amd import _native as N
    fr, ref = _frame(key), _reference(ob, group, key)
    ctx = (group, key, path)
    cloud = fr["cloud"]
    # K1 / K2 hand the whole cloud over, in input order: the oracle's K3 below was fed these very bytes
    assert (r.n_points, r.n_roi, r.n_cluster) == (len(cloud),) * 3, ctx
    assert got["cloud%d" % N.CLOUD_CLUSTER] == cloud.tobytes(), ctx
    # K3
    assert (r.status == N.NO_PLANE) == ref["no_plane"], ctx + (r.status,)
    if ref["no_plane"]:
        return
    assert r.n_plane == len(ref["idx"]), ctx + (r.n_plane, len(ref["idx"]))
    assert got["cloud%d" % N.CLOUD_CHESSBOARD] == ref["board"].tobytes(), ctx
    plane = np.array(r.plane, np.float32)
    if fr.get("exact_plane") or len(ref["idx"]) == 3:
        assert plane.tobytes() == ref["plane"].tobytes(), ctx + (plane, ref["plane"])
    else:
        assert np.abs(plane - ref["plane"]).max() < 1e-6, ctx + (plane, ref["plane"])
    # K4 (the oracle was fed ref["board"], which is what the GPU fetched)
    pca, pca_cloud = np.array(r.pca, np.float32).reshape(4, 4), _cloud_of(got, N.CLOUD_PCA)
    if fr.get("exact_pca"):
        assert pca.tobytes() == ref["pca"].tobytes() and pca_cloud.tobytes() == ref["pca_cloud"].tobytes(), ctx + (pca, ref["pca"])
    else:
        assert np.abs(pca - ref["pca"]).max() < 1e-6 and np.abs(pca_cloud - ref["pca_cloud"]).max() < 1e-6, ctx + (pca, ref["pca"])
    assert np.array_equal(pca_cloud[:, 3], ref["board"][:, 3]), ctx
    # K5 (the intensities are the fetched board's)
    assert (r.status == N.DEGENERATE_HIST) == ref["degenerate"], ctx + (r.status,)
    if ref["degenerate"]:
        return
    assert r.status in (N.OK, N.AMBIGUOUS), ctx + (r.status,)
    assert tuple(r.gray_zone) == ref["gz"] == tuple(float(v) for v in ref["python"]), ctx + (tuple(r.gray_zone), ref["gz"])
    cls = ref["classes"]
    assert (r.n_black, r.n_gray, r.n_white) == (int((cls == 0).sum()), int((cls == 1).sum()), int((cls == 2).sum())), ctx
    assert got["classes"] == cls.tobytes(), ctx
    keep = cls != 1
    yz, lab = got["labelled"]
    assert yz == np.ascontiguousarray(pca_cloud[keep][:, 1:3]).tobytes() and lab == (cls[keep] == 2).astype(np.uint8).tobytes(), ctx


def _check_group(ob, est, group, kinds=None):
    run = _run(est, group)
    keys = _groups()[group][1]
    n = 0
    for path in PATHS:
        for k, key in enumerate(keys):
            if kinds is None or key[0] in kinds:
                _check_frame(ob, group, key, *run[path][k], path)
                n += 1
    assert n >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_three_paths_agree_byte_for_byte(est, group):
    """Per frame, everything test_front_end_launches._everything collects -- the record's fields but grid_ties, the four clouds,
    the labelled points, the classes and, for solved frames, the walk layout (K5w reading the one launch's in-place data) -- is
    identical between K3 at 1024 threads, the one launch and the separate launches at 256 threads; a repeated frame equals its
    first copy."""
    run = _run(est, group)
    n = len(_groups()[group][1])
    for f in range(n):
        a, b, c = (run[path][f][1] for path in PATHS)
        assert a.keys() == b.keys() == c.keys(), (group, f)
        for k in a:
            assert a[k] == b[k] == c[k], (group, _groups()[group][1][f], k)
    for path in ("one_launch", "separate_256"):
        for f in range(n, len(run[path])):
            assert run[path][f][1] == run[path][f % n][1], (group, path, f)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["exact"] + ["fixed_%d" % h for h in (1, 4, 7, 16, 17)])
def test_exact_plane_and_threshold(ob, est, group):
    """A (and F's lattices): r.plane, the inlier cloud, r.pca and the PCA cloud byte-equal to the oracle -- the points AT the
    threshold out, 2^-21 inside it in, winners of both signs -- under the adaptive loop and under 1, 4, 7, 16 and 17 fixed
    hypotheses, whose merge across wavefronts is separate code.  Every sum is exact in any order: multiples of 2^-10 below 4 (the
    in-quadruple's four equal offsets aside), at most 4096 points."""
    _check_group(ob, est, group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["noisy", "noisy_p20"] + ["noisy_hyp%d" % h for h in cp.B_HYP_CAPS])
def test_loop_stops_where_pcl_stops(ob, est, group):
    """B: inlier cloud and n_plane equal to the oracle, r.plane within 1e-6 of it (the bound the suite uses for pca; the GPU
    adds the noisy coordinates in another order) -- with a better hypothesis behind the stop in the same round, the stop on every
    position of a round, and the iteration cap in mid-round."""
    _check_group(ob, est, group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["skips_1", "skips_2"])
def test_skip_cap(ob, est, group):
    """C: the first valid hypothesis just before the skip cap (the plane x = 2, every point) and just behind it (NO_PLANE)."""
    _check_group(ob, est, group)


@pytest.mark.gpu
def test_three_and_four_inliers(ob, est):
    """D: 3 inliers (no refit: the sample plane to the bit; K4 and K5 on three points), 4 (the first refit), a 3-point cluster."""
    _check_group(ob, est, "few")


@pytest.mark.gpu
@pytest.mark.parametrize("group", [g for g in GROUP_NAMES if g.startswith("masks")])
def test_keep_masks_and_sizes(ob, est, group):
    """E: both in-place compactions under every keep mask, at cluster sizes around 64, 256, 1024 and kRansacLdsPoints."""
    _check_group(ob, est, group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["exact", "exact_rate1.2", "zone_ends"])
def test_histogram_rule_on_count_patterns(ob, est, group):
    """F: status, gray_zone (== as doubles: every quantity is exact), counts, labels and classes on every count pattern, at
    gray_rate 2.5 and 1.2 (the inverted zone, black tested first), and with points exactly on both ends of the zone."""
    _check_group(ob, est, group, kinds=("F", "Z"))
