"""CPU tests: the oracle (oracle/ilcc_oracle.c) against everything the reference pins for this path.

The reference ships no tests and cannot be built here (parity unpinned for input->output); what it
does pin are (a) the cost functor's arithmetic (Optimization.h:31-107, hand-derived KATs), (b) the six
output files process_data/pointgrey_lidar_{1..6}.txt and (c) the writer format.  Independent
restatements in numpy/python back the remaining stage checks.
"""
import json
import math
import os

import numpy as np
import pytest

from lidar_camera_calibration_amd import synth


def load_fixture(golden_dir, n):
    path = os.path.join(golden_dir, "pointgrey_lidar_%d.txt" % n)
    return np.loadtxt(path, dtype=np.float64), open(path).read()


# ----------------------------------------------------------------------------- cost functor
def test_functor_known_answers(ob, golden_dir):
    kat = json.load(open(os.path.join(golden_dir, "functor_kat.json")))
    p = ob.default_params()
    assert (p.board_w, p.board_h) == (kat["board_w"], kat["board_h"])
    for row in kat["rows"]:
        r = ob.residual(row["theta_t"], row["y"], row["z"], kat["board_w"], kat["board_h"], kat["grid_length"],
                        row["topleft_white"], row["laser_white"], row["use_oob"])
        assert r == pytest.approx(row["r"], abs=1e-12), row
        c = ob.cost(row["theta_t"], [row["y"]], [row["z"]], [1 if row["laser_white"] else 0], p,
                    row["topleft_white"], row["use_oob"])
        # orc_cost takes the plane-frame coordinates as float32 (m_cloud_PCA is a float cloud)
        assert c == pytest.approx(row["half_rho"], abs=2e-7), row


def test_functor_survey_appendix_c_values(ob):
    # the rows quoted in SURVEY.md Appendix C
    r = lambda *a: ob.residual(*a)
    assert r([0, 0, 0], 0.01, 0.02, 6, 8, 0.15, 0, 1, 1) == 0.0
    assert r([0, 0, 0], 0.01, 0.02, 6, 8, 0.15, 0, 0, 1) == pytest.approx(0.2, abs=1e-12)
    assert r([0, 0, 0], 0.50, 0.10, 6, 8, 0.15, 0, 1, 1) == pytest.approx(3.0 + 2.0 / 3.0, abs=1e-12)
    assert r([0, 0, 0], 0.50, 0.10, 6, 8, 0.15, 0, 1, 0) == 0.0
    assert r([0, 0, 0], 0.50, 0.70, 6, 8, 0.15, 0, 0, 1) == pytest.approx(1.0, abs=1e-12)
    assert r([0.1, 0.02, -0.03], 0.10, 0.20, 6, 8, 0.15, 0, 1, 1) == pytest.approx(0.529670, abs=1e-6)


def test_functor_properties(ob):
    rng = np.random.default_rng(1)
    W, H, g = 6, 8, 0.15
    for _ in range(300):
        y, z = rng.uniform(-0.4, 0.4), rng.uniform(-0.55, 0.55)
        th = [rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)]
        tlw, lw = int(rng.integers(2)), int(rng.integers(2))
        r0 = ob.residual(th, y, z, W, H, g, tlw, lw, 0)
        # phase flip: exactly one of the two phases is a mismatch inside the board
        r1 = ob.residual(th, y, z, W, H, g, 1 - tlw, lw, 0)
        assert (r0 == 0.0) != (r1 == 0.0) or (r0 == 0.0 and r1 == 0.0)
        # 180 degree in-plane turn preserves colours for an even x even board
        r180 = ob.residual([th[0] + math.pi, -th[1], -th[2]], -y, -z, W, H, g, tlw, lw, 0)
        yy = math.cos(th[0]) * y - math.sin(th[0]) * z + th[1]
        zz = math.sin(th[0]) * y + math.cos(th[0]) * z + th[2]
        # rotate the transformed point by pi about the board centre: (yy,zz)->(-yy,-zz)
        ra = ob.residual([0, 0, 0], yy, zz, W, H, g, tlw, lw, 0)
        rb = ob.residual([0, 0, 0], -yy, -zz, W, H, g, tlw, lw, 0)
        assert ra == pytest.approx(rb, abs=1e-9)
        assert r180 >= 0
        # period 2g without the out-of-board term (while staying inside the board)
        if abs(yy) < 0.1 and abs(zz) < 0.25:
            assert ob.residual([0, 0, 0], yy + 2 * g, zz, W, H, g, tlw, lw, 0) == pytest.approx(ra, abs=1e-9)
            assert ob.residual([0, 0, 0], yy, zz - 2 * g, W, H, g, tlw, lw, 0) == pytest.approx(ra, abs=1e-9)


def test_functor_continuous_across_cell_borders(ob):
    W, H, g = 6, 8, 0.15
    eps = 1e-9
    for k in range(-2, 3):
        for lw in (0, 1):
            border = k * g
            a = ob.residual([0, 0, 0], border - eps, 0.031, W, H, g, 0, lw, 1)
            b = ob.residual([0, 0, 0], border + eps, 0.031, W, H, g, 0, lw, 1)
            # a mismatch residual tends to the j-part alone at a border; a match is 0 on one side
            assert min(a, b) == 0.0 or abs(a - b) < 1e-6


def test_functor_jacobian_matches_finite_differences(ob):
    rng = np.random.default_rng(2)
    W, H, g = 6, 8, 0.15
    checked = 0
    for _ in range(400):
        y, z = rng.uniform(-0.6, 0.6), rng.uniform(-0.8, 0.8)
        th = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        tlw, lw = int(rng.integers(2)), int(rng.integers(2))
        r, jac = ob.residual(th, y, z, W, H, g, tlw, lw, 1, want_jac=True)
        h = 1e-7
        ok = True
        num = np.zeros(3)
        for c in range(3):
            tp, tm = th.copy(), th.copy()
            tp[c] += h
            tm[c] -= h
            rp = ob.residual(tp, y, z, W, H, g, tlw, lw, 1)
            rm = ob.residual(tm, y, z, W, H, g, tlw, lw, 1)
            num[c] = (rp - rm) / (2 * h)
            # skip points within h of a kink (cell border / centre line / board edge)
            if abs((rp - r) - (r - rm)) > 1e-9:
                ok = False
        if ok and r > 0:
            assert np.allclose(jac, num, atol=1e-5), (jac, num)
            checked += 1
    assert checked > 100


def _functor_numpy(th, y, z, W, H, g, tlw, lw, oob):
    """VirtualboardError::operator() (Optimization.h:31-107) restated in numpy fp64 on arrays of points, with its Jacobian
    under Jet semantics (floor / ceil carry no derivative): strict bounds, the both-even / both-odd colour rule, the
    `> 0.5` ceil branch and the out-of-board term."""
    c, s = math.cos(th[0]), math.sin(th[0])
    r1 = c * y - s * z + th[1]
    r2 = s * y + c * z + th[2]
    i = (r1 + W * g / 2.0) / g
    j = (r2 + H * g / 2.0) / g
    di = np.stack([(-s * y - c * z) / g, np.full_like(y, 1.0 / g), np.zeros_like(y)], 1)
    dj = np.stack([(c * y - s * z) / g, np.zeros_like(y), np.full_like(y, 1.0 / g)], 1)
    inside = (i > 0) & (i < W) & (j > 0) & (j < H)
    ifl, jfl = np.floor(i), np.floor(j)
    i_even, j_even = ifl == np.floor(ifl / 2) * 2, jfl == np.floor(jfl / 2) * 2
    white = np.where(i_even == j_even, bool(tlw), not tlw)
    miss = inside & (white != bool(lw))
    si_in = np.where(i - ifl > 0.5, -1.0, 1.0)
    sj_in = np.where(j - jfl > 0.5, -1.0, 1.0)
    e_in = np.where(i - ifl > 0.5, np.ceil(i) - i, i - ifl) + np.where(j - jfl > 0.5, np.ceil(j) - j, j - jfl)
    near0_i, near0_j = np.abs(i) < np.abs(i - W), np.abs(j) < np.abs(j - H)
    e_out = np.where(near0_i, np.abs(i), np.abs(i - W)) + np.where(near0_j, np.abs(j), np.abs(j - H))
    si_out = np.where(near0_i, np.where(i < 0, -1.0, 1.0), np.where(i - W < 0, -1.0, 1.0))
    sj_out = np.where(near0_j, np.where(j < 0, -1.0, 1.0), np.where(j - H < 0, -1.0, 1.0))
    out = ~inside & bool(oob)
    r = np.where(miss, e_in, np.where(out, e_out, 0.0))
    si = np.where(miss, si_in, np.where(out, si_out, 0.0))
    sj = np.where(miss, sj_in, np.where(out, sj_out, 0.0))
    return r, si[:, None] * di + sj[:, None] * dj


_BOARDS = [(6, 8), (7, 9), (9, 12), (5, 5), (2, 3), (17, 17)]


@pytest.mark.parametrize("W,H", _BOARDS, ids=["%dx%d" % b for b in _BOARDS])
def test_functor_matches_numpy_restatement_on_other_boards(ob, W, H):
    """orc_residual and its Jacobian == the numpy restatement on even x even, odd x odd, odd x even and square boards, four
    square sizes, both phases, both laser colours, out-of-board term on and off -- points spread over the board, its
    outline and a band around it, a quarter of them snapped to within 1e-9 of a cell border."""
    rng = np.random.default_rng(W * 100 + H)
    n = 60
    for g in (0.08, 0.10, 0.12, 0.25):
        hw, hh = 0.5 * W * g, 0.5 * H * g
        y = rng.uniform(-hw - 2 * g, hw + 2 * g, n)
        z = rng.uniform(-hh - 2 * g, hh + 2 * g, n)
        snap = rng.random(n) < 0.25
        y = np.where(snap, np.round(y / g) * g + rng.choice([-1e-9, 1e-9], n), y)
        for tlw in (0, 1):
            for lw in (0, 1):
                for oob in (0, 1):
                    th = [rng.uniform(-0.2, 0.2), rng.uniform(-g, g), rng.uniform(-g, g)]
                    r_np, j_np = _functor_numpy(th, y, z, W, H, g, tlw, lw, oob)
                    for k in range(n):
                        r, jac = ob.residual(th, y[k], z[k], W, H, g, tlw, lw, oob, want_jac=True)
                        assert r == pytest.approx(r_np[k], abs=1e-9), (W, H, g, tlw, lw, oob, y[k], z[k])
                        assert np.allclose(jac, j_np[k], atol=1e-6), (W, H, g, y[k], z[k], jac, j_np[k])


@pytest.mark.parametrize("W,H", _BOARDS, ids=["%dx%d" % b for b in _BOARDS])
def test_functor_half_turn_rule_follows_the_board_parity(ob, W, H):
    """A half turn about the board centre maps square (a, b) to (W-1-a, H-1-b): the colours are kept when W + H is even
    (even x even, odd x odd) and swapped when it is odd (odd x even) -- i.e. the turned point is scored with the other
    phase.  Exactly one phase is a mismatch inside the board, and the period is 2g."""
    rng = np.random.default_rng(W * 31 + H)
    g = 0.12
    keep = (W + H) % 2 == 0
    n_in = 0
    for _ in range(300):
        yy, zz = rng.uniform(-0.5 * W * g, 0.5 * W * g), rng.uniform(-0.5 * H * g, 0.5 * H * g)
        tlw, lw = int(rng.integers(2)), int(rng.integers(2))
        ra = ob.residual([0, 0, 0], yy, zz, W, H, g, tlw, lw, 0)
        rb = ob.residual([0, 0, 0], -yy, -zz, W, H, g, tlw if keep else 1 - tlw, lw, 0)
        assert ra == pytest.approx(rb, abs=1e-9), (yy, zz, tlw, lw)
        r1 = ob.residual([0, 0, 0], yy, zz, W, H, g, 1 - tlw, lw, 0)
        assert (ra == 0.0) != (r1 == 0.0) or (ra == 0.0 and r1 == 0.0)
        n_in += (ra > 0) != (r1 > 0)
        if W >= 3 and abs(yy) < 0.5 * W * g - 2 * g:
            assert ob.residual([0, 0, 0], yy + 2 * g, zz, W, H, g, tlw, lw, 0) == pytest.approx(ra, abs=1e-9)
    assert n_in > 200


# ----------------------------------------------------------------------------- bundled corner files
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_fixture_files_are_exact_lattices(golden_dir, n):
    pts, _ = load_fixture(golden_dir, n)
    assert pts.shape == (35, 3)
    grid = pts.reshape(5, 7, 3)                      # 5 outer groups x 7 inner
    e_in = np.diff(grid, axis=1).reshape(-1, 3)
    e_out = np.diff(grid, axis=0).reshape(-1, 3)
    assert np.allclose(np.linalg.norm(e_in, axis=1), 0.15, atol=2e-5)
    assert np.allclose(np.linalg.norm(e_out, axis=1), 0.15, atol=2e-5)
    assert abs(float(e_in.mean(0) @ e_out.mean(0))) < 1e-5
    c, eo, ei = synth.FIXTURE_POSES[n - 1]
    assert np.allclose(grid[2, 3], c, atol=1e-5)
    assert np.allclose(e_out.mean(0), eo, atol=2e-5)
    assert np.allclose(e_in.mean(0), ei, atol=2e-5)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_oracle_corner_lattice_reproduces_fixture(ob, golden_dir, n):
    """orc_corners (getPCDcorners) fed with the plane frame of a bundled result must regenerate that
    file: pins ordering (short axis outer), spacing and the two inverse transforms."""
    pts, _ = load_fixture(golden_dir, n)
    grid = pts.reshape(5, 7, 3)
    centre = pts.mean(0)                               # lattice centre = corner (2,3)
    e1 = np.diff(grid, axis=0).reshape(-1, 3).mean(0)  # outer = plane-frame y
    e2 = np.diff(grid, axis=1).reshape(-1, 3).mean(0)  # inner = plane-frame z
    e1 = e1 / np.linalg.norm(e1)
    e2 = e2 - e1 * float(e1 @ e2)
    e2 = e2 / np.linalg.norm(e2)
    e0 = np.cross(e1, e2)
    R = np.stack([e0, e1, e2])
    pca = np.eye(4)
    pca[:3, :3] = R
    pca[:3, 3] = -R @ centre
    p = ob.default_params()
    out = ob.corners(pca.astype(np.float32), [0.0, 0.0, 0.0], p)
    assert out.shape == (35, 3)
    assert np.abs(out - pts).max() < 5e-5      # files carry 6 significant digits
    # and with a non-trivial (theta, ty, tz) folded into the plane frame instead
    th, ty, tz = 0.2, 0.03, -0.05
    T = np.eye(4)
    T[1:3, 1:3] = [[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]
    T[1, 3], T[2, 3] = ty, tz
    pca2 = np.linalg.inv(T) @ pca
    out2 = ob.corners(pca2.astype(np.float32), [th, ty, tz], p)
    assert np.abs(out2 - pts).max() < 1e-4


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_writer_format_regenerates_fixture_text(ob, golden_dir, n):
    pts, text = load_fixture(golden_dir, n)
    lines = []
    for x, y, z in pts.astype(np.float32):
        lines.append(" ".join(ob.format_float(float(v)) for v in (x, y, z)))
    assert "\n".join(lines) + "\n" == text


def test_writer_format_kat(ob):
    assert ob.format_float(np.float32(0.00304251)) == "0.00304251"
    assert ob.format_float(np.float32(0.000851726)) == "0.000851726"
    assert ob.format_float(np.float32(8.51726e-05)) == "8.51726e-05"
    assert ob.format_float(np.float32(2.105)) == "2.105"


# ----------------------------------------------------------------------------- stages vs independent restatements
def test_roi_crop_matches_numpy(ob):
    rng = np.random.default_rng(3)
    p = ob.default_params()
    pts = rng.uniform(-5, 5, (5000, 4)).astype(np.float32)
    pts[10, 0] = np.nan
    pts[11, 2] = np.inf
    click = np.array([0.3, -0.2, 0.1], dtype=np.float32)
    lo = (click.astype(np.float64) - np.array(p.roi_half[:])).astype(np.float32)
    hi = (click.astype(np.float64) + np.array(p.roi_half[:])).astype(np.float32)
    pts[12, 0] = hi[0]                                   # limits are inclusive
    pts[12, 1:3] = click[1:3]
    keep = np.isfinite(pts[:, :3]).all(1)
    for a in range(3):
        keep &= ~((pts[:, a] < lo[a]) | (pts[:, a] > hi[a]))
    idx = ob.roi_crop(pts, click, p)
    assert np.array_equal(idx, np.nonzero(keep)[0])
    assert 12 in idx and 10 not in idx and 11 not in idx
    assert len(ob.roi_crop(pts[:0], click, p)) == 0


def _components(points, tol2):
    n = len(points)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    p32 = points[:, :3].astype(np.float32)
    for i in range(n):
        d = p32 - p32[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for j in np.nonzero(d2 < tol2)[0]:
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)])


def test_cluster_matches_bruteforce_components(ob):
    rng = np.random.default_rng(4)
    p = ob.default_params()
    p.cluster_min = 5
    blobs = [rng.normal(c, 0.05, (n, 3)) for c, n in (((0, 0, 0), 120), ((1, 0, 0), 60), ((0, 1.5, 0), 8),
                                                        ((3, 3, 3), 3))]
    pts = np.concatenate(blobs).astype(np.float32)
    pts = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], 1)
    rng.shuffle(pts)
    tol2 = np.float32(p.cluster_tol * p.cluster_tol)
    labels = _components(pts, tol2)
    click = np.array([1.0, 0.02, 0.0], np.float32)
    idx, lab = ob.cluster(pts, click, p)
    assert np.array_equal(lab, labels)
    nn = int(np.argmin(((pts[:, :3] - click) ** 2).sum(1)))
    assert np.array_equal(idx, np.nonzero(labels == labels[nn])[0])
    # NN lands in a too-small component -> falls back to the largest valid cluster (index 0)
    click2 = np.array([3.0, 3.0, 3.0], np.float32)
    idx2, _ = ob.cluster(pts, click2, p)
    sizes = np.bincount(labels)
    assert len(idx2) == sizes.max()
    # nothing admissible
    p.cluster_min = 1000
    idx3, _ = ob.cluster(pts, click, p)
    assert len(idx3) == 0


def test_ransac_plane_recovers_plane_and_refits(ob):
    rng = np.random.default_rng(5)
    p = ob.default_params()
    n = np.array([0.6, -0.5, 0.62])
    n /= np.linalg.norm(n)
    basis = np.linalg.svd(n[None])[2][1:]
    inl = (rng.uniform(-0.6, 0.6, (800, 2)) @ basis) + 2.5 * n + rng.normal(0, 0.008, (800, 1)) * n
    out = rng.uniform(-1, 1, (60, 3)) + 2.5 * n
    pts = np.concatenate([inl, out]).astype(np.float32)
    pts = np.concatenate([pts, np.ones((len(pts), 1), np.float32)], 1)
    idx, pl = ob.ransac_plane(pts, p)
    d = np.abs(pts[:, :3].astype(np.float64) @ pl[:3] + pl[3])
    assert np.array_equal(idx, np.nonzero(d.astype(np.float32) < np.float32(0.03))[0]) or \
        abs(len(idx) - int((d < 0.03).sum())) <= 2
    assert abs(abs(float(pl[:3] @ n)) - 1) < 1e-4
    assert len(idx) >= 800
    assert len(ob.ransac_plane(pts[:2], p)[0]) == 0


def _gray_zone_python(intensity, bins, rate):
    """calHist/get_gray_zone restated with a python dict standing in for std::map<count, bin>."""
    d = np.sort(np.asarray(intensity, dtype=np.float64))
    mn, mx = d[0], d[-1]
    factor = bins / (mx - mn)
    hist = [0] * (bins + 1)
    for v in d:
        b = int(math.floor((v - mn) * factor + 0.5))        # round half away from zero (v - mn >= 0)
        hist[b] += 1
    mean = float(np.add.reduce(d)) if False else sum(d.tolist()) / len(d)
    width = (mx - mn) / bins
    m = {}
    for i in range(bins):
        m.setdefault(hist[i], i)
    low = high = None
    for count in sorted(m, reverse=True):
        edge = width * m[count] + mn
        if edge > mean and high is None:
            high = edge
        if edge < mean and low is None:
            low = edge
        if low is not None and high is not None:
            break
    if low is None or high is None:
        return None
    return ((rate - 1) * low + high) / rate, (low + (rate - 1) * high) / rate


def test_gray_zone_matches_python_restatement(ob):
    rng = np.random.default_rng(6)
    p = ob.default_params()
    for trial in range(20):
        n = int(rng.integers(900, 3000))
        inten = np.concatenate([rng.normal(12, 4, n // 2), rng.normal(100, 8, n - n // 2),
                                rng.uniform(12, 100, n // 10)]).clip(0, 255).astype(np.float32)
        st, rl, gz = ob.gray_zone(inten, p)
        ref = _gray_zone_python(inten, p.hist_bins, p.gray_rate)
        if ref is None:
            assert st == 4
        else:
            assert st == 0
            assert gz[0] == pytest.approx(ref[0], rel=1e-12) and gz[1] == pytest.approx(ref[1], rel=1e-12)
            assert gz[0] == pytest.approx(0.6 * rl[0] + 0.4 * rl[1], rel=1e-12)
    assert ob.gray_zone(np.full(10, 7.0, np.float32), p)[0] == 4        # max == min: reference divides by 0


def test_plane_frame_is_rigid_and_ordered(ob):
    rng = np.random.default_rng(7)
    p = ob.default_params()
    pose = synth.pose_from_fixture(3)
    uv = rng.uniform(-1, 1, (1500, 2)) * [0.45, 0.6]
    pts = pose.centre + uv[:, :1] * pose.u + uv[:, 1:] * pose.v + rng.normal(0, 0.005, (1500, 1)) * pose.normal
    cloud = np.concatenate([pts, rng.uniform(0, 100, (1500, 1))], 1).astype(np.float32)
    st, pca, out = ob.plane_frame(cloud, p)
    assert st == 0
    R = pca[:3, :3].astype(np.float64)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0
    assert np.allclose(out[:, 3], cloud[:, 3])
    v = out[:, :3].astype(np.float64).var(0)
    assert v[0] < v[1] < v[2]                               # x normal, y mid, z max variance
    assert abs(out[:, :3].mean(0)).max() < 1e-5
    assert float(R[0] @ pose.centre) < 0                    # normal towards the sensor
    assert abs(abs(R[1] @ pose.u) - 1) < 2e-2 and abs(abs(R[2] @ pose.v) - 1) < 2e-2
    p.accum_float = 1
    st2, pca2, out2 = ob.plane_frame(cloud, p)
    assert np.abs(out2[:, :3] - out[:, :3]).max() < 1e-4    # float vs double accumulation


def test_grid_search_selection_rule(ob):
    p = ob.default_params()
    p.n_th, p.n_ty, p.n_tz = 5, 6, 6
    p.th_min, p.th_step = -0.02, 0.01
    p.ty_min = p.tz_min = -0.03
    p.ty_step = p.tz_step = 0.01
    # no points: every candidate costs 0 -> nearest-to-zero candidate, phase 0
    flat, c, vol = ob.grid_search(np.zeros(0), np.zeros(0), np.zeros(0, np.int8), p, 1, want_volume=True)
    assert c == 0.0 and np.all(vol == 0.0)
    assert flat == ((2 * 6 + 3) * 6 + 3) * 2
    # volume equals orc_cost candidate by candidate
    rng = np.random.default_rng(8)
    y, z = rng.uniform(-0.4, 0.4, 50).astype(np.float32), rng.uniform(-0.55, 0.55, 50).astype(np.float32)
    lab = rng.integers(0, 2, 50).astype(np.int8)
    flat, c, vol = ob.grid_search(y, z, lab, p, 1, want_volume=True)
    for k, a, b, ph in ((0, 0, 0, 0), (4, 5, 5, 1), (2, 3, 1, 1)):
        th = [p.th_min + k * p.th_step, p.ty_min + a * p.ty_step, p.tz_min + b * p.tz_step]
        assert vol[((k * 6 + a) * 6 + b) * 2 + ph] == pytest.approx(ob.cost(th, y, z, lab, p, ph, 1), abs=1e-12)
    assert c == vol.min() and vol[flat] == c


def test_local_solver_reaches_zero_cost_on_clean_board(ob):
    """Noise-free checker samples, displaced by a known small motion: pass A+B must return to a
    zero-cost pose (every labelled point on a square of its own colour)."""
    p = ob.default_params()
    g = p.grid_length
    ys, zs = np.meshgrid(np.arange(-0.42, 0.43, 0.03), np.arange(-0.57, 0.58, 0.03), indexing="ij")
    y, z = ys.ravel(), zs.ravel()
    i = np.floor((y + 3 * g) / g).astype(int)
    j = np.floor((z + 4 * g) / g).astype(int)
    fi = (y + 3 * g) / g - i
    fj = (z + 4 * g) / g - j
    keep = (np.minimum(fi, 1 - fi) > 0.12) & (np.minimum(fj, 1 - fj) > 0.12)   # a gray-zone-like margin
    white = ((i + j) % 2 == 1)            # topleftWhite = False
    th0, ty0, tz0 = 0.03, 0.012, -0.02    # true board -> cloud motion
    yy = math.cos(-th0) * (y - ty0) - math.sin(-th0) * (z - tz0)
    zz = math.sin(-th0) * (y - ty0) + math.cos(-th0) * (z - tz0)
    pts = np.stack([np.zeros_like(yy), yy, zz, np.where(white, 100.0, 10.0)], 1)[keep].astype(np.float32)
    t, cost, it = ob.get_theta_t(pts, [40.0, 60.0], p, 0, 1)
    t, cost_b, it_b = ob.get_theta_t(pts, [40.0, 60.0], p, 0, 0, t)
    assert cost < 1e-12 and cost_b < 1e-12
    # any pose inside the zero-cost plateau (margin 0.12 cell = 18 mm) is a fixed point of the solver
    assert abs(t[0] - th0) < 0.03 and abs(t[1] - ty0) < 0.018 and abs(t[2] - tz0) < 0.018
    assert it <= 50


# ----------------------------------------------------------------------------- GRID-mode refinement (specification)
@pytest.mark.parametrize("bins", [1, 7, 4096])
@pytest.mark.parametrize("rate", [1.2, 6.0])
def test_gray_zone_matches_python_restatement_at_other_bins_and_rates(ob, bins, rate):
    """calHist / get_gray_zone away from 100 bins and rate 2.5, on continuous and on integer (VLP-16 reflectivity)
    intensities: one bin never finds both peaks (ILCC_DEGENERATE_HIST); 7 and 4096 bins follow the restatement."""
    rng = np.random.default_rng(bins * 10 + int(rate * 10))
    p = ob.default_params()
    p.hist_bins, p.gray_rate = bins, rate
    n_ok = 0
    for trial in range(12):
        n = int(rng.integers(900, 3000))
        inten = np.concatenate([rng.normal(12, 4, n // 2), rng.normal(100, 8, n - n // 2),
                                rng.uniform(12, 100, n // 10)]).clip(0, 255)
        if trial % 2:
            inten = np.round(inten)
        inten = inten.astype(np.float32)
        st, rl, gz = ob.gray_zone(inten, p)
        ref = _gray_zone_python(inten, bins, rate)
        if ref is None:
            assert st == 4
        else:
            assert st == 0
            n_ok += 1
            assert gz[0] == pytest.approx(ref[0], rel=1e-12) and gz[1] == pytest.approx(ref[1], rel=1e-12)
            assert gz[0] == pytest.approx(((rate - 1) * rl[0] + rl[1]) / rate, rel=1e-12)
            assert gz[1] == pytest.approx((rl[0] + (rate - 1) * rl[1]) / rate, rel=1e-12)
    if bins == 1:
        assert n_ok == 0
    else:
        assert n_ok >= 6


def _clean_board_points(p, th0, ty0, tz0, margin=0.12, step=0.03):
    """noise-free checker samples (topleftWhite = False) moved by a known board -> cloud motion"""
    g = p.grid_length
    ys, zs = np.meshgrid(np.arange(-0.42, 0.43, step), np.arange(-0.57, 0.58, step), indexing="ij")
    y, z = ys.ravel(), zs.ravel()
    i = np.floor((y + 3 * g) / g).astype(int)
    j = np.floor((z + 4 * g) / g).astype(int)
    fi = (y + 3 * g) / g - i
    fj = (z + 4 * g) / g - j
    keep = (np.minimum(fi, 1 - fi) > margin) & (np.minimum(fj, 1 - fj) > margin)
    white = ((i + j) % 2 == 1)
    yy = math.cos(-th0) * (y - ty0) - math.sin(-th0) * (z - tz0)
    zz = math.sin(-th0) * (y - ty0) + math.cos(-th0) * (z - tz0)
    return yy[keep].astype(np.float32), zz[keep].astype(np.float32), white[keep].astype(np.int8)


def test_fixed_point_cost_is_the_cost_and_ignores_summation_order(ob):
    """orc_cost_q = sum of per-point terms rounded to 2^-40: within m/2 quanta of orc_cost, and -- being an
    integer sum -- bit-identical under any permutation of the points (what lets a parallel reduction on the GPU
    take exactly the oracle's decisions)."""
    p = ob.default_params()
    rng = np.random.default_rng(11)
    m = 1500
    y, z = rng.uniform(-0.5, 0.5, m).astype(np.float32), rng.uniform(-0.7, 0.7, m).astype(np.float32)
    lab = rng.integers(0, 2, m).astype(np.int8)
    for th in ([0.0, 0.0, 0.0], [0.11, -0.031, 0.052], [-0.2, 0.07, -0.09]):
        for ph in (0, 1):
            for oob in (0, 1):
                cq = ob.cost_q(th, y, z, lab, p, ph, oob)
                assert abs(cq / ob.COST_Q_ONE - ob.cost(th, y, z, lab, p, ph, oob)) <= 0.5 * m / ob.COST_Q_ONE + 1e-12
                perm = rng.permutation(m)
                assert ob.cost_q(th, y[perm], z[perm], lab[perm], p, ph, oob) == cq
    assert ob.cost_q([0.0, 0.0, 0.0], y[:0], z[:0], lab[:0], p, 0, 1) == 0


@pytest.mark.parametrize("W,H,g", [(7, 9, 0.12), (9, 12, 0.10), (5, 5, 0.15), (2, 3, 0.25), (17, 17, 0.08)])
@pytest.mark.parametrize("delta", [0.02, 0.5, 5.0])
def test_fixed_point_cost_is_the_cost_on_other_boards_and_deltas(ob, W, H, g, delta):
    """orc_cost_q on other boards and Huber deltas: within m/2 quanta of orc_cost (the fp64 functor with Ceres' sqrt-form
    Huber), order-independent, and -- for the out-of-board term to matter -- points reach past the board's outline."""
    p = ob.default_params()
    p.board_w, p.board_h, p.grid_length, p.huber_delta = W, H, g, delta
    rng = np.random.default_rng(W * H + int(delta * 100))
    m = 1200
    y = rng.uniform(-0.6 * W * g, 0.6 * W * g, m).astype(np.float32)
    z = rng.uniform(-0.6 * H * g, 0.6 * H * g, m).astype(np.float32)
    lab = rng.integers(0, 2, m).astype(np.int8)
    for th in ([0.0, 0.0, 0.0], [0.11, -0.031, 0.052], [-0.2, 0.07, -0.09]):
        for ph in (0, 1):
            for oob in (0, 1):
                cq = ob.cost_q(th, y, z, lab, p, ph, oob)
                c = ob.cost(th, y, z, lab, p, ph, oob)
                assert c > 0
                assert abs(cq / ob.COST_Q_ONE - c) <= 0.5 * m / ob.COST_Q_ONE + 1e-12 * max(1.0, c)
                perm = rng.permutation(m)
                assert ob.cost_q(th, y[perm], z[perm], lab[perm], p, ph, oob) == cq


def _neighbour_costs(ob, p, y, z, lab, lat, phase, stride=1):
    out = {}
    for dk in (-1, 0, 1):
        for da in (-1, 0, 1):
            for db in (-1, 0, 1):
                q = [lat[0] + dk * stride, lat[1] + da * stride, lat[2] + db * stride]
                out[(dk, da, db)] = ob.cost_q(ob.lattice_point(p, q), y, z, lab, p, phase, 1)
    return out


def test_pattern_refine_is_monotone_and_ends_in_a_lattice_minimum(ob):
    p = ob.default_params()
    rng = np.random.default_rng(5)
    y, z, lab = _clean_board_points(p, 0.031, 0.0131, -0.0212, margin=0.02)
    y = (y + rng.normal(0, 0.004, len(y))).astype(np.float32)     # noise: a strict minimum instead of a plateau
    z = (z + rng.normal(0, 0.004, len(z))).astype(np.float32)
    flip = rng.random(len(lab)) < 0.03
    lab = np.where(flip, 1 - lab, lab).astype(np.int8)
    for start in ([30 * 16, 20 * 16, 20 * 16], [34 * 16, 22 * 16, 17 * 16], [27 * 16, 19 * 16, 18 * 16]):
        c0 = ob.cost_q(ob.lattice_point(p, start), y, z, lab, p, 0, 1)
        lat, ph, c, alt, rounds, hops = ob.pattern_refine(y, z, lab, p, start, 0)
        assert c <= c0 and ph == 0 and hops == 0 and 0 < rounds <= p.refine_max_rounds
        assert c == ob.cost_q(ob.lattice_point(p, lat), y, z, lab, p, ph, 1)
        nb = _neighbour_costs(ob, p, y, z, lab, lat, ph)
        assert min(nb.values()) == nb[(0, 0, 0)] == c            # no lattice neighbour is cheaper
        # (where inside the flat bottom of the basin it ends is not pinned here: samples away from the square
        # borders cost nothing anywhere on the plateau; accuracy is measured on synthetic frames below)
        th = ob.lattice_point(p, lat)
        assert abs(th[0] - 0.031) < 0.03 and abs(th[1] - 0.0131) < 0.03 and abs(th[2] + 0.0212) < 0.03, th
        assert alt > c                                            # the neighbouring basins are worse: unambiguous
    # refine_div = 0: the start is kept, only the basin check runs
    p0 = ob.default_params()
    p0.refine_div = 0
    lat, ph, c, alt, rounds, hops = ob.pattern_refine(y, z, lab, p0, [30, 20, 20], 0)
    assert list(lat) == [30, 20, 20] and rounds == 0 and hops == 0
    assert c == ob.cost_q(ob.lattice_point(p0, [30, 20, 20]), y, z, lab, p0, 0, 1)


def test_pattern_refine_hops_to_the_neighbouring_basin(ob):
    """Start one square off along y (the colour phase is then the opposite one): the pattern search cannot cross
    the ridge, the basin check finds the cheaper neighbour, adopts it (phase flipped back) and refines there."""
    p = ob.default_params()
    y, z, lab = _clean_board_points(p, 0.0, 0.0, 0.0)
    true_lat = [30 * 16, 20 * 16, 20 * 16]
    assert ob.cost_q(ob.lattice_point(p, true_lat), y, z, lab, p, 0, 1) == 0
    off = [30 * 16, 40 * 16, 20 * 16]          # ty = +g: 20 grid steps = one square
    lat, ph, c, alt, rounds, hops = ob.pattern_refine(y, z, lab, p, off, 1)
    assert hops == 1 and ph == 0 and c == 0 and alt > 0
    th = ob.lattice_point(p, lat)
    assert abs(th[1]) < 0.04 and abs(th[2]) < 0.04 and abs(th[0]) < 0.06     # back in the true basin (cost 0 = on its plateau)
    # a board seen only through its middle (no sample within a square of the border along z): a shift by one
    # square along z with the colours swapped costs exactly the same -> margin 0 -> the frame is flagged
    mid = np.abs(z) < 0.29
    lat2, ph2, c2, alt2, _, hops2 = ob.pattern_refine(y[mid], z[mid], lab[mid], p, true_lat, 0)
    assert c2 == 0 and alt2 == 0 and hops2 == 0


def test_grid_mode_extract_flags_ambiguity_and_is_monotone(ob):
    """orc_extract in GRID mode on a small grid: sel_cost <= grid cost (the refinement never raises the
    with-OOB cost), theta_t on the lattice, status / margin consistent."""
    p = ob.default_params()
    p.solver = ob.SOLVER_GRID
    p.n_th, p.th_min, p.th_step = 9, -4 * p.th_step, p.th_step          # +-2 deg: keeps the exhaustive oracle fast
    p.n_ty = p.n_tz = 20
    p.ty_step = p.tz_step = 0.015
    pose = synth.pose_from_fixture(0)
    cloud = synth.make_frame(synth.vlp16(), synth.Board(), pose, 0xC0FFEE)
    click = synth.make_click(pose, 0xC0FFEE)
    r = ob.extract(cloud, click, p)
    assert r.status in (ob.OK, ob.AMBIGUOUS) and r.n_corners == 35
    assert r.sel_cost <= r.grid_cost + 1e-15 and r.cost_a == r.sel_cost
    assert (r.status == ob.AMBIGUOUS) == (r.basin_margin < p.ambiguity_eps)
    assert r.basin_margin == pytest.approx((r.cost_b - r.sel_cost) / r.sel_cost, rel=1e-9)
    div = p.refine_div
    for k, (lo, st) in enumerate(((p.th_min, p.th_step), (p.ty_min, p.ty_step), (p.tz_min, p.tz_step))):
        q = (r.theta_t[k] - lo) / (st / div)
        assert abs(q - round(q)) < 1e-6
    assert 0 < r.iters_a <= 3 * p.refine_max_rounds and 0 <= r.iters_b <= 2
    gt = synth.true_corners(pose, synth.Board())
    assert synth.corner_error(ob.result_corners(r), gt, synth.Board()) < 0.02


# ----------------------------------------------------------------------------- closed loop at the fixture poses
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_config1_synthetic_frame_at_fixture_pose(ob, golden_dir, n, tmp_path):
    """BASELINE config 1/3 on the CPU path: synthetic VLP-16 frame with the board where bundled file n
    has it; reference-faithful trajectory (both phases) -> corners within the method's accuracy on
    16-ring data (cm-level in the ring-sparse direction; measured 1.9-5.3 mm at these poses)."""
    pts, _ = load_fixture(golden_dir, n)
    board = synth.Board()
    pose = synth.pose_from_fixture(n - 1)
    cloud = synth.make_frame(synth.vlp16(), board, pose, 0xC0FFEE + n - 1)
    assert cloud.shape == (28800, 4)
    click = synth.make_click(pose, 0xC0FFEE + n - 1)
    p = ob.default_params()
    p.solver = ob.SOLVER_REFERENCE_LOCAL
    res = ob.extract(cloud, click, p)
    assert res.status == 0 and res.n_corners == 35
    err = synth.corner_error(ob.result_corners(res), pts, board)
    assert err < 0.010, err


# ----------------------------------------------------------------------------------------------
# Solver pin: the reference ships the inputs (process_data/pointgrey{N}.txt, pointgrey_lidar_{N}.txt)
# AND the output (config/pointgrey.bin) of one Ceres solve made with exactly the options of the
# path's board fit (src/Optimization.cpp:55-66 vs :146-157).  The oracle's trust-region code, run on
# that 6-parameter problem, must land on the shipped matrix.
def _shipped_pairs(GOLD):
    cam = (1061.37439737547, 980.706836288949, 1061.02435228316, 601.685030610243)   # fx cx fy cy (pointgrey.yaml K)
    w, h = 7, 5

    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]),
                "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])}[axis]

    rough = rot("y", -1.57) @ rot("x", 1.57)                      # test/calib_lidar_cam.cpp:56-58
    p3_all, p2_all = [], []
    for i in range(1, 7):
        raw = np.loadtxt(os.path.join(GOLD, f"pointgrey{i}.txt"))
        assert raw.shape in ((14, 5), (10, 7))
        X, Y = raw[:len(raw) // 2], raw[len(raw) // 2:]
        if len(X) != h:                                             # column-major read (ImageCornersEst.cpp:262-266)
            X, Y = X.T, Y.T
        p2 = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        # read_lidar_corners parses into float and widens (src/ImageCornersEst.cpp:290-292)
        p3 = np.loadtxt(os.path.join(GOLD, f"pointgrey_lidar_{i}.txt"), dtype=np.float32).astype(np.float64) @ rough.T
        # check_order_lidar / check_order_cam (src/ImageCornersEst.cpp:430-488)
        g3, g2 = p3.reshape(h, w, 3), p2.reshape(h, w, 2)
        if p3[0, 1] > p3[w + 1, 1]:
            g3 = g3[::-1]
        if p3[0, 0] > p3[1, 0]:
            g3 = g3[:, ::-1]
        if p2[0, 1] > p2[w + 1, 1]:
            g2 = g2[::-1]
        if p2[0, 0] > p2[1, 0]:
            g2 = g2[:, ::-1]
        p3_all.append(g3.reshape(-1, 3))
        p2_all.append(g2.reshape(-1, 2))
    return np.concatenate(p3_all), np.concatenate(p2_all), cam, rough


def test_solver_pinned_by_shipped_extrinsic(ob, golden_dir):
    from scipy.spatial.transform import Rotation
    GOLD = golden_dir
    p3, p2, cam, rough = _shipped_pairs(GOLD)
    r, t, cost, it = ob.solve_pose_3d2d(p3, p2, cam)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(r).as_matrix()
    T[:3, 3] = t
    R4 = np.eye(4)
    R4[:3, :3] = rough
    T = T @ R4
    ref = np.fromfile(os.path.join(GOLD, "pointgrey.bin"), dtype=np.float64).reshape(4, 4, order="F")
    dev = np.abs(T - ref).max()
    print("iterations", it, "cost", cost, "max |T - shipped|", dev)
    assert 0 < it <= 50
    assert dev < 1e-12     # measured 4e-16: the shipped matrix is this solve, to the last bit or two


# ----------------------------------------------------------------------------- sanitizers
def test_oracle_runs_clean_under_asan_and_ubsan(ob, tmp_path):
    """`make -C oracle sanitize` builds the oracle with -fsanitize=address,undefined (-fno-sanitize-recover): the whole
    path (both solver modes, the online caller) on a synthetic frame, on an empty ROI and on a frame with non-finite
    points must finish with exit status 0, and print what the regular build computes."""
    import subprocess
    odir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.check_call(["make", "-C", odir, "-s", "sanitize"])
    pose = synth.pose_from_fixture(3)
    cloud = synth.make_frame(synth.vlp16(), synth.Board(), pose, 99)
    click = synth.make_click(pose, 99)
    nan_cloud = cloud.copy()
    nan_cloud[::53, 1] = np.nan
    nan_cloud[7::101, 0] = np.inf
    cases = [(cloud, click, 0, ()), (cloud, click, 1, (9, 10, 10)), (nan_cloud, click, 0, ()),
             (cloud, np.array([40, 40, 40], np.float32), 0, ()), (cloud[:0], click, 1, (9, 10, 10))]
    for k, (c, ck, solver, grid) in enumerate(cases):
        raw = tmp_path / ("f%d.bin" % k)
        np.ascontiguousarray(c, dtype=np.float32).tofile(raw)
        r = subprocess.run([os.path.join(odir, "selftest_san"), str(raw), *("%.9g" % v for v in ck), str(solver), *map(str, grid)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (k, r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        head = list(map(int, r.stdout.splitlines()[0].split()))
        p = ob.default_params()
        p.solver = solver
        if grid:
            p.n_th, p.n_ty, p.n_tz = grid
            p.th_min = -0.5 * (p.n_th - 1) * p.th_step
        if len(c):
            want = ob.extract(c, ck, p)
            assert head[:5] == [want.status, want.n_roi, want.n_cluster, want.n_plane, want.n_corners], k
            got = np.array([list(map(float, ln.split())) for ln in r.stdout.splitlines()[1:1 + head[4]]], dtype=np.float32)
            assert np.array_equal(got.reshape(-1, 3), ob.result_corners(want))
