"""Camera chessboard corners (include/ilcc_image_corners.h): K10 against the fp64 numpy restatement
(tests/cbdetect_ref.py), the reference's own input -> output pin (its six undistorted images, cropped
in tests/golden/pointgrey<i>_crop.npz, and the six corner files its detector wrote from them), the end
to end calibration from detected files, synthetic boards, and the host structure recovery."""
import ctypes as C
import math
import os
import re
import shutil

import numpy as np
import pytest

import cbdetect_ref as R
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import calib
from lidar_camera_calibration_amd import image_corners as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CAM = (1061.37439737547, 980.706836288949, 1061.02435228316, 601.685030610243)   # fx cx fy cy, pointgrey.yaml


def _crop(i):
    z = np.load(os.path.join(GOLD, f"pointgrey{i}_crop.npz"))
    return z["image"], z["origin"]


def _shipped_board(i):
    raw = np.loadtxt(os.path.join(GOLD, f"pointgrey{i}.txt"))
    X, Y = raw[:len(raw) // 2], raw[len(raw) // 2:]
    return np.stack([X - 1, Y - 1], -1)


# ------------------------------------------------------------------------------------------ CPU

def test_exports_match_header():
    hdr = open(os.path.join(ROOT, "include", "ilcc_image_corners.h")).read()
    declared = re.findall(r"^int32_t (ilcc_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(IC.IMAGE_CORNERS_EXPORTS)
    L = IC.lib()
    for s in IC.IMAGE_CORNERS_EXPORTS:
        assert hasattr(L, s), s
    assert C.sizeof(IC.ImageCorner) == 56


@pytest.mark.parametrize("i", range(1, 7))
def test_writer_reproduces_shipped_files(tmp_path, i):
    src = os.path.join(GOLD, f"pointgrey{i}.txt")
    out = tmp_path / f"pointgrey{i}.txt"
    IC.save_cam_corners(str(out), _shipped_board(i))
    assert out.read_bytes() == open(src, "rb").read()


def test_crops_hold_the_full_image_range():
    for i in range(1, 7):
        img, org = _crop(i)
        assert img.dtype == np.uint8 and img.min() == 0 and img.max() == 255
        b = _shipped_board(i)
        assert (b[..., 0] - org[0]).min() > 100 and (b[..., 1] - org[1]).min() > 100
        assert (b[..., 0] - org[0]).max() < img.shape[1] - 100 and (b[..., 1] - org[1]).max() < img.shape[0] - 100


def test_template_weights_and_quadrants():
    for a1, a2, r in R.TEMPLATE_PROPS:
        ks = R.template(a1, a2, r)
        for k in ks:
            assert abs(k.sum() - 1) < 1e-12 and k.shape == (2 * r + 1, 2 * r + 1)
        occupied = sum((k > 0).astype(int) for k in ks)
        assert occupied.max() == 1                       # quadrants are disjoint
        if a1 == 0:
            # axis-aligned: the centre row and column lie in the +-0.1 band, everything else is used
            assert not occupied[r, :].any() and not occupied[:, r].any()
            assert occupied.sum() == (2 * r) ** 2
        else:
            # diagonal: both diagonals lie in the band
            d = np.arange(2 * r + 1)
            assert not occupied[d, d].any() and not occupied[d, 2 * r - d].any()
        # the four quadrants are one rotation apart: equal sizes
        assert len({int((k > 0).sum()) for k in ks}) == 1
    # (0, pi/2), radius 4: a1 is the up-left quadrant (s1 = dv <= -0.1, s2 = -du <= -0.1)
    a1 = R.template(0, math.pi / 2, 4)[0]
    assert a1[0, 8] > 0 and a1[8, 0] == 0 and a1[0, 0] == 0


def test_nms_block_rules():
    L = np.zeros((40, 40))
    L[11, 12] = 0.5            # 1-based (u, v) = (13, 12): inside block (13, 9..)... a clear maximum
    L[25, 25] = 0.02           # below tau
    L[20, 9] = 0.3             # a maximum with a larger neighbour outside its block
    L[20, 11] = 0.4
    got, vals = R.nms(L)
    assert (13, 12) in got and (26, 26) not in got
    assert (10, 21) not in got and (12, 21) in got
    assert all(v >= R.NMS_TAU for v in vals)
    # equal values: the block's first scanned pixel wins and a tie outside the block does not fail it
    L2 = np.zeros((40, 40))
    L2[12, 12] = L2[12, 13] = 0.1
    got2, _ = R.nms(L2)
    assert got2 == [(13, 13), (14, 13)] or got2 == [(13, 13)]
    assert (13, 13) in got2
    # scan order: u outer, v inner
    L3 = np.zeros((40, 40))
    L3[20, 9] = L3[9, 20] = 0.2
    got3, _ = R.nms(L3)
    assert got3 == [(10, 21), (21, 10)]


def test_mean_shift_modes():
    modes, hs = R.mean_shift_modes(np.full(32, 3.0))
    assert modes == []                                   # flat: no modes (every bin within 1e-5)
    h = np.zeros(32)
    h[4], h[20] = 10.0, 6.0
    modes, _ = R.mean_shift_modes(h)
    assert [m[0] for m in modes] == [5, 21] and modes[0][1] > modes[1][1]
    # one bin differing by more than 1e-5 is not flat, even though bin 1 matches most others
    h2 = np.zeros(32)
    h2[10] = 1.0
    modes, _ = R.mean_shift_modes(h2)
    assert [m[0] for m in modes] == [11]
    # wrap-around: a mode straddling bin 32 / bin 1
    h3 = np.zeros(32)
    h3[31], h3[0], h3[15] = 5.0, 5.0, 2.0
    modes, _ = R.mean_shift_modes(h3)
    assert len(modes) == 2 and modes[0][0] in (1, 32) and modes[1][0] == 16


def _lattice(w, h, s=40.0, theta=0.3, origin=(200.0, 150.0), jitter=0.0, rng=None):
    c, sn = math.cos(theta), math.sin(theta)
    e1, e2 = np.array([c, sn]), np.array([-sn, c])
    pts = [np.array(origin) + x * s * e1 + y * s * e2 for y in range(h) for x in range(w)]
    pts = np.array(pts)
    if jitter:
        pts = pts + rng.normal(0, jitter, pts.shape)
    out = np.zeros(len(pts), IC.CORNER_DTYPE)
    out["u"], out["v"] = pts[:, 0], pts[:, 1]
    out["v1"], out["v2"], out["score"] = e1, e2, 0.5
    return out


def _is_planted(idx, corners, planted, w, h):
    """idx: recovered index matrix; planted: indices (into corners) of the planted w x h lattice, row-major."""
    P = np.asarray(planted).reshape(h, w)
    cands = [P, P[::-1], P[:, ::-1], P[::-1, ::-1], P.T, P.T[::-1], P.T[:, ::-1], P.T[::-1, ::-1]]
    return any(idx.shape == c.shape and np.array_equal(idx, c) for c in cands)


def test_structure_recovery_exact_lattice():
    c = _lattice(7, 5)
    idx = IC.chessboard_from_corners(c, (7, 5))
    assert idx.shape in ((5, 7), (7, 5)) and _is_planted(idx, c, np.arange(35), 7, 5)
    idx2 = IC.chessboard_from_corners(c, (5, 7))          # either orientation of the request
    assert np.array_equal(idx, idx2)
    with pytest.raises(IC.BoardNotFound) as e:
        IC.chessboard_from_corners(c, (6, 5))
    assert e.value.status == N.BOARD_NOT_FOUND


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_structure_recovery_jitter_and_distractors(seed):
    rng = np.random.default_rng(seed)
    board = _lattice(7, 5, theta=rng.uniform(-1.5, 1.5), jitter=0.8, rng=rng)
    far = np.zeros(12, IC.CORNER_DTYPE)      # distractors well off the lattice
    far["u"] = rng.uniform(600, 900, 12)
    far["v"] = rng.uniform(600, 900, 12)
    a = rng.uniform(0, math.pi, 12)
    far["v1"] = np.stack([np.cos(a), np.sin(a)], 1)
    far["v2"] = np.stack([-np.sin(a), np.cos(a)], 1)
    order = rng.permutation(len(board) + len(far))
    allc = np.concatenate([board, far])[order]
    where = np.argsort(order)[:35]           # position of planted corner k in allc
    idx = IC.chessboard_from_corners(allc, (7, 5))
    assert _is_planted(idx, allc, where, 7, 5)


def test_structure_recovery_missing_corner_and_second_board():
    c = _lattice(7, 5)
    with pytest.raises(IC.BoardNotFound) as e:
        IC.chessboard_from_corners(np.delete(c, 17), (7, 5))      # an interior corner missing
    assert e.value.status == N.BOARD_NOT_FOUND
    # a second, smaller board elsewhere is ignored
    other = _lattice(4, 3, s=30, theta=-0.4, origin=(900.0, 700.0))
    idx = IC.chessboard_from_corners(np.concatenate([c, other]), (7, 5))
    assert _is_planted(idx, c, np.arange(35), 7, 5)
    # two boards of the requested size: refused, never a guess
    twin = _lattice(7, 5, theta=0.1, origin=(900.0, 700.0))
    with pytest.raises(IC.BoardNotFound) as e:
        IC.chessboard_from_corners(np.concatenate([c, twin]), (7, 5))
    assert e.value.status == N.AMBIGUOUS
    # a larger lattice is one larger board, not a 7 x 5 one
    with pytest.raises(IC.BoardNotFound):
        IC.chessboard_from_corners(_lattice(9, 6), (7, 5))


# ------------------------------------------------------------------------------------------ synthetic images

def render_board(size, board=(7, 5), square=40.0, theta=0.0, centre=None, persp=(0.0, 0.0), blur=1.0, noise=2.0, seed=0,
                 occlude=None):
    """Anti-aliased chessboard (board = inner corners in x, y) under a homography; returns the uint8
    image and the true 0-based inner-corner positions [y][x] -> (u, v)."""
    W, H = size
    rng = np.random.default_rng(seed)
    c, s = math.cos(theta), math.sin(theta)
    cx, cy = centre if centre is not None else (W / 2, H / 2)
    bw, bh = board
    # board plane: inner corner (i, j) at ((i + 1) * square, (j + 1) * square); the board spans (bw+1) x (bh+1) squares
    ox, oy = (bw + 1) * square / 2, (bh + 1) * square / 2
    A = np.array([[c, -s, cx - (c * ox - s * oy)], [s, c, cy - (s * ox + c * oy)], [persp[0], persp[1], 1.0]])
    A[2, 2] = 1.0 - persp[0] * cx - persp[1] * cy   # keeps the board centre where it was placed (to first order)
    Hinv = np.linalg.inv(A)
    ss = (np.arange(4) + 0.5) / 4 - 0.5
    acc = np.zeros((H, W))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for dy in ss:
        for dx in ss:
            q = Hinv @ np.stack([(xs + dx).ravel(), (ys + dy).ravel(), np.ones(xs.size)])
            X, Y = (q[0] / q[2]).reshape(H, W), (q[1] / q[2]).reshape(H, W)
            inside = (X >= 0) & (X < (bw + 1) * square) & (Y >= 0) & (Y < (bh + 1) * square)
            black = (np.floor(X / square) + np.floor(Y / square)) % 2 == 0
            acc += np.where(inside & black, 30.0, 220.0)
    img = acc / 16
    if blur > 0:
        r = int(math.ceil(3 * blur))
        k = np.exp(-0.5 * (np.arange(-r, r + 1) / blur) ** 2)
        k /= k.sum()
        img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, np.pad(img, r, mode="edge"))
        img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, img)[r:-r, r:-r]
    img = img + rng.normal(0, noise, img.shape)
    if occlude is not None:
        ox_, oy_, rad = occlude
        img[(ys - oy_) ** 2 + (xs - ox_) ** 2 < rad * rad] = 220.0
    img[0, 0], img[-1, -1] = 0, 255
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    P = np.array([[A @ np.array([(i + 1) * square, (j + 1) * square, 1.0]) for i in range(bw)] for j in range(bh)])
    return img, P[..., :2] / P[..., 2:3]


def _match(board_xy, truth):
    """Largest distance from each true corner to its nearest detected corner."""
    d = np.linalg.norm(board_xy.reshape(-1, 1, 2) - truth.reshape(1, -1, 2), axis=2)
    return d.min(0).max(), d.min(1).max()


def _excused(L, c, tol=1e-5):
    """NMS candidate (1-based u, v) whose value lies within tol of tau or of a competing value nearby."""
    u, v = c
    val = L[v - 1, u - 1]
    if abs(val - R.NMS_TAU) < tol:
        return True
    win = L[max(v - 8, 0):v + 7, max(u - 8, 0):u + 7]
    return int((np.abs(win - val) < tol).sum()) > 1


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["crop2", "crop6", "synthetic"])
def test_stage_parity_with_restatement(which):
    if which == "synthetic":
        img, _ = render_board((320, 256), theta=0.35, square=24.0, persp=(2e-4, -1e-4), seed=7)
    else:
        img, _ = _crop(int(which[-1]))
    corners, st = IC.find_corners(img, stages=True)
    ref = R.find_corners(img, stages=True)
    Lg = st["likelihood"].cpu().numpy().astype(np.float64)
    dL = np.abs(Lg - ref["L"]).max()
    assert dL < 1e-5, dL
    gc = [tuple(x) for x in st["candidates"]]
    rc = list(ref["cand"])
    assert st["n_candidates"] == len(gc)
    only_g, only_r = set(gc) - set(rc), set(rc) - set(gc)
    excused = sorted(c for c in only_g | only_r if _excused(ref["L"], c))
    assert not (only_g | only_r) - set(excused), sorted((only_g | only_r) - set(excused))
    common_g = [c for c in gc if c not in excused]
    common_r = [c for c in rc if c not in excused]
    assert common_g == common_r
    print("%s: %d candidates, |dL| %.2e, excused %s" % (which, len(gc), dL, excused))
    # refinement of every common candidate
    Pr, V1r, V2r = ref["refined_all"]
    ri = {c: k for k, c in enumerate(rc)}
    gi = {c: k for k, c in enumerate(gc)}
    for c in common_r:
        g, r = st["refined"][gi[c]], ri[c]
        gvalid, rvalid = bool(g["v1"].any()), bool(V1r[r].any())
        assert gvalid == rvalid, c
        if not rvalid:
            continue
        assert abs(g["u"] - Pr[r, 0]) < 1e-3 and abs(g["v"] - Pr[r, 1]) < 1e-3, (c, g["u"], g["v"], Pr[r])
        for gv, rv in ((g["v1"], V1r[r]), (g["v2"], V2r[r])):
            assert abs(abs(float(gv @ rv)) - 1) < 1e-9, (c, gv, rv)
    # final list: same corners, same order, same directions and scores
    assert len(corners) == len(ref["p"]), (len(corners), len(ref["p"]))
    dp = np.abs(np.stack([corners["u"], corners["v"]], 1) - ref["p"]).max() if len(corners) else 0.0
    assert dp < 1e-3, dp
    assert np.abs(corners["v1"] - ref["v1"]).max() < 1e-6 and np.abs(corners["v2"] - ref["v2"]).max() < 1e-6
    assert np.abs(corners["score"] - ref["score"]).max() < 1e-9 + 1e-7 * np.abs(ref["score"]).max()


def _detected_file(i, path):
    img, org = _crop(i)
    b = IC.find_chessboard(img, (7, 5))
    assert b.shape[:2] in ((7, 5), (5, 7))
    IC.save_cam_corners(path, b + org[None, None, :].astype(np.float64))
    return b


@pytest.mark.gpu
def test_reference_pin_six_images(tmp_path):
    """The reference's detector output from its own images: every corner within 0.5 px, RMS <= 0.2 px."""
    rows = []
    for i in range(1, 7):
        f = str(tmp_path / f"pointgrey{i}.txt")
        _detected_file(i, f)
        got = calib.check_order_cam(calib.read_cam_corners(f, 35))
        want = calib.check_order_cam(calib.read_cam_corners(os.path.join(GOLD, f"pointgrey{i}.txt"), 35))
        assert got.shape == want.shape == (35, 2)
        d = np.linalg.norm(got - want, axis=1)
        rows.append((i, d.max(), math.sqrt((d ** 2).mean())))
    print("\n".join("pointgrey%d: max %.4f px, rms %.4f px" % r for r in rows))
    for i, mx, rms in rows:
        assert mx <= 0.5 and rms <= 0.2, (i, mx, rms)


@pytest.mark.gpu
def test_end_to_end_calibration_from_detected_files(tmp_path):
    for i in range(1, 7):
        _detected_file(i, str(tmp_path / f"pointgrey{i}.txt"))
        shutil.copy(os.path.join(GOLD, f"pointgrey_lidar_{i}.txt"), tmp_path / f"pointgrey_lidar_{i}.txt")
    T, err = calib.calib_lidar_cam(str(tmp_path), "pointgrey", 6, CAM)
    ref = calib.extrinsic_read(os.path.join(GOLD, "pointgrey.bin"))
    c = (np.trace(T[:3, :3].T @ ref[:3, :3]) - 1) / 2
    rot = math.degrees(math.acos(min(1.0, max(-1.0, c))))
    dt = np.linalg.norm(T[:3, 3] - ref[:3, 3])
    print("extrinsic vs pointgrey.bin: %.4f deg, %.2f mm, reprojection %.3f px" % (rot, dt * 1e3, err))
    assert rot < 0.1 and dt < 5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [0, 15, 30, 45, 60, 75, 90])
@pytest.mark.parametrize("board", [(7, 5), (5, 7)])
def test_synthetic_boards(deg, board):
    img, truth = render_board((480, 400), board=board, square=36.0, theta=math.radians(deg), persp=(1.5e-4, 1e-4),
                              seed=deg + board[0])
    b = IC.find_chessboard(img, board)
    assert b.shape[:2] in ((7, 5), (5, 7))
    a, bmax = _match(b, truth)
    assert a < 0.25 and bmax < 0.25, (a, bmax)


@pytest.mark.gpu
def test_synthetic_full_frame():
    img, truth = render_board((1920, 1200), square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    b = IC.find_chessboard(img, (7, 5))
    a, bmax = _match(b, truth)
    assert a < 0.25 and bmax < 0.25, (a, bmax)


@pytest.mark.gpu
def test_occluded_corner_and_empty_frame_not_found():
    img, truth = render_board((480, 400), theta=0.2, square=36.0, seed=3)
    u, v = truth[2, 3]
    occ, _ = render_board((480, 400), theta=0.2, square=36.0, seed=3, occlude=(u, v, 9.0))
    assert IC.find_chessboard(img, (7, 5)).shape[:2] in ((7, 5), (5, 7))
    with pytest.raises(IC.BoardNotFound) as e:
        IC.find_chessboard(occ, (7, 5))
    assert e.value.status == N.BOARD_NOT_FOUND
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:400, 0:480]
    empty = np.clip(128 + 60 * np.sin(xx / 37.0) * np.cos(yy / 53.0) + rng.normal(0, 3, xx.shape), 0, 255).astype(np.uint8)
    with pytest.raises(IC.BoardNotFound) as e:
        IC.find_chessboard(empty, (7, 5))
    assert e.value.status == N.BOARD_NOT_FOUND


@pytest.mark.gpu
def test_input_checks():
    import torch
    L = IC.lib()
    t = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    out = (IC.ImageCorner * 16)()
    n = C.c_int32(-1)

    def call(ptr, w, h, stride, corners=out, count=C.byref(n)):
        return L.ilcc_image_corners_device(ptr, w, h, stride, corners, 16, count, None, None)

    cases = [(C.c_void_p(t.data_ptr()), 64, 64, 63), (C.c_void_p(t.data_ptr()), 33, 64, 64),
             (C.c_void_p(t.data_ptr()), 64, 33, 64), (None, 64, 64, 64)]
    for args in cases:
        N.lib().ilcc_last_error(None)
        assert call(*args) == N.BAD_ARGUMENT, args
        assert N.lib().ilcc_last_error(None).decode(), args
    assert call(C.c_void_p(t.data_ptr()), 64, 64, 64, count=None) == N.BAD_ARGUMENT
    assert call(C.c_void_p(t.data_ptr()), 64, 64, 64, corners=None) == N.BAD_ARGUMENT
    # a constant image is valid and has no corners
    assert call(C.c_void_p(t.data_ptr()), 64, 64, 64) == N.OK and n.value == 0
    with pytest.raises(ValueError):
        IC.find_corners(np.zeros((40, 40), np.float32))
