"""Constructed corner lists for structure recovery (K18 and the host code): no image is needed.

A board is a lattice of nx x ny points with spacing sq, rotated by th, warped by (X, Y) -> (X, Y) / (1 + px X + py Y) and moved to
(cx, cy), with Gaussian jitter of 0.02 - 0.05 px -- never 0: an exact lattice makes ties that a last-bit difference of atan2 / cos /
sin between two libms could flip.  v1, v2 are the unit images of the lattice axes at the point under findCorners.m's sign rules
(v1.x + v1.y >= 0, (v1, v2) right-handed: v1.x v2.y - v1.y v2.x > 0).  Strays are uniform in the frame with a random orthogonal
direction pair, kept out of a disc around the board.  The list is then sorted by u, stably: the scan order of NMS.

Every case carries the board it asks for and the status the host code gives; the seeds are pinned, and the tests assert that
status, so a drifting generator cannot empty them."""
import numpy as np

from lidar_camera_calibration_amd import _native
from lidar_camera_calibration_amd.image_corners import CORNER_DTYPE

OK, NOT_FOUND, AMBIGUOUS = _native.OK, _native.BOARD_NOT_FOUND, _native.AMBIGUOUS


def lattice(rng, nx, ny, sq, th, persp, centre, sigma=0.03, drop=()):
    """[nx * ny - len(drop)] CORNER_DTYPE, in lattice order (x inner); `drop`: (ix, iy) points left out"""
    px, py = persp
    c, s = np.cos(th), np.sin(th)
    out = []
    for iy in range(ny):
        for ix in range(nx):
            if (ix, iy) in drop:
                continue
            x0, y0 = (ix - (nx - 1) / 2.0) * sq, (iy - (ny - 1) / 2.0) * sq
            X, Y = c * x0 - s * y0, s * x0 + c * y0
            w = 1.0 + px * X + py * Y
            J = np.array([[(w - X * px), -X * py], [-Y * px, (w - Y * py)]]) / (w * w)
            t1, t2 = J @ np.array([c, s]), J @ np.array([-s, c])
            v1, v2 = t1 / np.hypot(*t1), t2 / np.hypot(*t2)
            if v1[0] + v1[1] < 0:
                v1 = -v1
            if v1[0] * v2[1] - v1[1] * v2[0] < 0:
                v2 = -v2
            jit = rng.normal(0.0, sigma, 2)
            out.append((X / w + centre[0] + jit[0], Y / w + centre[1] + jit[1], v1, v2, 1.0))
    return np.array(out, CORNER_DTYPE)


def strays(rng, count, frame, centre, radius):
    out = []
    while len(out) < count:
        u, v = rng.uniform(0, frame[0]), rng.uniform(0, frame[1])
        if np.hypot(u - centre[0], v - centre[1]) < radius:
            continue
        a = rng.uniform(0, 2 * np.pi)
        v1, v2 = np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
        if v1[0] + v1[1] < 0:
            v1, v2 = -v1, -v2      # still right-handed
        out.append((u, v, v1, v2, 0.5))
    return np.array(out, CORNER_DTYPE)


def scan_order(*parts):
    c = np.concatenate([p for p in parts if len(p)]) if any(len(p) for p in parts) else np.zeros(0, CORNER_DTYPE)
    return c[np.argsort(c["u"], kind="stable")]


class Case:
    def __init__(self, name, corners, board, status, shape=None):
        self.name, self.corners, self.board, self.status, self.shape = name, corners, board, status, shape

    def __repr__(self):
        return "Case(%s, %d corners, %dx%d)" % (self.name, len(self.corners), self.board[0], self.board[1])


P = (2e-4, -1e-4)
MID = (320.0, 240.0)


def _case(name):
    seed = {"A": 11, "B": 12, "C": 13, "H": 14, "I": 15, "J": 16, "K": 17, "L": 18, "M": 19, "E": 20, "F": 21, "Z": 22, "W": 23, "N": 24}[name]
    rng = np.random.default_rng(seed)
    if name == "A":
        return Case(name, scan_order(lattice(rng, 7, 5, 40, 0.1, P, MID)), (7, 5), OK, (5, 7))
    if name == "B":
        return Case(name, scan_order(lattice(rng, 7, 5, 40, 0.3, P, MID), strays(rng, 300, (640, 480), MID, 230)), (7, 5), OK)
    if name == "C":
        return Case(name, scan_order(lattice(rng, 7, 5, 30, 0.1, P, (155.0, 240.0)), lattice(rng, 7, 5, 30, -0.15, P, (485.0, 240.0))), (7, 5), AMBIGUOUS)
    if name == "H":
        return Case(name, scan_order(lattice(rng, 11, 8, 25, 0.2, (1e-4, 1e-4), MID), strays(rng, 50, (640, 480), MID, 220)), (11, 8), OK, (8, 11))
    if name == "I":
        return Case(name, scan_order(lattice(rng, 7, 5, 40, 0.1, P, MID, drop={(3, 2)})), (7, 5), NOT_FOUND)
    if name == "J":
        mid = (960.0, 600.0)
        return Case(name, scan_order(lattice(rng, 7, 5, 60, 0.2, (1e-4, -5e-5), mid), strays(rng, 1200, (1920, 1200), mid, 380)), (7, 5), OK)
    if name == "K":
        return Case(name, scan_order(lattice(rng, 7, 5, 30, 0.1, P, (170.0, 240.0)), lattice(rng, 5, 4, 30, -0.2, P, (470.0, 240.0))), (7, 5), OK)
    if name == "L":
        return Case(name, scan_order(lattice(rng, 9, 7, 35, 0.15, P, MID)), (7, 5), NOT_FOUND)
    if name == "M":
        return Case(name, scan_order(lattice(rng, 16, 16, 20, 0.1, (1e-4, -1e-4), MID)), (16, 16), OK, (16, 16))
    if name == "E":
        return Case(name, scan_order(lattice(rng, 3, 3, 40, 0.1, P, MID)), (7, 5), NOT_FOUND)
    if name == "F":
        return Case(name, scan_order(lattice(rng, 3, 3, 40, 0.1, P, MID, drop={(2, 2)})), (7, 5), NOT_FOUND)
    if name == "Z":
        return Case(name, np.zeros(0, CORNER_DTYPE), (7, 5), NOT_FOUND)
    if name == "W":   # 272 cells, above the device's 256: the host recomputes it (about a second there)
        return Case(name, scan_order(lattice(rng, 17, 16, 20, 0.1, (1e-4, -1e-4), MID)), (7, 5), NOT_FOUND)
    if name == "N":   # stage parity only
        return Case(name, scan_order(lattice(rng, 12, 12, 25, 0.25, (1e-4, 1e-4), MID)), (12, 12), OK, (12, 12))
    raise KeyError(name)


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _case(name)
    return _cache[name]


BATCH_CASES = ["A", "B", "C", "H", "I", "J", "K", "L", "M", "E", "F", "Z"]   # W comes on top where a fallback is wanted


def replay_overlap_rule(seed_boards, board):
    """chessboardsFromCorners' keep-below--10 test and overlap rule on [(index matrix or None, energy)] in seed order, then the one
    board of the requested shape -> (status, index matrix or None)"""
    stored = []
    for b, e in seed_boards:
        if b is None or not e < -10:
            continue
        cells = set(b.reshape(-1).tolist())
        over = [k for k, (ob, _) in enumerate(stored) if cells & set(ob.reshape(-1).tolist())]
        if not over:
            stored.append((b, e))
        elif all(stored[k][1] > e for k in over):
            stored = [sb for k, sb in enumerate(stored) if k not in over] + [(b, e)]
    hits = [b for b, _ in stored if b.shape in ((board[0], board[1]), (board[1], board[0]))]
    if not hits:
        return NOT_FOUND, None
    if len(hits) > 1:
        return AMBIGUOUS, None
    return OK, hits[0]
