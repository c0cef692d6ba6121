"""Constructed corner lists for structure recovery (K18 and the host code): no image is needed.

A board is a lattice of nx x ny points with spacing sq, rotated by th, warped by (X, Y) -> (X, Y) / (1 + px X + py Y) and moved to
(cx, cy), with Gaussian jitter of 0.02 - 0.05 px -- never 0: an exact lattice makes ties that a last-bit difference of atan2 / cos /
sin between two libms could flip.  v1, v2 are the unit images of the lattice axes at the point under findCorners.m's sign rules
(v1.x + v1.y >= 0, (v1, v2) right-handed: v1.x v2.y - v1.y v2.x > 0).  Strays are uniform in the frame with a random orthogonal
direction pair, kept out of a disc around the board.  The list is then sorted by u, stably: the scan order of NMS.

Every case carries the board it asks for and the status the host code gives; the seeds are pinned, and the tests assert that
status, so a drifting generator cannot empty them.

The second table (EDGE_CASES) holds what the jittered lattices cannot: exact ties that no last bit can flip, the overlap events, the
board capacities, corner counts at the edges of K18's used words and the magnitude limit."""
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


# ---- ties, capacity edges, used-word edges, magnitudes, overlap events ---------------------------------------------------------------
#
# The cases above never meet an exact tie in a distance.  These do, built so that no last bit of atan2 / cos / sin can undo the
# tie: tests/test_structure_ref_cpu.py shows each T_ case DECISIVE (another answer under the wrong tie rule) and LIBM-PROOF.

def exact(points):
    """integer positions with the directions exactly (1, 0) and (0, 1)"""
    return np.array([(float(x), float(y), (1.0, 0.0), (0.0, 1.0), 1.0) for x, y in points], CORNER_DTYPE)


def defects(seed):
    """a 5 x 9 lattice, the long axis vertical so that the u-sorted seed order interleaves its halves, with one or two corners
    dropped, one or two displaced by 1 - 3 px and up to four strays inside its bounding box, and a 4 x 4 lattice of its own to the
    left: what the overlap events are searched in"""
    rng = np.random.default_rng(seed)
    cells = [(ix, iy) for iy in range(9) for ix in range(5)]
    drop = {cells[k] for k in rng.choice(len(cells), rng.integers(1, 3), replace=False)}
    mid = (400.0, 240.0)
    lat = lattice(rng, 5, 9, 30, rng.uniform(-0.2, 0.2), P, mid, drop=drop)
    for k in rng.choice(len(lat), rng.integers(1, 3), replace=False):
        a, r = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 3.0)
        lat["u"][k] += r * np.cos(a)
        lat["v"][k] += r * np.sin(a)
    near = strays(rng, 40, (640, 480), (-1e4, -1e4), 1.0)
    near = near[(np.abs(near["u"] - mid[0]) < 90) & (np.abs(near["v"] - mid[1]) < 150)][:rng.integers(0, 5)]
    return scan_order(lattice(rng, 4, 4, 30, 0.1, P, (120.0, 240.0)), lat, near)      # the small board is stored first, and stays


TIE_CASES = ["T_dup", "T_grid", "T_mid", "T_border", "T_equal"]
OVERLAP_CASES = ["O_one", "O_two", "O_mixed"]
COUNT_CASES = ["N63", "N64", "N65", "N127", "N128", "N129"]
CAPACITY_CASES = ["S64x4", "S65x4", "S80x3", "M_strays"]
MAGNITUDE_CASES = ["X_u", "X_u_above", "X_dir", "X_dir_above"]
MARKED = {"S65x4", "M_strays", "X_u_above", "X_dir_above"}      # the device marks them: the host's answer, one fallback each
EDGE_CASES = TIE_CASES + OVERLAP_CASES + COUNT_CASES + CAPACITY_CASES + MAGNITUDE_CASES
# the other half of an overlap event: the board that it must leave alone -- O_two's disjoint side board, O_mixed's worse board
SECOND_BOARDS = {"O_two": (4, 4), "O_mixed": (3, 5)}
OVERLAP_SEEDS = {"O_one": 0, "O_two": 19, "O_mixed": 61}      # of defects(), found by tools/dev_structure_overlap_search.py
MAX_ABS = 1e15      # ILCC_STRUCTURE_MAX_ABS


def _edge_case(name):
    rng = np.random.default_rng({"T_dup": 31, "S64x4": 32, "S65x4": 33, "S80x3": 34, "M_strays": 19}.get(name, 11))      # 19, 11: M's and A's lattices
    if name == "T_dup":
        # case A's generator; copies of board corners (a board corner, two edge corners, an inner one) and of two strays.  The stable
        # sort puts a copy right behind its original, and every distance to the two is equal whatever the prediction's last bit.
        lat, far = lattice(rng, 7, 5, 40, 0.1, P, MID), strays(rng, 6, (640, 480), MID, 230)
        return Case(name, scan_order(lat, far, lat[[0, 17, 20, 31]], far[[1, 4]]), (7, 5), OK)
    if name == "T_grid":
        # 6 x 5 exact lattice without (5, 2) and (2, 4); a pair mirrored about each hole, across the direction of growth that reaches
        # it (a new last column, a new last row: the two whose predictions are exact under any libm in bounds, see the CPU test)
        xs, ys = [544 + 32 * i for i in range(6)], [288 + 32 * j for j in range(5)]
        lat = [(x, y) for j, y in enumerate(ys) for i, x in enumerate(xs) if (i, j) not in ((5, 2), (2, 4))]
        pairs = [(xs[5], ys[2] - 2), (xs[5], ys[2] + 2), (xs[2] - 2, ys[4]), (xs[2] + 2, ys[4])]
        far = [(130, 140), (170, 700), (260, 130), (300, 900), (140, 420), (980, 140), (1000, 900), (400, 1000)]
        return Case(name, scan_order(exact(lat + pairs + far)), (6, 5), OK)
    if name == "T_mid":
        # 3 x 6 exact lattice; of a fourth row the corners of columns 0 .. 3, one corner midway between the predictions of columns 4
        # and 5 -- 16 px from both, and the lower prediction must take it -- and one 16 px right of column 5 and 1 px off the row: 16.03
        # px from its prediction, so that the midway tie is the minimum when it is met, and every triple stays below the 1/4 at
        # which a three-row board stops growing (the worst is 16 / sqrt(64^2 + 16^2) = 0.2425).  Six columns: with more, the 4 x (columns - 2)
        # board without the two, at exactly -cells, beats the full one and the tie no longer shows in the final answer
        xs, ys = [544 + 32 * i for i in range(6)], [288 + 32 * j for j in range(4)]
        lat = [(x, y) for y in ys[:3] for x in xs] + [(x, ys[3]) for x in xs[:4]] + [(xs[4] + 16, ys[3]), (xs[5] + 16, ys[3] + 1)]
        far = [(130, 140), (170, 700), (260, 130), (300, 900), (140, 420), (980, 140), (1000, 900), (400, 1000)]
        return Case(name, scan_order(exact(lat + far)), (6, 4), OK, (4, 6))
    if name == "T_border":
        # 5 x 5 exact lattice, every proposal inside it at exactly -cells, and three corners of a sixth row above columns 1 .. 3: a
        # board that takes the new first row while it is three wide keeps it and never widens; one that widens first never gets it
        xs, ys = [544 + 32 * i for i in range(5)], [320 + 32 * j for j in range(5)]
        lat = [(x, y) for y in ys for x in xs] + [(x, ys[0] - 32) for x in xs[1:4]]
        far = [(130, 140), (170, 700), (260, 130), (300, 900), (140, 420), (980, 140), (1000, 900), (400, 1000)]
        return Case(name, scan_order(exact(lat + far)), (5, 5), OK)
    if name == "T_equal":
        # an exact L: a 3 x 7 bar and a 7 x 3 bar that share a 3 x 3 square, both at exactly -21.  The horizontal bar's seeds come
        # first in u and the vertical bar's last, so the stored board is the horizontal one only while an equal newcomer loses
        xs, ys = [544 + 32 * i for i in range(7)], [288 + 32 * j for j in range(7)]
        return Case(name, scan_order(exact([(x, y) for y in ys[4:] for x in xs] + [(x, y) for y in ys[:4] for x in xs[4:]])), (7, 3), OK, (3, 7))
    if name in OVERLAP_CASES:
        # the board asked for is the one that the newcomer of the event leaves (O_one, O_two: the newcomer itself) or keeps (O_mixed)
        return Case(name, defects(OVERLAP_SEEDS[name]), (5, 5) if name == "O_mixed" else (3, 9), OK)
    if name in COUNT_CASES:      # the corner counts at the edges of the 64-bit used words; strays left of the board put it across an edge
        n = int(name[1:])
        rng = np.random.default_rng(100 + n)
        lat, far = lattice(rng, 7, 5, 40, 0.3, P, MID), strays(rng, 900, (640, 480), MID, 150)
        left = {63: 28, 64: 29, 65: 30, 127: 60, 128: 45, 129: 94}[n]      # the board's corners are left .. left + 34
        return Case(name, scan_order(lat, far[far["u"] < 170][:left], far[far["u"] > 470][:n - 35 - left]), (7, 5), OK)
    if name in ("S64x4", "S65x4"):
        # ILCC_STRUCTURE_MAX_SIDE and ILCC_STRUCTURE_MAX_CELLS exactly, and one column more.  The fourth row lies 1.649 spacings below
        # the third: its collinearity error of 0.245 keeps a new row (accepted below 1/4) behind every new column (better from
        # 0.25 - 0.75 / columns on), so a seed of the second row grows 3 x 64 first and then proposes a row of 64 predictions that
        # makes 256 cells -- or, with 65 columns, a row above the side capacity
        nx = int(name[1:3])
        lat = lattice(rng, nx, 4, 12, 0.02, (1e-5, -1e-5), (420.0, 240.0))
        lat["u"][3 * nx:] += 0.649 * 12 * -np.sin(0.02)
        lat["v"][3 * nx:] += 0.649 * 12 * np.cos(0.02)
        return Case(name, scan_order(lat), (64, 4) if nx == 64 else (7, 5), OK if nx == 64 else NOT_FOUND)
    if name == "S80x3":      # a side above 64 that only column borders (3 predictions) ever reach: from 61 columns on a row border
        return Case(name, scan_order(lattice(rng, 80, 3, 10, 0.02, (1e-5, -1e-5), (420.0, 240.0))), (80, 3), OK)      # has too few candidates
    if name == "M_strays":      # case M's 256 cells with candidates left: the next proposal would have 272
        return Case(name, scan_order(lattice(rng, 16, 16, 20, 0.1, (1e-4, -1e-4), MID), strays(rng, 20, (640, 480), MID, 230)), (16, 16), OK, (16, 16))
    if name in MAGNITUDE_CASES:      # case A and one stray with a coordinate or a direction component at, or just above, ILCC_STRUCTURE_MAX_ABS
        lat = lattice(rng, 7, 5, 40, 0.1, P, MID)
        big = MAX_ABS if not name.endswith("_above") else float(np.nextafter(MAX_ABS, np.inf))
        one = np.array([(big, 100.0, (1.0, 0.0), (0.0, 1.0), 0.5) if name.startswith("X_u") else (600.0, 50.0, (big, 0.0), (0.0, 1.0), 0.5)], CORNER_DTYPE)
        return Case(name, scan_order(lat, one), (7, 5), OK)
    raise KeyError(name)


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _edge_case(name) if name in EDGE_CASES else _case(name)
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
