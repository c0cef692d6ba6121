"""The specification of K15's seed proposer (include/ilcc_seed.h) in numpy: float32 for the quantisation, Python integers
for everything else, scipy's connected-component labelling (a flood fill where scipy is missing) for the components and
numpy.linalg.eigvalsh for the finishing.  The GPU's integer records must equal `components` exactly."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

RECORD_WORDS = 11
TABLE_MIN = 64
GRID_MAX = 1024


@dataclasses.dataclass
class SeedParams:
    """ilcc_default_seed_params for the default ilcc_params (6 x 8 squares of 0.15 m)."""
    cell: float = 0.12
    range: float = 20.0
    cluster_min: int = 100
    max_components: int = 64
    max_seeds: int = 4
    board_w: int = 6
    board_h: int = 8
    grid_length: float = 0.15
    max_rms: float = 0.03
    size_lo: float = 0.7
    size_hi: float = 1.3
    max_oob_share: float = 0.05


@dataclasses.dataclass
class Grid:
    range_q: int
    cq: int
    off: int
    N: int


def grid(sp: SeedParams, max_total_points: int = 1 << 20) -> Grid:
    range_q = min(int(math.floor(sp.range * 1024.0)), int(math.floor(math.sqrt(float(1 << 62) / max(max_total_points, 1)))))
    cq = int(math.ceil(sp.cell * 1024.0))
    off = -(-range_q // cq)
    if 2 * off + 1 > GRID_MAX:
        raise ValueError("range / cell too large")
    return Grid(range_q, cq, off, 2 * off + 1)


def table_size(n_points: int) -> int:
    t = TABLE_MIN
    while t < 2 * n_points:
        t <<= 1
    return t


def hash_slot(key: int, size: int) -> int:
    bits = size.bit_length() - 1
    return ((key * 2654435761) & 0xFFFFFFFF) >> (32 - bits)


def quantise(cloud: np.ndarray, g: Grid):
    """-> (keep mask over the points, q int64 [kept, 3])"""
    xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, cloud.shape[-1])[:, :3]
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor(xyz * np.float32(1024.0) + np.float32(0.5))
        keep = np.isfinite(xyz).all(1) & (np.abs(t) <= np.float32(g.range_q)).all(1)
    return keep, t[keep].astype(np.int64)


def _label(occ: np.ndarray):
    try:
        from scipy import ndimage
        return ndimage.label(occ, structure=np.ones((3, 3, 3), bool))
    except ImportError:
        lab = np.zeros(occ.shape, np.int32)
        n = 0
        for start in zip(*np.nonzero(occ)):
            if lab[start]:
                continue
            n += 1
            lab[start] = n
            stack = [start]
            while stack:
                x, y, z = stack.pop()
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            j = (x + dx, y + dy, z + dz)
                            if min(j) >= 0 and j[0] < occ.shape[0] and j[1] < occ.shape[1] and j[2] < occ.shape[2] and occ[j] and not lab[j]:
                                lab[j] = n
                                stack.append(j)
        return lab, n


def components(cloud: np.ndarray, sp: SeedParams, g: Grid | None = None, want_labels: bool = False):
    """Records of the components of at least sp.cluster_min points, sorted by root key: lists of 11 Python ints
    (key, n, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz).  want_labels: also (keep mask, root key of every kept point)."""
    g = g or grid(sp)
    keep, q = quantise(cloud, g)
    if len(q) == 0:
        return ([], keep, np.zeros(0, np.int64)) if want_labels else []
    cell = q // g.cq                                   # numpy's // on integers is floor division
    lo = cell.min(0)
    idx = cell - lo
    shape = tuple(int(v) for v in idx.max(0) + 1)
    occ = np.zeros(shape, bool)
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    lab, n_lab = _label(occ)
    plab = lab[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.int64)
    key = (cell[:, 0] + g.off) + g.N * ((cell[:, 1] + g.off) + g.N * (cell[:, 2] + g.off))
    order = np.argsort(plab, kind="stable")
    starts = np.nonzero(np.diff(plab[order], prepend=-1))[0]
    qo = q[order].astype(object)                       # Python integers from here on
    cols = [qo[:, 0], qo[:, 1], qo[:, 2], qo[:, 0] * qo[:, 0], qo[:, 0] * qo[:, 1], qo[:, 0] * qo[:, 2],
            qo[:, 1] * qo[:, 1], qo[:, 1] * qo[:, 2], qo[:, 2] * qo[:, 2]]
    sums = [np.add.reduceat(c, starts) for c in cols]
    counts = np.diff(np.append(starts, len(order)))
    roots = np.minimum.reduceat(key[order], starts)
    recs = []
    for k in range(len(starts)):
        if counts[k] >= sp.cluster_min:
            recs.append([int(roots[k]), int(counts[k])] + [int(s[k]) for s in sums])
    recs.sort(key=lambda r: r[0])
    if want_labels:
        root_of = np.zeros(n_lab + 1, np.int64)
        root_of[plab[order][starts]] = roots
        return recs, keep, root_of[plab]
    return recs


@dataclasses.dataclass
class Seed:
    centroid: np.ndarray   # float32 x 3
    n: int
    l1: float
    l2: float
    rms: float
    score: float
    key: int


def measure(rec) -> Seed:
    """centroid, sizes and score of one record, before any gate"""
    key, n = rec[0], rec[1]
    s = rec[2:5]
    ss = [[rec[5], rec[6], rec[7]], [rec[6], rec[8], rec[9]], [rec[7], rec[9], rec[10]]]
    scale = float(n) * float(n) * 1048576.0
    cov = np.array([[float(n * ss[a][b] - s[a] * s[b]) / scale for b in range(3)] for a in range(3)])
    ev = np.linalg.eigvalsh(cov)
    centroid = np.array([float(s[a]) / (float(n) * 1024.0) for a in range(3)]).astype(np.float32)
    return Seed(centroid, n, math.sqrt(12.0 * max(ev[1], 0.0)), math.sqrt(12.0 * max(ev[2], 0.0)), math.sqrt(max(ev[0], 0.0)), 0.0, key)


def finish(recs, sp: SeedParams):
    """Gates, score and order: at most sp.max_seeds Seed, ascending by (score, key)."""
    s1, s2 = sp.board_w * sp.grid_length, sp.board_h * sp.grid_length
    out = []
    for rec in recs:
        sd = measure(rec)
        sd.score = abs(sd.l1 - s1) / s1 + abs(sd.l2 - s2) / s2
        if sd.rms <= sp.max_rms and sp.size_lo * s1 <= sd.l1 <= sp.size_hi * s1 and sp.size_lo * s2 <= sd.l2 <= sp.size_hi * s2:
            out.append(sd)
    out.sort(key=lambda d: (d.score, d.key))
    return out[:sp.max_seeds]


def propose(cloud: np.ndarray, sp: SeedParams, g: Grid | None = None):
    recs = components(cloud, sp, g)
    if len(recs) > sp.max_components:
        return None                                    # ILCC_CAPACITY for the frame
    return finish(recs, sp)
